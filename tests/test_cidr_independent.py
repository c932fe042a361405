"""IP_ADDRESSES lists (parseIPList / addEntry on net.ParseCIDR, IPNet.Contains) against a reference
that shares nothing with oracle/ or the product: Go's documented behaviour written on top of Python's
`ipaddress` (what test_ip_vs_python_ipaddress.py does for net.ParseIP alone).

  entry -> net   "/32" appended when the entry holds no "/" (ipList.go addEntry -- so "::1" is
                 "::1/32" = "::/32"); split at the first "/"; the prefix is ASCII digits only and
                 at most the family's bit count; `ipaddress.ip_address` parses the address;
                 lo = address & mask, hi = lo | host bits.
  4-in-6         an IPv6 net whose masked network number lies in ::ffff:0:0/96 is an IPv4 net
                 (IPNet.Contains compares after To4) of prefix - 96; every other IPv6 net is IPv6.
  lookup         a string `ip_address` rejects is an error (-1); an IPv4 address, or an IPv6 address
                 in ::ffff:0:0/96, is the 32-bit IPv4 address, everything else IPv6; found = some net
                 of the same family has lo <= x <= hi.  A 4-in-6 lookup never matches an IPv6 net,
                 not even ::/0.
  tables         per family the ranges sorted and merged where they overlap or touch.

Go 1.9 and `ipaddress` differ on leading zeros in IPv4 octets (Go accepts, Python rejects), on
hextets of more than four digits with leading zeros (likewise), and on scope ids (`%eth0`: Python
accepts, Go rejects): the generators emit none of these, in entries or in lookups.  Netmask-style
prefixes (`/255.0.0.0`) are an error in Go, and the reference rejects them as well, so they stay
among the malformed entries.  GO_ONLY below holds a few such spellings with no expected value: the
oracle, the host program and the GPU must agree with each other (corroboration, not pinning --
`ipaddress` is not Go's net package).

What is checked here, on the CPU: the oracle's IPList (oracle/lists.py, lists_oracle.c), and the
product's host half (istio_amd/csrc/cidr.h: addEntry, merge, the 128-bit ranges, the /16 directory)
as a stand-alone program (tests/cidr_host.cpp) under ASan + UBSan -- mxp_list_create itself needs a
GPU.  tests/test_gpu_cidr_independent.py imports the reference, the lists and the lookups and runs
them through the device search."""
import functools
import ipaddress
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

TOP = {4: (1 << 32) - 1, 6: (1 << 128) - 1}
LOW64 = (1 << 64) - 1


# ------------------------------------------------------------------ the reference
def ref_net(entry: str):
    """One list entry -> (family, lo, hi), or None where ParseCIDR fails."""
    s = entry if "/" in entry else entry + "/32"
    addr, prefix = s.split("/", 1)
    if not (prefix.isascii() and prefix.isdigit()):
        return None
    try:
        a = ipaddress.ip_address(addr)
    except ValueError:
        return None
    bits = a.max_prefixlen
    p = int(prefix)
    if p > bits:
        return None
    host = (1 << (bits - p)) - 1
    lo = int(a) & ~host & TOP[a.version]
    hi = lo | host
    if a.version == 6 and lo >> 32 == 0xFFFF:  # network number in ::ffff:0:0/96 (so p >= 96)
        assert p >= 96
        return 4, lo & TOP[4], hi & TOP[4]
    return a.version, lo, hi


def ref_addr(s: str):
    """One lookup -> (family, value), or None where ParseIP fails."""
    try:
        a = ipaddress.ip_address(s)
    except ValueError:
        return None
    x = int(a)
    if a.version == 6 and x >> 32 == 0xFFFF:
        return 4, x & TOP[4]
    return a.version, x


def full_text(entry: str) -> str:
    return entry if "/" in entry else entry + "/32"


def parse_error(entry: str) -> str:
    return "could not parse list entry %s: invalid CIDR address: %s" % (entry, full_text(entry))


class RefList:
    """Entries must parse (first_error: the text of the first one that does not); overrides that
    do not parse are skipped and not counted."""

    def __init__(self, entries, overrides=()):
        self.entries, self.overrides = list(entries), list(overrides)
        self.e_ok = [ref_net(e) is not None for e in self.entries]
        self.o_ok = [ref_net(e) is not None for e in self.overrides]
        bad = [e for e, ok in zip(self.entries, self.e_ok) if not ok]
        self.first_error = parse_error(bad[0]) if bad else None
        nets = [ref_net(e) for e in self.entries + self.overrides]
        self.nets = {f: [(lo, hi) for n in nets if n is not None for (g, lo, hi) in [n] if g == f] for f in (4, 6)}
        self.n_entries = sum(self.e_ok) + sum(self.o_ok)
        self.tables = {f: merged(self.nets[f], TOP[f]) for f in (4, 6)}

    def found(self, lookups):
        out = []
        for s in lookups:
            a = ref_addr(s)
            if a is None:
                out.append(-1)
            else:
                f, x = a
                out.append(1 if any(lo <= x <= hi for lo, hi in self.nets[f]) else 0)
        return np.array(out, dtype=np.int8)


def merged(ranges, top):
    """Sorted ranges, merged where the next one overlaps or touches the current one."""
    out = []
    for lo, hi in sorted(ranges):
        if out and (lo <= out[-1][1] or (out[-1][1] != top and lo == out[-1][1] + 1)):
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


# ------------------------------------------------------------------ spellings
def quad(x: int) -> str:
    return "%d.%d.%d.%d" % (x >> 24, x >> 16 & 255, x >> 8 & 255, x & 255)


def spell4(x: int, rng) -> str:
    return quad(x) if rng.random() < 0.6 else ("::ffff:" if rng.random() < 0.8 else "::FFFF:") + quad(x)


def spell6(x: int, rng) -> str:
    """Compressed, exploded or upper-case.  (A value in ::ffff:0:0/96 comes out as a 4-in-6
    address, which the reference then reads as IPv4: the expected answer follows the string.)"""
    a = ipaddress.IPv6Address(x)
    r = rng.random()
    return str(a) if r < 0.7 else a.exploded if r < 0.85 else str(a).upper()


INVALID = ["", ".", ":", "1", "abc", "1.2.3", "1.2.3.4.5", "256.1.1.1", "1.2.3.4 ", " 1.2.3.4", "1..2.3", "1.2.3.",
           ".1.2.3", "1.2.3.4:80", "1.2.3.4/32", "-1.2.3.4", "1.2.3.+4", "a.b.c.d", "0x1.2.3.4", "::1::2", "12345::",
           "g::1", ":::", "1:2:3:4:5:6:7", "1:2:3:4:5:6:7:8:9", "1:2:3:4:5:6:7:8::", "::ffff:1.2.3", "::ffff:1.2.3.256",
           "2001:db8::1 ", "2001:db8::/32", "1.2.3.4\x00", "::1\x00", "1.2.3.4.", "255.255.255.2555", "99999999.1.1.1",
           "1:2:3:4:5:6:1.2.3.4.5", "::ffff:1.2.3.4:5"]


def invalid_string(rng, valid):
    if rng.random() < 0.6 or not valid:
        return INVALID[int(rng.integers(0, len(INVALID)))]
    return valid[int(rng.integers(0, len(valid)))] + [".", " ", "x", "/32", ":zz"][int(rng.integers(0, 5))]


# ------------------------------------------------------------------ lookups
def lookups_for(ref: RefList, rng, n_random=40, per_family=900):
    """The lookups of one list: lo - 1, lo, hi, hi + 1 of every expected interval (a sample of
    them where a table is long), address 0 and the top address of each family, IPv4 values as dotted
    quads and as ::ffff:a.b.c.d, IPv6 values that differ from an interval bound in one 64-bit word
    only, random addresses, and about 2 % invalid strings."""
    out = []
    for f in (4, 6):
        tab = ref.tables[f]
        if len(tab) * 4 > per_family:
            tab = [tab[i] for i in sorted(rng.choice(len(tab), per_family // 4, replace=False))]
        spell = spell4 if f == 4 else spell6
        vals = [0, TOP[f]]
        for lo, hi in tab:
            vals += [v for v in (lo - 1, lo, hi, hi + 1) if 0 <= v <= TOP[f]]
            if f == 6 and rng.random() < 0.5:
                b = lo if rng.random() < 0.5 else hi
                r = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
                # the low word changed / the high word changed, the other word the bound's own
                vals += [b ^ 1, b ^ (1 << 63), (b & ~LOW64) | r, b ^ (1 << 64), b ^ (1 << 127), (r << 64) | (b & LOW64)]
        out += [spell(v, rng) for v in vals]
        if f == 4 and vals:  # both spellings of some values
            out += [quad(v) for v in vals[:8]] + ["::ffff:" + quad(v) for v in vals[:8]]
    for _ in range(n_random):
        if rng.random() < 0.5:
            out.append(spell4(int(rng.integers(0, 1 << 32)), rng))
        else:
            out.append(spell6(int(rng.integers(0, 1 << 62)) << 66 | int(rng.integers(0, 1 << 62)), rng))
    for _ in range(max(1, len(out) // 45)):
        out.append(invalid_string(rng, out))
    order = rng.permutation(len(out))
    return [out[i] for i in order]


# ------------------------------------------------------------------ the fixed edge table
_WORDS = {"zero": 0, "ones": LOW64, "mixed": 0x123456789ABCDEF0}


def _word_nets(prefix):
    """One prefix on addresses whose high and low 64-bit words are 0, all ones and mixed."""
    return ["%s/%d" % (ipaddress.IPv6Address(h << 64 | lo), prefix) for h in _WORDS.values() for lo in _WORDS.values()]


EDGE_LISTS = {
    # very wide nets, in lists of their own
    "v4-all": ["0.0.0.0/0"],
    "v6-all": ["::/0"],
    "mapped-all": ["::ffff:0.0.0.0/96"],          # every IPv4 address
    "halves-high": ["128.0.0.0/1", "8000::/1"],
    "halves-low": ["::/1", "0.0.0.0/1"],
    "mapped-97": ["::ffff:1.2.3.4/97"],            # 0.0.0.0/1
    # IPv6 nets that cover the 4-in-6 range: no IPv4 or 4-in-6 lookup may match them
    "mapped-95": ["::ffff:1.2.3.4/95"],
    "mapped-90": ["::ffff:1.2.3.4/90"],
    "mapped-80": ["::ffff:1.2.3.4/80"],
    "mapped": ["::ffff:7.7.7.0/120", "::ffff:1.2.3.4/128", "::FFFF:9.9.9.9/127"],
    "v4-ends": ["255.255.255.255", "0.0.0.0/32"],
    "v4-top": ["255.255.255.255/32", "255.0.0.0/8"],
    "v4-nested": ["10.0.0.0/8", "10.1.0.0/16", "10.1.2.3"],
    "v4-adjacent": ["10.0.0.0/9", "10.128.0.0/9", "1.2.3.4/31", "1.2.3.6/31"],   # merge
    "v4-neighbours": ["1.2.3.0/31", "1.2.3.3/32"],                                # do not merge
    "v4-host-bits": ["10.9.8.7/8"],
    # nets starting exactly on a /16 boundary; one spanning four /16 blocks (30.4 .. 30.7) followed
    # by a block with no starts (30.8), then one starting inside 30.9; nets in block 65535
    "v4-blocks": ["20.5.0.0/16", "20.6.0.0/24", "20.7.0.0/32", "30.4.0.0/14", "30.9.128.0/17", "30.9.0.5",
                  "255.255.1.0/24", "255.255.255.254/31", "0.0.255.255", "0.1.0.0/32"],
    "v6-ends": ["::1", "ffff:ffff:ffff:ffff:ffff:ffff:ffff:ffff/128"],            # ::1 is ::/32
    "v6-halves-of-64": ["2001:db8:0:1::/65", "2001:db8:0:1:8000::/65", "fd00::/65", "fd00::8000:0:0:0/65"],                                 # merge
    "v6-doc": ["2001:db8::/32", "2001:DB8:ABCD:EF01::/64", "2001:0db9:0000:0000:0000:0000:0000:0001/128",
               "FE80::/10", "::2/127", "::4/127", "::8/128"],
    "p63": _word_nets(63), "p64": _word_nets(64), "p65": _word_nets(65), "p127": _word_nets(127),
    "p128": _word_nets(128),
    "both": ["10.0.0.0/8", "1.2.3.4", "255.255.255.0/24", "0.0.0.0/32", "2001:db8::/32", "::ffff:7.7.7.0/120",
             "fe80::/64", "::1/128", "ffff:ffff:ffff:ffff::/64"],
    "empty": [],
}

MALFORMED = ["1.2.3.4/33", "::1/129", "1.2.3/8", "1.2.3.4/", "/8",
             "1.2.3.4/8/9", "1.2.3.4/-1", "1.2.3.4/+8", "1.2.3.4/ 8", "1.2.3.4/8 ",
             "10.0.0.0/255.0.0.0", "2001:db8::/x", "1.2.3.4/0x8", "", "/",
             "1.2.3.4.5/8", "12345::/16", "::1::/8", "1.2.3.4/1000000000000"]

# Spellings Go 1.9 accepts and `ipaddress` does not (leading zeros), or that only the kernel treats
# specially (a quad whose first "." lies past byte 8 is classified from its first 8 bytes as "other").
# No expected value: the oracle, the host program and the GPU must agree.
GO_ONLY_ENTRIES = ["010.0.0.0/8", "1.2.3.004", "2001:db8::/032", "00001::/16"]
GO_ONLY_LOOKUPS = ["000000001.2.3.4", "01.2.3.4", "1.2.3.004", "010.1.1.1", "0000000010.1.1.1", "00001::", "1.2.3.4",
                   "10.255.255.255", "2001:0db8:0::00001", "000000000000001::", "1::", "::ffff:01.2.3.4", "11.0.0.0"]


# ------------------------------------------------------------------ the seeded generator
P4 = (0, 1, 8, 16, 17, 24, 31, 32)
P6 = (1, 32, 63, 64, 65, 95, 96, 97, 120, 127, 128)


def _special(bits, rng):
    r = rng.random()
    if r < 0.3:
        return 0
    if r < 0.6:
        return (1 << bits) - 1
    return 1 << int(rng.integers(0, bits))


def _rand(bits, rng):
    x = 0
    for _ in range(bits // 32):
        x = x << 32 | int(rng.integers(0, 1 << 32))
    return x


def gen_entry(rng, wide, p_special, family=None):
    """One entry: prefixes weighted towards P4 / P6, addresses towards 0, all ones and single-bit
    values.  wide=False leaves out the prefixes below 8 (IPv4) and below 32 (IPv6), which would
    swallow the rest of the list; they get lists of their own."""
    f = family or (4 if rng.random() < 0.55 else 6)
    bits = 32 if f == 4 else 128
    if rng.random() < 0.7:
        pool = P4 if f == 4 else P6
        if not wide:
            pool = [p for p in pool if p >= (9 if f == 4 else 33)]
        p = int(pool[int(rng.integers(0, len(pool)))])
    else:
        p = int(rng.integers(0 if wide else (9 if f == 4 else 33), bits + 1))
    x = _special(bits, rng) if rng.random() < p_special else _rand(bits, rng)
    if f == 6 and rng.random() < 0.15:  # a 4-in-6 address
        x = 0xFFFF << 32 | (x & TOP[4])
        if not wide and 96 <= p < 105:  # (an IPv4 net of prefix p - 96: as wide as an IPv4 /0 .. /8)
            p = 96 + int((16, 17, 24, 31, 32)[int(rng.integers(0, 5))])
    r = rng.random()
    if f == 4:
        text = quad(x)
    else:
        a = ipaddress.IPv6Address(x)
        text = str(a) if r < 0.7 else a.exploded if r < 0.85 else str(a).upper()
    if p == 32 and rng.random() < 0.5:
        return text  # no slash: "/32" is appended, for IPv6 too
    return "%s/%d" % (text, p)


class Case:
    def __init__(self, name, entries, overrides, rng, n_random=40):
        self.name, self.entries, self.overrides = name, entries, overrides
        self.ref = RefList(entries, overrides)
        assert self.ref.first_error is None, (name, self.ref.first_error)
        self.lookups = lookups_for(self.ref, rng, n_random)
        self.want = self.ref.found(self.lookups)


@functools.lru_cache(maxsize=None)
def cases():
    """Every list of the module with its lookups and the reference's answers, computed once."""
    rng = np.random.default_rng(20)
    out = [Case("edge-" + k, v, [], rng) for k, v in EDGE_LISTS.items()]
    # (overrides: counted when they parse, skipped when they do not)
    out.append(Case("edge-overrides", ["10.0.0.0/8"], ["11.11.11.11", "bad-override", "2001:db8::/32"] + MALFORMED, rng))
    for size, count in ((1, 30), (3, 30), (40, 30)):
        for k in range(count):
            wide = k % 6 == 5  # the very wide nets in lists of their own
            entries = [gen_entry(rng, wide, 0.5) for _ in range(size)]
            over = [gen_entry(rng, wide, 0.5) for _ in range(k % 3)]
            out.append(Case("gen-%d-%d%s" % (size, k, "-wide" if wide else ""), entries, over, rng))
    out.append(Case("gen-1000", [gen_entry(rng, False, 0.05) for _ in range(1000)], [], rng, 200))
    out.append(Case("gen-1000-v4", [gen_entry(rng, False, 0.15, 4) for _ in range(1000)], [], rng, 200))
    out.append(Case("gen-1000-v6", [gen_entry(rng, False, 0.15, 6) for _ in range(1000)], [], rng, 200))
    return out


def case_ids():
    return [c.name for c in cases()]


# ------------------------------------------------------------------ the restatements under test
def build_host_program(outdir) -> str:
    """tests/cidr_host.cpp with the host compiler, ASan + UBSan, the sanitizer runtimes linked
    statically (test_rfc3339_independent.build_host_program says why)."""
    exe = os.path.join(str(outdir), "cidr_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-I", os.path.join(ROOT, "istio_amd", "csrc"), os.path.join(HERE, "cidr_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "building the sanitized host program failed (it needs g++ with its static " \
                              "libasan / libubsan):\n" + r.stderr[-3000:]
    return exe


def host_run(exe, lists):
    """The host program on [(entries, overrides, lookups)] -> one dict per list: e_ok, o_ok, n, t4,
    t6, dir (all 65,537 values), found.  It must end with status 0 and an empty stderr (no
    sanitizer report)."""
    hx = lambda s: s.encode("utf-8", "surrogateescape").hex()  # noqa: E731
    text = []
    for entries, overrides, lookups in lists:
        text += ["e" + hx(s) for s in entries] + ["o" + hx(s) for s in overrides] + ["l" + hx(s) for s in lookups]
        text.append("=")
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    out, cur = [], None
    for ln in r.stdout.splitlines():
        if cur is None:
            cur = {"e_ok": [], "o_ok": [], "n": None, "t4": [], "t6": [], "runs": [], "found": []}
        tok = ln.split()
        if tok[0] == "E":
            cur["e_ok"].append(tok[1] == "1")
        elif tok[0] == "O":
            cur["o_ok"].append(tok[1] == "1")
        elif tok[0] == "N":
            cur["n"] = int(tok[1])
        elif tok[0] == "4":
            cur["t4"].append((int(tok[1]), int(tok[2])))
        elif tok[0] == "6":
            cur["t6"].append((int(tok[1], 16), int(tok[2], 16)))
        elif tok[0] == "D":
            cur["runs"].append((int(tok[1]), int(tok[2])))  # ("D size n" fails here: a wrong table size)
        elif tok[0] == "L":
            cur["found"].append(int(tok[1]))
        else:
            assert ln == "=", ln
            ks = [k for k, _ in cur["runs"]]
            assert ks and ks[0] == 0 and ks == sorted(set(ks)) and ks[-1] <= 65536, ks[:5]
            d = np.zeros(65537, dtype=np.int64)
            for (k, v), k1 in zip(cur["runs"], ks[1:] + [65537]):
                d[k:k1] = v
            cur["dir"] = d
            out.append(cur)
            cur = None
    assert cur is None and len(out) == len(lists)
    return out


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return build_host_program(tmp_path_factory.mktemp("cidr_host"))


@pytest.fixture(scope="module")
def host_out(host_exe):
    return host_run(host_exe, [(c.entries, c.overrides, c.lookups) for c in cases()])


# ------------------------------------------------------------------ tests
def test_reference_known_answers():
    """The reference against hand-worked rows (Go's documented behaviour, ip.go / ipList.go)."""
    assert ref_net("::1") == (6, 0, (1 << 96) - 1)                       # "::1/32" = ::/32
    assert ref_net("255.255.255.255") == (4, TOP[4], TOP[4])
    assert ref_net("10.9.8.7/8") == (4, 10 << 24, (10 << 24) + (1 << 24) - 1)
    assert ref_net("::ffff:7.7.7.0/120") == (4, 0x07070700, 0x070707FF)
    assert ref_net("::ffff:1.2.3.4/97") == (4, 0, (1 << 31) - 1)
    assert ref_net("::ffff:0.0.0.0/96") == (4, 0, TOP[4])
    assert ref_net("::ffff:1.2.3.4/95") == (6, 0xFFFE << 32, (0xFFFF << 32) + TOP[4])
    assert ref_net("::ffff:1.2.3.4/80") == (6, 0, (1 << 48) - 1)
    assert ref_net("0.0.0.0/0") == (4, 0, TOP[4]) and ref_net("::/0") == (6, 0, TOP[6])
    assert ref_net("2001:db8::/32") == (6, 0x20010DB8 << 96, (0x20010DB9 << 96) - 1)
    assert all(ref_net(e) is None for e in MALFORMED)
    assert ref_addr("::ffff:1.2.3.4") == (4, 0x01020304) == ref_addr("1.2.3.4")
    assert ref_addr("::fffe:1.2.3.4") == (6, (0xFFFE << 32) + 0x01020304)
    assert all(ref_addr(s) is None for s in INVALID)
    assert merged([(5, 9), (0, 3), (4, 4), (11, 12)], 12) == [(0, 9), (11, 12)]
    assert merged([(0, TOP[4]), (TOP[4], TOP[4])], TOP[4]) == [(0, TOP[4])]
    wide = RefList(["::/0"])
    assert list(wide.found(["::ffff:1.2.3.4", "1.2.3.4", "::1", "x"])) == [0, 0, 1, -1]
    for name in ("mapped-95", "mapped-90", "mapped-80"):  # IPv6 nets over the 4-in-6 range
        r = RefList(EDGE_LISTS[name])
        assert r.tables[4] == [] and list(r.found(["::ffff:1.2.3.4", "1.2.3.4", "::fffe:1.2.3.4"]))[:2] == [0, 0]
    r = RefList(EDGE_LISTS["v4-adjacent"])
    assert r.tables[4] == [(0x01020304, 0x01020307), (10 << 24, (11 << 24) - 1)]
    r = RefList(EDGE_LISTS["v4-neighbours"])
    assert r.tables[4] == [(0x01020300, 0x01020301), (0x01020303, 0x01020303)]
    r = RefList(EDGE_LISTS["v6-halves-of-64"])
    assert len(r.tables[6]) == 2 and all(hi - lo == LOW64 for lo, hi in r.tables[6])


def test_inputs_do_not_degenerate():
    """The outcome shares of the module's lookups, from the reference alone: found and not found
    each at least 25 % of the valid lookups, per family and overall; invalid at least 1 %; and the
    table shapes the searches must meet."""
    cs = cases()
    fam = {4: [0, 0], 6: [0, 0]}
    invalid = total = 0
    for c in cs:
        for s, w in zip(c.lookups, c.want):
            total += 1
            if w < 0:
                invalid += 1
            else:
                fam[ref_addr(s)[0]][int(w)] += 1
    print("lookups %d, invalid %d, IPv4 not found / found %s, IPv6 %s" % (total, invalid, fam[4], fam[6]))
    assert total > 10000 and invalid * 100 >= total
    for f in (4, 6):
        miss, hit = fam[f]
        assert hit * 4 >= hit + miss and miss * 4 >= hit + miss, (f, fam[f])
    hit, miss = fam[4][1] + fam[6][1], fam[4][0] + fam[6][0]
    assert hit * 4 >= hit + miss and miss * 4 >= hit + miss
    n4 = [len(c.ref.tables[4]) for c in cs]
    n6 = [len(c.ref.tables[6]) for c in cs]
    assert any(a == 0 and b > 0 for a, b in zip(n4, n6)) and any(b == 0 and a > 0 for a, b in zip(n4, n6))
    assert any(a + b == 1 for a, b in zip(n4, n6))
    assert any(a > 256 and b > 256 for a, b in zip(n4, n6)), (max(n4), max(n6))
    assert max(n4) > 256 and max(n6) > 256
    # merging happened, and nets that only touch were told from nets that leave a gap
    assert any(len(c.ref.tables[f]) < len(set(c.ref.nets[f])) for c in cs for f in (4, 6))
    assert sum(c.ref.n_entries for c in cs) > 4000
    assert sum(len(c.lookups) for c in cs) / len(cs) < 4000 and max(len(c.lookups) for c in cs) < 6000


def test_oracle_iplist_agrees_with_reference():
    """Assertion 1: the oracle's IPList answers every lookup as the reference does, counts the same
    entries, and raises -- with the full message -- on exactly the malformed entries."""
    import lists as L
    for c in cases():
        o = L.IPList(c.entries, c.overrides)
        assert o.num_entries() == c.ref.n_entries, c.name
        got = o.found(c.lookups, threads=4)
        bad = np.nonzero(got != c.want)[0]
        assert bad.size == 0, (c.name, [(c.lookups[i], int(got[i]), int(c.want[i])) for i in bad[:8]])
    for e in MALFORMED:
        assert RefList(["10.0.0.0/8", e]).first_error == parse_error(e)
        with pytest.raises(L.ListParseError) as ei:
            L.IPList(["10.0.0.0/8", e, "11.0.0.0/8"])
        assert str(ei.value) == parse_error(e), e
        o = L.IPList(["10.0.0.0/8"], [e, "11.0.0.0/8"])  # the same entry as an override: skipped, not counted
        assert o.num_entries() == 2 and list(o.found(["10.1.1.1", "11.1.1.1", "12.1.1.1"])) == [1, 1, 0]


def test_host_entry_status_and_count(host_exe, host_out):
    """Assertion 2: per entry parsed / refused, and numEntries."""
    for c, h in zip(cases(), host_out):
        assert h["e_ok"] == c.ref.e_ok and h["o_ok"] == c.ref.o_ok and h["n"] == c.ref.n_entries, c.name
    h = host_run(host_exe, [(MALFORMED + ["10.0.0.0/8"], MALFORMED + ["::1"], [])])[0]
    assert h["e_ok"] == [False] * len(MALFORMED) + [True] and h["o_ok"] == [False] * len(MALFORMED) + [True]
    assert h["n"] == 2 and h["t4"] == [(10 << 24, (11 << 24) - 1)] and h["t6"] == [(0, (1 << 96) - 1)]


def test_host_tables_equal_merged_reference(host_out):
    """Assertion 3: the product's IPv4 and IPv6 tables are the reference's merged intervals exactly
    (count, every lo, every hi), sorted, no two overlapping or touching."""
    for c, h in zip(cases(), host_out):
        for key, f in (("t4", 4), ("t6", 6)):
            tab = h[key]
            assert tab == c.ref.tables[f], (c.name, f, len(tab), len(c.ref.tables[f]))
            assert all(lo <= hi for lo, hi in tab)
            assert all(b[0] > a[1] + 1 for a, b in zip(tab, tab[1:])), (c.name, f)


def test_host_directory(host_out):
    """Assertion 4: the /16 directory is non-decreasing, dir[0] == 0, dir[65536] == n4, and dir[k]
    is the number of reference intervals that start below k << 16, at every k."""
    ks = np.arange(65537, dtype=np.uint64) << np.uint64(16)
    for c, h in zip(cases(), host_out):
        d = h["dir"]
        los = np.array([lo for lo, _ in c.ref.tables[4]], dtype=np.uint64)
        assert d.shape == (65537,) and d[0] == 0 and d[65536] == len(los) and (np.diff(d) >= 0).all(), c.name
        want = np.searchsorted(los, ks, side="left")
        bad = np.nonzero(d != want)[0]
        assert bad.size == 0, (c.name, [(int(k), int(d[k]), int(want[k])) for k in bad[:5]])
    blocks = next(c for c in cases() if c.name == "edge-v4-blocks")
    los = [lo for lo, _ in blocks.ref.tables[4]]
    k = (30 << 8) + 4  # 30.4.0.0/14 spans blocks 30.4 .. 30.7; block 30.8 has no starts
    d = next(h for c, h in zip(cases(), host_out) if c is blocks)["dir"]
    assert d[k + 1] == d[k] + 1 and d[k + 1] == d[k + 2] == d[k + 5] and d[k + 6] == d[k + 5] + 2
    assert d[65535] == len(los) - 2 and d[65536] == len(los)


def test_host_lookups_agree_with_reference(host_out):
    """Assertion 5 (and 6: host_run asserts exit status 0 and an empty stderr): mxpnet::parse_ip and
    a plain scan of the product's tables answer every lookup as the reference does."""
    for c, h in zip(cases(), host_out):
        got = np.array(h["found"], dtype=np.int8)
        assert got.shape == c.want.shape
        bad = np.nonzero(got != c.want)[0]
        assert bad.size == 0, (c.name, [(c.lookups[i], int(got[i]), int(c.want[i])) for i in bad[:8]])


def test_go_only_spellings_oracle_equals_host(host_exe):
    """No expected value: leading zeros, where Go 1.9 and `ipaddress` differ.  The oracle and the
    product's host half must agree on which entries parse and on every lookup."""
    import lists as L
    base = ["10.0.0.0/8", "1.2.3.4", "2001:db8::/32", "1::/16"]
    h = host_run(host_exe, [(base + GO_ONLY_ENTRIES, [], GO_ONLY_LOOKUPS)])[0]
    ok = []
    for e in GO_ONLY_ENTRIES:
        try:
            L.IPList([e])
            ok.append(True)
        except L.ListParseError:
            ok.append(False)
    assert h["e_ok"] == [True] * len(base) + ok
    o = L.IPList(base, [e for e, k in zip(GO_ONLY_ENTRIES, ok) if k])
    assert h["found"] == list(o.found(GO_ONLY_LOOKUPS, threads=1)), list(zip(GO_ONLY_LOOKUPS, h["found"]))
