"""time.Parse(time.RFC3339, s) against an independent reference (what test_ip_vs_python_ipaddress.py
does for net.ParseIP).  The oracle's oracle_parse_rfc3339 (oracle/goval.c) and the product's
mxptime::parse_rfc3339 (istio_amd/csrc/timeparse.h) are near copies of one reading of Go's
format.go, so their parity says little about either.  The reference here shares nothing with them:
a strict RFC3339 regular expression, calendar validity, and a day number counted from 0001-01-01 by
whole years and months (no days-from-civil era formula), itself checked against `datetime.date`.

The strings are built forward from field tuples, so the expected instant of a well-formed string
comes from its fields, not from any parse; about 35 % are then mutated into malformed ones.  The
generator emits none of the spellings where Go 1.9 and strict RFC3339 differ; those are GO_ONLY
below, where the only assertion is agreement of the restatements with each other (no expected
value: corroboration, not pinning).

CPU: the oracle through ctypes, and the product's definition as a stand-alone host program
(tests/extern_parse_host.cpp) built with AddressSanitizer and UBSan, each string in an exact-size
heap buffer.  GPU: tests/test_gpu_extern_values.py imports the generators."""
import ctypes
import datetime
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from test_ip_vs_python_ipaddress import _py_parse, _strings  # noqa: E402

# ------------------------------------------------------------------ the reference
_DIM = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)
_RX = re.compile(r"(\d{4})-(\d\d)-(\d\d)T(\d\d):(\d\d):(\d\d)(?:\.(\d{1,9}))?(Z|[+-]\d\d:\d\d)", re.ASCII)


def is_leap(y: int) -> bool:
    return y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)


def days_in_month(y: int, m: int) -> int:
    return 29 if m == 2 and is_leap(y) else _DIM[m - 1]


def day_number(y: int, m: int, d: int) -> int:
    """Days from 0001-01-01 (day 0) to y-m-d, proleptic Gregorian, y in 0..9999: the whole years
    before y, the whole months before m, the days before d."""
    if y >= 1:
        q = y - 1  # whole years 1..y-1, of which q//4 - q//100 + q//400 are leap
        days = 365 * q + q // 4 - q // 100 + q // 400
    else:
        days = -366  # year 0000 is a leap year and lies wholly before day 0
    for k in range(1, m):
        days += days_in_month(y, k)
    return days + d - 1


_EPOCH = day_number(1970, 1, 1)


def instant(y, mo, d, h, mi, s, frac, zone):
    """Field tuple -> (Unix seconds, nanoseconds), or None when the fields are out of range.
    frac: the fraction's digits ("" or None: none); zone: None (Z) or (sign, hh, mm)."""
    if not (1 <= mo <= 12 and 1 <= d <= days_in_month(y, mo) and h < 24 and mi < 60 and s < 60):
        return None
    off = 0
    if zone is not None:
        sign, zh, zm = zone
        if zh >= 24 or zm >= 60:
            return None
        off = (zh * 60 + zm) * 60 * (-1 if sign == "-" else 1)
    sec = (day_number(y, mo, d) - _EPOCH) * 86400 + h * 3600 + mi * 60 + s - off
    return sec, (int(frac.ljust(9, "0")) if frac else 0)


def ref(s: str):
    """Strict RFC3339 -> (sec, nsec) | None.  Python integers only."""
    m = _RX.fullmatch(s)
    if not m:
        return None
    y, mo, d, h, mi, sec = (int(m.group(k)) for k in range(1, 7))
    z = m.group(8)
    zone = None if z == "Z" else (z[0], int(z[1:3]), int(z[4:6]))
    return instant(y, mo, d, h, mi, sec, m.group(7), zone)


# ------------------------------------------------------------------ the generator
YEARS = (0, 1, 1600, 1900, 1969, 1970, 1972, 2000, 2016, 2038, 2100, 2400, 9999)
ZONE_MINUTES = (0, 15, 30, 45, 59)


def spell(y, mo, d, h, mi, s, frac, zone) -> str:
    out = "%04d-%02d-%02dT%02d:%02d:%02d" % (y, mo, d, h, mi, s)
    if frac:
        out += "." + frac
    return out + ("Z" if zone is None else "%s%02d:%02d" % zone)


def gen_fields(rng):
    """One well-formed field tuple (its day may still miss the month: Feb 29 of a common year)."""
    y = int(YEARS[int(rng.integers(0, len(YEARS)))]) if rng.random() < 0.5 else int(rng.integers(0, 10000))
    if rng.random() < 0.2:  # the end of February, whatever the year
        mo, d = 2, int(rng.integers(27, 30))
    else:
        mo = int(rng.integers(1, 13))
        d = int(rng.integers(1, days_in_month(y, mo) + 1))
    h, mi, s = int(rng.integers(0, 24)), int(rng.integers(0, 60)), int(rng.integers(0, 60))
    frac = None
    if rng.random() < 0.5:
        k = int(rng.integers(1, 10))
        frac = "".join(str(int(x)) for x in rng.integers(0, 10, k))
    zone = None
    if rng.random() >= 0.4:
        zone = ("+" if rng.random() < 0.5 else "-", int(rng.integers(0, 24)),
                int(ZONE_MINUTES[int(rng.integers(0, len(ZONE_MINUTES)))]))
    return y, mo, d, h, mi, s, frac, zone


def mutate(rng, f) -> str:
    """A malformed spelling of field tuple f (every variant is outside the grammar or the ranges)."""
    y, mo, d, h, mi, s, frac, zone = f
    good = spell(*f)
    kinds = ["drop_last", "T_space", "T_lower", "month13", "day32", "feb30", "hour24", "minute60", "second60",
             "trail_space", "lead_space", "dot_nodigit", "comma_frac", "drop_dash", "x_byte"]
    kinds.append("Z_lower" if zone is None else "zone_nocolon")
    k = kinds[int(rng.integers(0, len(kinds)))]
    if k == "drop_last":
        return good[:-1]
    if k == "T_space":
        return good.replace("T", " ", 1)
    if k == "T_lower":
        return good.replace("T", "t", 1)
    if k == "Z_lower":
        return good[:-1] + "z"
    if k == "zone_nocolon":
        return good[:-3] + good[-2:]
    if k == "month13":
        return spell(y, 13, d, h, mi, s, frac, zone)
    if k == "day32":
        return spell(y, mo, 32, h, mi, s, frac, zone)
    if k == "feb30":
        return spell(y, 2, 30, h, mi, s, frac, zone)
    if k == "hour24":
        return spell(y, mo, d, 24, mi, s, frac, zone)
    if k == "minute60":
        return spell(y, mo, d, h, 60, s, frac, zone)
    if k == "second60":
        return spell(y, mo, d, h, mi, 60, frac, zone)
    if k == "trail_space":
        return good + " "
    if k == "lead_space":
        return " " + good
    tail = "Z" if zone is None else "%s%02d:%02d" % zone
    head = spell(y, mo, d, h, mi, s, None, None)[:-1]
    if k == "dot_nodigit":
        return head + "." + tail
    if k == "comma_frac":
        return head + ",5" + tail
    if k == "drop_dash":
        i = 4 if rng.random() < 0.5 else 7
        return good[:i] + good[i + 1:]
    i = int(rng.integers(0, len(good)))
    return good[:i] + "x" + good[i + 1:]


def cases(seed=5, n=24000):
    """[(string, (sec, nsec) | None)]: the expected instant from the fields alone."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        f = gen_fields(rng)
        if rng.random() < 0.35:
            out.append((mutate(rng, f), None))
        else:
            out.append((spell(*f), instant(*f)))
    return out


TRUNCATED = ["", "2", "2015", "2015-", "2015-01-02T15:04:35", "2015-01-02T15:04:35.", "2015-01-02T15:04:35+01",
             "2015-01-02T15:04:35+01:0", "1.2.3.", ":", "::ffff:1.2.3", "1:2:3:4:5:6:7:"]

# Spellings Go 1.9's time.Parse accepts and strict RFC3339 does not, or where two readings of
# format.go could differ.  No expected value: the restatements must agree with each other.
GO_ONLY = [
    "2015-01-02T5:04:05Z", "2015-01-02T5:04:05+01:00", "2015-01-02T5:04:05.5Z",      # one-digit hour
    "2015-01-00T15:04:05Z", "2015-02-00T15:04:05+01:00", "0000-01-00T00:00:00Z",      # day 00
    "2015-01-02T15:04:05+99:99", "2015-01-02T15:04:05-99:99", "2015-01-02T15:04:05+24:00",
    "2015-01-02T15:04:05+00:60",                                                        # zone out of range
    "2015-01-02T15:04:05+-1:+5", "2015-01-02T15:04:05--1:-5", "2015-01-02T15:04:05++1:+5",
    "2015-01-02T15:04:05+ 1: 5",                                                        # signed zone digits
    "2015-01-02T15:04:05.0000000001Z", "2015-01-02T15:04:05.1234567891Z", "2015-01-02T15:04:05.0000000000Z",
    "2015-01-02T15:04:05.0000000001+01:00", "2015-01-02T15:04:05.9999999999999999999Z",
    "2015-01-02T15:04:05.99999999999999999999Z",                                        # >= 10 fraction digits
    "0000-01-01T00:00:00Z", "0000-02-29T23:59:59.999999999Z", "0000-12-31T23:59:59-23:59",
    "0000-01-01T00:00:00+23:59",                                                        # year 0000
]


# ------------------------------------------------------------------ the restatements under test
def oracle_parse(strs):
    """oracle_parse_rfc3339 on every string -> [(sec, nsec) | None]."""
    import oracle
    L = oracle.lib()
    L.oracle_parse_rfc3339.restype = ctypes.c_int
    L.oracle_parse_rfc3339.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int64),
                                       ctypes.POINTER(ctypes.c_int32)]
    out = []
    sec, ns = ctypes.c_int64(), ctypes.c_int32()
    for s in strs:
        b = s.encode()
        ok = L.oracle_parse_rfc3339(b, len(b), ctypes.byref(sec), ctypes.byref(ns))
        out.append((sec.value, ns.value) if ok else None)
    return out


def build_host_program(outdir) -> str:
    """tests/extern_parse_host.cpp with the host compiler, ASan + UBSan.  The sanitizer runtimes are
    linked statically (g++'s libasan.a / libubsan.a): with the shared runtime ASan refuses to start
    unless it comes first among the loaded libraries, which any unrelated library that the
    environment preloads into every process would break; linked in, the program needs nothing from
    its environment."""
    exe = os.path.join(str(outdir), "extern_parse_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-I", os.path.join(ROOT, "istio_amd", "csrc"), os.path.join(HERE, "extern_parse_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "building the sanitized host program failed (it needs g++ with its static " \
                              "libasan / libubsan):\n" + r.stderr[-3000:]
    return exe


def host_parse(exe, strs):
    """The host program on every string -> ([(sec, nsec) | None], [16 bytes | None]); it must end
    with status 0 and an empty stderr (no sanitizer report)."""
    text = "".join(s.encode().hex() + "\n" for s in strs)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(strs)
    ts, ips = [], []
    for ln in lines:
        tok, sec, ns, iok, hx = ln.split()
        ts.append((int(sec), int(ns)) if tok == "1" else None)
        ips.append(bytes.fromhex(hx) if iok == "1" else None)
    return ts, ips


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return build_host_program(tmp_path_factory.mktemp("extern_parse_host"))


@pytest.fixture(scope="module")
def seeded():
    return cases()


# ------------------------------------------------------------------ tests
def test_day_number_against_datetime():
    for y, m, d in [(1, 1, 1), (1969, 12, 31), (1970, 1, 1), (2000, 2, 29), (9999, 12, 31), (1600, 3, 1),
                    (1900, 3, 1), (2100, 2, 28), (2400, 12, 31)]:
        assert day_number(y, m, d) == (datetime.date(y, m, d) - datetime.date(1, 1, 1)).days, (y, m, d)
    assert day_number(0, 12, 31) == -1 and day_number(0, 1, 1) == -366 and day_number(0, 3, 1) == -306
    assert ref("1970-01-01T00:00:00Z") == (0, 0)
    assert ref("1969-12-31T23:59:59.000000001Z") == (-1, 1)
    tz = datetime.timezone(datetime.timedelta(minutes=90))
    assert ref("2015-01-02T15:04:35+01:30") == (int(datetime.datetime(2015, 1, 2, 15, 4, 35, tzinfo=tz).timestamp()), 0)
    assert ref("2015-01-02T15:04:35Z") == (1420211075, 0)


def test_reference_parses_what_the_fields_say(seeded):
    """The two halves of the reference: ref() of a string built from fields is those fields' instant."""
    for s, want in seeded:
        assert ref(s) == want, s
    assert all(ref(s) is None for s in TRUNCATED)


def test_oracle_rfc3339_agrees_with_reference(seeded):
    strs = [s for s, _ in seeded]
    assert len(strs) >= 20000
    got = oracle_parse(strs)
    bad = [(s, g, w) for (s, w), g in zip(seeded, got) if g != w]
    assert not bad, bad[:8]
    valid = sum(w is not None for _, w in seeded)
    assert valid >= len(strs) // 2 and len(strs) - valid >= len(strs) // 4, (valid, len(strs))
    assert sum(w is not None and w[1] != 0 for _, w in seeded) > 5000  # (non-zero nanoseconds)
    assert sum(w is not None and w[0] < 0 for _, w in seeded) > 3000   # (before 1970)
    assert oracle_parse(TRUNCATED) == [None] * len(TRUNCATED)


def test_product_definition_agrees_with_references_under_sanitizers(host_exe, seeded):
    """timeparse.h / netparse.h as compiled for the host, ASan + UBSan, exact-size buffers: the same
    instants as the reference, the same addresses as `ipaddress`, and no sanitizer report."""
    ip_strs = _strings()
    strs = [s for s, _ in seeded] + TRUNCATED + ip_strs
    ts, ips = host_parse(host_exe, strs)
    bad = [(s, g, w) for (s, w), g in zip(seeded, ts) if g != w]
    assert not bad, bad[:8]
    k = len(seeded)
    assert ts[k:k + len(TRUNCATED)] == [None] * len(TRUNCATED)
    assert ips[k:k + len(TRUNCATED)] == [None] * len(TRUNCATED)
    assert [_py_parse(s) for s in TRUNCATED] == [None] * len(TRUNCATED)
    k += len(TRUNCATED)
    want = [_py_parse(s) for s in ip_strs]
    bad = [(s, g, w) for s, g, w in zip(ip_strs, ips[k:], want) if g != w]
    assert not bad, bad[:8]
    assert sum(w is not None for w in want) > 2000 and sum(w is None for w in want) > 500


def test_go_only_forms_oracle_equals_product_definition(host_exe):
    """No expected value (the Go source is not at hand): the two restatements agree."""
    ts, _ = host_parse(host_exe, GO_ONLY)
    assert ts == oracle_parse(GO_ONLY), list(zip(GO_ONLY, ts, oracle_parse(GO_ONLY)))
