"""The values ip() and timestamp() make from per-request strings, and the TIMESTAMP / IP_ADDRESS
attributes they meet, on the GPU: mxp_pack_parse_kernel (timeparse.h / netparse.h on the device),
the MXP_IK_TIME / MXP_IK_RAW / MXP_IK_CANON passes of mxp_pack_intern_kernel (rule-set pool table,
then a batch table that the batch's own values and the parsed ones share), the pre-tables, and
VM_TSEQ / VM_IPEQ.

Expected codes come from independent references alone: tests/test_rfc3339_independent.py's strict
RFC3339 reference for instants, Python's `ipaddress` for addresses, and a restatement of
net.IP.Equal.  A pair is an error when either side is absent or does not parse.  The oracle is
checked against the same codes (on the CPU too) and is the authority for the error texts.

Every batch goes through the device packer, the host packer (MXP_HOST_PACK=1) and the narrow upload;
the three must give the same bitmaps and the expected codes, the two packers the same sampled error
texts.  An uploaded batch evaluated into device bitmaps records no errors, so the narrow upload's
texts are read through Resolve (test_narrow_upload_error_texts).  The batches hold
thousands of distinct instants and addresses (probe chains in tables sized 2x their items), instants
spelled in two zones or with two fractions, +1 ns / +-1 s / +2^32 s neighbours, pre-1970 seconds with
nanoseconds, and byte strings of lengths 0, 3, 4, 5, 15 and 16.

Two tests here need no GPU and are not marked `gpu` (test_batches_hold_what_they_claim,
test_oracle_gives_the_expected_codes): they check the generators and the oracle on the same batches."""
import datetime
import ipaddress

import numpy as np
import pytest

import oracle
import test_rfc3339_independent as T
from istio_amd.bags import BagBatch, GoTime, NarrowBatch
from test_ip_vs_python_ipaddress import _py_parse, _strings

MANIFEST = {"s1": "STRING", "s2": "STRING", "t": "TIMESTAMP", "a": "IP_ADDRESS", "b": "IP_ADDRESS"}
ERR = "error"  # (a side that is absent or does not parse)
V4 = b"\0" * 10 + b"\xff\xff"

# ------------------------------------------------------------------ instants
_DAY0 = datetime.datetime(1, 1, 1)
_SEC0 = (datetime.datetime(1970, 1, 1) - _DAY0).days * 86400  # 0001-01-01 .. 1970-01-01


def frac_digits(rng, nsec: int):
    """One of the fraction spellings of nsec: shortest, zero-padded to a random width, full."""
    short = ("%09d" % nsec).rstrip("0")
    k = int(rng.integers(0, 3))
    if k == 0:
        return short or None
    if k == 1:
        return short.ljust(int(rng.integers(max(len(short), 1), 10)), "0")
    return "%09d" % nsec


def spell_instant(rng, sec: int, nsec: int):
    """(sec, nsec) spelled in a random zone with a random fraction spelling, the local fields from
    `datetime` arithmetic; None when they leave years 1..9999."""
    zone = None
    off = 0
    if rng.random() < 0.7:
        zone = ("+" if rng.random() < 0.5 else "-", int(rng.integers(0, 24)),
                int(T.ZONE_MINUTES[int(rng.integers(0, len(T.ZONE_MINUTES)))]))
        off = (zone[1] * 60 + zone[2]) * 60 * (-1 if zone[0] == "-" else 1)
    try:
        dt = _DAY0 + datetime.timedelta(seconds=sec + off + _SEC0)
    except OverflowError:
        return None
    return T.spell(dt.year, dt.month, dt.day, dt.hour, dt.minute, dt.second, frac_digits(rng, nsec), zone)


def respell(rng, f, inst):
    """Another spelling of the instant of field tuple f: another zone, or (outside datetime's years)
    the same fields with another fraction spelling."""
    s = spell_instant(rng, *inst)
    return s if s is not None else T.spell(*f[:6], frac_digits(rng, inst[1]), f[7])


def const_instants():
    """The instants of the rules' constants: the epoch (an all-zero key), a pre-1970 second with
    nanoseconds, the reference's known answer, the first nanosecond of a leap day."""
    return [(0, 0), (-86400 * 365 - 1, 999999999), (1420211075, 0), (T.ref("2000-02-29T00:00:00Z")[0], 1)]


def _pick(rng, xs):
    return xs[int(rng.integers(0, len(xs)))]


def random_time(rng):
    """Anywhere in years 0..9999, mostly with nanoseconds."""
    return GoTime(int(rng.integers(-62167219200, 253402300800)), int(rng.integers(0, 10**9)) if rng.random() < 0.7 else 0)


def ts_row(rng, valid_strings, attrs):
    """(s1, s2, t) of a request that carries a timestamp pair: None is an absent attribute."""
    K = const_instants()
    r = rng.random()
    f = T.gen_fields(rng)
    if not valid_strings:
        s1, i1 = T.mutate(rng, f), None
    elif r < 0.40:  # an instant some rule's constant has
        i1 = _pick(rng, K)
        s1 = spell_instant(rng, *i1)
        f = None
    elif r < 0.43:
        s1, i1 = None, None
    elif r < 0.53:
        s1, i1 = T.mutate(rng, f), None
    else:
        s1, i1 = T.spell(*f), T.instant(*f)
    r = rng.random()
    g = T.gen_fields(rng)
    s2 = None
    if not valid_strings:
        s2 = T.mutate(rng, g) if r < 0.9 else None
    elif i1 is not None and r < 0.40:  # the same instant in another zone or with another fraction
        s2 = respell(rng, f, i1) if f is not None else spell_instant(rng, *i1)
    elif i1 is not None and r < 0.50:
        s2 = spell_instant(rng, i1[0] + (i1[1] + 1) // 10**9, (i1[1] + 1) % 10**9)
    elif i1 is not None and r < 0.60:
        s2 = spell_instant(rng, i1[0] + (1 if rng.random() < 0.5 else -1), i1[1])
    elif i1 is not None and r < 0.62:
        s2 = spell_instant(rng, i1[0] + (1 << 32), i1[1])
    elif r < 0.85:
        s2 = T.spell(*g)
    elif r < 0.97:
        s2 = T.mutate(rng, g)
    if valid_strings and s2 is None and r < 0.62:  # (a neighbour outside datetime's years)
        s2 = T.spell(*g)
    r = rng.random()
    if not attrs or r < 0.05:
        t = None
    elif r < 0.40 and i1 is not None:
        t = GoTime(*i1)
    elif r < 0.50:
        t = GoTime(*_pick(rng, K))
    elif r < 0.60 and i1 is not None:
        t = GoTime(i1[0] + int(rng.integers(-1, 2)), int(rng.integers(0, 10**9)))
    else:
        t = random_time(rng)
    return s1, s2, t


# ------------------------------------------------------------------ addresses
def ip_equal(x: bytes, y: bytes) -> bool:
    """net.IP.Equal."""
    if len(x) == len(y):
        return x == y
    if len(x) == 4 and len(y) == 16:
        return y[:12] == V4 and y[12:] == x
    if len(x) == 16 and len(y) == 4:
        return x[:12] == V4 and x[12:] == y
    return False


def ip_spellings(p: bytes):
    """Eight spellings of the 16-byte address p that Go and `ipaddress` read alike (some of them the
    same text when p has no run of zeros or no letter)."""
    a6 = ipaddress.IPv6Address(p)
    h = ["%x" % int.from_bytes(p[i:i + 2], "big") for i in range(0, 16, 2)]
    quad = ".".join(str(x) for x in p[12:])
    if p[:12] == V4:
        return [quad, "::ffff:" + quad, "::ffff:%s:%s" % (h[6], h[7]), "0:0:0:0:0:ffff:" + quad,
                "0:0:0:0:0:ffff:%s:%s" % (h[6], h[7]), "::FFFF:" + quad, "0::ffff:" + quad, "::0:ffff:%s:%s" % (h[6], h[7])]
    full, tail = ":".join(h), ":".join(h[:6]) + ":" + quad
    return [a6.compressed, full, a6.exploded, tail, a6.compressed.upper(), full.upper(), a6.exploded.upper(), tail.upper()]


def const_addresses():
    return [_py_parse(s) for s in ("1.2.3.4", "10.0.0.255", "2001:db8::8a2e:370:7334", "fe80::1:2:b")]


def random_bytes(rng, k):
    return bytes(int(x) for x in rng.integers(0, 256, k))


def attr_pair(rng, p1):
    """(a, b): IP_ADDRESS attributes, a often the address p1 that the request's s1 spells."""
    K = const_addresses()
    v4 = p1[12:] if p1 is not None else random_bytes(rng, 4)
    r = rng.random()
    if r < 0.05:
        a = None
    elif r < 0.40 and p1 is not None:
        a = p1[12:] if p1[:12] == V4 and rng.random() < 0.5 else p1
    elif r < 0.50:
        k = _pick(rng, K)
        a = k[12:] if k[:12] == V4 and rng.random() < 0.5 else k
    elif r < 0.60:
        a = b"\0" * 12 + v4  # ::a.b.c.d is not the IPv4 address a.b.c.d
    elif r < 0.75:
        a = (V4 + v4)[:_pick(rng, [0, 3, 5, 15])]
    else:
        a = random_bytes(rng, _pick(rng, [4, 16]))
    r = rng.random()
    if r < 0.05:
        b = None
    elif a is not None and r < 0.45:  # equal: the same bytes, or the other form of an IPv4 address
        b = V4 + a if len(a) == 4 and rng.random() < 0.5 else a[12:] if len(a) == 16 and a[:12] == V4 and rng.random() < 0.5 else a
    elif a is not None and r < 0.60:  # unequal by form or length
        b = b"\0" * 12 + a if len(a) == 4 else a[:-1] if a else b"\0"
    elif a and r < 0.70:
        b = a[:-1] + bytes([a[-1] ^ 0x80])
    else:
        b = random_bytes(rng, _pick(rng, [4, 16]))
    return a, b


def ip_row(rng, valid_strings, draw, bad, quads):
    """(s1, s2) of a request that carries an address pair; draw(): the next of _strings()."""
    K = const_addresses()
    r = rng.random()
    if not valid_strings:
        s1 = _pick(rng, bad)
    elif r < 0.40:  # an address some rule's constant has
        s1 = _pick(rng, ip_spellings(_pick(rng, K)))
    elif r < 0.43:
        s1 = None
    elif r < 0.50 and quads:  # another request's dotted quad, spelled v4-in-v6
        s1 = _pick(rng, ip_spellings(_pick(rng, quads))[1:])
    else:
        s1 = draw()
    p1 = _py_parse(s1) if s1 is not None else None
    if p1 is not None and p1[:12] == V4:
        quads.append(p1)
    r = rng.random()
    if not valid_strings:
        s2 = _pick(rng, bad) if r < 0.9 else None
    elif p1 is not None and r < 0.40:
        s2 = _pick(rng, ip_spellings(p1))
    elif p1 is not None and r < 0.55:
        s2 = _pick(rng, ip_spellings(p1[:15] + bytes([p1[15] ^ 1])))
    elif r < 0.58:
        s2 = None
    else:
        s2 = draw()
    return s1, s2, p1


def make_rows(seed, n, valid_strings=True, attrs=True):
    """n requests as dicts over s1, s2, t, a, b (None: absent).  The even ones carry a timestamp
    pair in s1 / s2 / t, the odd ones an address pair in s1 / s2 / a / b; the other attributes are
    there too (instants and addresses for the interning tables), unrelated to the strings."""
    rng = np.random.default_rng(seed)
    pool = _strings(seed=seed + 100, n=2 * n + 60)
    bad = [s for s in pool if _py_parse(s) is None]
    at = [0]

    def draw():
        at[0] += 1
        return pool[at[0] % len(pool)]

    rows, quads = [], []
    for q in range(n):
        if q % 2 == 0:
            s1, s2, t = ts_row(rng, valid_strings, attrs)
            a, b = attr_pair(rng, None) if attrs else (None, None)
        else:
            s1, s2, p1 = ip_row(rng, valid_strings, draw, bad, quads)
            a, b = attr_pair(rng, p1) if attrs else (None, None)
            t = random_time(rng) if attrs and rng.random() < 0.9 else None
        rows.append({"s1": s1, "s2": s2, "t": t, "a": a, "b": b})
    return rows


# ------------------------------------------------------------------ rules and expected codes
def _eq(x, y, same):
    return 2 if x is ERR or y is ERR else int(bool(same(x, y)))


def _ne(x, y, same):
    return 2 if x is ERR or y is ERR else int(not same(x, y))


def _ts_consts():
    rng = np.random.default_rng(21)
    out = []
    for inst in const_instants():
        seen = set()
        while len(seen) < 10:
            seen.add(spell_instant(rng, *inst))
        out += sorted(seen)
    return out


def _ip_consts():
    return [s for p in const_addresses() for s in ip_spellings(p)]


def _same_t(x, y):
    return x == y


# (rule text, f(values of one row) -> 0 / 1 / 2); a row's values: T1, T2, Tt, I1, I2, A, B
TS_PAIR_RULES = [
    ("timestamp(s1) == timestamp(s2)", lambda v: _eq(v["T1"], v["T2"], _same_t)),
    ("timestamp(s1) != timestamp(s2)", lambda v: _ne(v["T1"], v["T2"], _same_t)),
    ("timestamp(s1) == t", lambda v: _eq(v["T1"], v["Tt"], _same_t)),
    ("t == timestamp(s2)", lambda v: _eq(v["Tt"], v["T2"], _same_t)),
]
IP_PAIR_RULES = [
    ("ip(s1) == ip(s2)", lambda v: _eq(v["I1"], v["I2"], ip_equal)),
    ("ip(s1) == a", lambda v: _eq(v["I1"], v["A"], ip_equal)),
    ("a == b", lambda v: _eq(v["A"], v["B"], ip_equal)),
    ("a != ip(s2)", lambda v: _ne(v["A"], v["I2"], ip_equal)),
]


def _const_rule(fn, key, text, same, parse):
    want = parse(text)
    assert want is not None, text
    return ('%s(s1) == %s("%s")' % (fn, fn, text), lambda v: _eq(v[key], want, same))


TS_RULES = TS_PAIR_RULES + [_const_rule("timestamp", "T1", c, _same_t, T.ref) for c in _ts_consts()]
IP_RULES = IP_PAIR_RULES + [_const_rule("ip", "I1", c, ip_equal, _py_parse) for c in _ip_consts()]
ALL_RULES = TS_RULES + IP_RULES
PAIR_RULES = TS_PAIR_RULES + IP_PAIR_RULES  # (no constant: an empty rule-set pool of instants and addresses)
TS_TEXTS = {t for t, _ in TS_RULES}


def _parsed(s, parse):
    v = parse(s) if s is not None else None
    return ERR if v is None else v


def row_values(row):
    """What the rules read from one request: both references on both strings, the attributes."""
    s1, s2, t, a, b = (row[k] for k in ("s1", "s2", "t", "a", "b"))
    return {"T1": _parsed(s1, T.ref), "T2": _parsed(s2, T.ref), "Tt": ERR if t is None else (t.sec, t.nsec),
            "I1": _parsed(s1, _py_parse), "I2": _parsed(s2, _py_parse), "A": ERR if a is None else a,
            "B": ERR if b is None else b}


class Case:
    """A batch with its expected codes for `rules`.  The even requests carry a timestamp pair
    (s1, s2, t), the odd ones an address pair (s1, s2, a, b); every rule reads every request, so a
    timestamp string also goes through ip() and an address through timestamp()."""

    def __init__(self, seed, n, rules=None, valid_strings=True, attrs=True):
        self.rules = ALL_RULES if rules is None else rules
        self.rows = make_rows(seed, n, valid_strings, attrs)
        self.n = n
        self.batch = BagBatch.from_bags([{k: v for k, v in row.items() if v is not None} for row in self.rows],
                                        names=list(MANIFEST))
        self.want = np.array([[f(v) for _, f in self.rules] for v in map(row_values, self.rows)],
                             dtype=np.uint8).reshape(n, len(self.rules))

    @property
    def texts(self):
        return [t for t, _ in self.rules]

    def family(self, ts: bool, pair_rules_only=False):
        """The expected codes of the timestamp (address) rules on the requests that carry a
        timestamp (address) pair."""
        cols = [r for r, (t, _) in enumerate(self.rules) if (t in TS_TEXTS) == ts and not (pair_rules_only and '("' in t)]
        return self.want[(0 if ts else 1)::2][:, cols]

    def distinct(self):
        inst, addr = set(), set()
        for v in map(row_values, self.rows):
            inst |= {v[k] for k in ("T1", "T2", "Tt") if v[k] is not ERR}
            addr |= {v[k] for k in ("I1", "I2") if v[k] is not ERR}
            addr |= {V4 + v[k] if len(v[k]) == 4 else v[k] for k in ("A", "B") if v[k] is not ERR}
        return len(inst), len(addr)


_CASES = {}


SHAPES = {  # name -> (seed, requests, generator arguments)
    "one": (31, 1, {}),
    "two": (32, 2, {}),
    "n257": (33, 257, {}),
    "large": (34, 6001, {}),
    "large2": (35, 5003, {}),
    "no_parse": (36, 300, {"valid_strings": False}),  # TIMESTAMP / IP_ADDRESS attributes, no string that parses
    "no_attr": (37, 301, {"attrs": False}),           # no TIMESTAMP / IP_ADDRESS attribute at all (NT == 0)
}
RULE_SETS = {"all": ALL_RULES, "pairs": PAIR_RULES}


def case(name, key="all") -> Case:
    """The shapes (each built once, shared, never changed) with the expected codes of a rule set."""
    if (name, key) not in _CASES:
        seed, n, kw = SHAPES[name]
        _CASES[name, key] = Case(seed, n, rules=RULE_SETS[key], **kw)
    return _CASES[name, key]


def check_shares(c: Case):
    """True, false and error each make up a tenth of the timestamp pairs and of the address pairs:
    of each family's rules (all of them, and the four pair rules alone) on the requests that carry
    that family's pair, and of the four pair rules on all requests.  Not of all of a family's
    rules on all requests: s1 / s2 hold an instant or an address, never both, so a family's rules
    are errors on the other half of the requests, and its ~40 constant rules, each true only for
    its own instant (address), are true on about 5 % of all (request, rule) pairs."""
    for ts in (True, False):
        for pair_rules_only in (False, True):
            w = c.family(ts, pair_rules_only)
            for code in (0, 1, 2):
                assert (w == code).mean() >= 0.10, (ts, pair_rules_only, code, [(w == k).mean() for k in (0, 1, 2)])
        pair_texts = {t for t, _ in (TS_PAIR_RULES if ts else IP_PAIR_RULES)}
        w = c.want[:, [r for r, (t, _) in enumerate(c.rules) if t in pair_texts]]
        for code in (0, 1, 2):
            assert (w == code).mean() >= 0.10, (ts, "all requests", code, [(w == k).mean() for k in (0, 1, 2)])


# ------------------------------------------------------------------ CPU: the generators, the oracle
def test_batches_hold_what_they_claim():
    c = case("large")
    check_shares(c)
    check_shares(case("large", "pairs"))
    inst, addr = c.distinct()
    assert inst >= 4000 and addr >= 4000, (inst, addr)
    assert len(c.batch.time_sec) > 2000 and ((c.batch.time_sec < 0) & (c.batch.time_nsec != 0)).sum() > 100
    assert {0, 3, 4, 5, 15, 16} <= {len(row[k]) for row in c.rows for k in "ab" if row[k] is not None}
    vals = [row_values(row) for row in c.rows]
    # one instant (address) spelled twice in a request; a string's value that an attribute holds too
    assert sum(v["T1"] is not ERR and v["T1"] == v["T2"] and r["s1"] != r["s2"] for v, r in zip(vals, c.rows)) > 500
    assert sum(v["I1"] is not ERR and v["I1"] == v["I2"] and r["s1"] != r["s2"] for v, r in zip(vals, c.rows)) > 500
    assert sum(v["T1"] is not ERR and v["T1"] == v["Tt"] for v in vals) > 500
    assert sum(v["I1"] is not ERR and v["A"] is not ERR and len(v["A"]) == 4 and ip_equal(v["I1"], v["A"]) for v in vals) > 150
    c = case("no_parse")
    assert all(v[k] is ERR for v in map(row_values, c.rows) for k in ("T1", "T2", "I1", "I2"))
    assert len(c.batch.time_sec) > 100
    c = case("no_attr")
    assert len(c.batch.time_sec) == 0 and all(row[k] is None for row in c.rows for k in "tab")
    assert all(T.ref(s) is not None for s in _ts_consts()) and len(set(_ts_consts())) == 40
    assert len({T.ref(s) for s in _ts_consts()}) == 4 and len({_py_parse(s) for s in _ip_consts()}) == 4
    assert len(set(_ip_consts())) == 32


@pytest.mark.parametrize("name", ["n257", "large", "no_parse", "no_attr"])
def test_oracle_gives_the_expected_codes(name):
    """The oracle's interpreter (its own parse, interning-free values, ip_equal) on the same batches."""
    c = case(name)
    ev = oracle.OracleEvaluator(MANIFEST)
    got = oracle.oracle_matrix(ev, c.texts, c.batch, threads=16)
    bad = np.argwhere(np.minimum(got, 2) != c.want)
    assert bad.size == 0, [(c.texts[r], c.rows[q], int(got[q, r]), int(c.want[q, r])) for q, r in bad[:5]]


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def mxp(libmxp):
    import istio_amd.engine as mxp
    return mxp


def _engine(mxp, rules, host):
    mp = pytest.MonkeyPatch()
    mp.setenv("MXP_HOST_PACK", "1" if host else "0")
    mp.setenv("MXP_DEBUG_FLAGS", "0")
    try:
        eng = mxp.Engine(0)
    finally:
        mp.undo()
    eng.set_vocabulary(MANIFEST)
    st = eng.compile(rules)
    assert (st == 0).all(), [(rules[i], eng.rule_error(i)) for i in np.nonzero(st)[0][:3]]
    return eng


@pytest.fixture(scope="module")
def engines(mxp):
    """(device packer, host packer) engines for the full rule set and for the pair rules alone."""
    out = {}
    for key, rules in (("all", ALL_RULES), ("pairs", PAIR_RULES)):
        texts = [t for t, _ in rules]
        out[key] = (_engine(mxp, texts, False), _engine(mxp, texts, True))
    yield out
    for pair in out.values():
        for e in pair:
            e.close()


def _sample(want, k=150):
    errs = np.argwhere(want == 2)
    if len(errs) > k:
        errs = errs[np.random.default_rng(3).choice(len(errs), k, replace=False)]
    return [(int(q), int(r)) for q, r in errs]


def narrow_bitmaps(eng, c: Case):
    """The batch through the narrow upload -> (match, err) bitmaps."""
    from test_gpu_narrow import _bitmaps
    nb = NarrowBatch(c.batch)
    strings_only = all(row[k] is None for row in c.rows for k in "tab")
    assert nb.narrow.all() if strings_only else nb.narrow.any(), nb.narrow  # (else: the wide upload again)
    db = eng.upload2(nb)
    m, e = _bitmaps(db, c.n, len(c.rules))
    db.free()
    return m.view(np.uint32), e.view(np.uint32)


def three_paths(mxp, dev, host, c: Case):
    """The three packers on one batch -> codes: identical bitmaps from all three, identical sampled
    error texts from the device and the host packer.  (An evaluation of an uploaded batch into
    device bitmaps records no errors, so mxp_pair_error has no text for it: the narrow upload's
    texts are read through Resolve, in test_narrow_upload_error_texts.)"""
    R = len(c.rules)
    pairs = _sample(c.want)
    out = []
    for eng in (dev, host):
        m, e = eng.eval_batch(c.batch)
        out.append((m, e, [eng.pair_error(q, r) for q, r in pairs]))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]), "host packer"
    assert out[0][2] == out[1][2], "host packer"
    assert all(out[0][2])
    m, e = narrow_bitmaps(dev, c)
    assert np.array_equal(out[0][0], m) and np.array_equal(out[0][1], e), "narrow upload"
    return mxp.bits_to_codes(out[0][0], out[0][1], R), pairs, out[0][2]


def assert_codes(c: Case, got):
    bad = np.argwhere(got != c.want)
    assert bad.size == 0, [(c.texts[r], c.rows[q], int(got[q, r]), int(c.want[q, r])) for q, r in bad[:5]]


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["all", "pairs"])
@pytest.mark.parametrize("name", ["one", "two", "n257", "large", "no_parse", "no_attr"])
def test_three_packers_give_the_expected_codes(mxp, engines, name, key):
    """key "pairs": the rule set without constants, whose pool of instants and addresses is empty (so
    that in "no_parse" the second interning pass really finds nothing)."""
    c = case(name, key)
    dev, host = engines[key]
    got, pairs, texts = three_paths(mxp, dev, host, c)
    assert_codes(c, got)
    if name == "large":
        check_shares(c)
    ev = oracle.OracleEvaluator(MANIFEST)  # the authority for the error texts
    for (q, r), text in zip(pairs, texts):
        st, msg = ev.eval_predicate(c.texts[r], c.batch, q)
        assert st == "error" and text == msg, (c.texts[r], c.rows[q], text, msg)


@pytest.mark.gpu
def test_oracle_parity_on_the_large_batch(mxp, engines):
    """test_gpu_parity's compare(): every pair against the oracle, error texts sampled."""
    from test_gpu_parity import compare
    c = case("large")
    compare(engines["all"][0], oracle.OracleEvaluator(MANIFEST), c.texts, c.batch, sample_msgs=200)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["all", "pairs"])
def test_one_engine_reuses_its_tables(mxp, key):
    """The packer's scratch tables grow only and are reused: large, a batch without TIMESTAMP /
    IP_ADDRESS values (an empty first pass over a table the large batch filled), large again, a batch
    whose strings never parse, one request, and large once more, on one engine, each through the
    wide and the narrow upload.  What this can see is a wrong code: a value interned onto another
    value's representative, or not onto its own.  (It caught the time table reset before its second
    pass.  A table not reset at all leaves entries that name items of an earlier batch; as long as
    every probe still ends, equal values keep equal ids and the codes stay right, so that fault
    would show here only as a read past the batch or a probe that never ends -- nothing to try on
    purpose.)"""
    eng = _engine(mxp, [t for t, _ in RULE_SETS[key]], False)
    for name in ["large", "no_attr", "large2", "no_parse", "one", "large", "two", "n257"]:
        c = case(name, key)
        m, e = eng.eval_batch(c.batch)
        assert_codes(c, mxp.bits_to_codes(m, e, len(c.rules)))
        mn, en = narrow_bitmaps(eng, c)
        assert np.array_equal(m, mn) and np.array_equal(e, en), name
    eng.close()


@pytest.mark.gpu
def test_narrow_upload_error_texts(mxp):
    """Error texts that belong to a narrow upload.  mxp_pair_error answers for the batch of the last
    evaluation that recorded errors, and of the calls that take an uploaded batch only Resolve does
    (as in test_gpu_narrow.py).  So: the large batch with an identity attribute, a resolver over all
    rules, and an engine that does nothing but upload2 + resolve_uploaded.  Its status and first
    failing rule per request equal those of the wide Resolve on the device- and host-packing engines,
    the rule does fail on that request by the references, and its text -- which quotes the offending
    string, read from the narrow batch's host view -- is the oracle's."""
    c = case("large")
    manifest = dict(MANIFEST, **{"destination.service": "STRING"})
    bags = [dict({k: v for k, v in row.items() if v is not None}, **{"destination.service": "svc.istio-system.svc.cluster.local"})
            for row in c.rows]
    batch = BagBatch.from_bags(bags, names=list(manifest))
    R = len(c.rules)
    ns, vm, z = ["istio-system"] * R, np.ones(R, dtype=np.uint32), np.zeros(R, dtype=np.uint8)
    engs = []
    for host in (False, True, False):
        mp = pytest.MonkeyPatch()
        mp.setenv("MXP_HOST_PACK", "1" if host else "0")
        mp.setenv("MXP_DEBUG_FLAGS", "0")
        try:
            eng = mxp.Engine(0)
        finally:
            mp.undo()
        eng.set_vocabulary(manifest)
        assert (eng.compile(c.texts) == 0).all()
        eng.set_resolver("destination.service", "istio-system", ns, vm, z, z)
        engs.append(eng)
    dev, host, narrow = engs
    want = dev.resolve_arrays(batch, 0)
    for a, b in zip(host.resolve_arrays(batch, 0), want):
        assert np.array_equal(a, b)
    nb = NarrowBatch(batch)
    assert nb.narrow.any()
    got = narrow.resolve_uploaded(narrow.upload2(nb), 0, cap=max(16, len(want[3])))
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    failed = np.nonzero(got[0] == mxp.Engine.RESOLVE_PRED_ERROR)[0]
    assert len(failed) > 1000 and len(set(got[1][failed].tolist())) >= 3, (len(failed), set(got[1][failed].tolist()))
    ev = oracle.OracleEvaluator(manifest)
    sample = failed[np.random.default_rng(5).choice(len(failed), 150, replace=False)]
    texts = set()
    for q in sample:
        q, r = int(q), int(got[1][q])
        assert c.want[q, r] == 2, (q, c.texts[r])
        st, msg = ev.eval_predicate(c.texts[r], batch, q)
        text = narrow.pair_error(q, r)
        assert st == "error" and text and text == msg == dev.pair_error(q, r) == host.pair_error(q, r), (c.texts[r], c.rows[q], text, msg)
        texts.add(text)
    assert len(texts) > 20, texts  # (texts that quote the requests' own strings)
    for eng in engs:
        eng.close()


# ------------------------------------------------------------------ instants directly (Eval mode)
def utc_text(sec: int, nsec: int) -> str:
    """The engine's layout of a time.Time in UTC ("2006-01-02 15:04:05.999999999 +0000 UTC"), for
    instants of years 0..9999, from `datetime` (year 0000 by hand: a leap year of 366 days)."""
    days, rem = divmod(sec + _SEC0, 86400)
    if days >= 0:
        d = datetime.date.fromordinal(days + 1)
        y, mo, dd = d.year, d.month, d.day
    else:
        assert days >= -366
        y, mo, dd = 0, 1, days + 366 + 1
        for k in (31, 29, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31):
            if dd <= k:
                break
            dd -= k
            mo += 1
    out = "%04d-%02d-%02d %02d:%02d:%02d" % (y, mo, dd, rem // 3600, rem // 60 % 60, rem % 60)
    if nsec:
        out += "." + ("%09d" % nsec).rstrip("0")
    return out + " +0000 UTC"


@pytest.mark.gpu
def test_timestamp_values_in_eval_mode(mxp):
    """`timestamp(s1)` read back through eval_values / value_text: the instant the reference gives,
    in the engine's UTC layout -- year 0000, year 9999, pre-1970 seconds with nanoseconds.  (The
    instant only: Go prints a time parsed with an offset in that offset's zone, which neither the
    oracle nor the product models.)  Strings whose instant leaves years 0..9999 are not generated."""
    assert utc_text(0, 0) == "1970-01-01 00:00:00 +0000 UTC"
    assert utc_text(-1, 1) == "1969-12-31 23:59:59.000000001 +0000 UTC"
    assert utc_text(1420211075, 500000000) == "2015-01-02 15:04:35.5 +0000 UTC"
    assert utc_text(T.ref("0000-02-29T23:59:59Z")[0], 0) == "0000-02-29 23:59:59 +0000 UTC"
    lo, hi = T.ref("0000-01-01T00:00:00Z")[0], T.ref("9999-12-31T23:59:59Z")[0]
    strs = ["0000-01-01T00:00:00Z", "0000-12-31T23:59:59.999999999Z", "9999-12-31T23:59:59.999999999Z",
            "1969-12-31T23:59:59.000000001Z", "0001-01-01T00:00:00-00:15", "9999-12-31T23:59:59+00:15"]
    for s, w in T.cases(seed=41, n=1500):
        if w is None or lo <= w[0] <= hi:
            strs.append(s)
    want = [T.ref(s) for s in strs]
    assert sum(w is None for w in want) > 300 and sum(w is not None and w[0] < 0 and w[1] != 0 for w in want) > 100
    assert sum(s.startswith("0000") and w is not None for s, w in zip(strs, want)) > 10
    assert sum(s.startswith("9999") and w is not None for s, w in zip(strs, want)) > 10
    batch = BagBatch.from_bags([{"s1": s} for s in strs], names=list(MANIFEST))
    eng = _engine(mxp, ["timestamp(s1)"], False)
    vals, codes = eng.eval_values(batch)
    for q, (s, w) in enumerate(zip(strs, want)):
        if w is None:
            assert codes[q, 0] >= 2, s
        else:
            assert codes[q, 0] < 2, (s, eng.pair_error(q, 0))
            assert eng.value_text(0, vals[q, 0]) == utc_text(*w), s
    eng.close()


# ------------------------------------------------------------------ Go-only forms
@pytest.mark.gpu
def test_go_only_forms_agree(mxp, engines):
    """The spellings Go 1.9 accepts beyond RFC3339 (T.GO_ONLY): no expected value, the three packers
    and the oracle agree -- on validity, and on the instant (t is the oracle's instant of the row's
    string, s2 a plain spelling of it)."""
    from test_gpu_parity import compare
    rng = np.random.default_rng(51)
    insts = T.oracle_parse(T.GO_ONLY)
    assert sum(i is not None for i in insts) >= 5
    bags = []
    for s, i in zip(T.GO_ONLY, insts):
        bags.append({"s1": s, "s2": s, "t": GoTime(0, 0)})
        if i is not None:
            plain = spell_instant(rng, *i)
            bags.append({"s1": s, "t": GoTime(*i), **({"s2": plain} if plain is not None else {})})
            bags.append({"s1": "2015-01-02T15:04:05Z", "s2": s, "t": GoTime(i[0], i[1] + 1 if i[1] < 999999999 else 0)})
    c = case("one")  # (for the rule texts)
    batch = BagBatch.from_bags(bags, names=list(MANIFEST))
    dev, host = engines["all"]
    from test_gpu_narrow import _bitmaps
    md, ed = dev.eval_batch(batch)
    mh, eh = host.eval_batch(batch)
    nb = NarrowBatch(batch)
    assert nb.narrow.any()
    db = dev.upload2(nb)
    mn, en = _bitmaps(db, batch.n, len(c.rules))
    db.free()
    assert np.array_equal(md, mh) and np.array_equal(ed, eh)
    assert np.array_equal(md, mn.view(np.uint32)) and np.array_equal(ed, en.view(np.uint32))
    got, want = compare(dev, oracle.OracleEvaluator(MANIFEST), c.texts, batch, sample_msgs=100)
    assert (want[:, :4] == 1).any() and (want[:, :4] == 0).any()
