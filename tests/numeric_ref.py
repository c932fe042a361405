"""An independent reference for rules over 64-bit numeric attributes, and the inputs designed for it.

The reference interpreter compares INT64 and DOUBLE values alike, as two 32-bit words
(interpreterRun.go:285-297, 335-347): equality is equality of the 64-bit pattern, so a NaN equals a
NaN of the same payload and 0.0 does not equal -0.0.  This module restates just that, for a small
expression language, and imports neither the oracle nor the product.

Rules are built forward, from tuples; `text()` renders a tuple as rule text and `RuleSet.evaluate`
computes the expected outcome from the tuple and the bags -- never by parsing the text.

    operand  ("attr", name) | ("alt", name, name2) | ("altk", name, Const)       X, (X | Y), (X | K2)
    atom     ("eq", operand, Const | operand) | ("ne", operand, Const) | ("sw", name, prefix)
    rule     atom | ("and", r, r) | ("or", r, r) | ("par", r) | ("val", operand)

Semantics restated: `&&` and `||` short-circuit; `|` falls back when the attribute is absent, and only
then; a missing attribute is an error; a value of the wrong dynamic kind is an error (an INT64
attribute accepts a time.Duration: resolve_i, interpreterRun.go:455-708); a comparison is of the
64-bit patterns; the referenced set is what a short-circuit evaluation reads.

Bag values are (kind, payload) pairs: ("int64" | "duration" | "double", 64-bit pattern),
("string", str), ("bool", bool), ("other", text), ("map", dict), ("bytes", bytes).
"""
import struct
from collections import namedtuple

import numpy as np

# mixer/pkg/il/testing/tests.go:2414-2489 (defaultAttrs), the manifest the fuzz tests use
MANIFEST = {
    "ai": "INT64", "ab": "BOOL", "as": "STRING", "ad": "DOUBLE", "ar": "STRING_MAP", "adur": "DURATION",
    "at": "TIMESTAMP", "aip": "IP_ADDRESS", "bi": "INT64", "bb": "BOOL", "bs": "STRING", "bd": "DOUBLE",
    "br": "STRING_MAP", "bdur": "DURATION", "bt": "TIMESTAMP", "t1": "TIMESTAMP", "t2": "TIMESTAMP",
    "bip": "IP_ADDRESS", "b1": "BOOL", "b2": "BOOL", "sm": "STRING_MAP",
}
ATTRS = ("ai", "bi", "ad", "bd", "bs")  # the attributes the designed bags carry
N_REQUESTS = 4096 + 37
M64 = (1 << 64) - 1
FALSE, TRUE, ERROR = 0, 1, 2

Const = namedtuple("Const", "cls text bits")  # cls "i" | "d" | "s"; bits: the 64-bit pattern (numeric)


def dbits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def dfloat(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def iconst(v):
    """A non-negative decimal int literal (a minus sign would parse to SUB, an unknown function)."""
    assert 0 <= v < (1 << 63)
    return Const("i", str(v), v)


def dconst(text):
    """An unsigned float literal; its bits from Python's float(text) (correctly rounded, not strtod)."""
    x = float(text)
    assert x == x and x not in (float("inf"),) and not text.startswith("-")
    return Const("d", text, dbits(x))


def dconst_bits(bits):
    x = dfloat(bits)
    c = dconst(repr(x))
    assert c.bits == bits and any(ch in c.text for ch in ".e"), (hex(bits), c.text)
    return c


def sconst(s):
    return Const("s", '"%s"' % s, 0)


def cls_of(name):
    return {"INT64": "i", "DOUBLE": "d", "STRING": "s"}[MANIFEST[name]]


ACCEPTS = {"i": ("int64", "duration"), "d": ("double",), "s": ("string",)}

# ------------------------------------------------------------------------------------ value pools
# INT64 constants: a grid of low words x high words, so every value has neighbours that agree with
# it in exactly one word.  It contains 0, 1, 2^31-1, 2^31, 2^32-1, 2^32, 2^32+1, 7, 2^32+7, 7*2^32,
# 0x00000001_00000001, 0x00000000_FFFFFFFF, 2^56-1, 2^56, 2^56+3, 2^63-1 and one-bit-flip neighbours
# of 7 and 2^32+7 in each word (6, 2^32+6; 3 * 2^32 + 7, 5 * 2^32 + 7).
I_LO = [0, 1, 3, 7, 6, 2, 5, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0xFFFFFFFE, 0x80000007, 0x00010000, 0x55555555,
        0xAAAAAAAA, 0x12345678, 0xDEADBEEF, 0x00000100, 0x01000000, 0x7FFFFFF8]
I_HI = [0, 1, 3, 5, 7, 6, 0x00FFFFFF, 0x01000000, 0x7FFFFFFF, 0x7FFFFFFE, 0x00010000, 0x55555555, 0x2AAAAAAA,
        0x12345678, 0x40000000]
I_GRID = [(h << 32) | l for h in I_HI for l in I_LO]
I_HOT = [(1 << 32) + 7, (1 << 56) + 3]
# attribute values only: negative numbers (-1, -2^63, 0xFFFFFFFF_00000000, ...) have no literal
I_NEG = [(h << 32) | l for h in (0xFFFFFFFF, 0x80000000, 0xFFFFFFFE) for l in I_LO]
I_NAMED = [0, 1, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 7, (1 << 32) + 7, 7 << 32,
           0x0000000100000001, 0x00000000FFFFFFFF, (1 << 56) - 1, 1 << 56, (1 << 56) + 3, (1 << 63) - 1,
           6, (1 << 32) + 6, (3 << 32) + 7, (5 << 32) + 7]
assert set(I_NAMED) <= set(I_GRID) and set(I_HOT) <= set(I_GRID) and len(set(I_GRID)) == 300
assert {M64, 1 << 63, 0xFFFFFFFF00000000} <= set(I_NEG)

# DOUBLE constants: the same construction over finite non-negative patterns.  0.1 is
# 0x3FB99999_9999999A; its nextafter has low word ...9B; 0x3FA99999 / 0x3FF99999 flip one exponent
# bit of its high word.  High word 0 holds the denormals 5e-324 (low word 1) and 1e-320 (2024);
# 0x7FEFFFFF_FFFFFFFF is the largest finite double.
D_LO = [0, 1, 2024, 0x9999999A, 0x9999999B, 0x99999998, 0xFFFFFFFF, 0xFFFFFFFE, 0x80000000, 0x7FFFFFFF, 7,
        0x00010000, 0x55555555, 0xAAAAAAAA, 0x12345678, 0xDEADBEEF, 0x00000100, 0x01000000, 0x9999999E, 2]
D_HI = [0, 0x3FB99999, 0x3FA99999, 0x3FF99999, 0x3FB9999A, 0x3FF80000, 0x3FF00000, 0x7FEFFFFF, 0x00100000, 1,
        0x40000000, 0x3FE00000, 0x408F4000, 0x40140000, 0x12345678]
D_GRID = [(h << 32) | l for h in D_HI for l in D_LO]
D_HOT = [dbits(0.1), dbits(1.5)]
D_SPECIAL = [dbits(-0.0), dbits(float("inf")), dbits(float("-inf")), 0x7FF8000000000000, 0x7FF8000000000001,
             0xFFF8000000000000, 0x7FF0000000000001, dbits(-0.1), dbits(-1.5), 0x8000000000000001]
# the spellings a float literal takes in rule text
D_SPELLED = [dconst(t) for t in ("0.1", "1.5", "0.0", "1e-320", "5e-324", ".5", "5.", "1E3", "1.7976931348623157e+308",
                                 "0.10000000000000000555", "0.10000000000000001943", "1.7976931348623157e308")]
assert set(D_HOT) <= set(D_GRID) and len(set(D_GRID)) == 300 and dbits(5e-324) == 1 and dbits(1e-320) == 2024
assert dconst("0.10000000000000000555").bits == dbits(0.1) and dconst("0.10000000000000001943").bits == dbits(0.1) + 1
assert {c.bits for c in D_SPELLED if c.text in (".5", "5.", "1E3")} <= set(D_GRID)

BS_VALUES = ["x"] * 10 + ["abx"] * 5 + ["ab"] * 2 + ["abc", "a", ""]
WRONG = [("string", "str"), ("int64", 3), ("bool", True), ("other", "20"), ("map", {"a": "b"}),
         ("double", dbits(1.5)), ("bytes", b"\x01")]


def _pick(rng, xs):
    return xs[int(rng.integers(len(xs)))]


def make_bags(n=N_REQUESTS, seed=1, p_missing=0.25, p_wrong=0.05, p_hot=0.8):
    """Bags over ATTRS: numeric values hot (two values per class carry p_hot of the mass, so rules on
    them are true often) or spread over the grids and the values that have no literal; an INT64
    attribute holds a time.Duration of the same patterns one time in ten."""
    rng = np.random.default_rng(seed)
    bags = []
    for _ in range(n):
        b = {}
        for name in ATTRS:
            if rng.random() < p_missing:
                continue
            if rng.random() < p_wrong:
                b[name] = _pick(rng, WRONG)
                continue
            c = cls_of(name)
            if c == "s":
                b[name] = ("string", _pick(rng, BS_VALUES))
            elif c == "i":
                v = _pick(rng, I_HOT) if rng.random() < p_hot else _pick(rng, I_GRID + I_NEG + I_NEG)
                b[name] = ("duration" if rng.random() < 0.1 else "int64", v)
            else:
                v = _pick(rng, D_HOT) if rng.random() < p_hot else _pick(rng, D_GRID + D_SPECIAL * 6)
                b[name] = ("double", v)
        bags.append(b)
    return bags


# ------------------------------------------------------------------------------------ rule text
def And(a, b):
    if a[0] == "or":
        a = ("par", a)
    if b[0] in ("and", "or"):
        b = ("par", b)
    return ("and", a, b)


def Or(a, b):
    if b[0] in ("and", "or"):
        b = ("par", b)
    return ("or", a, b)


def _operand_text(op):
    if op[0] == "attr":
        return op[1]
    if op[0] == "alt":
        return "(%s | %s)" % (op[1], op[2])
    return "(%s | %s)" % (op[1], op[2].text)


def text(node):
    t = node[0]
    if t in ("eq", "ne"):
        r = node[2]
        return "%s %s %s" % (_operand_text(node[1]), "==" if t == "eq" else "!=",
                             r.text if isinstance(r, Const) else _operand_text(r))
    if t == "sw":
        return '%s.startsWith("%s")' % (node[1], node[2])
    if t == "and":
        return "%s && %s" % (text(node[1]), text(node[2]))
    if t == "or":
        return "%s || %s" % (text(node[1]), text(node[2]))
    if t == "par":
        return "(%s)" % text(node[1])
    if t == "val":
        s = _operand_text(node[1])
        return s[1:-1] if s.startswith("(") else s
    raise ValueError(t)


def leading_atom(node):
    while node[0] in ("and", "or", "par"):
        node = node[1]
    return node


# ------------------------------------------------------------------------------------ one pair, plain Python
def _get(bag, name, reads):
    """-> ("ok", payload) | ("absent",) | ("wrong",)"""
    reads.add(name)
    if name not in bag:
        return ("absent",)
    kind, payload = bag[name]
    return ("ok", payload) if kind in ACCEPTS[cls_of(name)] else ("wrong",)


def _operand_one(op, bag, reads):
    r = _get(bag, op[1], reads)
    if op[0] == "attr" or r[0] != "absent":
        return r if r[0] == "ok" else ("error",)
    if op[0] == "altk":
        return ("ok", op[2].bits)
    r = _get(bag, op[2], reads)
    return r if r[0] == "ok" else ("error",)


def eval_one(node, bag, reads):
    """EvalPredicate of one rule on one bag -> FALSE | TRUE | ERROR; the attributes read go to `reads`.
    For a ("val", ..) rule -> (ERROR, 0) | (FALSE, bits)."""
    t = node[0]
    if t in ("eq", "ne"):
        a = _operand_one(node[1], bag, reads)
        if a[0] != "ok":
            return ERROR
        r = node[2]
        if isinstance(r, Const):
            b = ("ok", r.text[1:-1] if r.cls == "s" else r.bits)
        else:
            b = _operand_one(r, bag, reads)
            if b[0] != "ok":
                return ERROR
        return int((a[1] == b[1]) == (t == "eq"))
    if t == "sw":
        a = _get(bag, node[1], reads)
        return int(a[1].startswith(node[2])) if a[0] == "ok" else ERROR
    if t == "par":
        return eval_one(node[1], bag, reads)
    if t == "val":
        a = _operand_one(node[1], bag, reads)
        return (FALSE, a[1]) if a[0] == "ok" else (ERROR, 0)
    a = eval_one(node[1], bag, reads)
    if a == ERROR or a == (FALSE if t == "and" else TRUE):
        return a
    return eval_one(node[2], bag, reads)


# ------------------------------------------------------------------------------------ a batch, by column
class Columns:
    """The bags by column: per attribute its kind (index into KINDS; 0 absent), 64-bit pattern and text."""
    KINDS = ("absent", "string", "int64", "double", "bool", "duration", "other", "map", "bytes")

    def __init__(self, bags):
        self.n = len(bags)
        self.kind, self.bits, self.strs = {}, {}, {}
        for name in ATTRS:
            k = np.zeros(self.n, dtype=np.uint8)
            v = np.zeros(self.n, dtype=np.uint64)
            s = np.full(self.n, "", dtype=object)
            for q, b in enumerate(bags):
                if name in b:
                    kind, payload = b[name]
                    k[q] = self.KINDS.index(kind)
                    if kind in ("int64", "duration", "double"):
                        v[q] = payload
                    elif kind == "string":
                        s[q] = payload
            self.kind[name], self.bits[name], self.strs[name] = k, v, s

    def good(self, name):
        return np.isin(self.kind[name], [self.KINDS.index(k) for k in ACCEPTS[cls_of(name)]])


class _Run:
    def __init__(self, cols, record=True):
        self.c = cols
        self.reads = {name: np.zeros(cols.n, dtype=bool) for name in ATTRS} if record else None

    def get(self, name, active):
        if self.reads is not None:
            self.reads[name] |= active
        good = self.c.good(name)
        return active & good, active & (self.c.kind[name] == 0), self.c.bits[name]

    def operand(self, op, active):
        """-> (ok, bits): ok a subset of active; the rest of active is in error"""
        ok, absent, bits = self.get(op[1], active)
        if op[0] == "attr":
            return ok, bits
        if op[0] == "altk":
            return ok | absent, np.where(absent, np.uint64(op[2].bits), bits)
        ok2, _, bits2 = self.get(op[2], absent)
        return ok | ok2, np.where(absent, bits2, bits)

    def node(self, node, active):
        """-> codes (FALSE where not active)"""
        t = node[0]
        if t in ("eq", "ne"):
            ok, a = self.operand(node[1], active)
            r = node[2]
            if isinstance(r, Const) and r.cls == "s":
                same = self.c.strs[node[1][1]] == r.text[1:-1]
            elif isinstance(r, Const):
                same = a == np.uint64(r.bits)
            else:
                ok, b = self.operand(r, ok)
                same = a == b
            hit = same if t == "eq" else ~same
            return np.where(active & ~ok, ERROR, np.where(ok & hit, TRUE, FALSE)).astype(np.uint8)
        if t == "sw":
            ok, _, _ = self.get(node[1], active)
            hit = np.array([s.startswith(node[2]) for s in self.c.strs[node[1]]], dtype=bool)
            return np.where(active & ~ok, ERROR, np.where(ok & hit, TRUE, FALSE)).astype(np.uint8)
        if t == "par":
            return self.node(node[1], active)
        a = self.node(node[1], active)
        go = active & (a == (TRUE if t == "and" else FALSE))
        b = self.node(node[2], go)
        return np.where(go, b, a).astype(np.uint8)


class RuleSet:
    def __init__(self, name, nodes):
        self.name = name
        self.nodes = list(nodes)
        self.rules = [text(x) for x in self.nodes]

    def evaluate(self, cols):
        """-> codes u8 [n, R] (EvalPredicate), reads {attribute: bool [n]} (the union over the rules)."""
        run = _Run(cols)
        every = np.ones(cols.n, dtype=bool)
        codes = np.stack([run.node(x, every) for x in self.nodes], axis=1)
        return codes, run.reads

    def values(self, cols):
        """Eval of ("val", operand) rules -> (ok bool [n, R], bits u64 [n, R])."""
        run = _Run(cols, record=False)
        every = np.ones(cols.n, dtype=bool)
        out = [run.operand(x[1], every) for x in self.nodes]
        return np.stack([o[0] for o in out], axis=1), np.stack([np.where(o[0], o[1], np.uint64(0)) for o in out], axis=1)

    def leading(self, cols):
        """The leading compare of each rule: (valid bool [n, R], left u64 [n, R], right u64 [n, R]) --
        valid where both sides hold a numeric value."""
        run = _Run(cols, record=False)
        every = np.ones(cols.n, dtype=bool)
        V, L, Rt = [], [], []
        for x in self.nodes:
            at = leading_atom(x)
            ok, a = run.operand(at[1], every)
            if isinstance(at[2], Const):
                b = np.full(cols.n, at[2].bits, dtype=np.uint64)
            else:
                ok, b = run.operand(at[2], ok)
            V.append(ok)
            L.append(a)
            Rt.append(b)
        return np.stack(V, axis=1), np.stack(L, axis=1), np.stack(Rt, axis=1)


def referenced(reads, q):
    """FakeBag.ReferencedList form of request q: the sorted names."""
    return sorted(name for name, m in reads.items() if m[q])


# ------------------------------------------------------------------------------------ families
def _neighbour(rng, v, grid, word):
    """A grid value that agrees with v in `word` ("lo" | "hi") only."""
    if word == "lo":
        xs = [g for g in grid if (g & 0xFFFFFFFF) == (v & 0xFFFFFFFF) and g != v]
    else:
        xs = [g for g in grid if (g >> 32) == (v >> 32) and g != v]
    return _pick(rng, xs)


def pick_k(rng, cls):
    """A constant related to the hot values: equal, equal in the low word only, equal in the high word
    only, or any constant of the class (grid, the named values, the float spellings)."""
    grid, hot = (I_GRID, I_HOT) if cls == "i" else (D_GRID, D_HOT)
    mk = iconst if cls == "i" else dconst_bits
    r = rng.random()
    h = _pick(rng, hot)
    if r < 0.3:
        return mk(h)
    if r < 0.55:
        return mk(_neighbour(rng, h, grid, "lo"))
    if r < 0.8:
        return mk(_neighbour(rng, h, grid, "hi"))
    if cls == "d" and r < 0.9:
        return _pick(rng, D_SPELLED)
    return mk(_pick(rng, I_NAMED if cls == "i" and r < 0.9 else grid))


_PAIR = {"i": ("ai", "bi"), "d": ("ad", "bd")}


def atom(rng, cls=None):
    cls = cls or _pick(rng, ["i", "i", "d"])
    x, y = _PAIR[cls]
    if rng.random() < 0.3:
        x, y = y, x
    r = rng.random()
    if r < 0.35:
        return ("eq", ("attr", x), pick_k(rng, cls))
    if r < 0.5:
        return ("ne", ("attr", x), pick_k(rng, cls))
    if r < 0.65:
        return ("eq", ("attr", x), ("attr", y))
    if r < 0.85:
        return ("eq", ("alt", x, y), pick_k(rng, cls))
    return ("eq", ("altk", x, pick_k(rng, cls)), pick_k(rng, cls))


def continuation(rng, lead_attr, lead_k):
    """`bs == "x"`, `bi == K2` (a 64-bit per-rule constant of a shared continuation) or `ad == K3`."""
    r = rng.random()
    if r < 0.5:
        return ("eq", ("attr", "bs"), sconst("x"))
    if r < 0.75:
        return ("eq", ("attr", "bi"), pick_k(rng, "i"))
    if lead_attr == "ad" and rng.random() < 0.5:
        return ("eq", ("attr", "ad"), lead_k)
    return ("eq", ("attr", "ad"), pick_k(rng, "d"))


def family_a(seed=11, n=320):
    """Atoms alone, and atoms under &&, || and parentheses."""
    rng = np.random.default_rng(seed)

    def expr(d):
        r = rng.random()
        if d == 0 or r < 0.4:
            return atom(rng)
        if r < 0.65:
            return And(expr(d - 1), expr(d - 1))
        if r < 0.9:
            return Or(expr(d - 1), expr(d - 1))
        return ("par", expr(d - 1))
    return [RuleSet("a", [expr(2) for _ in range(n)])]


def family_b(seed=12):
    """Guard-only rules `X == K` in 32-rule groups: even groups hold 32 rules on one column, odd ones
    7 on each numeric column and 4 on bs -- the >= 8 and < 8 branches of the group compare."""
    rng = np.random.default_rng(seed)
    nodes = []
    for g in range(12):
        if g % 2 == 0:
            col = ("ai", "ad", "bi", "bd")[(g // 2) % 4]
            nodes += [("eq", ("attr", col), pick_k(rng, cls_of(col))) for _ in range(32)]
        else:
            grp = [("eq", ("attr", col), pick_k(rng, cls_of(col))) for col in ("ai", "bi", "ad", "bd") for _ in range(7)]
            grp += [("eq", ("attr", "bs"), sconst(s)) for s in ("x", "abx", "ab", "")]
            nodes += [grp[int(i)] for i in rng.permutation(32)]
    return [RuleSet("b", nodes)]


def family_c(seed=13):
    """`X == K && <continuation>`: per column every one of the 300 grid constants once (the half-equal
    pairs among them) and the two hot ones fifty times each."""
    sets = []
    for col in ("ai", "ad"):
        rng = np.random.default_rng(seed + len(sets))
        cls = cls_of(col)
        mk = iconst if cls == "i" else dconst_bits
        ks = [mk(v) for v in (I_GRID if cls == "i" else D_GRID)] + [mk(h) for h in (I_HOT if cls == "i" else D_HOT)] * 50
        ks = [ks[int(i)] for i in rng.permutation(len(ks))]
        sets.append(RuleSet("c_" + col, [And(("eq", ("attr", col), k), continuation(rng, col, k)) for k in ks]))
    return sets


def family_d(seed=14, n=320):
    """`X != K && ...` and `X == K || ...`."""
    rng = np.random.default_rng(seed)
    nodes = []
    for _ in range(n):
        col = _pick(rng, ["ai", "ai", "bi", "ad", "bd"])
        k = pick_k(rng, cls_of(col))
        tail = continuation(rng, col, k) if rng.random() < 0.7 else atom(rng)
        nodes.append(And(("ne", ("attr", col), k), tail) if rng.random() < 0.5 else Or(("eq", ("attr", col), k), tail))
    return [RuleSet("d", nodes)]


def family_e(seed=15, n=300):
    """The numeric composite `ai == K && bs.startsWith("ab")`, alone and with a tail."""
    rng = np.random.default_rng(seed)
    nodes = []
    for _ in range(n):
        k = pick_k(rng, "i")
        x = And(("eq", ("attr", "ai"), k), ("sw", "bs", _pick(rng, ["ab", "ab", "ab", "a", "abx", ""])))
        r = rng.random()
        if r < 0.2:
            x = And(x, ("eq", ("attr", "bi"), pick_k(rng, "i")))
        elif r < 0.35:
            x = And(x, ("eq", ("attr", "ad"), pick_k(rng, "d")))
        elif r < 0.45:
            x = And(x, ("eq", ("attr", "bs"), sconst("abx")))
        nodes.append(x)
    return [RuleSet("e", nodes)]


def family_f():
    """Value rules for Eval: `ai`, `ai | bi`, `ai | 4294967303`, `ad | 0.1`, ..."""
    ops = [("attr", "ai"), ("alt", "ai", "bi"), ("altk", "ai", iconst((1 << 32) + 7)), ("altk", "ad", dconst("0.1")),
           ("attr", "ad"), ("alt", "ad", "bd"), ("alt", "bi", "ai"), ("altk", "bd", dconst("1e-320")),
           ("altk", "bi", iconst((1 << 63) - 1)), ("altk", "ad", dconst("1.7976931348623157e+308")), ("attr", "bd"),
           ("altk", "bi", iconst(7 << 32))]
    return [RuleSet("f", [("val", op) for op in ops])]


FAMILIES = {"a": family_a, "b": family_b, "c": family_c, "d": family_d, "e": family_e}
