"""An independent reference for rules over string values, and the inputs designed for it.

Go strings are byte strings.  The reference interpreter compares them with `==`, and its three
string externs are three lines each (mixer/pkg/il/runtime/externs.go:108-128): startsWith is
strings.HasPrefix, endsWith is strings.HasSuffix, and match(s, p) is a prefix test on p[:-1] when p
ends in `*`, else a suffix test on p[1:] when p begins with `*`, else equality -- so "*a*" is the
literal prefix "*a", "**" the prefix "*", "*" is always true and "" matches only "".  This module
restates just that over Python `bytes`, for a small expression language, and imports neither the
oracle nor the product.

Rules are built forward, from tuples; `text()` renders a tuple as rule text and `RuleSet.evaluate`
computes the expected outcome from the tuple and the bags' bytes -- never by parsing the text.

    operand  ("attr", name) | ("k", Const) | ("idx", map name, operand) | ("or", operand, operand)
    atom     (op, operand, operand), op in "eq" "ne" "sw" "ew" "match" | ("ieq", name, int)
    rule     atom | ("and", r, r) | ("or2", r, r) | ("par", r) | ("val", operand)

Semantics restated: `&&` and `||` short-circuit; `a | b` falls back on absence only -- an absent
attribute or an absent map key -- and a value of the wrong dynamic kind is an error that never falls
back; an operand that stays absent is an error.  Outside a fallback `sm[k]` resolves its map and its
key strictly and gives "" for a key the map does not hold (compiler.go:396-409, the NLookup of
interpreterRun.go:1045-1124); as the left side of a fallback, an absent map, an absent key
attribute and a key the map does not hold all fall back (compiler.go:411-456).  A map attribute is
resolved as an interface value (ResolveF / TResolveF): that it is no string map shows only at the
lookup, after the key -- so `sm[as] | bs` over a wrongly typed `sm` falls back where `as` is absent.

Bag values are (kind, payload) pairs: ("string", bytes), ("map", {bytes: bytes}), ("int64", int),
("bool", bool), ("other", text), ("double", float), ("bytes", bytes).  `as_str` gives the `str` with
surrogate escapes that the product's bag model takes for a Go string.
"""
from collections import namedtuple

import numpy as np

# mixer/pkg/il/testing/tests.go:2414-2489 (defaultAttrs), the manifest the fuzz tests use
MANIFEST = {
    "ai": "INT64", "ab": "BOOL", "as": "STRING", "ad": "DOUBLE", "ar": "STRING_MAP", "adur": "DURATION",
    "at": "TIMESTAMP", "aip": "IP_ADDRESS", "bi": "INT64", "bb": "BOOL", "bs": "STRING", "bd": "DOUBLE",
    "br": "STRING_MAP", "bdur": "DURATION", "bt": "TIMESTAMP", "t1": "TIMESTAMP", "t2": "TIMESTAMP",
    "bip": "IP_ADDRESS", "b1": "BOOL", "b2": "BOOL", "sm": "STRING_MAP",
}
ATTRS = ("as", "bs", "sm", "ai")  # the attributes the designed bags carry
ACCEPTS = {"as": "string", "bs": "string", "sm": "map", "ai": "int64"}
N_REQUESTS = 4096 + 37
FALSE, TRUE, ERROR = 0, 1, 2

Const = namedtuple("Const", "text bytes")


def as_str(b):
    return b.decode("utf-8", "surrogateescape")


# ------------------------------------------------------------------------------------ literals
STYLES = ("plain", "u", "nt", "oct", "raw")


def _rune_at(b, i):
    """The length of the valid multi-byte UTF-8 sequence at b[i], or 0."""
    for k in (2, 3, 4):
        try:
            if len(b[i:i + k].decode("utf-8")) == 1:
                return k
        except UnicodeDecodeError:
            pass
    return 0


def literal(b, style="plain"):
    """A Go string literal for the bytes b.  Printable ASCII goes as is (the quote and the backslash
    as \\xNN), everything else as \\xNN; "u" spells a valid rune \\uXXXX, "nt" spells \\n and \\t,
    "oct" uses three-digit octal, "raw" a back-quoted literal where the bytes allow one."""
    assert style in STYLES
    if style == "raw" and b and all(0x20 <= c < 0x7F and c != 0x60 for c in b):
        return "`%s`" % b.decode("ascii")
    out, i = [], 0
    while i < len(b):
        c = b[i]
        if 0x20 <= c < 0x7F and c not in (0x22, 0x5C):
            out.append(chr(c))
        elif style == "u" and c >= 0x80 and _rune_at(b, i):
            k = _rune_at(b, i)
            cp = ord(b[i:i + k].decode("utf-8"))
            out.append("\\u%04x" % cp if cp < 0x10000 else "\\U%08x" % cp)
            i += k
            continue
        elif style == "nt" and c in (0x0A, 0x09):
            out.append("\\n" if c == 0x0A else "\\t")
        elif style == "oct":
            out.append("\\%03o" % c)
        else:
            out.append("\\x%02x" % c)
        i += 1
    return '"%s"' % "".join(out)


def K(rng, b):
    """A constant for the bytes b, spelled one of the ways above: half plain, an eighth each of the rest."""
    r = int(rng.integers(8))
    return Const(literal(b, STYLES[r - 3] if r >= 4 else "plain"), bytes(b))


# ------------------------------------------------------------------------------------ value pool
def _base(seed=7, n=300):
    """300 bytes over a 4-letter alphabet (so coincidences happen) with a few bytes >= 0x80 -- a valid
    rune (C3 A9) among them --, NULs, a newline and a tab."""
    rng = np.random.default_rng(seed)
    toks = [b"a", b"b", b"c", b"d", b"\xc3\xa9", b"\xff", b"\x80", b"\0", b"\n", b"\t"]
    p = np.array([22, 22, 21, 21, 4, 3, 2, 3, 1, 1], dtype=float)
    out = b""
    while len(out) < n:
        out += toks[int(rng.choice(len(toks), p=p / p.sum()))]
    out = bytearray(out[:n])
    out[13] = 0        # a NUL inside the second word of every value of 14 bytes and more
    out[17:19] = b"\xc3\xa9"
    out[29], out[61], out[290] = 0x0A, 0x09, 0xFF
    return bytes(out)


B = _base()
LENGTHS = [0, 1, 2, 7, 8, 9, 11, 12, 13, 15, 16, 17, 19, 20, 21, 23, 24, 25, 31, 32, 33, 63, 64, 65, 254, 255, 256,
           257, 300]
assert len(B) == 300 and B[13] == 0 and b"\xc3\xa9" in B and 0xFF in B and 0x0A in B and 0x09 in B


def flip(x, pos):
    """x with the byte at pos changed (to another letter of the alphabet)."""
    assert 0 <= pos < len(x)
    return x[:pos] + (b"b" if x[pos] == 0x61 else b"a") + x[pos + 1:]


def flip_positions(n):
    """0, 7, 8, n-8, n-1 and the two bytes around the start of the last partial word, where they exist."""
    return sorted({p for p in (0, 7, 8, n - 8, n - 1, 8 * (n // 8) - 1, 8 * (n // 8)) if 0 <= p < n})


def _pool():
    out = []
    for n in LENGTHS:
        v = B[:n]
        out += [v] + [flip(v, p) for p in flip_positions(n)] + [v + b"\0", v + b"z", b"q" + v]
    out += [b"*", b"*" + B[:5], b"*" + B[:12], B[:8] + b"*", b"*" + B[279:300]]
    seen = set()
    return [v for v in out if not (v in seen or seen.add(v))]


POOL = _pool()
H1, H2 = B[:21], B[:257]
# hot values: most of the mass, so that rules built around them are true -- and nearly true -- often
HOT = [(H1, 8), (H2, 3), (flip(H1, 20), 2), (H1 + b"\0", 2), (flip(H1, 0), 1), (B[:1], 1), (flip(H2, 256), 1),
       (b"q" + H1, 1), (B[:12] + b"*", 1), (b"*" + B[249:257], 1), (b"*" + B[:5], 1)]
HOT_VALUES = [v for v, _ in HOT]
_HOT_P = np.array([w for _, w in HOT], dtype=float) / sum(w for _, w in HOT)
# map keys: "k" and "k\0"; 9- and 21-byte keys that differ in their last byte only (the 21-byte ones
# are hot values of `as`, so sm[as] finds them)
KEYS = [b"k", b"k\0", B[:9], flip(B[:9], 8), H1, flip(H1, 20)]
WRONG = {"string": [("int64", 3), ("bool", True), ("other", "20"), ("map", {b"a": b"b"}), ("double", 1.5),
                    ("bytes", b"\x01")],
         "map": [("string", b"str"), ("int64", 3), ("bool", True), ("other", "20"), ("bytes", b"\x01")],
         "int64": [("string", b"str"), ("bool", True), ("other", "20"), ("double", 1.5), ("map", {b"a": b"b"})]}


def _pick(rng, xs):
    return xs[int(rng.integers(len(xs)))]


def hot(rng):
    return HOT_VALUES[int(rng.choice(len(HOT_VALUES), p=_HOT_P))]


def make_bags(n=N_REQUESTS, seed=1, p_missing=0.25, p_wrong=0.05, p_hot=0.8):
    """Bags over ATTRS: string values hot (p_hot of the mass) or spread over the pool; absent and
    wrongly typed values as numeric_ref.make_bags draws them; `sm` holds each of KEYS six times in
    ten, its values drawn like the string attributes'; `ai` is 0..3."""
    rng = np.random.default_rng(seed)

    def value():
        return hot(rng) if rng.random() < p_hot else _pick(rng, POOL)
    bags = []
    for _ in range(n):
        b = {}
        for name in ATTRS:
            if rng.random() < p_missing:
                continue
            kind = ACCEPTS[name]
            if rng.random() < p_wrong:
                b[name] = _pick(rng, WRONG[kind])
            elif kind == "string":
                b[name] = ("string", value())
            elif kind == "map":
                b[name] = ("map", {k: value() for k in KEYS if rng.random() < 0.6})
            else:
                b[name] = ("int64", int(rng.integers(4)))
        bags.append(b)
    return bags


SHARED24 = B[40:64]


def make_distinct_bags(n=N_REQUESTS, seed=3):
    """A string column that is nearly all distinct: `as` is 24 shared bytes, then a decimal counter
    (so every value ends in a partial word); `bs` equals `as` on half the requests and differs from it
    in one byte of that last partial word on the rest; `sm` maps the request's own `as` one time in two."""
    rng = np.random.default_rng(seed)
    bags = []
    for i in range(n):
        a = SHARED24 + b"%d" % (i - i % 16 if rng.random() < 0.1 else i)   # (a few repeats)
        b = {"as": ("string", a)}
        if rng.random() < 0.5:
            b["bs"] = ("string", a)
        else:
            pos = 24 + int(rng.integers(len(a) - 24))
            b["bs"] = ("string", a[:pos] + (b"x" if a[pos] != 0x78 else b"y") + a[pos + 1:])
        if rng.random() < 0.5:
            b["sm"] = ("map", {a: b"v", b"k": a})
        if rng.random() < 0.1:
            del b["as" if rng.random() < 0.5 else "bs"]
        bags.append(b)
    return bags


# ------------------------------------------------------------------------------------ comparators
class Exact:
    """The semantics themselves."""
    name = "exact"

    def eq(self, a, b):
        return a == b

    def sw(self, s, p):
        return s.startswith(p)

    def ew(self, s, p):
        return s.endswith(p)

    def match(self, s, p):
        if p.endswith(b"*"):
            return self.sw(s, p[:-1])
        if p.startswith(b"*"):
            return self.ew(s, p[1:])
        return self.eq(s, p)


def _region(op, s, p):
    """The bytes of s that op compares with p, or None where the lengths already decide."""
    if op == "eq":
        return s if len(s) == len(p) else None
    if len(s) < len(p):
        return None
    return s[:len(p)] if op == "sw" else s[len(s) - len(p):]


class First8(Exact):
    """Compares the first 8 bytes only (a compare that is wrong from the second word on)."""
    name = "first8"

    def _cmp(self, op, s, p):
        a = _region(op, s, p)
        return a is not None and a[:8] == p[:8]

    def eq(self, a, b):
        return self._cmp("eq", a, b)

    def sw(self, s, p):
        return self._cmp("sw", s, p)

    def ew(self, s, p):
        return self._cmp("ew", s, p)


class NoTail(First8):
    """Ignores the last partial word."""
    name = "notail"

    def _cmp(self, op, s, p):
        a = _region(op, s, p)
        return a is not None and a[:len(p) & ~7] == p[:len(p) & ~7]


class Mod256(Exact):
    """Compares lengths modulo 256 (a length tag of 8 bits): equal where the lengths agree modulo 256
    and the bytes of the shorter agree; a prefix of L bytes is tested as one of L % 256."""
    name = "mod256"

    def eq(self, a, b):
        k = min(len(a), len(b))
        return len(a) % 256 == len(b) % 256 and a[:k] == b[:k]

    def sw(self, s, p):
        return s.startswith(p[:len(p) % 256])


class Floor8(Exact):
    """Takes the suffix at the offset rounded down to 8."""
    name = "floor8"

    def ew(self, s, p):
        off = (len(s) - len(p)) & ~7
        return len(s) >= len(p) and s[off:off + len(p)] == p


class NoLen(Exact):
    """A prefix test without the length check."""
    name = "nolen"

    def sw(self, s, p):
        k = min(len(s), len(p))
        return s[:k] == p[:k]


class StarAnywhere(Exact):
    """Treats a `*` anywhere in the pattern as a wildcard."""
    name = "star"

    def match(self, s, p):
        parts = p.split(b"*")
        if len(parts) == 1:
            return s == p
        if not s.startswith(parts[0]):
            return False
        at = len(parts[0])
        for mid in parts[1:-1]:
            j = s.find(mid, at)
            if j < 0:
                return False
            at = j + len(mid)
        return len(s) - at >= len(parts[-1]) and s.endswith(parts[-1])


class StopAtNul(Exact):
    """Stops at the first NUL."""
    name = "nul"

    @staticmethod
    def _c(x):
        return x.split(b"\0")[0]

    def eq(self, a, b):
        return self._c(a) == self._c(b)

    def sw(self, s, p):
        return self._c(s).startswith(self._c(p))

    def ew(self, s, p):
        return self._c(s).endswith(self._c(p))


# each wrong comparator and the families it bears on
WRONG_COMPARATORS = [(First8(), "abcde"), (NoTail(), "abcde"), (Mod256(), "ab"), (Floor8(), "cde"), (NoLen(), "bd"),
                     (StarAnywhere(), "de"), (StopAtNul(), "abcde")]

ONE_BYTE, FIRST8, LENGTH_ONLY = 1, 2, 4


def near_miss(op, s, p):
    """How a false compare of s with p is nearly true: ONE_BYTE -- the compared bytes differ in one
    byte; FIRST8 -- they agree in their first 8 bytes (and are longer); LENGTH_ONLY -- the operands
    agree in every byte of the shorter and differ in length only."""
    if op == "ne":
        op = "eq"
    if op == "match":
        if p.endswith(b"*"):
            op, p = "sw", p[:-1]
        elif p.startswith(b"*"):
            op, p = "ew", p[1:]
        else:
            op = "eq"
    if getattr(Exact(), op)(s, p):
        return 0
    a = _region(op, s, p)
    if a is None:
        short, long_ = (s, p) if len(s) < len(p) else (p, s)
        same = long_.endswith(short) if op == "ew" else long_.startswith(short)
        return LENGTH_ONLY if same else 0
    out = 0
    if sum(x != y for x, y in zip(a, p)) == 1:
        out |= ONE_BYTE
    if len(p) > 8 and a[:8] == p[:8]:
        out |= FIRST8
    return out


# ------------------------------------------------------------------------------------ rule text
def And(a, b):
    if a[0] == "or2":
        a = ("par", a)
    if b[0] in ("and", "or2"):
        b = ("par", b)
    return ("and", a, b)


def Or(a, b):
    if b[0] in ("and", "or2"):
        b = ("par", b)
    return ("or2", a, b)


def attr(name):
    return ("attr", name)


def _operand_text(op, bare=False):
    if op[0] == "attr":
        return op[1]
    if op[0] == "k":
        return op[1].text
    if op[0] == "idx":
        return "%s[%s]" % (op[1], _operand_text(op[2]))
    s = "%s | %s" % (_operand_text(op[1]), _operand_text(op[2], bare=True))
    return s if bare else "(%s)" % s


def text(node):
    t = node[0]
    if t in ("eq", "ne"):
        return "%s %s %s" % (_operand_text(node[1]), "==" if t == "eq" else "!=", _operand_text(node[2]))
    if t in ("sw", "ew"):
        return "%s.%s(%s)" % (_operand_text(node[1]), "startsWith" if t == "sw" else "endsWith", _operand_text(node[2]))
    if t == "match":
        return "match(%s, %s)" % (_operand_text(node[1]), _operand_text(node[2]))
    if t == "ieq":
        return "%s == %d" % (node[1], node[2])
    if t == "and":
        return "%s && %s" % (text(node[1]), text(node[2]))
    if t == "or2":
        return "%s || %s" % (text(node[1]), text(node[2]))
    if t == "par":
        return "(%s)" % text(node[1])
    if t == "val":
        return _operand_text(node[1], bare=True)
    raise ValueError(t)


STRING_OPS = ("eq", "ne", "sw", "ew", "match")


def constants(node):
    """The constants of a rule in text order."""
    if isinstance(node, Const):
        return [node]
    return [c for x in node[1:] if isinstance(x, (tuple, Const)) for c in constants(x)]


# ------------------------------------------------------------------------------------ one pair, plain Python
def _get(bag, name):
    """-> ("ok", payload) | ("absent",) | ("error",)"""
    if name not in bag:
        return ("absent",)
    kind, payload = bag[name]
    return ("ok", payload) if kind == ACCEPTS[name] else ("error",)


def _operand_one(op, bag, strict=True):
    """strict: outside a fallback, where absence is an error (and a key the map lacks gives "")."""
    t = op[0]
    if t == "k":
        return ("ok", op[1].bytes)
    if t == "or":
        a = _operand_one(op[1], bag, strict=False)
        return _operand_one(op[2], bag, strict) if a[0] == "absent" else a
    if t == "attr":
        r = _get(bag, op[1])
    else:
        r = ("absent",)
        if op[1] in bag:
            k = _operand_one(op[2], bag, strict)
            m = _get(bag, op[1])
            if k[0] != "ok" or m[0] != "ok":
                return k if k[0] != "ok" else m
            r = ("ok", m[1][k[1]]) if k[1] in m[1] else ("ok", b"") if strict else ("absent",)
    return ("error",) if strict and r[0] == "absent" else r


def eval_one(node, bag, cmp=Exact()):
    """EvalPredicate of one rule on one bag -> FALSE | TRUE | ERROR; for a ("val", ..) rule ->
    (ERROR, None) | (FALSE, bytes)."""
    t = node[0]
    if t in STRING_OPS:
        a = _operand_one(node[1], bag)
        if a[0] != "ok":
            return ERROR
        b = _operand_one(node[2], bag)
        if b[0] != "ok":
            return ERROR
        hit = getattr(cmp, "eq" if t == "ne" else t)(a[1], b[1])
        return int(hit != (t == "ne"))
    if t == "ieq":
        a = _get(bag, node[1])
        return int(a[1] == node[2]) if a[0] == "ok" else ERROR
    if t == "par":
        return eval_one(node[1], bag, cmp)
    if t == "val":
        a = _operand_one(node[1], bag)
        return (FALSE, a[1]) if a[0] == "ok" else (ERROR, None)
    a = eval_one(node[1], bag, cmp)
    if a == ERROR or a == (FALSE if t == "and" else TRUE):
        return a
    return eval_one(node[2], bag, cmp)


# ------------------------------------------------------------------------------------ a batch, by column
NA, OK, ABSENT, BAD = 0, 1, 2, 3  # the state of an operand on a request


class Columns:
    """The bags by column.  Byte strings are interned (`pool`, `intern`): a string column holds ids."""

    def __init__(self, bags):
        self.n = len(bags)
        self.pool, self._ids = [], {}
        self.state = {name: np.full(self.n, ABSENT, dtype=np.uint8) for name in ATTRS}
        self.value = {name: np.zeros(self.n, dtype=np.int64) for name in ATTRS}
        self.maps = []
        for q, b in enumerate(bags):
            for name, (kind, payload) in b.items():
                if kind != ACCEPTS[name]:
                    self.state[name][q] = BAD
                    continue
                self.state[name][q] = OK
                if kind == "string":
                    self.value[name][q] = self.intern(payload)
                elif kind == "map":
                    self.value[name][q] = len(self.maps)
                    self.maps.append({self.intern(k): self.intern(v) for k, v in payload.items()})
                else:
                    self.value[name][q] = payload

    def intern(self, b):
        i = self._ids.get(b)
        if i is None:
            i = self._ids[b] = len(self.pool)
            self.pool.append(b)
        return i


def _by_pairs(fn, ia, ib, where, dtype):
    """fn(a, b) over the distinct (ia, ib) pairs of the requests in `where`."""
    out = np.zeros(len(ia), dtype=dtype)
    if where.any():
        key = ia[where] * (1 << 32) + ib[where]
        uniq, inv = np.unique(key, return_inverse=True)
        out[where] = np.array([fn(int(k) >> 32, int(k) & 0xFFFFFFFF) for k in uniq], dtype=dtype)[inv]
    return out


class _Run:
    def __init__(self, cols, cmp, focus=None):
        self.c, self.cmp, self.focus_node, self.focus = cols, cmp, focus, None

    def operand(self, op, active, strict=True):
        """-> (state u8 [n] (NA where not active; never ABSENT when strict), ids i64 [n])"""
        c, t = self.c, op[0]
        if t == "k":
            return np.where(active, OK, NA).astype(np.uint8), np.full(c.n, c.intern(op[1].bytes), dtype=np.int64)
        if t == "or":
            sa, ia = self.operand(op[1], active, strict=False)
            sb, ib = self.operand(op[2], sa == ABSENT, strict)
            return np.where(sa == ABSENT, sb, sa).astype(np.uint8), np.where(sa == ABSENT, ib, ia)
        if t == "attr":
            st, ids = np.where(active, c.state[op[1]], NA).astype(np.uint8), c.value[op[1]]
        else:
            sm, im = self.operand(("attr", op[1]), active, strict=False)
            there = (sm == OK) | (sm == BAD)
            sk, ik = self.operand(op[2], there, strict)
            look = (sk == OK) & (sm == OK)
            found = _by_pairs(lambda m, k: c.maps[m].get(k, -1), im, ik, look, np.int64)
            miss = c.intern(b"") if strict else -1
            st = np.where(~there, sm, np.where(sk != OK, sk, np.where(sm == BAD, BAD, np.where((found >= 0) | strict, OK, ABSENT))))
            st = st.astype(np.uint8)
            ids = np.where(found >= 0, found, max(miss, 0))
        return (np.where(st == ABSENT, BAD, st).astype(np.uint8) if strict else st), ids

    def node(self, node, active):
        """-> codes (FALSE where not active)"""
        c, t = self.c, node[0]
        if t in STRING_OPS:
            sa, ia = self.operand(node[1], active)
            sb, ib = self.operand(node[2], sa == OK)
            ok = sb == OK
            if node is self.focus_node:
                self.focus = (ok, ia, ib)
            fn = getattr(self.cmp, "eq" if t == "ne" else t)
            hit = _by_pairs(lambda a, b: fn(c.pool[a], c.pool[b]), ia, ib, ok, bool)
            if t == "ne":
                hit = ~hit
            return np.where(active & ~ok, ERROR, np.where(ok & hit, TRUE, FALSE)).astype(np.uint8)
        if t == "ieq":
            st = c.state[node[1]]
            return np.where(active & (st != OK), ERROR,
                            np.where(active & (c.value[node[1]] == node[2]), TRUE, FALSE)).astype(np.uint8)
        if t == "par":
            return self.node(node[1], active)
        a = self.node(node[1], active)
        go = active & (a == (TRUE if t == "and" else FALSE))
        b = self.node(node[2], go)
        return np.where(go, b, a).astype(np.uint8)


def focus_atom(node):
    """The string atom a rule is about: the last one in text order (behind its guards)."""
    if node[0] in STRING_OPS:
        return node
    for x in reversed(node[1:]):
        if isinstance(x, tuple):
            f = focus_atom(x)
            if f is not None:
                return f
    return None


class RuleSet:
    def __init__(self, name, nodes):
        self.name = name
        self.nodes = list(nodes)
        self.rules = [text(x) for x in self.nodes]

    def evaluate(self, cols, cmp=Exact()):
        """-> codes u8 [n, R] (EvalPredicate)."""
        every = np.ones(cols.n, dtype=bool)
        return np.stack([_Run(cols, cmp).node(x, every) for x in self.nodes], axis=1)

    def values(self, cols):
        """Eval of ("val", operand) rules -> (ok bool [n, R], ids i64 [n, R] into cols.pool)."""
        every = np.ones(cols.n, dtype=bool)
        out = [_Run(cols, Exact()).operand(x[1], every) for x in self.nodes]
        return np.stack([o[0] == OK for o in out], axis=1), np.stack([o[1] for o in out], axis=1)

    def near_misses(self, cols):
        """Per rule's focus atom, where it ran on two strings: (ran bool [n, R], kinds u8 [n, R]) --
        kinds the near_miss() of its operands (0 where it is true or not near)."""
        every = np.ones(cols.n, dtype=bool)
        ran, kinds = [], []
        for x in self.nodes:
            f = focus_atom(x)
            run = _Run(cols, Exact(), focus=f)
            run.node(x, every)
            ok, ia, ib = run.focus if run.focus is not None else (np.zeros(cols.n, dtype=bool),) * 3
            ran.append(ok)
            kinds.append(_by_pairs(lambda a, b: near_miss(f[0], cols.pool[a], cols.pool[b]), ia, ib, ok, np.uint8))
        return np.stack(ran, axis=1), np.stack(kinds, axis=1)


# ------------------------------------------------------------------------------------ families
def related(rng, op, h):
    """A comparand for `op` built around the value h: one that makes the compare true, one that
    misses by one byte, one that agrees in the first 8 bytes, one that differs in length only, or any
    value or pattern of the pool."""
    n = len(h)
    r = rng.random()
    ms = [m for m in LENGTHS if 0 < m <= n]
    if op == "eq":
        if r < 0.3 or n == 0:
            return h
        if r < 0.5:
            return flip(h, _pick(rng, flip_positions(n)))
        if r < 0.65 and n > 8:
            return flip(h, _pick(rng, [p for p in flip_positions(n) if p >= 8]))
        if r < 0.85:
            return _pick(rng, [h + b"\0", h + b"z", h[:-1], h[:n & ~7], B[:n % 256] if h == B[:n] else h[:8],
                               B[:n + 256] if h == B[:n] and n + 256 <= 300 else h + b"\0"])
        return _pick(rng, POOL)
    if op in ("sw", "ew") and not ms:
        return _pick(rng, [b"", B[:1], b"q"])
    if op == "sw":
        m = _pick(rng, ms)
        if r < 0.3:
            return h[:m]
        if r < 0.5:
            return flip(h[:m], _pick(rng, [0, m - 1]))
        if r < 0.65:
            m = _pick(rng, [x for x in ms if x > 8] or ms)
            return flip(h[:m], m - 1 if m > 8 else 0)
        if r < 0.85:
            longer = [B[:x] for x in LENGTHS if x > n] if h == B[:n] else []
            return _pick(rng, longer + [h + b"\0", h + b"z"])
        m = _pick(rng, LENGTHS)
        return _pick(rng, [B[:m], flip(B[:m], m - 1) if m else b"q", B[:m] + b"z"])
    if op == "ew":
        m = _pick(rng, ms)
        if r < 0.3:
            return h[n - m:]
        if r < 0.5:
            return flip(h[n - m:], _pick(rng, [0, m - 1]))
        if r < 0.65:
            m = _pick(rng, [x for x in ms if x > 8] or ms)
            return flip(h[n - m:], m - 1 if m > 8 else 0)
        if r < 0.85:
            return _pick(rng, [b"q" + h, b"\0" + h, B[:3] + h])
        m = _pick(rng, LENGTHS)
        return _pick(rng, [B[300 - m:], B[:m], b"q" + B[300 - m:]])
    assert op == "match"
    shape = int(rng.integers(8))
    if shape < 3:
        return related(rng, "sw", h) + b"*"
    if shape < 6:
        return b"*" + related(rng, "ew", h)
    if shape == 6:
        return related(rng, "eq", h)
    return _pick(rng, [b"*" + related(rng, "sw", h) + b"*", b"*" + B[1:2] + b"*", b"**", b"*", b""])


def _x(rng):
    return _pick(rng, ["as", "as", "bs"])


def family_a(seed=21, n=320):
    """`X == K`, `X != K`, `as == bs`, `sm["K"] == K2`, `sm[as] == K`, `(as | "K") == K2`."""
    rng = np.random.default_rng(seed)
    nodes = []
    for _ in range(n):
        r = rng.random()
        k = K(rng, related(rng, "eq", hot(rng)))
        if r < 0.3:
            x = ("eq", attr(_x(rng)), ("k", k))
        elif r < 0.4:
            x = ("ne", attr(_x(rng)), ("k", k))
        elif r < 0.5:
            x = ("eq", attr("as"), attr("bs")) if rng.random() < 0.7 else ("ne", attr("bs"), attr("as"))
        elif r < 0.7:
            x = ("eq", ("idx", "sm", ("k", K(rng, _pick(rng, KEYS)))), ("k", k))
        elif r < 0.85:
            x = ("eq", ("idx", "sm", attr("as")), ("k", k))
        else:
            x = ("eq", ("or", attr("as"), ("k", K(rng, hot(rng)))), ("k", k))
        nodes.append(x)
    return [RuleSet("a", nodes)]


def _tail(rng):
    return ("ieq", "ai", int(rng.integers(4)))


def family_b(seed=22, n=240):
    """`X.startsWith(P)`, P a constant or an attribute, alone and as `as == K && bs.startsWith(P)
    [&& tail]`.  Every head B[:m] of the length list is there alone and behind `as == H1`: among
    them the 12/13, 20/21, 24 and 255/256/257 bytes of the composite and prefix index boundaries
    (the 256- and 257-byte keys share their first 255 bytes with the 255-byte key)."""
    rng = np.random.default_rng(seed)
    nodes = []
    for m in LENGTHS[1:]:
        nodes.append(("sw", attr("bs"), ("k", K(rng, B[:m]))))
        nodes.append(And(("eq", attr("as"), ("k", K(rng, H1))), ("sw", attr("bs"), ("k", K(rng, B[:m])))))
    for _ in range(n):
        r = rng.random()
        x = _x(rng)
        if r < 0.4:
            node = ("sw", attr(x), ("k", K(rng, related(rng, "sw", hot(rng)))))
        elif r < 0.5:
            node = ("sw", attr(x), attr("bs" if x == "as" else "as"))
        else:
            guard = ("eq", attr("as"), ("k", K(rng, H1 if rng.random() < 0.7 else related(rng, "eq", hot(rng)))))
            node = And(guard, ("sw", attr("bs"), ("k", K(rng, related(rng, "sw", hot(rng))))))
            if r > 0.8:
                node = And(node, _tail(rng))
        nodes.append(node)
    return [RuleSet("b", nodes)]


def family_c(seed=23, n=240):
    """`X.endsWith(P)`: the tails of the two hot values at every length 1..24, so that the compare
    starts at every offset (n - m) & 7 of its subject, and patterns related to the hot values."""
    rng = np.random.default_rng(seed)
    nodes = []
    for h in (H1, H2):
        for m in range(1, 25):
            if m <= len(h):
                nodes.append(("ew", attr(_x(rng)), ("k", K(rng, h[len(h) - m:]))))
    for _ in range(n):
        x = _x(rng)
        if rng.random() < 0.85:
            nodes.append(("ew", attr(x), ("k", K(rng, related(rng, "ew", hot(rng))))))
        else:
            nodes.append(("ew", attr(x), attr("bs" if x == "as" else "as")))
    return [RuleSet("c", nodes)]


def family_d(seed=24, n=320):
    """`match(X, P)` in all four star shapes, P a constant or an attribute."""
    rng = np.random.default_rng(seed)
    nodes = []
    for p in (b"*" + B[1:2] + b"*", b"**", b"*", b"", b"*" + B[:1] + b"*"):
        for x in ("as", "bs"):
            nodes.append(("match", attr(x), ("k", K(rng, p))))
    for _ in range(n):
        x = _x(rng)
        if rng.random() < 0.85:
            nodes.append(("match", attr(x), ("k", K(rng, related(rng, "match", hot(rng))))))
        else:
            nodes.append(("match", attr(x), attr("bs" if x == "as" else "as")))
    return [RuleSet("d", nodes)]


def family_e(seed=25, n=320):
    """The string function as a continuation behind a guard index: `as == K && bs.endsWith(P)` and
    `ai == k || match(bs, P)`."""
    rng = np.random.default_rng(seed)
    nodes = []
    for _ in range(n):
        if rng.random() < 0.5:
            guard = ("eq", attr("as"), ("k", K(rng, H1 if rng.random() < 0.9 else related(rng, "eq", hot(rng)))))
            nodes.append(And(guard, ("ew", attr("bs"), ("k", K(rng, related(rng, "ew", hot(rng)))))))
        else:
            nodes.append(Or(_tail(rng), ("match", attr("bs"), ("k", K(rng, related(rng, "match", hot(rng)))))))
    return [RuleSet("e", nodes)]


def family_f(seed=26):
    """Value rules for Eval: `as`, `as | bs`, `as | "K"`, `sm["K"] | "d"`."""
    rng = np.random.default_rng(seed)
    ops = [attr("as"), ("or", attr("as"), attr("bs")), ("or", attr("as"), ("k", K(rng, B))), attr("bs"),
           ("or", attr("bs"), ("k", K(rng, H1 + b"\0"))), ("or", attr("bs"), attr("as")),
           ("or", attr("as"), ("k", Const(literal(b"\xc3\xa9\xff\n\t\0", "u"), b"\xc3\xa9\xff\n\t\0")))]
    ops += [("or", ("idx", "sm", ("k", K(rng, k))), ("k", K(rng, d))) for k, d in zip(KEYS, [b"d", b"", B[:255], b"d\0", H2, b"d"])]
    ops += [("idx", "sm", attr("as")), ("or", ("idx", "sm", attr("as")), attr("bs"))]
    return [RuleSet("f", [("val", op) for op in ops])]


def family_n(seed=27):
    """Rules for the nearly-distinct column (make_distinct_bags)."""
    rng = np.random.default_rng(seed)
    a, b = attr("as"), attr("bs")
    nodes = [("eq", a, b), ("ne", a, b), ("sw", b, a), ("ew", a, b), ("match", a, b), ("eq", ("or", a, b), b),
             ("eq", ("idx", "sm", a), ("k", K(rng, b"v"))), ("eq", ("idx", "sm", ("k", K(rng, b"k"))), b),
             ("sw", a, ("k", K(rng, SHARED24))), ("sw", b, ("k", K(rng, SHARED24 + b"1"))),
             ("ew", b, ("k", K(rng, b"7"))), ("match", b, ("k", K(rng, SHARED24 + b"40*")))]
    nodes += [("eq", _pick(rng, [a, b]), ("k", K(rng, SHARED24 + b"%d" % int(rng.integers(N_REQUESTS))))) for _ in range(52)]
    return [RuleSet("n", nodes)]


FAMILIES = {"a": family_a, "b": family_b, "c": family_c, "d": family_d, "e": family_e}
