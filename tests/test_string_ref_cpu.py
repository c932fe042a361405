"""String values on the host: the designed inputs of string_ref.py meet their conditions, each
deliberately wrong comparator of that module answers differently on every family it bears on, the
batch blob holds long strings at every alignment, the oracle agrees with that independent reference
on every family, and the product's compiler carries every string constant, however it is spelled,
byte for byte into the rule-set pool."""
import ctypes
import re

import numpy as np
import pytest

import oracle
import string_ref as SR
from istio_amd.bags import BagBatch, GoFloat64, GoInt64, GoOther


def to_go(value):
    """A (kind, payload) bag value of string_ref as the product's Go value model."""
    kind, p = value
    if kind == "string":
        return SR.as_str(p)
    if kind == "map":
        return {SR.as_str(k): SR.as_str(v) for k, v in p.items()}
    if kind == "int64":
        return GoInt64(p)
    if kind == "double":
        return GoFloat64(p)
    if kind == "other":
        return GoOther(p)
    return p  # bool, bytes


def to_batch(bags):
    return BagBatch.from_bags([{k: to_go(v) for k, v in b.items()} for b in bags], names=list(SR.MANIFEST))


class Case:
    """The designed batches, shared by every test of a session: bags, columns, BagBatch, and per rule
    set the reference's codes (computed once, never changed).  `near` is the nearly-distinct column."""
    _one = None

    def __init__(self):
        self.bags = SR.make_bags()
        self.cols = SR.Columns(self.bags)
        self.batch = to_batch(self.bags)
        self.sets = {f: make() for f, make in SR.FAMILIES.items()}
        self.sets["f"] = SR.family_f()
        self.sets["n"] = SR.family_n()
        self.near_bags = SR.make_distinct_bags()
        self.near_cols = SR.Columns(self.near_bags)
        self.near_batch = to_batch(self.near_bags)
        self._ref = {}

    @classmethod
    def get(cls):
        if cls._one is None:
            cls._one = cls()
        return cls._one

    def inputs(self, fam):
        """(bags, columns, batch) a family runs on."""
        return (self.near_bags, self.near_cols, self.near_batch) if fam == "n" else (self.bags, self.cols, self.batch)

    def ref(self, rs):
        if rs.name not in self._ref:
            self._ref[rs.name] = rs.evaluate(self.inputs(rs.name)[1])
        return self._ref[rs.name]

    def ref_values(self, rs):
        """Eval of value rules: (ok bool [n, R], payload bytes as an object array [n, R])."""
        cols = self.inputs(rs.name)[1]
        ok, ids = rs.values(cols)
        return ok, np.array(cols.pool + [b""], dtype=object)[np.where(ok, ids, len(cols.pool))]


@pytest.fixture(scope="module")
def case():
    return Case.get()


@pytest.fixture(scope="module")
def host(libmxp):
    from istio_amd.engine import Engine

    def compiled(rules):
        e = Engine(-1)
        e.set_vocabulary(SR.MANIFEST)
        return e, e.compile(rules)
    return compiled


FAMS = ["a", "b", "c", "d", "e"]


@pytest.mark.parametrize("fam", FAMS)
def test_inputs_meet_their_conditions(case, fam):
    """On the reference alone: the true pairs, the error pairs and the false pairs of each near-miss
    kind -- the operands equal except one byte, equal in their first 8 bytes, equal in every byte of
    the shorter -- are each >= 2 % of the family's pairs; the true and the near ones also >= 500."""
    true = err = pairs = 0
    near = {SR.ONE_BYTE: 0, SR.FIRST8: 0, SR.LENGTH_ONLY: 0}
    for rs in case.sets[fam]:
        assert len(rs.rules) <= 400
        codes = case.ref(rs)
        ran, kinds = rs.near_misses(case.cols)
        assert not kinds[~ran].any()
        for k in near:
            near[k] += int(((kinds & k) != 0).sum())
        true += int((codes == SR.TRUE).sum())
        err += int((codes == SR.ERROR).sum())
        pairs += codes.size
    print("family %s: %d pairs, true %d, error %d, one byte %d, first 8 %d, length only %d" % (
        fam, pairs, true, err, near[SR.ONE_BYTE], near[SR.FIRST8], near[SR.LENGTH_ONLY]))
    for k in [true] + list(near.values()):
        assert k >= 500 and k >= 0.02 * pairs
    assert err >= 0.02 * pairs


@pytest.mark.parametrize("cmp,fams", SR.WRONG_COMPARATORS, ids=[c.name for c, _ in SR.WRONG_COMPARATORS])
def test_wrong_comparators_are_caught(case, cmp, fams):
    """A kernel that compared as one of the wrong comparators does would answer differently from the
    reference on at least 100 pairs of every family the comparator bears on."""
    for fam in fams:
        diff = sum(int((rs.evaluate(case.cols, cmp) != case.ref(rs)).sum()) for rs in case.sets[fam])
        print("%s on family %s: %d pairs differ" % (cmp.name, fam, diff))
        assert diff >= 100, (cmp.name, fam, diff)


def _consts(rs, op):
    return [x[2][1].bytes for node in rs.nodes for x in [SR.focus_atom(node)] if x[0] == op and x[2][0] == "k"]


def test_family_shapes(case):
    """The boundaries the families are there for."""
    b = case.sets["b"][0]
    lens = {len(p) for p in _consts(b, "sw")}
    assert {1, 8, 9, 12, 13, 20, 21, 24, 255, 256, 257, 300} <= lens
    composite = {len(SR.focus_atom(x)[2][1].bytes) for x in b.nodes if x[0] == "and"}
    assert {12, 13, 20, 21, 24, 255, 256, 257} <= composite
    # (c): true pairs of more than one word whose compare starts at every offset (n - m) & 7 of the subject
    c = case.sets["c"][0]
    codes = case.ref(c)
    seen = set()
    for r, node in enumerate(c.nodes):
        at = SR.focus_atom(node)
        if at[2][0] == "k" and len(at[2][1].bytes) >= 9:
            col = case.cols.value[at[1][1]][codes[:, r] == SR.TRUE]
            seen |= {(len(case.cols.pool[i]) - len(at[2][1].bytes)) & 7 for i in set(col.tolist())}
    assert seen == set(range(8)), seen
    # (d): all four star shapes, the degenerate patterns, and attribute patterns
    pats = _consts(case.sets["d"][0], "match")
    shapes = {(p.startswith(b"*"), p.endswith(b"*") and len(p) > 1) for p in pats if p}
    assert len(shapes) == 4 and {b"*", b"**", b"", b"*" + SR.B[1:2] + b"*"} <= set(pats)
    assert any(SR.focus_atom(x)[2][0] == "attr" for x in case.sets["d"][0].nodes)
    assert any(x[0] == "and" for x in case.sets["e"][0].nodes) and any(x[0] == "or2" for x in case.sets["e"][0].nodes)
    # every spelling of a constant is used
    texts = " ".join(r for f in "abcdef" for rs in case.sets[f] for r in rs.rules)
    for spelled in ("\\u00e9", "\\n", "\\t", "\\000", "\\303\\251", "\\xff", "\\x00", "`"):
        assert spelled in texts, spelled
    assert case.sets["f"][0].rules[:2] == ["as", "as | bs"] and 'sm["k"] | "d"' in case.sets["f"][0].rules
    # the pool: every length, each with its one-byte neighbours and its extensions by a NUL and a letter
    for n in SR.LENGTHS:
        v = SR.B[:n]
        assert {v, v + b"\0", v + b"z", b"q" + v} <= set(SR.POOL)
        assert {SR.flip(v, p) for p in SR.flip_positions(n)} <= set(SR.POOL)
    assert {b"k", b"k\0"} <= set(SR.KEYS) and sorted(len(k) for k in SR.KEYS) == [1, 2, 9, 9, 21, 21]


def test_literal_writer():
    """Each spelling of a constant denotes the constant's bytes (read back as a Python bytes literal,
    a \\uXXXX rewritten as its UTF-8 bytes)."""
    import ast
    used = set()
    for v in SR.POOL + SR.KEYS + [b"\"\\`", b"`", b"\xc3\xa9\xff\n\t\0", bytes(range(256))]:
        for style in SR.STYLES:
            t = SR.literal(v, style)
            used.add(t[0])
            if t[0] == "`":
                assert t[1:-1].encode() == v and "`" not in t[1:-1]
                continue
            assert all(0x20 <= ord(ch) < 0x7F for ch in t)
            body = re.sub(r"\\u([0-9a-f]{4})", lambda m: "".join("\\x%02x" % x for x in chr(int(m.group(1), 16)).encode()), t)
            assert ast.literal_eval("b" + body) == v, (v, style, t)
    assert used == {'"', "`"}


def test_vector_reference_equals_plain_python(case):
    """The column-wise evaluation against the pair-at-a-time one over plain bytes."""
    rng = np.random.default_rng(5)
    for fam in FAMS + ["n"]:
        bags, cols, _ = case.inputs(fam)
        for rs in case.sets[fam]:
            codes = case.ref(rs)
            for q in rng.choice(cols.n, 40, replace=False):
                for r, node in enumerate(rs.nodes):
                    assert SR.eval_one(node, bags[q]) == codes[q, r], (rs.rules[r], bags[q])
    f = case.sets["f"][0]
    ok, vals = case.ref_values(f)
    for q in range(0, case.cols.n, 7):
        for r, node in enumerate(f.nodes):
            c, v = SR.eval_one(node, case.bags[q])
            assert (c == SR.FALSE) == ok[q, r] and (v is None or v == vals[q, r])


def test_blob_alignment(case):
    """Strings of 17 bytes and more start at every residue 0..7 of their offset in the batch's string
    blob (the device packer reads them as 8-byte words from wherever they start)."""
    for batch in (case.batch, case.near_batch):
        offs = batch.str_offsets.astype(np.int64)
        long_ = np.diff(offs) >= 17
        assert set((offs[:-1][long_] & 7).tolist()) == set(range(8))


@pytest.mark.parametrize("fam", FAMS + ["n"])
def test_oracle_equals_reference(case, fam):
    ev = oracle.OracleEvaluator(SR.MANIFEST)
    bags, _, batch = case.inputs(fam)
    rng = np.random.default_rng(6)
    for rs in case.sets[fam]:
        want = case.ref(rs)
        got = oracle.oracle_matrix(ev, rs.rules, batch, threads=8)
        got = np.where(got >= 2, 2, got)
        bad = np.argwhere(got != want)
        assert bad.size == 0, [(rs.rules[r], bags[q], int(got[q, r]), int(want[q, r])) for q, r in bad[:3]]
        errs = np.argwhere(want == SR.ERROR)
        for q, r in errs[rng.choice(len(errs), 200, replace=False)]:
            st, msg = ev.eval_predicate(rs.rules[r], batch, int(q))
            assert st in ("error", "panic") and msg, (rs.rules[r], bags[q], st, msg)


def test_oracle_values_equal_reference(case):
    """Eval of the value rules: the oracle's string is the reference's, byte for byte."""
    from istio_amd.bags import go_str_bytes
    ev = oracle.OracleEvaluator(SR.MANIFEST)
    f = case.sets["f"][0]
    ok, vals = case.ref_values(f)
    lens = set()
    for q in range(0, case.cols.n, 3):
        for r, rule in enumerate(f.rules):
            st, v = ev.eval(rule, case.batch, q)
            assert (st == "ok") == bool(ok[q, r]), (rule, case.bags[q])
            if st == "ok":
                assert isinstance(v, str) and go_str_bytes(v) == vals[q, r], (rule, case.bags[q], v)
                lens.add(len(vals[q, r]))
            else:
                assert v
    assert {0, 1, 21, 22, 257, 300} <= lens and any(b"\0" in v for v in vals[ok])


_INS = re.compile(r"^\s*\d+\*?\s+(\w+)\s+d=\d+ a=\d+ b=\d+ x=(\d+) y=(\d+) z=(\d+)", re.M)
_CAP = 1 << 12


def pool_bytes(eng, sid):
    """The bytes of string `sid` of the rule-set pool, NULs included: mxp_string_text into two buffers
    filled differently -- the bytes it wrote (the string and a terminator) are where the two agree."""
    out = []
    for fill in (0x55, 0xAA):
        buf = ctypes.create_string_buffer(bytes([fill]) * _CAP, _CAP)
        if eng.lib.mxp_string_text(eng.h, sid, buf, _CAP) != 0:
            return None
        out.append(np.frombuffer(buf.raw, dtype=np.uint8))
    wrote = int(np.argmax(out[0] != out[1]))
    assert wrote >= 1 and out[0][wrote - 1] == 0
    return out[0][:wrote - 1].tobytes()


def program_strings(eng, vm_text, cache):
    """The pool strings a rule's program names, in program order: the operand of each eqk / const
    (y) and strfnk (x).  (A numeric eqk names whatever string has its number: read as one more entry.)"""
    out = []
    for op, x, y, z in _INS.findall(vm_text):
        if op in ("eqk", "const", "strfnk"):
            sid = int(x) if op == "strfnk" else int(y)
            if sid not in cache:
                cache[sid] = pool_bytes(eng, sid)
            out.append(cache[sid])
    return out


def required_constants(node):
    """The constants a rule's program must name, in text order: the right-hand constant of every
    string atom and the fallback constant of a value rule.  (A constant map key goes to a virtual
    column, and the K of `(as | K) == K2` may be folded into a constant result.)"""
    t = node[0]
    if t in SR.STRING_OPS:
        return [node[2][1].bytes] if node[2][0] == "k" else []
    if t == "val":
        op = node[1]
        return [op[2][1].bytes] if op[0] == "or" and op[2][0] == "k" else []
    if t == "ieq":
        return []
    return [c for x in node[1:] if isinstance(x, tuple) for c in required_constants(x)]


@pytest.mark.parametrize("fam", FAMS + ["f", "n"])
def test_host_engine_constants_whole(case, host, fam):
    """Every rule compiles, and the string constants its program names are, in order, the tuple's
    bytes: no spelling (\\xNN, \\uXXXX, \\n, octal, raw) loses or changes a byte between the parser and
    the rule-set pool, a NUL or a byte past the first word included."""
    n_checked = 0
    for rs in case.sets[fam]:
        eng, st = host(rs.rules)
        assert (st == 0).all(), [(rs.rules[i], eng.rule_error(i)) for i in np.where(st != 0)[0][:3]]
        cache = {}
        for i, node in enumerate(rs.nodes):
            want = required_constants(node)
            got = program_strings(eng, eng.rule_vm_text(i), cache)
            at = 0
            for w in want:
                while at < len(got) and got[at] != w:
                    at += 1
                assert at < len(got), (rs.rules[i], w, got, eng.rule_vm_text(i))
                at += 1
            n_checked += len(want)
    assert n_checked >= (5 if fam == "f" else 50)
