"""64-bit numeric values on the host: the designed inputs of numeric_ref.py meet their conditions,
the oracle agrees with that independent reference on every family, and the product's compiler
carries every numeric constant whole (both words) into its VM programs and indexes."""
import re

import numpy as np
import pytest

import numeric_ref as NR
import oracle
from istio_amd.bags import BagBatch, GoDuration, GoFloat64, GoInt64, GoOther


def to_go(value):
    """A (kind, payload) bag value of numeric_ref as the product's Go value model."""
    kind, p = value
    if kind == "int64":
        return GoInt64(p - (1 << 64) if p >> 63 else p)
    if kind == "duration":
        return GoDuration(p - (1 << 64) if p >> 63 else p)
    if kind == "double":
        return GoFloat64(NR.dfloat(p))
    if kind == "other":
        return GoOther(p)
    return p  # str, bool, dict, bytes


class Case:
    """The designed batch, shared by every test of a session: bags, columns, BagBatch, and per rule
    set the reference's codes and reads (computed once, never changed)."""
    _one = None

    def __init__(self):
        self.bags = NR.make_bags()
        self.cols = NR.Columns(self.bags)
        self.batch = BagBatch.from_bags([{k: to_go(v) for k, v in b.items()} for b in self.bags],
                                        names=list(NR.MANIFEST))
        # (a NaN keeps its payload through GoFloat64 and struct.pack)
        for name in NR.ATTRS:
            c = self.batch.names.index(name)
            num = np.isin(self.cols.kind[name], [2, 3, 5])
            assert np.array_equal(self.batch.values[c][num], self.cols.bits[name][num]), name
        self.sets = {f: make() for f, make in NR.FAMILIES.items()}
        self.sets["f"] = NR.family_f()
        self._ref = {}

    @classmethod
    def get(cls):
        if cls._one is None:
            cls._one = cls()
        return cls._one

    def ref(self, rs):
        if rs.name not in self._ref:
            self._ref[rs.name] = rs.evaluate(self.cols)
        return self._ref[rs.name]


@pytest.fixture(scope="module")
def case():
    return Case.get()


@pytest.fixture(scope="module")
def host(libmxp):
    from istio_amd.engine import Engine

    def compiled(rules):
        e = Engine(-1)
        e.set_vocabulary(NR.MANIFEST)
        return e, e.compile(rules)
    return compiled


FAMS = ["a", "b", "c", "d", "e"]


@pytest.mark.parametrize("fam", FAMS)
def test_inputs_meet_their_conditions(case, fam):
    """On the reference alone: the pairs whose leading compare agrees in exactly one word -- where a
    compare of one word would answer differently -- and the true and error pairs are each >= 2 % of
    the family's pairs; the half-equal ones also >= 500."""
    lo_only = hi_only = true = err = pairs = 0
    for rs in case.sets[fam]:
        assert len(rs.rules) <= 400
        codes, _ = case.ref(rs)
        v, a, b = rs.leading(case.cols)
        lo = (a & np.uint64(0xFFFFFFFF)) == (b & np.uint64(0xFFFFFFFF))
        hi = (a >> np.uint64(32)) == (b >> np.uint64(32))
        lo_only += int((v & lo & ~hi).sum())
        hi_only += int((v & hi & ~lo).sum())
        true += int((codes == NR.TRUE).sum())
        err += int((codes == NR.ERROR).sum())
        pairs += codes.size
    print("family %s: %d pairs, low-only %d, high-only %d, true %d, error %d" % (fam, pairs, lo_only, hi_only, true, err))
    for k in (lo_only, hi_only):
        assert k >= 500 and k >= 0.02 * pairs
    assert true >= 0.02 * pairs and err >= 0.02 * pairs


def test_family_shapes(case):
    b = case.sets["b"][0]
    per_group = []
    for g in range(0, len(b.nodes), 32):
        cols = [x[1][1] for x in b.nodes[g:g + 32]]
        per_group.append(max(cols.count(c) for c in set(cols)))
    assert any(m >= 8 for m in per_group) and any(m < 8 for m in per_group)
    for rs in case.sets["c"]:
        ks = {x[1][2].bits for x in rs.nodes}
        assert len(ks) >= 300
        assert any((k ^ j) >> 32 == 0 and k != j for k in list(ks)[:20] for j in ks)
    texts = " ".join(r for f in "abcde" for rs in case.sets[f] for r in rs.rules)
    for spelled in ("1e-320", " .5", " 5.", "1E3", "0.10000000000000000555", str((1 << 63) - 1), str(7 << 32)):
        assert spelled in texts, spelled
    assert [r for r in case.sets["f"][0].rules[:4]] == ["ai", "ai | bi", "ai | 4294967303", "ad | 0.1"]


def test_vector_reference_equals_plain_python(case):
    """The column-wise evaluation against the pair-at-a-time one in plain Python ints, codes and reads."""
    rng = np.random.default_rng(5)
    for fam in FAMS:
        for rs in case.sets[fam]:
            codes, reads = case.ref(rs)
            for q in rng.choice(case.cols.n, 40, replace=False):
                got = set()
                for r, node in enumerate(rs.nodes):
                    assert NR.eval_one(node, case.bags[q], got) == codes[q, r], (rs.rules[r], case.bags[q])
                assert sorted(got) == NR.referenced(reads, q)
    f = case.sets["f"][0]
    ok, bits = f.values(case.cols)
    for q in range(0, case.cols.n, 7):
        for r, node in enumerate(f.nodes):
            c, v = NR.eval_one(node, case.bags[q], set())
            assert (c == NR.FALSE) == ok[q, r] and v == int(bits[q, r])


@pytest.mark.parametrize("fam", FAMS)
def test_oracle_equals_reference(case, fam):
    ev = oracle.OracleEvaluator(NR.MANIFEST)
    for rs in case.sets[fam]:
        want, reads = case.ref(rs)
        got = oracle.oracle_matrix(ev, rs.rules, case.batch, threads=8)
        got = np.where(got >= 2, 2, got)
        bad = np.argwhere(got != want)
        assert bad.size == 0, [(rs.rules[r], case.bags[q], int(got[q, r]), int(want[q, r])) for q, r in bad[:3]]
        if fam in ("c", "e"):
            for q in range(0, case.cols.n, 5):
                o = [x.decode() for x in oracle.oracle_referenced(ev, rs.rules, case.batch, q)]
                assert o == NR.referenced(reads, q), q


def test_oracle_values_equal_reference(case):
    """Eval of the value rules: the oracle's result, as a 64-bit pattern, is the reference's."""
    ev = oracle.OracleEvaluator(NR.MANIFEST)
    f = case.sets["f"][0]
    ok, bits = f.values(case.cols)
    for q in range(0, case.cols.n, 3):
        for r, rule in enumerate(f.rules):
            st, v = ev.eval(rule, case.batch, q)
            assert (st == "ok") == bool(ok[q, r]), (rule, q)
            if st == "ok":
                got = NR.dbits(float(v)) if isinstance(v, float) else int(v) & NR.M64
                assert got == int(bits[q, r]), (rule, q, hex(got), hex(int(bits[q, r])))


_INS = re.compile(r"^\s*\d+\*?\s+(\w+)\s+d=\d+ a=\d+ b=\d+ x=(\d+) y=(\d+) z=(\d+)", re.M)


def vm_constants(vm_text):
    """y | z << 32 of each eqk / const instruction whose constant is numeric (a string constant's eqk
    carries its string id; those rules' string atoms are told by position)."""
    return [(op, int(y) | int(z) << 32) for op, x, y, z in _INS.findall(vm_text) if op in ("eqk", "const", "retk")]


def expected_constants(node):
    """The numeric payloads a rule's program carries, in program order: a list of alternatives, each a
    sequence.  `(X | K2) == K` either loads K2 and compares, or is folded where it ends the rule: the
    fallback returns the constant K2 == K (`retk`) instead of loading K2."""
    t = node[0]
    if t in ("and", "or"):
        return expected_constants(node[1]) + expected_constants(node[2])
    if t == "par":
        return expected_constants(node[1])
    if t == "sw":
        return []
    left, right = node[1], node[2] if t != "val" else None
    out = []
    if isinstance(right, NR.Const):
        if right.cls == "s":
            return []
        if left[0] == "altk":
            return [([left[2].bits, right.bits], [int(left[2].bits == right.bits), right.bits])]
        return [([right.bits],)]
    return [([op[2].bits],) for op in (left, right) if op is not None and op[0] == "altk"]


def carries(got, want):
    """got holds, in order, one alternative of each item of want."""
    pos = 0
    for alternatives in want:
        for seq in alternatives:
            p = pos
            for w in seq:
                while p < len(got) and got[p] != w:
                    p += 1
                p += 1
            if p <= len(got):
                pos = p
                break
        else:
            return False
    return True


@pytest.mark.parametrize("fam", FAMS + ["f"])
def test_host_engine_constants_whole(case, host, fam):
    """Every rule compiles, and the numeric constants of its VM text, in program order, are the
    reference's 64-bit patterns: no constant loses its high word between the parser and the program."""
    for rs in case.sets[fam]:
        eng, st = host(rs.rules)
        assert (st == 0).all(), [(rs.rules[i], eng.rule_error(i)) for i in np.where(st != 0)[0][:3]]
        for i, node in enumerate(rs.nodes):
            want = expected_constants(node)
            got = [v for _, v in vm_constants(eng.rule_vm_text(i))]
            # (string constants carry ids in between: the numeric ones must appear, whole and in order)
            assert carries(got, want), (rs.rules[i], want, got, eng.rule_vm_text(i))
        info = eng.ruleset_info()
        if fam == "c":
            assert info["indexed"] == len(rs.rules), info
        if fam == "e":
            assert info["composite"] == len({r for r in rs.rules}), info


def test_literal_edges(host):
    ev = oracle.OracleEvaluator(NR.MANIFEST)
    bad = ["ai == 9223372036854775808", "ad == 1e400", "ai == 0x10", "ai == -2"]
    eng, st = host(bad + ["ai == 012"])
    for i, r in enumerate(bad):
        with pytest.raises(Exception) as ei:
            ev.compile(r)
        assert st[i] != 0 and eng.rule_error(i) == str(ei.value), (r, eng.rule_error(i), str(ei.value))
    assert st[4] == 0 and ("eqk", 12) in vm_constants(eng.rule_vm_text(4))
