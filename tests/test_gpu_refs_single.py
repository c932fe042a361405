"""Referenced attributes (mxp_eval_refs) one rule shape at a time.  Each rule set holds one rule, or
40 rules that differ only in their constants, so no other rule's reads can mask a missing one (the
union over a few hundred mixed rules reads nearly every column for every request).  Per request:
the FakeBag list and the ProtoBag set against the oracle's tracking, for the numeric shapes also
against the independent reference (numeric_ref.py), and the bitmaps against mxp_eval_batch."""
import numpy as np
import pytest

import numeric_ref as NR
import oracle
from istio_amd import workloads as W
from istio_amd.bags import BagBatch
from test_gpu_refs import expected_protobag
from test_numeric_wide_cpu import Case

pytestmark = pytest.mark.gpu

N = 400
STRS = [v for v in W._STR_VALS if v != "19ms"]  # ("19ms" is a DURATION literal: a type error)
I40 = [NR.iconst(v) for v in (NR.I_NAMED + NR.I_HOT * 2 + NR.I_GRID[5::17])[:40]]
D40 = [NR.dconst_bits(v) for v in (NR.D_HOT + NR.D_GRID[1::8])[:40]]
assert len(I40) == 40 and len(D40) == 40


@pytest.fixture(scope="module")
def mxp(libmxp):
    import istio_amd.engine as mxp
    return mxp


@pytest.fixture(scope="module")
def fuzz_batch():
    return BagBatch.from_bags(W.fuzz_bags(N, seed=71), names=list(W.DEFAULT_TEST_MANIFEST))


@pytest.fixture(scope="module")
def num():
    """The first N requests of the designed numeric batch, with their columns for the reference."""
    c = Case.get()
    return c.batch.subset(np.arange(N)), NR.Columns(c.bags[:N])


def check_refs(mxp, manifest, rules, batch, reads=None, composite=None, varied=True):
    eng = mxp.Engine(0)
    eng.set_vocabulary(manifest)
    assert (eng.compile(rules) == 0).all(), rules[0]
    if composite is not None:
        assert (eng.ruleset_info()["composite"] > 0) == composite, (rules[0], eng.ruleset_info())
    match, err, refs = eng.eval_refs(batch)
    m2, e2 = eng.eval_batch(batch)
    assert np.array_equal(match, m2) and np.array_equal(err, e2), rules[0]
    ev = oracle.OracleEvaluator(manifest)
    sizes = set()
    for q in range(batch.n):
        want = [x.decode("utf-8", "surrogateescape") for x in oracle.oracle_referenced(ev, rules, batch, q)]
        got = mxp.fakebag_list(refs[q])
        assert got == want, (rules[0], len(rules), q, sorted(set(got) ^ set(want)))
        assert mxp.protobag_set(refs[q]) == expected_protobag(batch, q, want), (rules[0], q)
        if reads is not None:
            assert got == NR.referenced(reads, q), (rules[0], q)
        sizes.add(len(want))
    assert len(sizes) > 1 or not varied, (rules[0], sizes)  # (some requests stop at the first read, some go on)


def _c(i, xs):
    return xs[i % len(xs)]


# guarded_fuzz_rules' shapes, one by one: guard kinds x modes x continuation templates.  f(i) is
# variant i; the variants of a shape differ in constants only.
STRING_SHAPES = {
    "str_and_map": lambda i: 'as == "%s" && br["%s"] == "%s"' % (_c(i, STRS), _c(i, W._KEYS), _c(i + 3, STRS)),
    "ne_and_prefix_ip": lambda i: 'bs != "%s" && as.startsWith("%s") && aip != ip("%s")' % (
        _c(i, STRS), _c(i, ["a", "ab", "st", ""]), _c(i, ["1.2.3.4", "10.0.0.1"])),
    "mapkey_and_match_or": lambda i: 'ar["%s"] == "%s" && match(bs, "%s") || bi == %d' % (
        _c(i, W._KEYS), _c(i, STRS), _c(i, ["a*", "*c", "abc", "*"]), i % 5),
    "mapkey_ne_or_map": lambda i: 'sm["%s"] != "%s" || br["%s"] == "%s"' % (
        _c(i, W._KEYS), _c(i, STRS), _c(i + 1, W._KEYS), _c(i + 5, STRS)),
    "int_and_map": lambda i: 'ai == %d && br["%s"] == "%s"' % (i % 5, _c(i, W._KEYS), _c(i, STRS)),
    "bool_and_prefix": lambda i: 'ab == %s && bs.startsWith("%s") && aip != ip("1.2.3.4")' % (
        _c(i, ["true", "false"]), _c(i, ["a", "ab", "st", ""])),
    "double_or_match": lambda i: 'ad == %s || match(bs, "%s") || bi == %d' % (
        _c(i, ["1.5", "2.5", "0.0"]), _c(i, ["a*", "*c"]), i % 5),
    "prefix_and_map": lambda i: 'as.startsWith("%s") && br["%s"] == "%s"' % (
        _c(i, ["", "a", "ab", "abc", "st", "1.2", "x"]), _c(i, W._KEYS), _c(i, STRS)),
    "not_prefix_and": lambda i: 'bs.startsWith("%s") == false && as.startsWith("%s") && aip != ip("10.0.0.1")' % (
        _c(i, ["a", "ab"]), _c(i, ["a", "st"])),
    "regex_and_map": lambda i: '"^%s".matches(bs) && br["%s"] == "%s"' % (
        _c(i, ["a", "ab", "st", "str", "a[bc]", "1.2"]), _c(i, W._KEYS), _c(i, STRS)),
    "regex_mapkey_or": lambda i: '"^%s".matches(ar["%s"]) || bi == %d' % (_c(i, ["a", "fo", "ba"]), _c(i, W._KEYS), i % 5),
    "guard_only": lambda i: 'as == "%s"' % _c(i, STRS),
    "str_or_prefix": lambda i: 'as == "%s" || bs.startsWith("%s")' % (_c(i, STRS), _c(i, ["a", "ab", "st"])),
}


@pytest.mark.parametrize("count", [1, 40])
@pytest.mark.parametrize("shape", sorted(STRING_SHAPES))
def test_guarded_shapes(mxp, fuzz_batch, shape, count):
    rules = [STRING_SHAPES[shape](i + 2) for i in range(count)]
    check_refs(mxp, W.DEFAULT_TEST_MANIFEST, rules, fuzz_batch, varied=shape != "guard_only")


COMPOSITES = {
    "string": lambda i: 'as == "%s" && bs.startsWith("%s")' % (_c(i, STRS), _c(i, ["a", "ab", "", "st", "1.2"])),
    "string_tail": lambda i: 'as == "%s" && bs.startsWith("%s") && ai == %d' % (_c(i, STRS), _c(i, ["a", "ab", ""]), i % 4),
    # A is a map[key] virtual column: B is read when the map's value for the key ("" without the key) is K1
    "mapkey": lambda i: 'ar["%s"] == "%s" && bs.startsWith("%s")' % (_c(i, W._KEYS[:2]), _c(i, STRS), _c(i, ["a", "ab", ""])),
    "mapkey_tail": lambda i: 'ar["a"] == "%s" && bs.startsWith("%s") && bi == %d' % (_c(i, STRS), _c(i, ["a", ""]), i % 4),
    "bool": lambda i: 'ab == %s && bs.startsWith("%s")' % (_c(i, ["true", "false"]), _c(i, ["a", "ab", "", "st", "1.2"])),
}


@pytest.mark.parametrize("count", [1, 40])
@pytest.mark.parametrize("shape", sorted(COMPOSITES))
def test_composite_shapes(mxp, fuzz_batch, shape, count):
    rules = [COMPOSITES[shape](i + 1) for i in range(count)]
    check_refs(mxp, W.DEFAULT_TEST_MANIFEST, rules, fuzz_batch, composite=True)


def test_numeric_composite_small_k(mxp, fuzz_batch):
    """`ai == 3 && bs.startsWith("ab")`, alone: bs is read exactly where ai holds 3 (an int64 or a
    time.Duration).  A K1 taken for a string id never names the read."""
    rules = ['ai == 3 && bs.startsWith("ab")']
    ai = fuzz_batch.names.index("ai")
    assert ((fuzz_batch.values[ai] == 3) & np.isin(fuzz_batch.kinds[ai], [2, 5])).sum() > 20
    check_refs(mxp, W.DEFAULT_TEST_MANIFEST, rules, fuzz_batch, composite=True)


def _numeric(nodes, cols):
    rs = NR.RuleSet("refs", nodes)
    return rs.rules, rs.evaluate(cols)[1]


NUMERIC_SHAPES = {
    # (the wide K after test_numeric_composite_small_k, in file order: 2^32 + 7 and its kin are far
    # past any string id)
    "composite_wide": lambda k, d: NR.And(("eq", ("attr", "ai"), k), ("sw", "bs", "ab")),
    "composite_wide_tail": lambda k, d: NR.And(NR.And(("eq", ("attr", "ai"), k), ("sw", "bs", "ab")),
                                               ("eq", ("attr", "bi"), NR.iconst(NR.I_HOT[0]))),
    "composite_double": lambda k, d: NR.And(("eq", ("attr", "ad"), d), ("sw", "bs", "ab")),
    "eq_and_hoisted": lambda k, d: NR.And(("eq", ("attr", "ai"), k), ("eq", ("attr", "bi"), NR.iconst(k.bits ^ (1 << 32)))),
    "eq_and_double": lambda k, d: NR.And(("eq", ("attr", "ai"), k), ("eq", ("attr", "ad"), d)),
    "eq_or_eq": lambda k, d: NR.Or(("eq", ("attr", "ai"), k), ("eq", ("attr", "bi"), k)),
    "ne_and_string": lambda k, d: NR.And(("ne", ("attr", "ad"), d), ("eq", ("attr", "bs"), NR.sconst("x"))),
    "fallback_or": lambda k, d: NR.Or(("eq", ("alt", "ai", "bi"), k), ("eq", ("attr", "ad"), d)),
}


@pytest.mark.parametrize("count", [1, 40])
@pytest.mark.parametrize("shape", sorted(NUMERIC_SHAPES))
def test_numeric_shapes(mxp, num, shape, count):
    batch, cols = num
    # (one rule: on a hot constant, so that it is true for many requests)
    ks = [(NR.iconst(NR.I_HOT[0]), NR.dconst_bits(NR.D_HOT[0]))] if count == 1 else list(zip(I40, D40))
    rules, reads = _numeric([NUMERIC_SHAPES[shape](k, d) for k, d in ks], cols)
    check_refs(mxp, NR.MANIFEST, rules, batch, reads=reads, composite=shape.startswith("composite"))
