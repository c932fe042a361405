"""64-bit numeric values through the match path on the GPU: the families of numeric_ref.py, whose
INT64 / DOUBLE / DURATION values and constants differ in one 32-bit word only as often as they
agree, under every routing of the guard, index and VM kernels and every way a batch reaches the
device.  Three results must agree exactly: the engine's, the oracle's (test_gpu_parity.compare,
codes and error texts) and the independent reference's."""
import numpy as np
import pytest
import torch

import numeric_ref as NR
import oracle
from istio_amd.bags import BagBatch, NarrowBatch
from test_gpu_parity import compare
from test_numeric_wide_cpu import FAMS, Case, to_go

pytestmark = pytest.mark.gpu

ROUTINGS = [{}] + [{"MXP_DEBUG_FLAGS": str(f)} for f in (2, 8, 4, 512, 8192, 65536, 64, 1 << 23)] + \
           [{"MXP_GPW": "1"}, {"MXP_DTP": "0"}, {"MXP_INDEX_SPARSITY": "0"}]


def _id(knobs):
    return "-".join("%s=%s" % kv for kv in knobs.items()) or "default"


@pytest.fixture(scope="module")
def mxp(libmxp):
    import istio_amd.engine as mxp
    return mxp


@pytest.fixture(scope="module")
def case():
    return Case.get()


@pytest.fixture(scope="module")
def ev():
    return oracle.OracleEvaluator(NR.MANIFEST)


def engine_for(mxp, rules):
    eng = mxp.Engine(0)
    eng.set_vocabulary(NR.MANIFEST)
    st = eng.compile(rules)
    assert (st == 0).all(), [(rules[i], eng.rule_error(i)) for i in np.where(st != 0)[0][:3]]
    return eng


def assert_codes(got, want, rs, bags):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first mismatches (request, rule, got, reference): %s" % (
        [(int(q), rs.rules[r], bags[q], int(got[q, r]), int(want[q, r])) for q, r in bad[:3]],)


def check_family(mxp, case, ev, fam):
    for rs in case.sets[fam]:
        eng = engine_for(mxp, rs.rules)
        got, _ = compare(eng, ev, rs.rules, case.batch, sample_msgs=60)
        assert_codes(got, case.ref(rs)[0], rs, case.bags)


@pytest.mark.parametrize("knobs", ROUTINGS, ids=_id)
@pytest.mark.parametrize("fam", FAMS)
def test_family_parity(mxp, case, ev, fam, knobs, monkeypatch):
    """default; MXP_DEBUG_FLAGS 2, 8 (no guard index: every continuation in-wave), 4, 512 (guard-only
    equality atoms indexed too), 8192, 65536 (the lean kernel), 64, 1 << 23; one group per wave;
    MXP_DTP=0; the densest index tables (MXP_INDEX_SPARSITY=0: longest probe chains)."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    check_family(mxp, case, ev, fam)


def test_numeric_composite_without_composite_index(mxp, case, ev, monkeypatch):
    """Family (e) with the composite index off (MXP_DEBUG_FLAGS=16): the plain equality index over K."""
    monkeypatch.setenv("MXP_DEBUG_FLAGS", "16")
    check_family(mxp, case, ev, "e")


def _bitmaps(db, n, R):
    Wd = (R + 31) // 32
    dm = torch.zeros((Wd, n), dtype=torch.int32, device="cuda")
    de = torch.zeros((Wd, n), dtype=torch.int32, device="cuda")
    db.eval(dm.data_ptr(), de.data_ptr(), 0)
    torch.cuda.synchronize()
    return dm.cpu().numpy().view(np.uint32), de.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("host_pack", ["1", "0"], ids=["host-packer", "device-packer"])
def test_packers(mxp, case, ev, host_pack, monkeypatch):
    monkeypatch.setenv("MXP_HOST_PACK", host_pack)
    check_family(mxp, case, ev, "c")


def test_narrow_upload(mxp, case):
    """A NarrowBatch through upload2: the numeric columns travel wide, the string columns narrow; the
    result is bit-identical to the wide upload's and equal to the reference."""
    bags = NR.make_bags(seed=2, p_wrong=0.0)  # (a wrongly typed value keeps its column wide)
    cols = NR.Columns(bags)
    batch = BagBatch.from_bags([{k: to_go(v) for k, v in b.items()} for b in bags], names=list(NR.MANIFEST))
    nb = NarrowBatch(batch)
    for name, f in zip(batch.names, nb.narrow):
        assert bool(f) == (name not in ("ai", "bi", "ad", "bd")), name
    for rs in case.sets["c"]:
        eng = engine_for(mxp, rs.rules)
        R = len(rs.rules)
        wide = _bitmaps(eng.upload(batch), batch.n, R)
        narrow = _bitmaps(eng.upload2(nb), batch.n, R)
        assert np.array_equal(wide[0], narrow[0]) and np.array_equal(wide[1], narrow[1])
        assert_codes(mxp.bits_to_codes(narrow[0], narrow[1], R), rs.evaluate(cols)[0], rs, bags)


def test_wire_path(mxp, case):
    """The bags as CompressedAttributes, decoded by the engine (as test_wire_path_parity): int64s,
    doubles and durations keep both words.  (A value of another Go type has no wire form.)"""
    from istio_amd import wire
    bags = [{k: v for k, v in b.items() if v[0] != "other"} for b in case.bags]
    cols = NR.Columns(bags)
    gobags = [{k: to_go(v) for k, v in b.items()} for b in bags]
    for rs in case.sets["c"]:
        eng = engine_for(mxp, rs.rules)
        dec = wire.decode(eng, wire.from_bags(gobags, sorted(NR.MANIFEST)[::3]))
        m1, e1 = eng.eval_batch(dec)
        m2, e2 = eng.eval_batch(BagBatch.from_bags(gobags, names=list(NR.MANIFEST)))
        assert np.array_equal(m1, m2) and np.array_equal(e1, e2)
        assert_codes(mxp.bits_to_codes(m1, e1, len(rs.rules)), rs.evaluate(cols)[0], rs, bags)


def test_eval_values_bit_for_bit(mxp, case):
    """Eval of the value rules: every payload is the reference's 64-bit pattern -- NaN payloads, -0.0,
    denormals, both words of an INT64 or a fallback constant."""
    f = case.sets["f"][0]
    eng = engine_for(mxp, f.rules)
    vals, codes = eng.eval_values(case.batch)
    ok, bits = f.values(case.cols)
    assert np.array_equal(codes, np.where(ok, 0, 2))
    bad = np.argwhere(ok & (vals != bits))
    assert bad.size == 0, [(f.rules[r], case.bags[q], hex(int(vals[q, r])), hex(int(bits[q, r]))) for q, r in bad[:3]]
    seen = set(int(x) for x in vals[ok])
    assert {NR.dbits(-0.0), 0x7FF8000000000001, 0xFFF8000000000000, NR.M64, 1 << 63, 1, (1 << 32) + 7} <= seen


def test_resolve_selects_the_true_rules(mxp, case):
    """One Resolve over family (c): a request none of whose rules fails gets exactly the rules the
    reference marks true, in order; any other stops at the first rule the reference marks failed."""
    rs = case.sets["c"][0]
    want, _ = case.ref(rs)
    manifest = dict(NR.MANIFEST)
    manifest.update({"destination.service": "STRING", "context.protocol": "STRING"})
    extra = {"destination.service": "svc.istio-system.svc.cluster.local", "context.protocol": "http"}
    batch = BagBatch.from_bags([dict({k: to_go(v) for k, v in b.items()}, **extra) for b in case.bags],
                               names=list(manifest))
    eng = mxp.Engine(0)
    eng.set_vocabulary(manifest)
    assert (eng.compile(rs.rules) == 0).all()
    R = len(rs.rules)
    eng.set_resolver("destination.service", "istio-system", ["istio-system"] * R, np.ones(R, dtype=np.uint32),
                     np.zeros(R, dtype=np.uint8), np.zeros(R, dtype=np.uint8))
    status, err_rule, off, sel = eng.resolve_arrays(batch, 0, ids16=True)
    assert sel.dtype == np.uint16
    failed = (want == NR.ERROR).any(axis=1)
    assert np.array_equal(status == eng.RESOLVE_PRED_ERROR, failed) and (status[~failed] == eng.RESOLVE_OK).all()
    assert np.array_equal(err_rule[failed], (want == NR.ERROR).argmax(axis=1)[failed])
    n_sel = 0
    for q in np.nonzero(~failed)[0]:
        got = sel[int(off[q]):int(off[q + 1])]
        assert np.array_equal(got, np.nonzero(want[q] == NR.TRUE)[0]), q
        n_sel += len(got)
    assert n_sel > 1000 and failed.any()
