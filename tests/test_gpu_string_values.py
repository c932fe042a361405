"""String values through the match path on the GPU: the families of string_ref.py, whose values,
constants, patterns and map keys sit at the boundaries of the device string paths -- the 8-byte
word and its masked tail, every alignment of a suffix compare, the 12-byte head, the inline keys of
the composite (12 bytes) and prefix (20 bytes) index, the length tag min(L, 255), NULs and bytes
>= 0x80 -- under every routing of the guard, index and VM kernels and every way a batch reaches the
device.  Three results must agree exactly: the engine's, the oracle's (test_gpu_parity.compare,
codes and error texts) and the independent reference's."""
import re

import numpy as np
import pytest
import torch

import oracle
import string_ref as SR
from istio_amd.bags import BagBatch, NarrowBatch, go_str_bytes
from test_gpu_parity import compare
from test_string_ref_cpu import FAMS, Case, to_batch, to_go

pytestmark = pytest.mark.gpu

ROUTINGS = [{}] + [{"MXP_DEBUG_FLAGS": str(f)} for f in (2, 4, 8, 16, 512, 8192, 65536, 131072, 262144, 8388608)] + \
           [{"MXP_HEADS": "0"}, {"MXP_INDEX_SPARSITY": "0"}, {"MXP_GPW": "1"}, {"MXP_DTP": "0"}]


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
    return oracle.OracleEvaluator(SR.MANIFEST)


def engine_for(mxp, rules, manifest=SR.MANIFEST):
    eng = mxp.Engine(0)
    eng.set_vocabulary(manifest)
    st = eng.compile(rules)
    assert (st == 0).all(), [(rules[i], eng.rule_error(i)) for i in np.where(st != 0)[0][:3]]
    return eng


def assert_codes(got, want, rs, bags):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%d mismatches; first (request, rule, bag, got, reference): %s" % (
        len(bad), [(int(q), rs.rules[r], bags[q], int(got[q, r]), int(want[q, r])) for q, r in bad[:3]],)


def check_family(mxp, case, ev, fam):
    bags, _, batch = case.inputs(fam)
    for rs in case.sets[fam]:
        eng = engine_for(mxp, rs.rules)
        got, _ = compare(eng, ev, rs.rules, batch, sample_msgs=60)
        assert_codes(got, case.ref(rs), rs, bags)


@pytest.mark.parametrize("knobs", ROUTINGS, ids=_id)
@pytest.mark.parametrize("fam", FAMS)
def test_family_parity(mxp, case, ev, fam, knobs, monkeypatch):
    """default; MXP_DEBUG_FLAGS 2, 4, 8 (no guard index: every string function in-wave), 16 (no
    composite index), 512, 8192, 65536, 131072, 262144, 1 << 23; the index reading strings instead
    of heads (MXP_HEADS=0); the densest index tables (MXP_INDEX_SPARSITY=0); one group per wave;
    MXP_DTP=0."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    check_family(mxp, case, ev, fam)


@pytest.mark.parametrize("host_pack", ["1", "0"], ids=["host-packer", "device-packer"])
@pytest.mark.parametrize("fam", ["a", "c", "n"])
def test_packers(mxp, case, ev, fam, host_pack, monkeypatch):
    """Both packers intern the batch's strings: equality and map keys are compares of the ids they
    give.  Family n runs on the nearly-distinct column -- 4k strings that share their first 24 bytes."""
    monkeypatch.setenv("MXP_HOST_PACK", host_pack)
    check_family(mxp, case, ev, fam)


def _bitmaps(db, n, R):
    Wd = (R + 31) // 32
    dm = torch.zeros((Wd, n), dtype=torch.int32, device="cuda")
    de = torch.zeros((Wd, n), dtype=torch.int32, device="cuda")
    db.eval(dm.data_ptr(), de.data_ptr(), 0)
    torch.cuda.synchronize()
    return dm.cpu().numpy().view(np.uint32), de.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("fam", ["a", "c", "n"])
def test_narrow_upload(mxp, case, fam):
    """The same bags (without wrongly typed values, which keep a column wide) as a NarrowBatch through
    upload2: bit-identical to the wide upload's result and equal to the reference."""
    src = case.inputs(fam)[0]
    bags = [{k: v for k, v in b.items() if v[0] == SR.ACCEPTS[k]} for b in src]
    cols = SR.Columns(bags)
    batch = to_batch(bags)
    nb = NarrowBatch(batch)
    for name, f in zip(batch.names, nb.narrow):
        assert bool(f) == (name != "ai" or fam == "n"), name
    for rs in case.sets[fam]:
        eng = engine_for(mxp, rs.rules)
        R = len(rs.rules)
        wide = _bitmaps(eng.upload(batch), batch.n, R)
        narrow = _bitmaps(eng.upload2(nb), batch.n, R)
        assert np.array_equal(wide[0], narrow[0]) and np.array_equal(wide[1], narrow[1])
        assert_codes(mxp.bits_to_codes(narrow[0], narrow[1], R), rs.evaluate(cols), rs, bags)


@pytest.mark.parametrize("fam", ["a", "c", "n"])
def test_wire_path(mxp, case, fam):
    """The bags as CompressedAttributes, decoded by the engine.  (A value of another Go type has no
    wire form.)"""
    from istio_amd import wire
    src = case.inputs(fam)[0]
    bags = [{k: v for k, v in b.items() if v[0] != "other"} for b in src]
    cols = SR.Columns(bags)
    gobags = [{k: to_go(v) for k, v in b.items()} for b in bags]
    for rs in case.sets[fam]:
        eng = engine_for(mxp, rs.rules)
        dec = wire.decode(eng, wire.from_bags(gobags, sorted(SR.MANIFEST)[::3]))
        m1, e1 = eng.eval_batch(dec)
        m2, e2 = eng.eval_batch(BagBatch.from_bags(gobags, names=list(SR.MANIFEST)))
        assert np.array_equal(m1, m2) and np.array_equal(e1, e2)
        assert_codes(mxp.bits_to_codes(m1, e1, len(rs.rules)), rs.evaluate(cols), rs, bags)


def test_eval_values_byte_for_byte(mxp, case):
    """Eval of the value rules: every returned string is the reference's bytes -- the 300-byte and
    NUL-bearing ones, a map value, a fallback constant in each spelling."""
    f = case.sets["f"][0]
    eng = engine_for(mxp, f.rules)
    vals, codes = eng.eval_values(case.batch)
    ok, want = case.ref_values(f)
    assert np.array_equal(codes >= 2, ~ok), np.argwhere((codes >= 2) != ~ok)[:3]
    assert (codes[ok] == 0).all()
    seen = set()
    for r in range(len(f.rules)):
        text = {}
        for q in np.nonzero(ok[:, r])[0]:
            v = int(vals[q, r])
            if v not in text:
                got = mxp.decode_value(eng, r, v)
                assert isinstance(got, str), (f.rules[r], got)
                text[v] = go_str_bytes(got)
            assert text[v] == want[q, r], (f.rules[r], case.bags[q], text[v], want[q, r])
        seen |= set(text.values())
    assert {len(v) for v in seen} >= {0, 1, 21, 22, 257, 300} and sum(b"\0" in v for v in seen) > 20
    assert SR.B in seen and SR.H1 + b"\0" in seen and b"\xc3\xa9\xff\n\t\0" in seen


def test_resolve_selects_the_true_rules(mxp, case):
    """One Resolve over family (c): a request none of whose rules fails gets exactly the rules the
    reference marks true, in order; any other stops at the first rule the reference marks failed."""
    rs = case.sets["c"][0]
    want = case.ref(rs)
    manifest = dict(SR.MANIFEST)
    manifest.update({"destination.service": "STRING", "context.protocol": "STRING"})
    extra = {"destination.service": "svc.istio-system.svc.cluster.local", "context.protocol": "http"}
    batch = BagBatch.from_bags([dict({k: to_go(v) for k, v in b.items()}, **extra) for b in case.bags],
                               names=list(manifest))
    eng = engine_for(mxp, rs.rules, manifest)
    R = len(rs.rules)
    eng.set_resolver("destination.service", "istio-system", ["istio-system"] * R, np.ones(R, dtype=np.uint32),
                     np.zeros(R, dtype=np.uint8), np.zeros(R, dtype=np.uint8))
    status, err_rule, off, sel = eng.resolve_arrays(batch, 0, ids16=True)
    assert sel.dtype == np.uint16
    failed = (want == SR.ERROR).any(axis=1)
    assert np.array_equal(status == eng.RESOLVE_PRED_ERROR, failed) and (status[~failed] == eng.RESOLVE_OK).all()
    assert np.array_equal(err_rule[failed], (want == SR.ERROR).argmax(axis=1)[failed])
    n_sel = 0
    for q in np.nonzero(~failed)[0]:
        got = sel[int(off[q]):int(off[q + 1])]
        assert np.array_equal(got, np.nonzero(want[q] == SR.TRUE)[0]), q
        n_sel += len(got)
    assert n_sel > 1000 and failed.any()


def test_length_limit(mxp):
    """A string descriptor holds a 24-bit length.  A batch string of exactly 2^24 bytes is refused at
    upload with the engine's 16 MiB error ("malformed batch: string 0 is 16 MiB or longer"), and
    the engine evaluates a normal batch afterwards; one of 2^24 - 1 bytes is accepted, and its
    prefix, its suffix, and its equality with an identical copy and with a copy that differs in the
    last byte are the reference's."""
    def big(n):
        return (SR.B * (n // 300 + 1))[:n]

    def batch_of(a):
        """3 requests: `as` the long string; `bs` a copy of it, a copy but for the last byte, H1."""
        strings = [a, bytes(bytearray(a)), a[:-1] + (b"!" if a[-1:] != b"!" else b"?"), SR.H1]
        ones = np.ones(3, dtype=np.uint8)
        columns = {"as": (ones, np.array([0, 0, 3], dtype=np.uint64)), "bs": (ones, np.array([1, 2, 3], dtype=np.uint64))}
        bags = [{"as": ("string", strings[i]), "bs": ("string", strings[j])} for i, j in ((0, 1), (0, 2), (3, 3))]
        return BagBatch.from_columns(3, columns, strings), bags

    a = big((1 << 24) - 1)
    rng = np.random.default_rng(1)
    A, Bs = SR.attr("as"), SR.attr("bs")
    nodes = [("sw", A, ("k", SR.K(rng, a[:21]))), ("sw", A, ("k", SR.K(rng, SR.flip(a[:21], 20)))),
             ("ew", A, ("k", SR.K(rng, a[-21:]))), ("ew", A, ("k", SR.K(rng, SR.flip(a[-21:], 0)))),
             ("ew", A, ("k", SR.K(rng, SR.flip(a[-21:], 20)))), ("eq", A, Bs), ("ne", A, Bs), ("sw", A, Bs), ("ew", Bs, A),
             ("match", A, Bs)]
    rs = SR.RuleSet("limit", nodes)
    eng = engine_for(mxp, rs.rules)
    refused, _ = batch_of(big(1 << 24))
    with pytest.raises(mxp.MxpError) as ei:
        eng.upload(refused)
    assert re.search(r"16 MiB", str(ei.value)), str(ei.value)
    for batch, bags in (batch_of(SR.H2), batch_of(a)):
        assert int(np.diff(batch.str_offsets.astype(np.int64)).max()) == len(bags[0]["as"][1])
        m, e = eng.eval_batch(batch)
        want = rs.evaluate(SR.Columns(bags))
        assert_codes(mxp.bits_to_codes(m, e, len(rs.rules)), want, rs, [sorted(b) for b in bags])
        assert want[:, 5].tolist() == [1, 0, 1]
    assert want[0].tolist() == [1, 0, 1, 0, 0, 1, 0, 1, 1, 1] and want[1].tolist() == [1, 0, 1, 0, 0, 0, 1, 0, 0, 0]
