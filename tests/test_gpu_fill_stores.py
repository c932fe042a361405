"""One batch through every writer of the match / error bitmaps (kernels.hip: the plain fill, the
deferred-pair fill, the retained-bitmap fill sparse and in its dense fallback, the value-class fill
from global memory, from LDS rows and with immediate offsets), each with its default stores and with
the store-policy flags (MXP_DEBUG_FLAGS 128: plain stores in the streaming fills, 4194304:
non-temporal stores in the retained fill), in both output forms (eval_hits: match and error planes;
eval_compact: match plane and per-request flags).  n = 1028 (a tile and one quad: vector stores) and
1029 (rows not 16-byte aligned: word stores, a partial last quad).  Bar: every variant's planes,
flags and hit counters equal the ones the Python oracle's matrix gives (and so each other), and
the engine's own evaluation with error records passes test_gpu_parity.compare."""
import numpy as np
import pytest

import oracle
from istio_amd import workloads as W
from istio_amd.bags import ABSENT, INT64
from test_gpu_dtp import PATHS, deferred_ran, engine_for
from test_gpu_dtp_handoff import Bufs, pool  # noqa: F401  (pool: a fixture)
from test_gpu_fill_retain import batches, retained
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu

SIZES = [1028, 1029]
STORES = [0, 128 | 4194304]
FORCE, GLOBAL, LDS = 262144, 262144 | 2097152, 262144 | 33554432


@pytest.fixture(scope="module")
def mxp(libmxp):
    import istio_amd.engine as mxp
    return mxp


def planes(want):
    """[match plane, error plane, flags, hits] of an oracle matrix [n][R] (1 true, >= 2 error)."""
    n, R = want.shape
    Wd = (R + 31) // 32

    def plane(bits):
        b = np.zeros((n, Wd * 32), dtype=np.uint64)
        b[:, :R] = bits
        return (b.reshape(n, Wd, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32).view(np.int32).T
    return [plane(want == 1), plane(want >= 2), (want >= 2).any(axis=1).astype(np.uint8), (want == 1).sum(axis=0)]


def check_both_forms(eng, batch, R, want, what):
    """eval_hits and eval_compact of `batch` into fresh buffers against the oracle's planes."""
    dm, de, hits, cm, flags, hc = Bufs(R, batch.n).run(eng, batch, reps=1)
    m, e, f, h = planes(want)
    for got, ref, name in ((dm, m, "match"), (de, e, "error"), (hits, h, "hits"), (cm, m, "compact match"),
                           (flags, f, "compact flags"), (hc, h, "compact hits")):
        assert np.array_equal(got, ref), (what, name)


def check_retained(eng, other, batch, R, want, fallback, what):
    """`other`, then `batch`, into one retained buffer: the second fill is the tile kernel's (sparse,
    or its dense branch when `other` filled the overflow list) and equals the oracle's planes."""
    out = retained(eng, R, batch.n)
    _, st = out.run(eng, other)
    assert st["sparse"] == 0
    got, st = out.run(eng, batch)
    assert st["sparse"] == 1 and st["fallbacks"] == fallback, (what, st)
    m, _, f, h = planes(want)
    for x, ref, name in zip(got, (m, f, h), ("match", "flags", "hits")):
        assert np.array_equal(x, ref), (what, name)


_C2 = {}


def c2_batch(mxp, pool, n):
    """(batch, another batch of n, oracle matrix of the first), once per n.  The batch: half its quads
    one request with true pairs four times over, the rest drawn from the whole pool (path-less
    requests with error pairs, requests with no pair at all); every seventh request lacks the fills'
    guard attribute (destination.service) or carries it as an INT64: the fill's own failed type
    checks.  The other batch has every fourth quad rich: more true pairs per wave than a wave list of
    4 and an overflow list of 8 hold.  The engine's evaluation with error records goes through
    compare()."""
    if n not in _C2:
        B = batches(pool, n)
        batch, other = B["P"].subset(np.arange(n)), B["P4"]
        c = list(batch.names).index("destination.service")
        kinds = batch.kinds[c].copy()
        kinds[0::14] = ABSENT
        kinds[7::14] = INT64
        batch.kinds[c] = kinds
        mp = pytest.MonkeyPatch()
        eng = engine_for(mxp, mp, {}, pool["manifest"], pool["rules"], flags="0")
        mp.undo()
        _, want = compare(eng, oracle.OracleEvaluator(pool["manifest"]), pool["rules"], batch, sample_msgs=100)
        eng.close()
        seventh = np.arange(n) % 7 == 0
        err, true = (want >= 2).any(axis=1), (want == 1).any(axis=1)
        assert err[seventh].all() and err[~seventh].any() and true.any() and (~err & ~true).any()
        assert true[-4:].any() or err[-4:].any()  # (the last quad is not all zeros)
        _C2[n] = (batch, other, want)
    return _C2[n]


@pytest.mark.parametrize("stores", STORES)
@pytest.mark.parametrize("n", SIZES)
def test_plain_and_deferred_fill(mxp, monkeypatch, pool, n, stores):
    batch, _, want = c2_batch(mxp, pool, n)
    R = len(pool["rules"])
    for env, deferred in (({"MXP_DTP": "0"}, False), ({}, True)):
        eng = engine_for(mxp, monkeypatch, env, pool["manifest"], pool["rules"], flags=str(stores))
        assert deferred_ran(eng, batch, R) == deferred
        check_both_forms(eng, batch, R, want, (env, n, stores))
        eng.close()


@pytest.mark.parametrize("stores", STORES)
@pytest.mark.parametrize("n", SIZES)
def test_retained_fill_sparse_and_dense_fallback(mxp, monkeypatch, pool, n, stores):
    batch, other, want = c2_batch(mxp, pool, n)
    R = len(pool["rules"])
    monkeypatch.delenv("MXP_FILL_RETAIN", raising=False)
    for env, fallback in (({}, 0), (PATHS[2], 1)):  # (an overflow list of 8: `other` fills it)
        eng = engine_for(mxp, monkeypatch, env, pool["manifest"], pool["rules"], flags=str(stores))
        assert deferred_ran(eng, batch, R)
        check_retained(eng, other, batch, R, want, fallback, (env, n, stores))
        eng.close()


_C4 = {}


def c4_batch(mxp, n):
    """(manifest, rules, batch, oracle matrix), once per n: some 1290 C4 rules (41 bitmap words: the
    last fill chunk is partial), a twentieth of them continuation rules whose lookups fail on some
    requests.  C4's header rules leave no request without a true pair, so the rules comparing a
    header with "v0" are dropped and every sixteenth request gets "v0" in its three headers.
    request.path, the guard column of the value-class fill chunks, fails its type check on a stride."""
    if n not in _C4:
        manifest, rules, batch = W.c4_workload(n_rules=1300, n_requests=n, seed=73, cont_frac=0.05)
        rules = [r for r in rules if '== "v0"' not in r]
        assert 16 < (len(rules) + 31) // 32 and (len(rules) + 31) // 32 % 16
        assert batch.string(5) == b"v0"
        batch.map_values.reshape(-1, 3)[5::16] = 5
        # the fill's own failed type checks: every seventh request, and the last one (alone in its
        # quad at n = 1029), lacks the chunks' guard attribute or carries it as an INT64
        c = list(batch.names).index("request.path")
        kinds = batch.kinds[c].copy()
        kinds[0::14] = ABSENT
        kinds[7::14] = INT64
        kinds[n - 1] = ABSENT
        batch.kinds[c] = kinds
        bad = np.arange(n) % 7 == 0
        bad[n - 1] = True
        mp = pytest.MonkeyPatch()
        eng = engine_for(mxp, mp, {}, manifest, rules, flags=str(FORCE))
        mp.undo()
        _, want = compare(eng, oracle.OracleEvaluator(manifest), rules, batch, sample_msgs=100)
        eng.close()
        err, true = (want >= 2).any(axis=1), (want == 1).any(axis=1)
        assert true.any() and (~err & ~true).any()
        # exactly those requests err on the path rules (on all of them; the others only where a
        # continuation's source.ip lookup fails, which some do)
        path = np.array(["request.path" in r for r in rules])
        pure = path & np.array(["source.ip" not in r for r in rules])
        assert path.sum() > 900 and (want[bad][:, path] >= 2).all() and not (want[~bad][:, pure] >= 2).any()
        assert not (want[bad][:, ~path] >= 2).any() and (err & ~bad).any()
        _C4[n] = (manifest, rules, batch, want)
    return _C4[n]


@pytest.mark.parametrize("stores", STORES)
@pytest.mark.parametrize("flags", [GLOBAL, LDS, FORCE], ids=["global", "lds-rows", "immediate"])
@pytest.mark.parametrize("n", SIZES)
def test_value_class_fill(mxp, monkeypatch, n, flags, stores):
    manifest, rules, batch, want = c4_batch(mxp, n)
    eng = engine_for(mxp, monkeypatch, {}, manifest, rules, flags=str(flags | stores))
    assert eng.ruleset_info()["value_class_columns"] >= 5
    check_both_forms(eng, batch, len(rules), want, (n, flags, stores))
    eng.close()
