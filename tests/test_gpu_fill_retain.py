"""Retained match bitmap (mxp_match_retain): an engine that knows a buffer still holds
what its previous evaluation wrote lets mxp_fill_dtp_kernel store only the 16-byte quad rows that
held a match-plane pair then or hold one now; mxp_dtp_sort_kernel first clears the bits the previous
overflow list OR-ed in, and sends the fill down its dense branch when that list was full.  C2 family
(every word a plain fill chunk's), compact errors.  Bar: match bitmap, compact flags and hit
counters identical to an engine with deferred pairs off (MXP_DTP=0) that never retains anything --
never to the retained engine itself -- and the hook (DeviceBatch.fill_retain_stats) says the sparse
path ran: a silent dense fallback would pass every comparison."""
import numpy as np
import pytest

from istio_amd import workloads as W
from test_gpu_dtp import PATHS, deferred_ran, engine_for
from test_gpu_dtp_handoff import N_RULES, N_SERVICES, dtp_lists, pool  # noqa: F401  (pool: a fixture)

pytestmark = pytest.mark.gpu

N_MAIN = 2048 + 37


@pytest.fixture(scope="module")
def mxp(libmxp):
    import istio_amd.engine as mxp
    return mxp


_BATCHES = {}


def batches(pool, n):
    """Batches of n requests, built once per n.  The pool's path-less `heavy` requests carry error
    pairs only, which a compact evaluation files nowhere, so the busy quads here are `rich` ones: one
    request with true pairs four times over (each of its true pairs then sits four times in one
    quad and chunk).  P: half the quads rich, the rest drawn from the whole pool (path-less ones
    included: error flags); Z: no pair at all; P4: every fourth quad rich; Pe: the first and last
    quad of every fill wave's 256 requests rich; Q: another draw of the whole pool."""
    if n in _BATCHES:
        return _BATCHES[n]
    big = pool["big"]
    rng = np.random.default_rng(9)
    true = (pool["want"] == 1).sum(axis=1)
    rich, z = np.flatnonzero(true >= 1), pool["zero"]
    assert len(rich) > 1000
    q = np.arange(n) // 4
    nq = (n + 3) // 4
    rich_q = rng.choice(rich, nq)[q]  # (one rich request per quad)
    _, _, other = W.c2_workload(n_rules=N_RULES, n_requests=8 * N_MAIN, seed=62, n_services=2 * N_SERVICES,
                                p_missing_path=0.2)
    svc = other.values[list(other.names).index("destination.service")]
    b = {"P": big.subset(np.where((rng.random(nq) < 0.5)[q], rich_q, rng.integers(0, big.n, n))),
         "Z": other.subset(np.flatnonzero(svc >= N_SERVICES)[:n]),
         "P4": big.subset(np.where(q % 4 == 0, rich_q, rng.choice(z, n))),
         "Pe": big.subset(np.where((q % 64 == 0) | (q % 64 == 63), rich_q, rng.choice(z, n))),
         "Q": big.subset(rng.integers(0, big.n, n))}
    assert b["Z"].n == n
    _BATCHES[n] = b
    return b


class Out:
    """A device match buffer of `words` u32 (filled with -1), compact flags and hit counters."""

    def __init__(self, words, n_max, R):
        import torch
        self.dm = torch.full((words,), -1, dtype=torch.int32, device="cuda:0")
        self.flags = torch.ones(n_max, dtype=torch.uint8, device="cuda:0")  # (stale flags must be cleared)
        self.hits = torch.zeros(R, dtype=torch.int64, device="cuda:0")
        self.R = R

    def nbytes(self):
        return self.dm.numel() * 4

    def run(self, eng, batch, stream=0, stats=True, R=None):
        """One compact evaluation of `batch` at pitch batch.n -> ([match, flags, hits], hook values)."""
        import torch
        R = R or self.R
        Wd = (R + 31) // 32
        db = eng.upload(batch)
        self.hits.zero_()
        torch.cuda.synchronize()
        db.eval_compact(self.dm.data_ptr(), self.flags.data_ptr(), self.hits.data_ptr(), stream)
        torch.cuda.synchronize()
        st = db.fill_retain_stats() if stats else None
        out = [self.dm[: Wd * batch.n].cpu().numpy().copy().reshape(Wd, batch.n),
               self.flags[: batch.n].cpu().numpy().copy(), self.hits[:R].cpu().numpy().copy()]
        db.free()
        return out, st


def retained(eng, R, n_max):
    o = Out((R + 31) // 32 * n_max, n_max, R)
    eng.match_retain(o.dm.data_ptr(), o.nbytes())
    return o


def same(a, b, what):
    for x, y, name in zip(a, b, ("match", "flags", "hits")):
        assert np.array_equal(x, y), (what, name)


def make_ref(mxp, manifest, rules):
    """A reference: an engine with deferred pairs off, evaluating into a buffer it does not retain;
    results kept per batch."""
    mp = pytest.MonkeyPatch()
    eng = engine_for(mxp, mp, {"MXP_DTP": "0"}, manifest, rules, flags="0")
    mp.undo()
    R = len(rules)
    out = Out((R + 31) // 32 * 4096, 4096, R)
    cache = {}

    def get(batch):
        if id(batch) not in cache:
            cache[id(batch)] = (batch, out.run(eng, batch, stats=False)[0])
        return cache[id(batch)][1]
    return get


@pytest.fixture(scope="module")
def ref(mxp, pool):
    return make_ref(mxp, pool["manifest"], pool["rules"])


def rules4(pool):
    """Every pool rule four times in a row (under the 8 copies that make a dense rule): a true pair
    becomes four in one fill chunk, a rich quad's 16 or more -- past its 8 slots."""
    return [r for r in pool["rules"] for _ in range(4)]


@pytest.fixture(scope="module")
def ref4(mxp, pool):
    return make_ref(mxp, pool["manifest"], rules4(pool))


def pool_engine(mxp, monkeypatch, pool, env=None):
    monkeypatch.delenv("MXP_FILL_RETAIN", raising=False)
    return engine_for(mxp, monkeypatch, env or {}, pool["manifest"], pool["rules"], flags="0")


@pytest.mark.parametrize("n", [N_MAIN, 1, 63, 65, 1025])
def test_sequences_on_one_retained_buffer(mxp, monkeypatch, pool, ref4, n):
    """P, Z, P, P4, Z, Pe, P4, P into one retained buffer, every rule four times over so that busy
    quads hold more than 8 true pairs in a chunk: every step equals the reference, Z is all zero (a
    bit set at step k and missed at k + 1 would stay), every step but the first is sparse and none
    falls back.  The heavy property is asserted from the compact evaluations themselves: quads with
    all 8 slots taken and pairs in the overflow list (which the next step must clear)."""
    rules = rules4(pool)
    R = len(rules)
    B = batches(pool, n)
    monkeypatch.delenv("MXP_FILL_RETAIN", raising=False)
    eng = engine_for(mxp, monkeypatch, {}, pool["manifest"], rules, flags="0")
    assert deferred_ran(eng, B["P"], R)
    out = retained(eng, R, n)
    stats = []
    for k, name in enumerate(["P", "Z", "P", "P4", "Z", "Pe", "P4", "P"]):
        got, st = out.run(eng, B[name])
        print(n, k, name, st)
        same(got, ref4(B[name]), (n, k, name))
        assert st["sparse"] == (1 if k else 0) and st["fallbacks"] == 0, (k, name, st)
        if name == "Z":
            assert not got[0].any() and not got[1].any() and not got[2].any()
            assert st["live"] == 0 and st["overflow"] == 0 and st["live_prev"] == stats[-1]["live"]
        elif n >= 63:  # quads past their 8 slots, the rest through the overflow list
            assert st["live"] > 0 and st["full"] > 0 and st["overflow"] > 0, (k, name, st)
        stats.append(st)
    if n == N_MAIN:
        assert stats[0]["live"] > stats[3]["live"] > stats[5]["live"]
        pe = ref4(B["Pe"])[0]  # true pairs in the first and the last quad of a fill wave, nowhere else
        lane = np.arange(n) % 256 // 4
        assert pe[:, lane == 0].any() and pe[:, lane == 63].any() and not pe[:, (lane > 0) & (lane < 63)].any()
        assert ref4(B["P"])[1].any()  # (and error flags, from the path-less requests of the pool draw)


@pytest.mark.parametrize("env", PATHS, ids=["lists", "overflow", "rerun"])
def test_overflow_paths(mxp, monkeypatch, pool, ref, env):
    """P, Z, P with 4 pairs per wave list (the rest through the overflow list, whose bits the next
    evaluation clears before its fill) and with an overflow list of 8 (it fills: the re-run ORs
    pairs nobody recorded, so the next fill must take the dense branch on the device)."""
    R = len(pool["rules"])
    B = batches(pool, N_MAIN)
    eng = pool_engine(mxp, monkeypatch, pool, env)
    if "MXP_DTP_CAP" in env:  # true pairs beyond what the wave lists hold
        shape, lens = dtp_lists(eng, B["P"], R)
        true_pairs = int(np.unpackbits(ref(B["P"])[0].view(np.uint8)).sum())
        assert shape["cap"] == 4 and true_pairs > 4 * len(lens)
    out = retained(eng, R, N_MAIN)
    full = "MXP_DTP_OVF" in env
    want_fb = [0, 1, 1] if full else [0, 0, 0]  # (Z overflows nothing: the third fill is sparse again)
    for k, name in enumerate(["P", "Z", "P"]):
        got, st = out.run(eng, B[name])
        print(env, k, name, st)
        same(got, ref(B[name]), (env, k, name))
        assert st["sparse"] == (1 if k else 0) and st["fallbacks"] == want_fb[k], (k, st)
    assert ref(B["P"])[0].any() and not ref(B["Z"])[0].any()


def test_other_sizes_invalidate(mxp, monkeypatch, pool, ref):
    """A smaller and a larger batch at their own pitch in the same retained buffer, and back: the
    first evaluation at each new pitch is dense, the second sparse; all equal the reference."""
    R = len(pool["rules"])
    eng = pool_engine(mxp, monkeypatch, pool)
    out = retained(eng, R, 3000)
    a, s, b = batches(pool, N_MAIN), batches(pool, 1025), batches(pool, 3000)
    seq = [(a["P"], 0), (a["Q"], 1), (s["P"], 0), (s["Q"], 1), (a["P"], 0), (b["P"], 0), (b["Q"], 1), (a["Q"], 0),
           (a["P"], 1)]
    for k, (batch, sparse) in enumerate(seq):
        got, st = out.run(eng, batch)
        same(got, ref(batch), k)
        assert st["sparse"] == sparse and st["fallbacks"] == 0, (k, st)


def test_compile_invalidates(mxp, monkeypatch, pool, ref):
    """Another rule set compiled between two retained evaluations, and the first one again."""
    rules, R = pool["rules"], len(pool["rules"])
    rules2 = rules[100:500]
    B = batches(pool, N_MAIN)
    eng = pool_engine(mxp, monkeypatch, pool)
    ref2 = engine_for(mxp, monkeypatch, {"MXP_DTP": "0"}, pool["manifest"], rules2, flags="0")
    out = retained(eng, R, N_MAIN)
    assert out.run(eng, B["P"])[1]["sparse"] == 0 and out.run(eng, B["Q"])[1]["sparse"] == 1
    eng.compile(rules2)
    for k, name in enumerate(["P", "Q"]):
        got, st = out.run(eng, B[name], R=len(rules2))
        same(got, Out((len(rules2) + 31) // 32 * N_MAIN, N_MAIN, len(rules2)).run(ref2, B[name], stats=False)[0], name)
        assert st["sparse"] == k
    eng.compile(rules)
    for k, name in enumerate(["Q", "P"]):
        got, st = out.run(eng, B[name])
        same(got, ref(B[name]), name)
        assert st["sparse"] == k


def test_error_bitmap_evaluation_invalidates(mxp, monkeypatch, pool, ref):
    """An error-bitmap evaluation into the retained match buffer writes it densely and leaves the
    record unknown: the next compact evaluation is dense, the one after it sparse."""
    import torch
    R = len(pool["rules"])
    B = batches(pool, N_MAIN)
    eng = pool_engine(mxp, monkeypatch, pool)
    out = retained(eng, R, N_MAIN)
    out.run(eng, B["P"])
    assert out.run(eng, B["Q"])[1]["sparse"] == 1
    de = torch.zeros_like(out.dm)
    db = eng.upload(B["P4"])
    db.eval_hits(out.dm.data_ptr(), de.data_ptr(), out.hits.data_ptr(), 0)
    torch.cuda.synchronize()
    assert np.array_equal(out.dm.cpu().numpy().reshape(-1, N_MAIN), ref(B["P4"])[0])
    db.free()
    for k, name in enumerate(["Z", "P"]):
        got, st = out.run(eng, B[name])
        same(got, ref(B[name]), name)
        assert st["sparse"] == k and st["fallbacks"] == 0


def test_other_buffer_and_resolve_keep_the_record(mxp, monkeypatch, pool, ref):
    """An evaluation into another buffer and a pair Resolve on the same engine between two retained
    evaluations: both write the scratch generation that does not hold the retained bitmap's pairs,
    so the next retained evaluation is still sparse and equal to the reference."""
    R = len(pool["rules"])
    B = batches(pool, N_MAIN)
    monkeypatch.setenv("MXP_RESOLVE_PAIRS", "2")  # (a Resolve that cannot take the pair path fails)
    eng = pool_engine(mxp, monkeypatch, pool)
    z = np.zeros(R, dtype=np.uint8)
    eng.set_resolver("destination.service", "istio-system", ["istio-system"] * R, np.ones(R, dtype=np.uint32), z, z)
    out = retained(eng, R, N_MAIN)
    other = Out((R + 31) // 32 * N_MAIN, N_MAIN, R)
    out.run(eng, B["P"])
    for k, (name, between) in enumerate([("Q", "buffer"), ("Z", "resolve"), ("P", "both"), ("P4", "buffer")]):
        if between in ("buffer", "both"):
            got, st = other.run(eng, B["Pe"])
            same(got, ref(B["Pe"]), (k, "other buffer"))
            assert st["sparse"] == 0
        if between in ("resolve", "both"):
            status = eng.resolve_arrays(B["P4"], 0, ids16=True)[0]
            assert len(status) == N_MAIN
        got, st = out.run(eng, B[name])
        same(got, ref(B[name]), (k, name))
        assert st["sparse"] == 1 and st["fallbacks"] == 0, (k, st)


def test_release_overwrite_retain(mxp, monkeypatch, pool, ref):
    """Released, overwritten by the caller, retained again: the next fill is dense."""
    R = len(pool["rules"])
    B = batches(pool, N_MAIN)
    eng = pool_engine(mxp, monkeypatch, pool)
    out = retained(eng, R, N_MAIN)
    out.run(eng, B["P"])
    assert out.run(eng, B["Q"])[1]["sparse"] == 1
    eng.match_retain()
    out.dm.fill_(-1)
    got, st = out.run(eng, B["Z"])  # (released: an ordinary buffer)
    same(got, ref(B["Z"]), "released")
    assert st["sparse"] == 0
    out.dm.fill_(-1)
    eng.match_retain(out.dm.data_ptr(), out.nbytes())
    for k, name in enumerate(["Z", "P"]):
        got, st = out.run(eng, B[name])
        same(got, ref(B[name]), name)
        assert st["sparse"] == k


def test_second_stream(mxp, monkeypatch, pool, ref):
    """Retained evaluations queued on two streams with no host synchronisation between them: the
    second waits for the first (the engine-wide pair scratch), is sparse and equals the reference."""
    import torch
    R = len(pool["rules"])
    Wd = (R + 31) // 32
    B = batches(pool, N_MAIN)
    eng = pool_engine(mxp, monkeypatch, pool)
    out = retained(eng, R, N_MAIN)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    out.run(eng, B["Q"])
    for first, second in (("P", "P4"), ("Q", "Z"), ("P4", "P")):
        dbs = [eng.upload(B[first]), eng.upload(B[second])]
        torch.cuda.synchronize()
        for db, s in zip(dbs, (s1, s2)):
            db.eval_compact(out.dm.data_ptr(), out.flags.data_ptr(), 0, s.cuda_stream)
        torch.cuda.synchronize()
        st = dbs[1].fill_retain_stats()
        assert st["sparse"] == 1 and st["fallbacks"] == 0 and st["live_prev"] > 0
        want = ref(B[second])
        assert np.array_equal(out.dm.cpu().numpy().reshape(Wd, N_MAIN), want[0]), second
        assert np.array_equal(out.flags.cpu().numpy(), want[1]), second
        for db in dbs:
            db.free()


def test_switch_off(mxp, monkeypatch, pool, ref):
    """MXP_FILL_RETAIN=0: never sparse, same results."""
    R = len(pool["rules"])
    B = batches(pool, N_MAIN)
    monkeypatch.setenv("MXP_FILL_RETAIN", "0")
    eng = engine_for(mxp, monkeypatch, {}, pool["manifest"], pool["rules"], flags="0")
    out = retained(eng, R, N_MAIN)
    for name in ("P", "Z", "P4", "P"):
        got, st = out.run(eng, B[name])
        same(got, ref(B[name]), name)
        assert st["sparse"] == 0 and st["fallbacks"] == 0


def test_more_than_one_window(mxp, monkeypatch):
    """17k C2 rules (over 32 plain fill chunks: two chunk windows in the sort), two different ragged
    batches into a retained buffer: the second is sparse, both equal MXP_DTP=0."""
    manifest, rules, big = W.c2_workload(n_rules=17_000, n_requests=2 * 1029, seed=63, n_services=64,
                                         p_missing_path=0.1)
    R = len(rules)
    bs = [big.subset(np.arange(0, 1029)), big.subset(np.arange(1029, 2058))]
    ref_eng = engine_for(mxp, monkeypatch, {"MXP_DTP": "0"}, manifest, rules, flags="0")
    ro = Out((R + 31) // 32 * 1029, 1029, R)
    want = [ro.run(ref_eng, b, stats=False)[0] for b in bs]
    monkeypatch.delenv("MXP_FILL_RETAIN", raising=False)
    eng = engine_for(mxp, monkeypatch, {}, manifest, rules, flags="0")
    shape, _ = dtp_lists(eng, bs[0], R)
    assert shape["fills"] > 32 and shape["vtfills"] == 0
    out = retained(eng, R, 1029)
    for step, k in enumerate((0, 1, 0)):
        got, st = out.run(eng, bs[k])
        same(got, want[k], k)
        assert st["sparse"] == (1 if step else 0) and st["fallbacks"] == 0 and st["live"] > 0, (step, st)
        assert (st["live_prev"] > 0) == (step > 0), (step, st)
    assert want[0][0].any() and want[1][0].any() and not np.array_equal(want[0][0], want[1][0])


def test_group(mxp, monkeypatch, pool, ref):
    """Group([0, 0]): mxp_group_eval retains each member's bitmap.  Two different batches of equal
    size in turn, a Resolve in between, then a batch of another size (and the error-bitmap form,
    which leaves the record unknown): every download equals the un-retained reference engine, and
    the members' engines report the sparse fill where the bitmap was known."""
    R = len(pool["rules"])
    monkeypatch.delenv("MXP_FILL_RETAIN", raising=False)
    monkeypatch.setenv("MXP_DEBUG_FLAGS", "0")
    for k in ("MXP_DTP", "MXP_DTP_CAP", "MXP_DTP_OVF"):
        monkeypatch.delenv(k, raising=False)
    g = mxp.Group([0, 0])
    g.set_vocabulary(pool["manifest"])
    g.compile(pool["rules"])
    z = np.zeros(R, dtype=np.uint8)
    g.set_resolver("destination.service", "istio-system", ["istio-system"] * R, np.ones(R, dtype=np.uint32), z, z)
    for k in range(2):
        g.engine(k).set_timing(True)
    a, s = batches(pool, N_MAIN), batches(pool, 1025)

    def step(shards, sparse, err_bitmap=False):
        gb = g.upload(shards)
        g.eval(gb, err_bitmap=err_bitmap)
        g.sync()
        for k, b in enumerate(shards):
            match, err = g.download(k, b.n, err_bitmap=err_bitmap)
            assert np.array_equal(match.view(np.int32), ref(b)[0]), (k, sparse)
            if not err_bitmap:
                assert np.array_equal(err, ref(b)[1])
            want = sparse[k] if isinstance(sparse, tuple) else sparse
            assert g.engine(k).kernel_times(4)[3] == float(want), (k, sparse)
        gb.free()

    step([a["P"], a["P4"]], 0)
    step([a["Q"], a["Z"]], 1)
    step([a["Z"], a["P"]], 1)
    g.resolve_arrays([a["Pe"], a["Q"]], 0, ids16=True)
    step([a["P4"], a["Q"]], 1)
    step([s["P"], s["Q"]], 0)
    step([s["Q"], s["Z"]], 1)
    step([s["P"], s["P"]], 0, err_bitmap=True)
    step([s["Z"], s["Q"]], 0)
    step([a["P"], s["P"]], (0, 1))  # (member 1's batch keeps its size)
    g.close()
