"""The hand-off of deferred index pairs from mxp_dtp_sort_kernel to mxp_fill_dtp_kernel at C2's pair
density (kernels.hip "Deferred pairs"): the sort walks a tile's 16 wave lists as one concatenated
range (short tiles in one step of 4 entries per thread, long ones in steps of 16) and writes the
quads' count bytes four to a store; it never clears a slot row, so the fill must take nothing from
a row whose count is zero, whatever an earlier evaluation left there.  C2 family (every indexed
group is a plain fill chunk, so mxp_fill_dtp_kernel is the consumer).  Bar: device
match bitmap, error bitmap, compact flags and hit counters identical to the engine with deferred
pairs off (MXP_DTP=0), and bit-exact against the oracle where noted."""
import numpy as np
import pytest

import oracle
from istio_amd import workloads as W
from test_gpu_dtp import PATHS, deferred_ran, engine_for
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu

N_RULES, N_SERVICES = 600, 6  # 100 rules per service: a path-less request errors on 100 rules
SIZES = [1, 63, 64, 65, 1023, 1025, 3 * 1024 + 77]


@pytest.fixture(scope="module")
def mxp(libmxp):
    import istio_amd.engine as mxp
    return mxp


@pytest.fixture(scope="module")
def pool():
    """A C2 request pool with its oracle matrix (computed once): requests by pair count -- `zero`
    (no true or error pair on any rule), `light` (1-3 pairs), `heavy` (path-less: an error pair on
    each of its service's 100 rules)."""
    manifest, rules, big = W.c2_workload(n_rules=N_RULES, n_requests=6000, seed=61, n_services=N_SERVICES,
                                         p_missing_path=0.2)
    want = oracle.oracle_matrix(oracle.OracleEvaluator(manifest), rules, big, threads=16)
    cnt = (want >= 1).sum(axis=1)
    p = {"manifest": manifest, "rules": rules, "big": big, "want": want, "cnt": cnt,
         "zero": np.flatnonzero(cnt == 0), "light": np.flatnonzero((cnt >= 1) & (cnt <= 3)),
         "heavy": np.flatnonzero(cnt >= 100)}
    assert len(p["zero"]) > 500 and len(p["light"]) > 50 and len(p["heavy"]) > 300
    return p


def wave_counts(cnt_rows):
    """Pairs per 64 consecutive requests (an index wave's list length before clamping)."""
    return np.add.reduceat(cnt_rows, np.arange(0, len(cnt_rows), 64))


def ragged_order(pool, n, seed=5):
    """Request rows for a batch of n: each tile of 16 waves holds a wave of 14 heavy requests (1400
    pairs: > 1024, under the list capacity), one of 64 heavy (6400: clamped to the capacity, the rest
    to the overflow list), an empty wave, one with a handful and one of 4 heavy (400: > 256), then 11
    waves drawn from the whole pool; the wave classes rotate by the tile index, so the ragged last
    tile and the last wave start with pair-bearing requests.  Heavy requests lead their wave."""
    rng = np.random.default_rng(seed)
    z, l, h = pool["zero"], pool["light"], pool["heavy"]

    def wave(kind):
        if kind == "A":
            return np.concatenate([rng.choice(h, 14), rng.choice(z, 50)])
        if kind == "E":
            return rng.choice(h, 64)
        if kind == "B":
            return rng.choice(z, 64)
        if kind == "C":
            return np.concatenate([rng.choice(l, 3), rng.choice(z, 61)])
        if kind == "D":
            return np.concatenate([rng.choice(h, 4), rng.choice(z, 60)])
        return rng.integers(0, pool["big"].n, 64)
    base = ["A", "E", "B", "C", "D"] + ["R"] * 11
    rows = []
    for t in range((n + 1023) // 1024):
        for w in range(16):
            rows.append(wave(base[(w + t) % 16]))
    return np.concatenate(rows)[:n]


class Bufs:
    """Device output buffers of one shape, reused across evaluations."""

    def __init__(self, R, n):
        import torch
        Wd = (R + 31) // 32
        self.dm = torch.full((Wd, n), -1, dtype=torch.int32, device="cuda:0")
        self.de = torch.full_like(self.dm, -1)
        self.cm = torch.full_like(self.dm, -1)
        self.flags = torch.ones(n, dtype=torch.uint8, device="cuda:0")  # (stale flags must be cleared)
        self.hits = torch.zeros(R, dtype=torch.int64, device="cuda:0")
        self.hc = torch.zeros_like(self.hits)

    def run(self, eng, batch, reps=2):
        """[match, error, hits, compact match, compact flags, compact hits] after `reps` evaluations
        of each output form (the fused / streamed hit-counter choice follows the previous one)."""
        import torch
        db = eng.upload(batch)
        for _ in range(reps):
            db.eval_hits(self.dm.data_ptr(), self.de.data_ptr(), self.hits.data_ptr(), 0)
            db.eval_compact(self.cm.data_ptr(), self.flags.data_ptr(), self.hc.data_ptr(), 0)
        torch.cuda.synchronize()
        out = [x.cpu().numpy().copy() for x in (self.dm, self.de, self.hits, self.cm, self.flags, self.hc)]
        db.free()
        return out


def dtp_lists(eng, batch, R):
    """({"waves", "fills", "vtfills", "cap"}, wave list lengths) of one evaluation of `batch`."""
    import torch
    db = eng.upload(batch)
    dm = torch.zeros(((R + 31) // 32, batch.n), dtype=torch.int32, device="cuda:0")
    de = torch.zeros_like(dm)
    hits = torch.zeros(R, dtype=torch.int64, device="cuda:0")
    db.eval_hits(dm.data_ptr(), de.data_ptr(), hits.data_ptr(), 0)
    out = db.dtp_lists()
    db.free()
    return out


def same(a, b, what):
    for x, y, name in zip(a, b, ("match", "error", "hits", "compact match", "compact flags", "compact hits")):
        assert np.array_equal(x, y), (what, name)


def test_ragged_lists(mxp, monkeypatch, pool):
    """Wave lists of 0, a handful, > 256 and > 1024 entries inside one tile, batches whose last tile
    has fewer than 16 waves and whose last wave has fewer than 64 lanes; lists, overflow list and
    re-run (MXP_DTP_CAP / MXP_DTP_OVF) against MXP_DTP=0, the full batch also against the oracle."""
    manifest, rules = pool["manifest"], pool["rules"]
    R = len(rules)
    order = ragged_order(pool, SIZES[-1])
    wc = wave_counts(pool["cnt"][order])
    print("pairs per wave, tile 0:", wc[:16].tolist(), "last tile:", wc[48:].tolist())
    for tile in (wc[:16], wc):  # every class inside the first tile (and so in the batch)
        assert (tile == 0).any() and ((tile >= 1) & (tile <= 16)).any()
        assert ((tile > 256) & (tile <= 1024)).any() and ((tile > 1024) & (tile <= 2080)).any() and (tile > 2080).any()
    assert wc[48] > 0 and wc[49] > 0  # the ragged last tile's two waves (the last one: 13 lanes)
    batches = {n: pool["big"].subset(order[:n]) for n in SIZES}
    ref_eng = engine_for(mxp, monkeypatch, {"MXP_DTP": "0"}, manifest, rules, flags="0")
    assert not deferred_ran(ref_eng, batches[SIZES[-1]], R)
    ref = {n: Bufs(R, n).run(ref_eng, b) for n, b in batches.items()}
    for env in PATHS:
        eng = engine_for(mxp, monkeypatch, env, manifest, rules, flags="0")
        assert deferred_ran(eng, batches[SIZES[-1]], R)
        for n in SIZES + SIZES[::-1][1:]:  # up, then down again: smaller batches over larger ones' scratch
            same(Bufs(R, n).run(eng, batches[n]), ref[n], (env, n))
        if not env:
            got, want = compare(eng, oracle.OracleEvaluator(manifest), rules, batches[SIZES[-1]], sample_msgs=200)
            assert np.array_equal(want, pool["want"][order])
    assert ref[SIZES[-1]][2].sum() > 0 and ref[SIZES[-1]][1].any() and ref[SIZES[-1]][4].any()


def test_stale_rows_under_zero_counts(mxp, monkeypatch, pool):
    """One engine, one set of output buffers: a dense batch P (heavy requests: far more than 8
    pairs of a quad in one chunk), a batch Z with no pairs at all (no request's service occurs in a
    rule), P again; then batches whose non-empty quads sit beside empty ones in a 64-byte line of
    slot rows (every fourth quad; only the first and last quad of a fill wave's 256 requests), Z and
    P once more.  Every result equals MXP_DTP=0; Z is all zero and moves no hit counter."""
    manifest, rules, big = pool["manifest"], pool["rules"], pool["big"]
    R, n = len(rules), 2048 + 37
    rng = np.random.default_rng(9)
    z, l, h = pool["zero"], pool["light"], pool["heavy"]
    busy = np.concatenate([h, l])
    p_rows = np.where(rng.random(n) < 0.5, rng.choice(h, n), rng.integers(0, big.n, n))
    P = big.subset(p_rows)
    q = np.arange(n) // 4
    P4 = big.subset(np.where(q % 4 == 0, rng.choice(busy, n), rng.choice(z, n)))
    Pe = big.subset(np.where((q % 64 == 0) | (q % 64 == 63), rng.choice(h, n), rng.choice(z, n)))
    _, _, other = W.c2_workload(n_rules=N_RULES, n_requests=8 * n, seed=62, n_services=2 * N_SERVICES,
                                p_missing_path=0.2)
    svc = other.values[list(other.names).index("destination.service")]
    Z = other.subset(np.flatnonzero(svc >= N_SERVICES)[:n])
    assert Z.n == n
    seq = [("P", P), ("Z", Z), ("P", P), ("P4", P4), ("Z", Z), ("Pe", Pe), ("P4", P4), ("P", P)]
    ref_eng = engine_for(mxp, monkeypatch, {"MXP_DTP": "0"}, manifest, rules, flags="0")
    rb = Bufs(R, n)
    ref = [rb.run(ref_eng, b) for _, b in seq]
    eng = engine_for(mxp, monkeypatch, {}, manifest, rules, flags="0")
    assert deferred_ran(eng, Z, R) and deferred_ran(eng, P, R)
    # a quad with 8 or more pairs in one chunk: P's fullest request has `most` pairs by the oracle,
    # spread over `fills` plain fill chunks, so one chunk holds at least most / fills of them
    shape, lens = dtp_lists(eng, P, R)
    most = int(pool["cnt"][p_rows].max())
    print("fill chunks:", shape, "most pairs of one request:", most, "entries in the lists:", int(lens.sum()))
    assert shape["fills"] >= 1 and shape["vtfills"] == 0 and most >= 8 * shape["fills"]
    assert lens.sum() > 0
    gb = Bufs(R, n)
    got = []
    for k, (name, b) in enumerate(seq):
        got.append(gb.run(eng, b))
        same(got[k], ref[k], (k, name))
        if name == "Z":
            assert not got[k][0].any() and not got[k][1].any() and not got[k][3].any() and not got[k][4].any()
            assert np.array_equal(got[k][2], got[k - 1][2]) and np.array_equal(got[k][5], got[k - 1][5])
    # P's bitmaps: the same at every visit (hit counters accumulate)
    for k in (2, 7):
        for i in (0, 1, 3, 4):
            assert np.array_equal(got[k][i], got[0][i])
    assert got[0][1].any() and got[0][2].sum() > 0 and got[3][1].any() and got[5][1].any()
    compare(eng, oracle.OracleEvaluator(manifest), rules, P4, sample_msgs=100)


def test_more_than_one_window(mxp, monkeypatch):
    """17k C2 rules (over 32 plain fill chunks: two chunk windows in the sort), a ragged batch with
    path-less requests: equal to MXP_DTP=0."""
    manifest, rules, batch = W.c2_workload(n_rules=17_000, n_requests=1024 + 5, seed=63, n_services=64,
                                           p_missing_path=0.1)
    R = len(rules)
    outs = []
    for env in ({}, {"MXP_DTP": "0"}):
        eng = engine_for(mxp, monkeypatch, env, manifest, rules, flags="0")
        assert deferred_ran(eng, batch, R) == (not env)
        if not env:  # more plain fill chunks than one window of 32 (MXP_DTP_WIN) holds
            shape, _ = dtp_lists(eng, batch, R)
            print("fill chunks:", shape)
            assert shape["fills"] > 32 and shape["vtfills"] == 0
        outs.append(Bufs(R, batch.n).run(eng, batch))
    same(outs[0], outs[1], "windows")
    assert outs[0][1].any() and outs[0][2].sum() > 0
