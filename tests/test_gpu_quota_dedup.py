"""GPU memquota with DeduplicationIDs (mxp_quota_alloc_dedup, mxp_quota_dedup_reap) against the
reference's own tests and the model (tests/quota_dedup_model.py).  Bar: identical granted amounts,
ValidDurations and dup flags; no Python-side map anywhere."""
import json
import os

import numpy as np
import pytest

import quota_dedup_model as QM
from istio_amd import workloads as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "memquota_cases.json")))
REAPER = json.load(open(os.path.join(HERE, "golden", "memquota_reaper.json")))
BASE_NS = QM.BASE_NS


@pytest.fixture(scope="module")
def eng(libmxp):
    import istio_amd.engine as mxp
    return mxp.Engine(0)


@pytest.fixture(scope="module")
def modelled():
    """The random batches and the model's answers, computed once."""
    mx, vd, batches = QM.random_batches()
    out, cov = QM.run_model(mx, vd, batches)
    out3, cov3 = QM.run_model(mx, vd, batches[:3])
    return mx, vd, batches, out, cov, out3


def table_rows():
    """TestAllocAndRelease as requests: per row the alloc "A" + dedup, then the release "R" + dedup."""
    t = CASES["alloc_and_release"]
    names = list(t["limits"])
    rows = []
    for name, dedup, aa, ar, abe, exp, sec, ra, rr in t["cases"]:
        k = names.index(name)
        rows.append((sec, k, aa, int(abe), ("A" + dedup).encode(), ar, exp))
        rows.append((sec, k, -ra, 0, ("R" + dedup).encode(), rr, 0))
    limits = [t["limits"][n] for n in names]
    return limits, rows


def test_reference_table_one_request_per_call(eng):
    limits, rows = table_rows()
    q = eng.quota_create([l[0] for l in limits], [l[1] for l in limits])
    for sec, k, amount, be, did, want, exp in rows:
        g, v, d = q.alloc_dedup([k], [amount], [be], [did], BASE_NS + sec * 10**9)
        assert (int(g[0]), int(v[0])) == (want, exp), (did, amount)
        if amount == 0:
            assert int(d[0]) == 0


def test_reference_table_batched(eng):
    """All rows of one `seconds` value as one batch, in table order: A0 twice and R5b twice inside
    the first batch."""
    limits, rows = table_rows()
    q = eng.quota_create([l[0] for l in limits], [l[1] for l in limits])
    seconds = list(dict.fromkeys(r[0] for r in rows))
    for sec in seconds:
        part = [r for r in rows if r[0] == sec]
        g, v, d = q.alloc_dedup([r[1] for r in part], [r[2] for r in part], [r[3] for r in part],
                                [r[4] for r in part], BASE_NS + sec * 10**9)
        assert g.tolist() == [r[5] for r in part], sec
        assert v.tolist() == [r[6] for r in part], sec
    first = [r[4] for r in rows if r[0] == seconds[0]]
    assert first.count(b"A0") == 2 and first.count(b"R5b") == 2


@pytest.mark.parametrize("batched", [False, True])
def test_reaper_fixture(eng, batched):
    """TestReaper: one request per call, then the requests between two reaps as one batch."""
    lim = REAPER["limit"]
    q = eng.quota_create([lim["max_amount"]], [lim["valid_duration_ns"]])
    group = []

    def flush():
        if group:
            g, _, _ = q.alloc_dedup([0] * len(group), [s[2] for s in group], [0] * len(group),
                                    [s[1].encode() for s in group], BASE_NS)
            assert g.tolist() == [s[3] for s in group], group
            group.clear()
    for step in REAPER["steps"]:
        if step[0] == "reap":
            flush()
            q.reap()
        else:
            group.append(step)
            if not batched:
                flush()
    flush()


def run_parity(q, batches, want, reap_after, device=False):
    for b, (keys, amounts, be, ids, now) in enumerate(batches):
        wg, wv, wd, wr = want[b]
        if device:
            g, v, d, delta = alloc_device(q, keys, amounts, be, ids, now)
            want_delta = np.zeros(QM.N_KEYS, dtype=np.int64)
            rep = wr.astype(bool)
            np.add.at(want_delta, keys[rep].astype(np.int64), (np.sign(amounts) * wg)[rep])  # replayed allocs - frees
            assert np.array_equal(delta, want_delta), b
        else:
            g, v, d = q.alloc_dedup(keys, amounts, be, ids, now)
        for name, got, exp in (("granted", g, wg), ("valid_ns", v, wv), ("dup", d, wd)):
            bad = np.nonzero(got != exp)[0]
            assert bad.size == 0, (b, name, bad[:5], got[bad[:5]], exp[bad[:5]], [ids[i] for i in bad[:5]])
        if b in reap_after:
            q.reap()


def alloc_device(q, keys, amounts, be, ids, now):
    import torch
    n = len(keys)
    blob = b"".join(ids)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(i) for i in ids])
    dk = torch.from_numpy(keys.view(np.int32).copy()).cuda()
    da = torch.from_numpy(amounts.copy()).cuda()
    db = torch.from_numpy(be.copy()).cuda()
    di = torch.from_numpy(np.frombuffer(blob + bytes(16), dtype=np.uint8).copy()).cuda()  # (16 bytes of slack)
    do = torch.from_numpy(off.astype(np.uint32).view(np.int32).copy()).cuda()
    dg = torch.full((n,), 99, dtype=torch.int64, device="cuda")
    dv = torch.full((n,), 99, dtype=torch.int64, device="cuda")
    dd = torch.full((n,), 99, dtype=torch.uint8, device="cuda")
    delta = torch.zeros(QM.N_KEYS, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    q.alloc_dedup_device(n, dk.data_ptr(), da.data_ptr(), db.data_ptr(), di.data_ptr(), do.data_ptr(), len(blob), now, 0,
                         dg.data_ptr(), dv.data_ptr(), dd.data_ptr(), delta.data_ptr())
    torch.cuda.synchronize()
    return dg.cpu().numpy(), dv.cpu().numpy(), dd.cpu().numpy(), delta.cpu().numpy()


@pytest.mark.parametrize("device", [False, True])
def test_random_parity(eng, modelled, device):
    """200 keys, 6 batches of 10,000, reaps after batches 2, 3 and 5; through the device form also
    d_delta against the model's replayed grants."""
    mx, vd, batches, out, cov, _ = modelled
    assert all(c > 0 for c in cov.values()), cov
    q = eng.quota_create(mx, vd)
    run_parity(q, batches, out, QM.REAP_AFTER, device=device)


def test_masked_hash_parity(eng, modelled, monkeypatch):
    """MXP_QDD_HASH_BITS=4: sixteen stored hashes for 30,000 ids, so only the byte compare tells ids
    apart."""
    monkeypatch.setenv("MXP_QDD_HASH_BITS", "4")
    mx, vd, batches, _, _, out3 = modelled
    q = eng.quota_create(mx, vd)
    run_parity(q, batches[:3], out3, QM.REAP_AFTER)


def test_growth(eng, monkeypatch):
    """From 64 slots: three batches of 4,000 distinct ids, then one repeating ids of each."""
    monkeypatch.setenv("MXP_QDD_SLOTS", "64")
    mx, vd, keys, amounts, be = W.quota_workload(n_keys=50, n_requests=15000, seed=59, p_zero=0.0)
    q = eng.quota_create(mx, vd)
    ref = QM.DedupQuota({k: (int(mx[k]), int(vd[k])) for k in range(50)})
    ids = [b"growth-%05d-" % i + bytes([65 + i % 26]) * (i % 40) for i in range(12000)]
    ids += [ids[j] for j in range(0, 12000, 4)]  # 3,000 repeats, a quarter of each batch
    now = BASE_NS
    for lo, hi in ((0, 4000), (4000, 8000), (8000, 12000), (12000, 15000)):
        g, v, d = q.alloc_dedup(keys[lo:hi], amounts[lo:hi], be[lo:hi], ids[lo:hi], now)
        want = np.array([ref.handle(int(k), int(a), bool(e), i, now)[:3]
                         for k, a, e, i in zip(keys[lo:hi], amounts[lo:hi], be[lo:hi], ids[lo:hi])])
        assert np.array_equal(g, want[:, 0]) and np.array_equal(v, want[:, 1]) and np.array_equal(d, want[:, 2]), lo
        now += 200_000_000
    assert d.all()
    st = q.dedup_stats()
    assert st["recent_ids"] >= 12000 and st["recent_slots"] >= 2 * st["recent_ids"], st
    assert st["recent_ids"] == 12000 and st["old_ids"] == 0 and st["recent_pool_bytes"] >= sum(map(len, ids[:12000]))


def test_lowest_arrival_index_wins(eng):
    """Id X at index 5 (alloc 3, key a) and at index 70,000 (alloc 9, key b, best effort), every other
    id unique: both get 3 and key b is charged nothing."""
    n = 70001
    q = eng.quota_create([10, 10, 1 << 40], [0, 0, 0])
    keys = np.full(n, 2, dtype=np.uint32)
    amounts = np.ones(n, dtype=np.int64)
    be = np.zeros(n, dtype=np.uint8)
    ids = [b"u%d" % i for i in range(n)]
    keys[5], amounts[5], ids[5] = 0, 3, b"X"
    keys[n - 1], amounts[n - 1], be[n - 1], ids[n - 1] = 1, 9, 1, b"X"
    g, v, d = q.alloc_dedup(keys, amounts, be, ids, BASE_NS)
    assert (int(g[5]), int(d[5])) == (3, 0) and (int(g[n - 1]), int(d[n - 1])) == (3, 1)
    assert g.sum() == n - 2 + 6 and d.sum() == 1
    # key b is untouched: all 10 are still there; key a holds 3
    assert q.alloc([1, 0], [10, 8], [0, 0], BASE_NS).tolist() == [10, 0]


def test_mixing_plain_and_dedup_calls(eng):
    """alloc, alloc_dedup, alloc on one quota: one key state, and the plain calls neither read nor
    fill the dedup state."""
    mx, vd, keys, amounts, be = W.quota_workload(n_keys=20, n_requests=3000, seed=63)
    q = eng.quota_create(mx, vd)
    ref = QM.DedupQuota({k: (int(mx[k]), int(vd[k])) for k in range(20)})
    ids = [b"mix-%d" % (i % 700) for i in range(3000)]
    now = BASE_NS
    for part, dedup in ((slice(0, 1000), False), (slice(1000, 2000), True), (slice(2000, 3000), False),
                        (slice(0, 1000), True)):
        k, a, e, i = keys[part], amounts[part], be[part], ids[part]
        if dedup:
            g, v, d = q.alloc_dedup(k, a, e, i, now)
            want = np.array([ref.handle(int(kk), int(aa), bool(ee), ii, now)[:3] for kk, aa, ee, ii in zip(k, a, e, i)])
            assert np.array_equal(g, want[:, 0]) and np.array_equal(v, want[:, 1]) and np.array_equal(d, want[:, 2])
        else:
            g = q.alloc(k, a, e, now)
            want = np.array([ref.q.handle(int(kk), int(aa), bool(ee), now) for kk, aa, ee in zip(k, a, e)])
            assert np.array_equal(g, want)
        now += 300_000_000
    assert q.dedup_stats()["recent_ids"] == len(ref.recent) > 600


def test_host_checks(eng):
    """A decreasing id_off, id_off[0] != 0 and a key >= n_keys are MXP_ERR_ARG naming the request; the
    same handle then answers a good batch exactly."""
    from istio_amd.engine import MxpError
    q = eng.quota_create([10, 10], [0, 10**9])
    for keys, off, what in (([0, 1, 0], [0, 4, 2, 6], "request 1"), ([0, 1, 0], [1, 2, 4, 6], "request 0"),
                            ([0, 2, 0], [0, 2, 4, 6], "request 1")):
        with pytest.raises(MxpError) as ex:
            q.alloc_dedup(keys, [1, 1, 1], [0, 0, 0], b"abcdef", BASE_NS, id_off=off)
        assert "failed (1)" in str(ex.value) and what in str(ex.value)  # MXP_ERR_ARG
    g, v, d = q.alloc_dedup([0, 1, 0, 1], [4, 4, 4, -1], [0, 0, 0, 0], [b"ab", b"cd", b"ab", b"cd"], BASE_NS)
    assert (g.tolist(), v.tolist(), d.tolist()) == ([4, 4, 4, 4], [0, 10**9, 0, 0], [0, 0, 1, 1])
    assert q.dedup_stats()["recent_ids"] == 2
