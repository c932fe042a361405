"""The DeduplicationID model (tests/quota_dedup_model.py) against the reference's own tests, the
coverage of the random batches the GPU parity tests replay, and the new C-ABI entry points (no GPU
needed)."""
import json
import os
import re

import pytest

import quota_dedup_model as QM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = json.load(open(os.path.join(HERE, "golden", "memquota_cases.json")))
REAPER = json.load(open(os.path.join(HERE, "golden", "memquota_reaper.json")))
BASE_NS = QM.BASE_NS
NEW_CALLS = ("mxp_quota_alloc_dedup", "mxp_quota_alloc_dedup_device", "mxp_quota_dedup_reap", "mxp_quota_dedup_stats")


def test_model_alloc_and_release():
    """TestAllocAndRelease (memquota_test.go:64-197): ids "A" + dedup / "R" + dedup, Amount of the
    alloc and of the release, and the alloc's ValidDuration (the exp column, :174)."""
    t = CASES["alloc_and_release"]
    names = list(t["limits"])
    ref = QM.DedupQuota({k: tuple(t["limits"][n]) for k, n in enumerate(names)})
    for name, dedup, aa, ar, abe, exp, sec, ra, rr in t["cases"]:
        now = BASE_NS + sec * 10**9
        k = names.index(name)
        g, valid, dup, _ = ref.handle(k, aa, abe, ("A" + dedup).encode(), now)
        assert (g, valid) == (ar, exp), (name, dedup)
        if aa == 0:
            assert (g, valid, dup) == (0, 0, 0)
        g, valid, dup, _ = ref.handle(k, -ra, False, ("R" + dedup).encode(), now)
        assert (g, valid) == (rr, 0), (name, dedup)
        if ra == 0:
            assert (g, valid, dup) == (0, 0, 0)


def test_model_reaper():
    """TestReaper (memquota_test.go:229-300)."""
    lim = REAPER["limit"]
    ref = QM.DedupQuota({0: (lim["max_amount"], lim["valid_duration_ns"])})
    for step in REAPER["steps"]:
        if step[0] == "reap":
            ref.reap()
            continue
        _, dedup, amount, want = step
        assert ref.handle(0, amount, False, dedup.encode(), BASE_NS)[0] == want, step


@pytest.fixture(scope="module")
def modelled():
    mx, vd, batches = QM.random_batches()
    return batches, QM.run_model(mx, vd, batches)


def test_random_batches_cover_every_path(modelled):
    """What the GPU parity tests can only show if the batches hold it: each count > 0."""
    batches, (out, cov) = modelled
    assert all(v > 0 for v in cov.values()), cov
    for keys, amounts, be, ids, now in batches:
        lens = {len(i) for i in ids}
        assert lens >= set(QM.FORCED_LENGTHS) and min(lens) == 0 and max(lens) == 70
        assert sum(1 for a, b in zip(ids[100:140:2], ids[101:140:2]) if a[:64] == b[:64] and a != b) >= 10
        repeats = len(ids) - len(set(ids))
        assert 0.2 * len(ids) < repeats < 0.45 * len(ids)
    # batches 0-2 alone (the masked-hash test) still hold hits, followers and other-key followers
    mx, vd, _ = QM.random_batches()
    _, cov3 = QM.run_model(mx, vd, batches[:3])
    assert cov3["hits_recent"] > 0 and cov3["followers"] > 0 and cov3["follower_other_key"] > 0


def declared():
    src = open(os.path.join(ROOT, "include", "mxp.h")).read()
    return set(re.findall(r"^int (mxp_quota_[a-z_]+)\(", src, re.M))


def test_new_entry_points_declared_and_exported(libmxp):
    assert set(NEW_CALLS) <= declared()
    for name in NEW_CALLS:
        assert hasattr(libmxp, name), name
    from istio_amd.engine import QuotaHandle
    for method in ("alloc_dedup", "alloc_dedup_device", "reap", "dedup_stats"):
        assert callable(getattr(QuotaHandle, method))
