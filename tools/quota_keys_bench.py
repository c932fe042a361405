#!/usr/bin/env python3
"""QuotaPlan.batch against the replay it feeds, in one process on one GPU, the profiler off:
  batch   one mxp_quota_batch: instance evaluation, Resolve, key stage, replay, answers -- the host
          arrays in, the 24-byte answers back;
  replay  mxp_quota_alloc_dedup_device on the same key ids, amounts and DeduplicationIDs, already on
          the device: the replay alone, which is all the device did for Quota before the key stage.
workloads.quota_instance_workload; the two calls alternate after two warm-up rounds; `now` advances
100 ms a round and the dedup state is reaped every round, so every round replays.  One JSON line:
median / min / max ms of both, the codes' counts, the keys interned.
    python tools/quota_keys_bench.py [--rules 1000] [--requests 1000000] [--keys 1024] [--reps 5]
(MXP_TRACE=1: the engines' timelines on stderr.)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rules", type=int, default=1000)
    p.add_argument("--requests", type=int, default=1000000)
    p.add_argument("--keys", type=int, default=1024)
    p.add_argument("--reps", type=int, default=5)
    a = p.parse_args()
    from istio_amd import build
    build.build()
    import torch
    import istio_amd.engine as mxp
    from istio_amd import workloads as W
    w = W.quota_instance_workload(n_rules=a.rules, n_requests=a.requests, n_keys=a.keys)
    c = w["conf"]
    eng = mxp.Engine(0)
    eng.set_vocabulary(w["manifest"])
    assert (eng.compile(w["rules"]) == 0).all()
    eng.set_resolver(c["identity_attr"], c["default_ns"], c["rule_ns"], c["variety_mask"], c["is_tcp"], c["empty_match"])
    inst = mxp.Engine(0)
    inst.set_vocabulary(w["manifest"])
    assert (inst.compile(w["inst_rules"]) == 0).all()
    plan = mxp.QuotaPlan(eng, inst, w["limits"], w["units"], w["rule_unit"])
    batch, amounts, be, ids = w["batch"], w["amounts"], w["best_effort"], w["ids"]
    n = batch.n
    now = 1_500_000_000 * 10 ** 9
    packed = plan.pack_ids(ids)  # (outside the timing: a binding holds its ids as bytes already)
    _, _, first = plan.batch(batch, W.QUOTA_VARIETY, amounts, be, now, packed)
    codes, counts = np.unique(first["code"], return_counts=True)
    # the replay alone: a plain quota with the plan's limits per id, the first call's key ids
    lim = w["limits"][0]
    caps = [lim["key_cap"]] + [o["key_cap"] for o in lim["overrides"]]
    mx = np.concatenate([np.full(k, x["max_amount"], dtype=np.int64) for k, x in zip(caps, [lim] + lim["overrides"])])
    vd = np.concatenate([np.full(k, x["valid_duration_ns"], dtype=np.int64) for k, x in zip(caps, [lim] + lim["overrides"])])
    q = eng.quota_create(mx, vd)
    keyed = (first["code"] == 0) & (first["key"] != mxp.QUOTA_NO_KEY)
    off = packed[1]
    blob = b"".join(ids)
    # (requests that did not reach HandleQuota: amount 0 under a key id past n_keys, as the plan passes them)
    dk = torch.from_numpy(np.where(keyed, first["key"], mxp.QUOTA_NO_KEY).astype(np.uint32).view(np.int32)).cuda()
    da = torch.from_numpy(np.where(keyed, amounts, 0).astype(np.int64)).cuda()
    db = torch.from_numpy(be.copy()).cuda()
    di = torch.from_numpy(np.frombuffer(blob + bytes(16), dtype=np.uint8).copy()).cuda()
    do = torch.from_numpy(off.view(np.int32).copy()).cuda()
    dg = torch.zeros(n, dtype=torch.int64, device="cuda")
    dv = torch.zeros(n, dtype=torch.int64, device="cuda")
    dd = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def run_batch(t):
        plan.reap()
        t0 = time.perf_counter()
        plan.batch(batch, W.QUOTA_VARIETY, amounts, be, t, packed)
        return (time.perf_counter() - t0) * 1e3

    def run_replay(t):
        q.reap()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        q.alloc_dedup_device(n, dk.data_ptr(), da.data_ptr(), db.data_ptr(), di.data_ptr(), do.data_ptr(), len(blob), t, 0,
                             dg.data_ptr(), dv.data_ptr(), dd.data_ptr())
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    ts = {"batch": [], "replay": []}
    for r in range(2 + a.reps):
        now += 100_000_000
        tb, tr = run_batch(now), run_replay(now)
        if r >= 2:
            ts["batch"].append(tb)
            ts["replay"].append(tr)
    stat = lambda x: dict(median_ms=round(float(np.median(x)), 3), min_ms=round(min(x), 3), max_ms=round(max(x), 3))  # noqa: E731
    st = plan.stats()
    print(json.dumps(dict(requests=n, rules=a.rules, popular_keys=a.keys, keys_interned=st["keys"], pool_bytes=st["pool_bytes"],
                          codes={int(k): int(v) for k, v in zip(codes, counts)}, quota_batch=stat(ts["batch"]),
                          replay_alone=stat(ts["replay"]))), flush=True)
    plan.close()
    inst.close()
    eng.close()


if __name__ == "__main__":
    main()
