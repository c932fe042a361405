#!/usr/bin/env python3
"""The end-to-end Resolve call with u16 ids against the delta-coded stream (MXP_RESOLVE_IDS_U16 /
MXP_RESOLVE_IDS_DELTA8), in one process on one GPU.  The set-up is bench.py's end_to_end block: all
rules in one default namespace, variety 0, pinned narrow shards and pinned outputs, one call = the
narrow upload (MXP_UPLOAD_NO_WAIT) + mxp_group_resolve_uploaded.  The two formats' calls alternate,
each warmed; per workload one JSON line: median / min / max ms per batch of both, the bytes brought
back, their ratio and the escapes' share of the ids.  Once, outside the timing, the decoded stream
is compared with the u16 list.
    python tools/e2e_delta8.py [--kinds c4,c2] [--rules 10000] [--requests 1048576] [--reps 7] [--no-verify]
(MXP_TRACE=1: the engine's timeline of every call on stderr.)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def verify(off, ids, boff, stream, chunk=32768):
    """decode_delta8(stream) == the u16 list, a chunk of requests at a time"""
    from istio_amd.engine import decode_delta8
    n = len(off) - 1
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        o, d = decode_delta8(boff[lo:hi + 1], stream)
        a = int(off[lo])
        if not (np.array_equal(o, off[lo:hi + 1] - off[lo]) and np.array_equal(d, ids[a:int(off[hi])])):
            return False
    return True


def run(kind, n_rules, n_requests, reps, check):
    from istio_amd.engine import PinnedArena
    args = bench.parse(["--gen-procs", "1", "--fresh-steps", "0", "--rules", str(n_rules), "--requests", str(n_requests)])
    data = bench.Data(args, 1, {kind})
    manifest, rules = bench.rule_set(kind, n_rules)
    g = bench.make_group([0])
    g.set_vocabulary(manifest)
    assert (g.compile(rules) == 0).all()
    g.set_resolver("destination.service", "istio-system", ["istio-system"] * n_rules,
                   np.ones(n_rules, dtype=np.uint32), np.zeros(n_rules, dtype=np.uint8), np.zeros(n_rules, dtype=np.uint8))
    sets, _h2d, _keep = bench.host_sets([data.shards(kind)], "narrow")
    st = sets[0]
    n = sum(b.n for b in st)
    wide = [getattr(b, "batch", b) for b in st]
    fmts = {"u16": dict(ids16=True), "delta8": dict(delta8=True)}
    # sizes (and the lists to compare) from the one-shot call, which retries when its capacity is short
    ref = {k: [x.copy() for x in g.resolve_arrays(wide, 0, **f)] for k, f in fmts.items()}
    n_ids, n_bytes = len(ref["u16"][3]), len(ref["delta8"][3])
    ok = None
    if check:
        ok = bool(np.array_equal(ref["u16"][0], ref["delta8"][0]) and np.array_equal(ref["u16"][1], ref["delta8"][1])
                  and verify(ref["u16"][2], ref["u16"][3], ref["delta8"][2], ref["delta8"][3]))
    cap = {"u16": max(16, 2 * n_ids), "delta8": max(16, 2 * n_bytes)}
    isz = {"u16": 2, "delta8": 1}
    out = {}
    for k in fmts:
        arena = PinnedArena(n * 13 + 8 + cap[k] * isz[k] + 4 * 64)
        out[k] = (arena, (arena.empty(n, np.uint8), arena.empty(n, np.uint32), arena.empty(n + 1, np.uint64),
                          arena.empty(cap[k], np.uint16 if k == "u16" else np.uint8)))
    del ref

    def call(k):
        t0 = time.perf_counter()
        got = g.resolve_arrays(None, 0, cap[k], out=out[k][1], uploaded=bench.upload_set(g, st, "narrow", True), **fmts[k])
        return time.perf_counter() - t0, got
    ts = {k: [] for k in fmts}
    for k in fmts:  # warm-up (allocations)
        for _ in range(2):
            call(k)
    for _ in range(reps):
        for k in fmts:
            t, got = call(k)
            ts[k].append(t * 1e3)
            assert int(got[2][-1]) == (n_ids if k == "u16" else n_bytes)
    g.close()
    res = {"workload": kind, "rules": n_rules, "requests": n, "reps": reps, "ids": n_ids, "ids_per_request": n_ids / max(n, 1),
           "escape_share_of_ids": (n_bytes - n_ids) / 2 / max(n_ids, 1), "bytes_ratio": n_bytes / max(2 * n_ids, 1),
           "decoded_equals_u16": ok}
    for k in fmts:
        res[k] = {"ms_median": float(np.median(ts[k])), "ms_min": float(np.min(ts[k])), "ms_max": float(np.max(ts[k])),
                  "bytes": n_ids * 2 if k == "u16" else n_bytes}
    res["ms_ratio"] = res["delta8"]["ms_median"] / res["u16"]["ms_median"]
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--kinds", default="c4,c2")
    p.add_argument("--rules", type=int, default=10000)
    p.add_argument("--requests", type=int, default=1 << 20)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--no-verify", action="store_true")
    a = p.parse_args()
    from istio_amd import build
    build.build()
    for kind in a.kinds.split(","):
        print(json.dumps(run(kind, a.rules, a.requests, max(a.reps, 1), not a.no_verify)), flush=True)


if __name__ == "__main__":
    main()
