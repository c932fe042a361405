#!/usr/bin/env python3
"""CheckPlan.check against what a caller had to do before it existed, in one process on one GPU:
  new   one mxp_check_batch: results, record offsets and records come back;
  old   a u16 Resolve (pinned outputs), one mxp_listentry_check per distinct unit, and the fold of
        the action lists on the host (tests/check_model.py's semantics, vectorised in numpy for the
        one-unit-per-rule plans used here).
All rules sit in one default namespace, variety 0, one blacklist unit shared by every rule.  The two
paths' calls alternate, each warmed; per workload one JSON line: median / min / max ms of both and
the bytes each brings back.  Once, outside the timing, the two paths' results are compared.
    python tools/check_timing.py [--kinds c2,c4] [--rules 10000] [--requests 1000000] [--reps 5]
(MXP_TRACE=1: the engines' timelines on stderr; MXP_CHECK_GROUP: the fold's lanes per request.)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S = 10 ** 9
DUR, USE, DEF = 5 * S, 100, (10 * S, 200)


def host_fold(mxp, status, off, codes):
    """the model's fold for one list unit on every rule: a request's units all see the same code"""
    n = len(status)
    cnt = np.diff(off.astype(np.int64))
    res = np.zeros(n, mxp.CHECK_RESULT)
    bad = status != 0
    has = ~bad & (cnt > 0) & (codes != -2)
    ev = has & (codes == -1)
    res["valid_duration_ns"] = np.where(has, np.where(ev, 0, DUR), DEF[0])
    res["valid_use_count"] = np.where(has, np.where(ev, 0, USE), DEF[1])
    res["code"] = np.where(bad, 13, np.where(has, np.maximum(codes, 0), np.where((cnt > 0) & (codes == -2), 13, 0)))
    res["n_records"] = np.where(bad | (codes == 0), 0, cnt)
    panic = ~bad & (cnt > 0) & (codes == -2)
    res["flags"] = (np.where(bad, mxp.CHECK_RESOLVE_ERROR, 0) | np.where(~bad & ~has, mxp.CHECK_NO_CHECKS, 0)
                    | np.where(ev, mxp.CHECK_EVAL_ERROR, 0) | np.where(panic, mxp.CHECK_UNIT_PANIC, 0))
    return res


def run(kind, n_rules, n_requests, reps):
    import istio_amd.engine as mxp
    from istio_amd import workloads as W
    from istio_amd.bags import STRING
    if kind == "c2":
        manifest, rules, batch = W.c2_workload(n_rules=n_rules, n_requests=n_requests)
        expr = "destination.service"
    else:
        manifest, rules, batch = W.c4_workload(n_rules=n_rules, n_requests=n_requests)
        expr = 'request.path | "none"'
    eng = mxp.Engine(0)
    eng.set_vocabulary(manifest)
    assert (eng.compile(rules) == 0).all()
    eng.set_resolver("destination.service", "istio-system", ["istio-system"] * n_rules, np.ones(n_rules, dtype=np.uint32),
                     np.zeros(n_rules, dtype=np.uint8), np.zeros(n_rules, dtype=np.uint8))
    inst = mxp.Engine(0)
    inst.set_vocabulary(manifest)
    assert (inst.compile(["true", expr]) == 0).all()
    col = batch.names.index(expr.split(" ")[0])
    seen = sorted({batch.string(int(v)) for k, v in zip(batch.kinds[col][:4096], batch.values[col][:4096]) if k == STRING})
    # (a blacklist, so that a record is the exception: C2 denies half its services, C4 -- hundreds of
    # selected rules per request, a record for each on a hit -- one path)
    lst = eng.list_create(mxp.ListHandle.STRINGS, seen[::2] if kind == "c2" else seen[:1])
    units = [mxp.list_unit(1, lst, True, DUR, USE, "denylist")]
    plan = mxp.CheckPlan(eng, inst, units, [[0]] * n_rules, DEF[0], DEF[1])
    n = batch.n

    def new():
        t0 = time.perf_counter()
        got = plan.check(batch, 0, cap=new.cap)
        return time.perf_counter() - t0, got

    def old():
        t0 = time.perf_counter()
        status, err_rule, off, ids = eng.resolve_arrays(batch, 0, cap=old.cap, ids16=True, pinned=True)
        codes = lst.check_entries(inst, batch, 1, True)
        res = host_fold(mxp, status, off, codes)
        return time.perf_counter() - t0, (status, err_rule, res, off, ids)

    new.cap, old.cap = 0, 0
    _, g = new()
    _, o = old()
    new.cap, old.cap = max(16, len(g[4])), max(16, len(o[4]))
    same = bool(np.array_equal(g[0], o[0]) and np.array_equal(g[1], o[1]) and g[2].tobytes() == o[2].tobytes())
    n_ids, n_recs = len(o[4]), len(g[4])
    ts = {"new": [], "old": []}
    for f in (new, old):
        f()
    for _ in range(reps):
        for name, f in (("new", new), ("old", old)):
            ts[name].append(f()[0] * 1e3)
    stat = lambda x: dict(median_ms=round(float(np.median(x)), 3), min_ms=round(min(x), 3), max_ms=round(max(x), 3))  # noqa: E731
    out = dict(workload=kind, rules=n_rules, requests=n, ids=n_ids, ids_per_request=round(n_ids / n, 2), records=n_recs,
               results_equal=same, group=os.environ.get("MXP_CHECK_GROUP", "auto"),
               check_plan=dict(stat(ts["new"]), bytes_back=n * (1 + 4 + 24) + 8 * (n + 1) + 24 * n_recs),
               resolve_listentry_fold=dict(stat(ts["old"]), bytes_back=n * (1 + 4) + 8 * (n + 1) + 2 * n_ids + 4 * n))
    print(json.dumps(out), flush=True)
    plan.close()
    inst.close()
    eng.close()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--kinds", default="c2,c4")
    p.add_argument("--rules", type=int, default=10000)
    p.add_argument("--requests", type=int, default=1000000)
    p.add_argument("--reps", type=int, default=5)
    a = p.parse_args()
    from istio_amd import build
    build.build()
    for kind in a.kinds.split(","):
        run(kind, a.rules, a.requests, a.reps)


if __name__ == "__main__":
    main()
