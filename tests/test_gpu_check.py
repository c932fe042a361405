"""mxp_check_batch (include/mxp.h; check.cpp, check.hip): the batched Check against
tests/check_model.py (a transcription of the Go, pinned by test_check_model.py) fed with outputs
that are pinned elsewhere: the same engine's u16 Resolve (test_gpu_resolver.py / test_gpu_delta8.py)
and mxp_listentry_check per distinct (value_rule, list, blacklist) (test_gpu_lists.py).  Nothing
expected here comes from the code under test.

Left out: a batch uploaded narrow (mxp_batch_upload2) -- the plan takes host batches only; device
groups (mxp_group_check_* is the follow-up)."""
import ctypes

import numpy as np
import pytest

import check_model as M
from istio_amd import workloads as W
from istio_amd.bags import ABSENT, INT64, STRING, BagBatch
from istio_amd.workloads import c2_resolve_case

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_NOMEM = 1, 4
S = 10 ** 9


@pytest.fixture(scope="module")
def mxp(libmxp):
    import istio_amd.engine as mxp
    return mxp


def make_engine(mxp, manifest, rules, conf):
    eng = mxp.Engine(0)
    eng.set_vocabulary(manifest)
    eng.compile(rules)
    eng.set_resolver(conf["identity_attr"], conf["default_ns"], conf["rule_ns"], conf["variety_mask"],
                     conf["is_tcp"], conf["empty_match"])
    return eng


def listentry(inst, lst, batch, value_rule, blacklist):
    """mxp_listentry_check -> (codes, Value registers, Value texts)"""
    codes = np.zeros(batch.n, dtype=np.int32)
    vals = np.zeros(batch.n, dtype=np.uint64)
    inst._check(inst.lib.mxp_listentry_check(inst.h, lst.h, int(blacklist), ctypes.byref(batch.c_struct()), value_rule,
                                             codes.ctypes.data, vals.ctypes.data), "mxp_listentry_check")
    texts = [inst.value_text(value_rule, int(v)) if c > 0 else None for c, v in zip(codes, vals)]
    return codes, vals, texts


def model(mxp, units, rule_units, planes, u16, defaults=M.DEFAULTS):
    """The model over a u16 Resolve and the planes' pinned codes -> (status, err_rule, results, rec_off,
    recs, messages {request: text}) as mxp_check_batch lays them out."""
    status, err_rule, off, ids = u16
    n = len(status)
    results = np.zeros(n, mxp.CHECK_RESULT)
    rec_off = np.zeros(n + 1, np.uint64)
    recs, msgs = [], {}
    for q in range(n):
        def unit_result(u):
            d = units[u]
            if d["kind"] == mxp.CHECK_UNIT_CONST:
                return d["const_code"], d["valid_duration_ns"], d["valid_use_count"], 0
            codes, vals, _ = planes[(d["value_rule"], id(d["list"]), d["blacklist"])]
            return int(codes[q]), d["valid_duration_ns"], d["valid_use_count"], int(vals[q])

        def unit_message(u, c, v):
            d = units[u]
            if d["kind"] == mxp.CHECK_UNIT_CONST:
                return d["const_message"]
            return M.list_message(c, planes[(d["value_rule"], id(d["list"]), d["blacklist"])][2][q])

        rules = [int(r) for r in ids[int(off[q]):int(off[q + 1])]]
        res, rr = M.check_request(int(status[q]), rules, rule_units, unit_result, defaults)
        results[q] = res
        rec_off[q + 1] = rec_off[q] + len(rr)
        recs += [(r, u, c, 0, v) for r, u, c, v in rr]
        if res[2] > 0 and rr:
            msgs[q] = M.message(rr, lambda u: units[u]["handler_name"], unit_message)
    return status.copy(), err_rule.copy(), results, rec_off, np.array(recs, dtype=mxp.CHECK_RECORD).reshape(-1), msgs


def same(got, want, what):
    for name, x, y in zip(("status", "err_rule", "results", "rec_off", "recs"), got, want):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, name)


# ------------------------------------------------------------------------------ 1. designed case
# (namespace, rules): no default namespace has rules, so a request's list is its namespace's block
# under the variety's mask -- lengths 1, 3, 4, 5, 63, 64, 65 under variety 0 (ns7: 0), 300 under variety 1
BLOCKS = [("ns0", 1), ("ns1", 3), ("ns2", 4), ("ns3", 5), ("ns4", 63), ("ns5", 64), ("ns6", 65), ("ns7", 300)]
N_RULES = sum(k for _, k in BLOCKS)
INST_RULES = ["true", "request.path", "source.ip"]  # rule 2: IP_ADDRESS, an interface-typed Value
BIG = 300  # units of the one long rule (the 64-bit key's path)


def designed_batch():
    manifest, rules, b = W.c2_workload(n_rules=N_RULES, n_requests=4097, seed=61)
    rng = np.random.default_rng(62)
    n = b.n
    strings = [b.string(i) for i in range(b.n_strings)] + [b"nodots"]
    offs = np.zeros(len(strings) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in strings])
    blob = np.frombuffer(b"".join(strings) + b"\0", dtype=np.uint8).copy()
    kinds = [k.copy() for k in b.kinds]
    values = [v.copy() for v in b.values]
    di, pi, ii = (b.names.index(x) for x in ("destination.service", "request.path", "source.ip"))
    r = rng.random(n)
    kinds[di][r < 0.01] = ABSENT                      # no destination.service
    kinds[di][(r >= 0.01) & (r < 0.02)] = INT64       # ... one that is not a string
    values[di][(r >= 0.02) & (r < 0.03)] = len(strings) - 1  # ... and one without a namespace
    # source.ip (declared IP_ADDRESS): most requests hold bytes -- not a string -- a sixth a string
    s = (rng.random(n) < 0.17) & (kinds[ii] != ABSENT) & (kinds[pi] != ABSENT)
    kinds[ii][s] = STRING
    values[ii][s] = values[pi][s]
    return manifest, rules, BagBatch(n, b.names, kinds, values, blob, offs)


def designed_conf():
    rule_ns, vmask = [], []
    for ns, k in BLOCKS:
        rule_ns += [ns] * k
        vmask += [2 if ns == "ns7" else 1] * k
    return dict(rule_ns=rule_ns, variety_mask=vmask, is_tcp=[0] * N_RULES, empty_match=[1] * N_RULES,
                identity_attr="destination.service", default_ns="istio-system")


def designed_units(mxp, eng, batch):
    """six units; durations 0, 3 s, 4 s, 7 s, 10 s, 2^40 ns and use counts 0 .. 1000, all distinct"""
    pi = batch.names.index("request.path")
    paths = sorted({batch.string(int(v)) for k, v in zip(batch.kinds[pi], batch.values[pi]) if k == STRING})
    wl = eng.list_create(mxp.ListHandle.STRINGS, paths[::2])
    bl = eng.list_create(mxp.ListHandle.STRINGS, paths[::3])
    ipl = eng.list_create(mxp.ListHandle.IP_ADDRESSES, ["10.0.0.0/8"])
    return [mxp.list_unit(1, wl, False, 3 * S, 50, "wl"),                       # 0: string whitelist
            mxp.list_unit(1, bl, True, 10 * S, 7, "bl"),                        # 1: string blacklist
            mxp.list_unit(1, ipl, False, 1 << 40, 1000, "ipwl"),                # 2: IP whitelist: a path is no address
            mxp.const_unit(0, "", 0, 300, "allow"),                             # 3: const OK
            mxp.const_unit(7, "denied by policy", 7 * S, 0, "denier"),          # 4: const PERMISSION_DENIED
            mxp.list_unit(2, wl, False, 4 * S, 20, "ifwl")]                     # 5: interface-typed Value


def designed_rule_units(big):
    """rules with 0, 1 and 3 units; `big`: the second rule of ns7 has BIG units (else 3)"""
    ru = {}
    at = 0
    for ns, k in BLOCKS:
        for p in range(k):
            r = at + p
            if ns == "ns0":
                ru[r] = [5]                                   # the interface unit alone
            elif ns == "ns1":
                ru[r] = [[], [1], [5, 2, 1]][p]               # durations 10 s, 2^40 ns and (a string ip) 4 s
            elif ns == "ns2":
                ru[r] = [[2], [2, 5, 2], [], [2]][p]          # code 3 first; 2^40 ns unless the ip is a string
            elif ns == "ns3":
                ru[r] = [[1], [0], [], [0, 5, 1], [1]][p]     # 10 s against 3 s
            elif ns == "ns7" and p == 1:
                # (a 32-bit key would file index 280 of position 1 as index 24 of position 2, behind
                # position 2's own first unit)
                ru[r] = ([3] * 280 + [4] + [3] * 19) if big else [3, 4, 3]
            elif ns == "ns7" and p == 299:
                ru[r] = [1]
            elif (ns, p) in (("ns5", 40), ("ns6", 64)):
                ru[r] = [4]                                   # (ns6: the 65th id, a round of its own at G = 64)
            else:
                ru[r] = [[], [(p // 3) % 2], [5, 3, 1] if p % 2 else [0, 5, 1]][p % 3]
        at += k
    assert max(len(x) for x in ru.values()) == (BIG if big else 3)
    return [ru[r] for r in range(N_RULES)]


@pytest.fixture(scope="module")
def designed(mxp):
    manifest, rules, batch = designed_batch()
    eng = make_engine(mxp, manifest, rules, designed_conf())
    inst = mxp.Engine(0)
    inst.set_vocabulary(manifest)
    assert (inst.compile(INST_RULES) == 0).all()
    units = designed_units(mxp, eng, batch)
    u16 = {v: [x.copy() for x in eng.resolve_arrays(batch, v, ids16=True)] for v in (0, 1)}
    planes = {}
    for d in units:
        if d["kind"] == mxp.CHECK_UNIT_LIST:
            key = (d["value_rule"], id(d["list"]), d["blacklist"])
            if key not in planes:
                planes[key] = listentry(inst, d["list"], batch, d["value_rule"], d["blacklist"])
    assert len(planes) == 4
    want, plans = {}, {}
    for big in (False, True):
        ru = designed_rule_units(big)
        plans[big] = mxp.CheckPlan(eng, inst, units, ru)
        for v in (0, 1):
            want[big, v] = model(mxp, units, ru, planes, u16[v])
    yield dict(eng=eng, inst=inst, batch=batch, units=units, plans=plans, want=want, u16=u16, planes=planes)
    for p in plans.values():
        p.close()
    inst.close()
    eng.close()


def test_designed_case_holds_every_row(mxp, designed):
    """From the model's output and its inputs alone: every row of the semantics table, every flag, the
    response cases and the long rule occur (the comparison below cannot pass on an input that lost
    what it is for)."""
    u16, planes, want = designed["u16"], designed["planes"], designed["want"]
    lens = set()
    for v in (0, 1):
        lens |= set(np.diff(u16[v][2].astype(np.int64)).tolist())
    assert {0, 1, 3, 4, 5, 63, 64, 65} <= lens and max(lens) > 256
    codes = np.concatenate([p[0] for p in planes.values()])
    assert {-2, -1, 0, 3, 5, 7} <= set(codes.tolist())          # every unit result of the table
    iface = [p[0] for k, p in planes.items() if k[0] == 2][0]
    assert (iface == -2).sum() > 100 and (iface >= 0).sum() > 100 and (iface == -1).sum() > 5
    st = np.concatenate([want[False, v][0] for v in (0, 1)])
    assert {0, 1, 2} <= set(st.tolist())
    res = np.concatenate([want[False, v][2] for v in (0, 1)])
    fl, code = res["flags"], res["code"]
    for f in (M.F_RESOLVE_ERROR, M.F_NO_CHECKS, M.F_EVAL_ERROR, M.F_UNIT_PANIC):
        assert (fl & f).any(), f
    assert ((fl == M.F_NO_CHECKS) & (code == 0)).any()                               # nothing selected
    assert ((fl == (M.F_NO_CHECKS | M.F_UNIT_PANIC)) & (code == 13)).any()           # a panic alone
    assert (((fl & M.F_UNIT_PANIC) != 0) & ((fl & M.F_NO_CHECKS) == 0) & (code == 0)).any()  # ... beside a result
    ev = (fl & M.F_EVAL_ERROR) != 0
    assert (ev & (code == 0) & (res["valid_duration_ns"] == 0) & (res["valid_use_count"] == 0)).any()
    assert (ev & (code > 0)).any()                               # an Eval error beside a failure: the code stays
    assert {0, 3, 5, 7, 13} <= set(code.tolist())
    durs = set(res["valid_duration_ns"].tolist())
    assert {0, 3 * S, 4 * S, 10 * S, 1 << 40} <= durs and (res["n_records"] > 3).any()
    # the long rule: selected under variety 1; its const PERMISSION_DENIED at unit index 280 decides
    # requests whose next rule (position 2) fails first with NOT_FOUND
    big = want[True, 1]
    base = sum(k for _, k in BLOCKS[:7])
    assert len(designed_rule_units(True)[base + 1]) == BIG
    off, recs = big[3].astype(np.int64), big[4]
    decided = 0
    for q in np.nonzero(big[2]["code"] == 7)[0]:
        rr = recs[off[q]:off[q + 1]]
        decided += len(rr) >= 2 and tuple(rr[0])[:3] == (base + 1, 4, 7) and tuple(rr[1])[:3] == (base + 2, 0, 5)
    assert decided > 10
    assert len(want[False, 0][5]) > 100 and len(want[True, 1][5]) > 10


@pytest.mark.parametrize("ids32", [False, True], ids=["u16", "u32"])
@pytest.mark.parametrize("group", ["", "1", "4", "16", "64"])
def test_designed_case(mxp, designed, monkeypatch, group, ids32):
    """results, rec_off, recs, status and err_rule byte for byte, both varieties, with and without the
    long rule, every group width, u16 and (forced) u32 ids on the device."""
    if group:
        monkeypatch.setenv("MXP_CHECK_GROUP", group)
    if ids32:
        monkeypatch.setenv("MXP_CHECK_IDS32", "1")
    batch = designed["batch"]
    for big in (False, True):
        for v in (0, 1):
            got = designed["plans"][big].check(batch, v)
            same(got, designed["want"][big, v][:5], (big, v, group, ids32))


def test_designed_messages(mxp, designed):
    """message() for every failing request (the batch still the instance engine's last)."""
    batch = designed["batch"]
    for big, v in ((False, 0), (True, 1)):
        plan, want = designed["plans"][big], designed["want"][big, v]
        status, err_rule, results, off, recs = plan.check(batch, v)
        failing = np.nonzero(results["code"] > 0)[0]
        msgs = want[5]
        assert set(q for q in failing.tolist() if results["n_records"][q]) == set(msgs) and len(msgs) > 10
        for q in msgs:
            assert plan.message(recs[int(off[q]):int(off[q + 1])]) == msgs[q], q
    assert plan.message(recs[:0]) == ""


# ------------------------------------------------------------------------------- 2. small C2 case
def test_c2_case(mxp):
    """Real predicates (errors, TCP rules, two namespaces' blocks per request), a whitelist or a
    blacklist unit on a quarter of the rules."""
    manifest, rules, conf, batch = c2_resolve_case(65, 2, 4097)
    eng = make_engine(mxp, manifest, rules, conf)
    inst = mxp.Engine(0)
    inst.set_vocabulary(manifest)
    assert (inst.compile(["true", "request.path"]) == 0).all()
    pi = batch.names.index("request.path")
    paths = sorted({batch.string(int(v)) for k, v in zip(batch.kinds[pi], batch.values[pi]) if k == STRING})
    wl = eng.list_create(mxp.ListHandle.STRINGS, paths[::2])
    bl = eng.list_create(mxp.ListHandle.STRINGS, paths[::5])
    units = [mxp.list_unit(1, wl, False, 5 * S, 100, "staticversion"), mxp.list_unit(1, bl, True, 1 * S, 10, "denylist")]
    ru = [([0] if r % 8 == 0 else [1]) if r % 4 == 0 else [] for r in range(len(rules))]
    u16 = [x.copy() for x in eng.resolve_arrays(batch, 1, ids16=True)]
    planes = {(1, id(u["list"]), u["blacklist"]): listentry(inst, u["list"], batch, 1, u["blacklist"]) for u in units}
    want = model(mxp, units, ru, planes, u16)
    st, res = want[0], want[2]
    assert (st == 3).sum() > 2 and (st == 1).sum() > 2 and (res["code"] == 5).sum() > 10 and (res["code"] == 7).sum() > 10
    # (a request without request.path fails its predicates and does not resolve: no Eval error here)
    assert (res["flags"] == M.F_NO_CHECKS).sum() > 100 and (res["n_records"] > 1).any()
    plan = mxp.CheckPlan(eng, inst, units, ru)
    same(plan.check(batch, 1), want[:5], "c2")
    sub = batch.subset(np.arange(5, 5 + 1025))
    u16s = [x.copy() for x in eng.resolve_arrays(sub, 1, ids16=True)]
    # (Value registers are ids of the batch they came from: the subset's are taken from its own run)
    planes_s = {(1, id(u["list"]), u["blacklist"]): listentry(inst, u["list"], sub, 1, u["blacklist"]) for u in units}
    same(plan.check(sub, 1), model(mxp, units, ru, planes_s, u16s)[:5], "c2 subset")
    plan.close()
    inst.close()
    eng.close()


# ----------------------------------------------------------------------------------- 3. API edges
def test_record_capacity(mxp, designed):
    plan, batch, want = designed["plans"][False], designed["batch"], designed["want"][False, 0]
    total = len(want[4])
    assert total > 100
    for cap in (0, total - 1):
        rc, st, er, res, off, recs = plan.check_raw(batch, 0, cap)
        assert rc == ERR_NOMEM, cap
        same((st, er, res, off), want[:4], ("short", cap))   # complete without the records
        rc, st, er, res, off2, recs = plan.check_raw(batch, 0, int(off[-1]))
        assert rc == 0
        same((st, er, res, off2, recs[:total]), want[:5], ("retry", cap))
    rc, st, er, res, off, recs = plan.check_raw(batch, 0, total + 100)
    assert rc == 0
    same((st, er, res, off, recs[:total]), want[:5], "room to spare")


def test_empty_batch(mxp, designed):
    plan, batch = designed["plans"][False], designed["batch"]
    st, er, res, off, recs = plan.check(batch.subset(np.arange(0)), 0)
    assert len(st) == 0 and len(res) == 0 and off.tolist() == [0] and len(recs) == 0


def test_second_batch_is_independent(mxp, designed):
    """Another batch (other size, other requests) through the same plan, then the first again."""
    plan, batch, eng, inst = designed["plans"][False], designed["batch"], designed["eng"], designed["inst"]
    rows = np.arange(batch.n - 1, 1000, -3)
    sub = batch.subset(rows)
    u16 = [x.copy() for x in eng.resolve_arrays(sub, 0, ids16=True)]
    planes = {}
    for d in designed["units"]:
        if d["kind"] == mxp.CHECK_UNIT_LIST:
            planes.setdefault((d["value_rule"], id(d["list"]), d["blacklist"]),
                              listentry(inst, d["list"], sub, d["value_rule"], d["blacklist"]))
    want = model(mxp, designed["units"], designed_rule_units(False), planes, u16)
    same(plan.check(batch, 0), designed["want"][False, 0][:5], "first")
    same(plan.check(sub, 0), want[:5], "second")
    same(plan.check(batch, 0), designed["want"][False, 0][:5], "first again")


def test_plan_validation(mxp, designed):
    eng, inst, units = designed["eng"], designed["inst"], designed["units"]
    ru = designed_rule_units(False)

    def refused(match, inst=inst, units=units, ru=ru, **kw):
        with pytest.raises(mxp.MxpError, match=r"failed \(1\): .*" + match):
            mxp.CheckPlan(eng, inst, units, ru, **kw)

    wl = units[0]["list"]
    refused("no such value rule", units=units[:5] + [mxp.list_unit(len(INST_RULES), wl, False, 0, 0)])
    refused("not of type STRING", units=units[:5] + [mxp.list_unit(0, wl, False, 0, 0)])   # rule 0: `true`
    refused("is not a unit", ru=ru[:-1] + [[len(units)]])
    off = np.zeros(N_RULES + 1, dtype=np.uint32)
    off[1:] = 2
    off[7] = 1
    refused("rule_unit_off", ru=[0, 1], rule_unit_off=off)
    host = mxp.Engine(-1)  # (an engine without a device stands in for one on another device)
    host.set_vocabulary(W.TESTDATA_MANIFEST)
    host.compile(INST_RULES)
    refused("different devices", inst=host)
    refused("without an instance engine", inst=None)
    const_only = [u for u in units if u["kind"] == mxp.CHECK_UNIT_CONST]
    mxp.CheckPlan(eng, None, const_only, [[0, 1]] + [[]] * (N_RULES - 1)).close()  # (no instance engine needed)
    # a rule set compiled after the plan was created
    inst2 = mxp.Engine(0)
    inst2.set_vocabulary(W.TESTDATA_MANIFEST)
    inst2.compile(INST_RULES)
    plan = mxp.CheckPlan(eng, inst2, units, ru)
    batch = designed["batch"].subset(np.arange(300))
    assert plan.check_raw(batch, 0, 4096)[0] == 0
    inst2.compile(INST_RULES)
    assert plan.check_raw(batch, 0, 4096)[0] == ERR_ARG
    assert b"after the plan was created" in eng.lib.mxp_last_error(eng.h)
    plan.close()
    inst2.close()
    host.close()
