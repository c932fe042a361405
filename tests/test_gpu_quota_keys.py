"""mxp_quota_batch / mxp_quota_keys_device (include/mxp.h; quota_keys.cpp, quota_keys.hip): the
batched Quota path bit for bit against tests/quota_keys_model.py (a transcription of the Go, pinned
by test_quota_keys_model.py), fed with the same engine's u16 Resolve (pinned by test_gpu_resolver.py /
test_gpu_delta8.py) and with dimension values read from the batch's own columns in Python.  Nothing
expected here comes from the code under test.

The dimension expressions are bare attributes, so a dimension's value is the attribute's value when
its kind fits the declared type, and an Eval error when it is absent or of another kind; `q.ip`
(IP_ADDRESS) is interface-typed: whatever kind the batch holds arrives at run time."""
import numpy as np
import pytest

import quota_keys_model as QM
from istio_amd.bags import BagBatch, GoFloat64, GoInt64

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_NOMEM = 1, 4
S = 10 ** 9
BASE_NS = 1_500_000_000 * S

MANIFEST = {"destination.service": "STRING", "context.protocol": "STRING", "q.a": "STRING", "q.b": "STRING",
            "q.i": "INT64", "q.f": "DOUBLE", "q.t": "BOOL", "q.ip": "IP_ADDRESS", "q.d": "DURATION"}
INST_RULES = ["q.a", "q.b", "q.i", "q.f", "q.t", "q.ip", "q.d"]
KIND_OF_RULE = ["S", "S", "I", "F", "B", None, "D"]  # None: interface-typed

# namespace -> the units of its rules, in resolution order (every rule selected: empty matches)
NO, OTHER = QM.NO_UNIT, QM.OTHER_UNIT
BLOCKS = [("nsa", [NO, 0]), ("nsb", [OTHER, 0]), ("nsc", [NO, NO]), ("nsd", [1]), ("nse", [NO, NO, 2]), ("nsf", [3, 0])]
RULE_UNIT = [u for _, us in BLOCKS for u in us]
# (label, instance rule) in configuration order: unit 0's labels are given unsorted
UNITS = [("rq", [("b", 1), ("a", 0)]),
         ("rq2", [("s", 0), ("i", 2), ("f", 3), ("t", 4), ("x", 5)]),
         ("rq", []),
         ("rq2", [("x", 5)])]
LIMITS = [{"name": "rq", "max_amount": 40, "valid_duration_ns": 0, "key_cap": 4096,
           "overrides": [{"dimensions": {"a": "va1"}, "max_amount": 9, "valid_duration_ns": 1 * S, "key_cap": 256},
                         {"dimensions": {}, "max_amount": 25, "valid_duration_ns": 2 * S + 1, "key_cap": 4096}]},
          {"name": "rq2", "max_amount": 30, "valid_duration_ns": 1 * S, "key_cap": 8192}]


@pytest.fixture(scope="module")
def mxp(libmxp):
    import istio_amd.engine as mxp
    return mxp


def conf():
    rule_ns = [ns for ns, us in BLOCKS for _ in us]
    k = len(rule_ns)
    return dict(rule_ns=rule_ns, variety_mask=[1] * k, is_tcp=[0] * k, empty_match=[1] * k,
                identity_attr="destination.service", default_ns="istio-system")


def engines(mxp, inst_rules=INST_RULES):
    c = conf()
    eng = mxp.Engine(0)
    eng.set_vocabulary(MANIFEST)
    eng.compile(["true"] * len(RULE_UNIT))
    eng.set_resolver(c["identity_attr"], c["default_ns"], c["rule_ns"], c["variety_mask"], c["is_tcp"], c["empty_match"])
    inst = mxp.Engine(0)
    inst.set_vocabulary(MANIFEST)
    assert (inst.compile(inst_rules) == 0).all()
    return eng, inst


def unit_dicts(units=UNITS):
    return [dict(instance_name=name, labels=[lab for lab, _ in dims], value_rules=[r for _, r in dims]) for name, dims in units]


def make_plan(mxp, eng, inst, limits=LIMITS, units=UNITS, rule_unit=RULE_UNIT):
    return mxp.QuotaPlan(eng, inst, limits, unit_dicts(units), rule_unit)


def make_model(limits=LIMITS, units=UNITS, rule_unit=RULE_UNIT):
    return QM.QuotaPlanModel(limits, unit_dicts(units), rule_unit)


def dimension(batch, q, rule):
    """What the instance expression `rule` evaluates to for request q, in the model's terms."""
    v, found = batch.get(q, INST_RULES[rule])
    kind = KIND_OF_RULE[rule]
    if not found:
        return QM.EvalError
    if kind is None:
        if isinstance(v, (str, bool, bytes)):  # ([]byte: makeKey writes the bytes)
            return v
        return QM.Unsupported  # (an interface register keeps 56 bits of a number)
    if kind == "S":
        return v if isinstance(v, str) else QM.EvalError
    if kind == "B":
        return v if isinstance(v, bool) else QM.EvalError
    if kind == "I":
        return int(v) if isinstance(v, GoInt64) else QM.EvalError
    if kind == "F":
        return float(v) if isinstance(v, GoFloat64) else QM.EvalError
    raise AssertionError(kind)


def dims_of(batch, units=UNITS):
    return lambda q, u: {lab: dimension(batch, q, r) for lab, r in units[u][1]}


def model_batch(model, eng, batch, amounts, be, ids, skip, now):
    """-> (QUOTA_ANSWER array as mxp_quota_batch lays it out, status, err_rule)"""
    import istio_amd.engine as mxp
    status, err_rule, off, rid = [x.copy() for x in eng.resolve_arrays(batch, 0, ids16=True)]
    rows = model.batch(status, lambda q: [int(r) for r in rid[int(off[q]):int(off[q + 1])]], dims_of(batch),
                       [int(a) for a in amounts], [int(b) for b in be], ids, skip, now)
    return np.array(rows, dtype=mxp.QUOTA_ANSWER).reshape(-1), status, err_rule


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = [i for i in range(len(got)) if got[i] != want[i]]
        raise AssertionError((what, len(bad), [(i, got[i], want[i]) for i in bad[:6]]))


# ------------------------------------------------------------------------------ 1. designed case
A_VALS = ["va1", "", "x"] + ["a%d" % i for i in range(37)]
B_VALS = ["", "b"] + ["bee%d" % i for i in range(28)]
I_VALS = [0, 1, -1, 255, -4096, 2 ** 63 - 1, -2 ** 63, 10 ** 12]
F_VALS = [0.0, -0.0, 1.0, 3.0, -1.5, 5e-324, float("inf"), float("-inf"), float("nan"), 1e300, 2.5e-310]
SEED = 7


def designed_call(call, n=4097):
    rng = np.random.default_rng(SEED + call)
    ns_names = [ns for ns, _ in BLOCKS]
    ns_p = [0.40, 0.03, 0.03, 0.27, 0.05, 0.22]
    bags = []
    for q in range(n):
        b = {"context.protocol": "http"}
        r = rng.random()
        if r >= 0.02:  # (else no identity: the Resolve errs)
            b["destination.service"] = "svc%d.%s.svc.cluster.local" % (rng.integers(0, 9), ns_names[rng.choice(6, p=ns_p)])
        r = rng.random()
        if r < 0.005:
            pass  # both labels of unit 0 absent
        else:
            if r >= 0.03:
                b["q.a"] = A_VALS[int(rng.integers(len(A_VALS)))] if rng.random() < 0.85 else "va1"
            if not 0.03 <= r < 0.05:
                b["q.b"] = B_VALS[int(rng.integers(len(B_VALS)))]
        if rng.random() < 0.01:
            b["q.b"] = GoInt64(3)  # not a string: a conversion error
        if rng.random() >= 0.01:
            b["q.i"] = GoInt64(I_VALS[int(rng.integers(len(I_VALS)))])
        if rng.random() >= 0.01:
            b["q.f"] = GoFloat64(F_VALS[int(rng.integers(len(F_VALS)))])
        if rng.random() >= 0.01:
            b["q.t"] = bool(rng.random() < 0.5)
        r = rng.random()
        if r < 0.84:
            b["q.ip"] = "10.0.0.%d" % rng.integers(0, 40)   # a string where an address is declared
        elif r < 0.88:
            b["q.ip"] = bool(r < 0.86)
        elif r < 0.93:
            b["q.ip"] = bytes([10, 0, 0, int(rng.integers(0, 9))])  # []byte, as the attribute is declared
        elif r < 0.96:
            b["q.ip"] = GoInt64(7)
        bags.append(b)
    batch = BagBatch.from_bags(bags, names=list(MANIFEST))
    r = rng.random(n)
    amounts = np.where(r < 0.05, 0, np.where(r < 0.17, -rng.integers(1, 6, n), rng.integers(1, 8, n))).astype(np.int64)
    be = (rng.random(n) < 0.5).astype(np.uint8)
    skip = (rng.random(n) < 0.03).astype(np.uint8)
    ids = [b"c%d-%d" % (call, q) for q in range(n)]
    for q in np.nonzero(rng.random(n) < 0.15)[0]:       # repeats within the call
        if q:
            ids[q] = ids[int(rng.integers(0, q))]
    if call:
        for q in np.nonzero(rng.random(n) < 0.10)[0]:   # ... and of earlier calls
            ids[q] = b"c%d-%d" % (int(rng.integers(0, call)), int(rng.integers(0, n)))
    now = BASE_NS + (0, 400_000_000, 1_500_000_000)[call]  # (the last past a 1 s window's boundary)
    return batch, amounts, be, ids, skip, now


@pytest.fixture(scope="module")
def designed(mxp):
    eng, inst = engines(mxp)
    calls = [designed_call(c) for c in range(3)]
    model = make_model()
    want = [model_batch(model, eng, *c) for c in calls]
    yield dict(eng=eng, inst=inst, calls=calls, want=want, model=model)
    inst.close()
    eng.close()


def run_calls(mxp, d, upto=3, with_ids=True):
    plan = make_plan(mxp, d["eng"], d["inst"])
    got = []
    for batch, amounts, be, ids, skip, now in d["calls"][:upto]:
        got.append(plan.batch(batch, 0, amounts, be, now, ids if with_ids else None, skip))
    return plan, got


def test_designed_case_holds_every_row(designed):
    """On the model's output alone: what the comparison below is for occurs in it."""
    codes = np.concatenate([w[0]["code"] for w in designed["want"]])
    assert (codes == QM.OK).sum() * 2 >= len(codes)
    for c in (QM.NOT_APPLIED, QM.OTHER, QM.SKIPPED, QM.RESOLVE_ERROR, QM.EVAL_ERROR, QM.KEY_UNSUPPORTED):
        assert (codes == c).sum() >= 20, c
    assert not (codes == QM.KEYS_FULL).any() and not (codes == QM.KEY_CONFLICT).any()
    failed = np.concatenate([w[0]["failed"] for w in designed["want"]])
    assert {1, 2, 3} <= set(failed.tolist())          # one label, the other, two
    repeated_first = 0
    seen = set()
    for w in designed["want"]:
        keys = w[0]["key"][w[0]["key"] != QM.NO_KEY]
        ks, cnt = np.unique(keys, return_counts=True)
        repeated_first += sum(1 for k, c in zip(ks.tolist(), cnt.tolist()) if c > 1 and k not in seen)
        seen |= set(ks.tolist())
    assert repeated_first >= 100
    m = designed["model"]
    assert all(m.next_free[c] > 0 for c in m.next_free if c != (0, -1))  # every class but rq's shadowed default
    texts = b"".join(m.text.values())
    for piece in (b"\0" * 32 + b"true", b"\0" * 32 + b"-8000000000000000", b"p-1074", b"NaN", b"+Inf", b"rq;a=va1;b="):
        assert piece in texts, piece
    assert b"rq" in m.text.values()                    # the unit without dimensions
    ans = np.concatenate([w[0] for w in designed["want"]])
    ok = (ans["code"] == QM.OK) & (ans["key"] != QM.NO_KEY)
    assert (ans["dup"][ok] == 1).sum() > 100 and (ans["granted"][ok] == 0).sum() > 50 and (ans["granted"][ok] > 0).sum() > 2000
    na = ans["code"] == QM.NOT_APPLIED  # the amount asked, negative ones included, and the default duration
    assert (ans["granted"][na] < 0).any() and (ans["valid_ns"][na] == 10 * S).all()
    assert len(set(ans["valid_ns"][ok].tolist())) > 4  # durations of hits partly run down
    assert ((ans["code"] == QM.OK) & (ans["key"] == QM.NO_KEY)).sum() > 20  # amount 0


def test_designed_case(mxp, designed):
    plan, got = run_calls(mxp, designed)
    for c, ((st, er, ans), (want, wst, wer)) in enumerate(zip(got, designed["want"])):
        assert st.tobytes() == wst.tobytes() and er.tobytes() == wer.tobytes(), c
        same(ans, want, ("call", c))
    m = designed["model"]
    stats = plan.stats()
    assert stats["keys"] == len(m.text) and stats["classes"] == 4
    assert stats["class_keys"] == [m.next_free[c] for c in ((0, -1), (0, 0), (0, 1), (1, -1))]
    for kid in list(m.text)[::37]:
        assert plan.key_text(kid) == m.text[kid], kid
    plan.close()


def test_designed_case_u32_ids(mxp, designed, monkeypatch):
    monkeypatch.setenv("MXP_CHECK_IDS32", "1")
    plan, got = run_calls(mxp, designed, upto=1)
    same(got[0][2], designed["want"][0][0], "u32 ids")
    plan.close()


# --------------------------------------------------------------------------------- 3. probe chains
def test_probe_chains(mxp, designed, monkeypatch):
    """16 hash values for ~1,500 keys: every probe walks a chain, every tag collides"""
    monkeypatch.setenv("MXP_QKEY_HASH_BITS", "4")
    plan, got = run_calls(mxp, designed, upto=2)
    same(got[0][2], designed["want"][0][0], "call 0")
    same(got[1][2], designed["want"][1][0], "call 1")
    plan.close()


# ------------------------------------------------------------------------------ 6. independent path
def test_replay_through_the_plain_quota(mxp, designed):
    """The model's key ids through mxp_quota_alloc_dedup on a fresh mxp_quota with the expanded limits
    (test_gpu_quota_dedup.py's subject) give mxp_quota_batch's granted, valid_ns and dup."""
    plan, got = run_calls(mxp, designed)
    m = designed["model"]
    mx = np.array([m.expanded[k][0] for k in range(m.n_keys)], dtype=np.int64)
    vd = np.array([m.expanded[k][1] for k in range(m.n_keys)], dtype=np.int64)
    q = designed["eng"].quota_create(mx, vd)
    for (batch, amounts, be, ids, skip, now), (want, _, _), (_, _, ans) in zip(designed["calls"], designed["want"], got):
        ok = (want["code"] == QM.OK) & (want["key"] != QM.NO_KEY)
        keys = np.where(ok, want["key"], 0).astype(np.uint32)
        g, v, d = q.alloc_dedup(keys, np.where(ok, amounts, 0), be, ids, now)
        assert ok.sum() > 2000
        assert (ans["granted"][ok] == g[ok]).all() and (ans["valid_ns"][ok] == v[ok]).all() and (ans["dup"][ok] == d[ok]).all()
    plan.close()


def test_without_dedup_ids(mxp, designed):
    model = make_model()
    plan = make_plan(mxp, designed["eng"], designed["inst"])
    for c, (batch, amounts, be, ids, skip, now) in enumerate(designed["calls"][:2]):
        want, _, _ = model_batch(model, designed["eng"], batch, amounts, be, None, skip, now)
        _, _, ans = plan.batch(batch, 0, amounts, be, now, None, skip)
        same(ans, want, ("no ids", c))
        assert (want["dup"] == 0).all() and (want["valid_ns"] > 0).sum() > 500
    plan.close()


# --------------------------------------------------------------------------------- 7. the stage alone
def test_stage_alone(mxp, designed):
    import torch
    batch, amounts, be, ids, skip, now = designed["calls"][0]
    n = batch.n
    eng = designed["eng"]
    status, _, off, rid = eng.resolve_arrays(batch, 0, ids16=True)
    unit_of = []
    for q in range(n):
        code, u = QM.dispatch(int(status[q]), [int(r) for r in rid[int(off[q]):int(off[q + 1])]], RULE_UNIT)
        unit_of.append(u if code == QM.OK else None)
    model = make_model()
    want = model.stage(unit_of, dims_of(batch), [int(a) for a in amounts])
    plan = make_plan(mxp, eng, designed["inst"])
    plan.eval(batch)
    du = torch.from_numpy(np.array([QM.NO_UNIT if u is None else u for u in unit_of], dtype=np.uint32).view(np.int32)).cuda()
    da = torch.from_numpy(amounts.copy()).cuda()
    dk = torch.full((n,), 99, dtype=torch.int32, device="cuda")
    dc = torch.full((n,), 99, dtype=torch.int32, device="cuda")
    df = torch.full((n,), 99, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    plan.keys_device(n, du.data_ptr(), da.data_ptr(), 0, dk.data_ptr(), dc.data_ptr(), df.data_ptr())
    torch.cuda.synchronize()
    key, code, failed = dk.cpu().numpy().view(np.uint32), dc.cpu().numpy(), df.cpu().numpy().view(np.uint32)
    wk = np.array([QM.NO_KEY if w is None else w[1] for w in want], dtype=np.uint32)
    wc = np.array([QM.NOT_APPLIED if w is None else w[0] for w in want], dtype=np.int32)
    wf = np.array([0 if w is None else w[2] for w in want], dtype=np.uint32)
    assert (code == wc).all() and (key == wk).all() and (failed == wf).all()
    assert len(model.text) > 500
    for kid, text in model.text.items():  # every interned id's bytes, 32 NULs included
        assert plan.key_text(kid) == text, kid
    assert sum(b"\0" * 32 in t for t in model.text.values()) > 200
    plan.close()


# ----------------------------------------------------------------------------- 2. strings at the edges
def simple_case(mxp, bags, limits, units, amounts=None, ids=None, now=BASE_NS, plan=None, model=None, eng_inst=None,
                dims_fn=None):
    """Every request of namespace nsd (one rule, unit 0 of `units`) -> (rc, answers, want, plan, model)"""
    n = len(bags)
    for b in bags:
        b.setdefault("destination.service", "svc.nsd.svc.cluster.local")
    batch = BagBatch.from_bags(bags, names=list(MANIFEST))
    eng, inst = eng_inst
    nsd = sum(len(us) for ns, us in BLOCKS[:3])  # nsd's one rule
    assert BLOCKS[3][0] == "nsd" and RULE_UNIT[nsd] == 1
    rule_unit = [0 if r == nsd else NO for r in range(len(RULE_UNIT))]
    plan = plan or mxp.QuotaPlan(eng, inst, limits, unit_dicts(units), rule_unit)
    model = model or QM.QuotaPlanModel(limits, unit_dicts(units), rule_unit)
    amounts = np.ones(n, dtype=np.int64) if amounts is None else np.asarray(amounts, dtype=np.int64)
    be = np.zeros(n, dtype=np.uint8)
    status, _, off, rid = eng.resolve_arrays(batch, 0, ids16=True)
    rows = model.batch(status, lambda q: [int(r) for r in rid[int(off[q]):int(off[q + 1])]],
                       dims_fn(batch) if dims_fn else dims_of(batch, units), [int(a) for a in amounts], [0] * n, ids, None, now)
    want = np.array(rows, dtype=mxp.QUOTA_ANSWER).reshape(-1)
    rc, _, _, ans = plan.batch_raw(batch, 0, amounts, be, now, ids, None)
    return rc, ans, want, plan, model


@pytest.fixture(scope="module")
def eng_inst(mxp):
    eng, inst = engines(mxp)
    yield eng, inst
    inst.close()
    eng.close()


def test_strings_at_the_edges(mxp, eng_inst):
    ov = "override-value-of-21b"
    limits = [{"name": "e", "max_amount": 100, "valid_duration_ns": 0, "key_cap": 600,
               "overrides": [{"dimensions": {"a": ov}, "max_amount": 5, "valid_duration_ns": 0, "key_cap": 40}]}]
    units = [("e", [("a", 0), ("b", 1)])]
    bags = []
    for i in range(512):
        # a: every length 0 .. 40; b: every length 0 .. 40 behind it, so b starts at every alignment
        bags.append({"q.a": "".join(chr(97 + (i + k) % 26) for k in range(i % 41)),
                     "q.b": "".join(chr(65 + (i + k) % 26) for k in range((i // 41 + i * 7) % 41))})
    bags[500]["q.a"] = "L" * 5000
    bags[501]["q.a"] = ov
    bags[502]["q.a"] = ov + "!"          # the override's value and a trailing byte
    bags[503]["q.a"] = ov[:-1]           # a strict prefix of it
    bags[504]["q.a"], bags[504]["q.b"] = ov, ""
    bags[505]["q.b"] = "M" * 5000
    rc, ans, want, plan, model = simple_case(mxp, bags, limits, units, eng_inst=eng_inst)
    assert rc == 0
    same(ans, want, "edges")
    assert model.next_free[0, 0] == 2 and model.next_free[0, -1] > 400
    lens = {len(t) for t in model.text.values()}
    assert len({x % 8 for x in lens}) == 8 and max(lens) > 5000
    for kid, text in model.text.items():
        assert plan.key_text(kid) == text, kid
    plan.close()


# ------------------------------------------------------------------------------------- []byte values
BYTES_RULES = ['q.ip | ip("10.1.2.3")', "ip(q.a)", "q.ip"]


def ip16(text):
    """net.ParseIP's 16-byte form, from `ipaddress`"""
    import ipaddress
    a = ipaddress.ip_address(text)
    return a.packed if a.version == 6 else b"\0" * 10 + b"\xff\xff" + a.packed


@pytest.mark.parametrize("host_pack", [False, True], ids=["device-packer", "host-packer"])
def test_bytes_dimensions(mxp, monkeypatch, host_pack):
    """[]byte dimension values from every pool they can live in: a constant of the rule set (the
    ip() literal), the batch's own byte strings of 4 and 16 bytes, parsed ip() results; written into
    the key as they are (keys.go:64-65), read back through mxp_quota_key_text.  []byte "1234" does not
    match the override's string "1234" (memquota.go:69-80)."""
    if host_pack:
        monkeypatch.setenv("MXP_HOST_PACK", "1")
    eng, inst = engines(mxp, BYTES_RULES)
    limits = [{"name": "ipq", "max_amount": 100, "valid_duration_ns": 0, "key_cap": 700,
               "overrides": [{"dimensions": {"u": "1234"}, "max_amount": 5, "valid_duration_ns": 0, "key_cap": 8}]}]
    units = [("ipq", [("src", 0), ("peer", 1), ("u", 2)])]
    rng = np.random.default_rng(91)
    texts = ["10.0.0.%d" % i for i in range(20)] + ["::1", "2001:db8::7", "::ffff:10.1.2.3", "junk", "10.0.0"]
    bags, want_dims = [], []
    for i in range(600):
        b, r = {}, rng.random()
        if r < 0.45:
            b["q.ip"] = bytes([10, 0, int(rng.integers(0, 3)), int(rng.integers(0, 9))])
        elif r < 0.6:
            b["q.ip"] = ip16("2001:db8::%x" % rng.integers(0, 9))
        elif r < 0.7:
            b["q.ip"] = b"1234"
        elif r < 0.8:
            b["q.ip"] = ip16("10.1.2.3")    # the literal's own bytes: the rule set's pool holds them
        elif r < 0.85:
            b["q.ip"] = b""
        if rng.random() < 0.95:
            b["q.a"] = texts[int(rng.integers(len(texts)))]
        d = {"src": b.get("q.ip", ip16("10.1.2.3")), "u": b.get("q.ip", QM.EvalError), "peer": QM.EvalError}
        try:
            d["peer"] = ip16(b["q.a"])
        except (KeyError, ValueError):
            pass
        bags.append(b)
        want_dims.append(d)
    rc, ans, want, plan, model = simple_case(mxp, bags, limits, units, eng_inst=(eng, inst),
                                            dims_fn=lambda batch: (lambda q, u: want_dims[q]))
    assert rc == 0
    same(ans, want, "bytes")
    assert (want["code"] == QM.OK).sum() > 350 and (want["code"] == QM.EVAL_ERROR).sum() > 50
    assert {2, 4, 6} <= set(want["failed"].tolist())  # (bits 1 and 2: peer, u; src never fails)
    assert model.next_free[0, 0] == 0 and len(model.text) > 150
    joined = b"".join(model.text.values())
    for piece in (b";src=" + ip16("10.1.2.3") + b";", b";u=1234", b";u=\n\0", b";peer=" + ip16("::1") + b";",
                  b";u=" + ip16("2001:db8::3")):
        assert piece in joined, piece
    assert any(t.endswith(b";u=") for t in model.text.values())  # the empty []byte
    for kid, text in model.text.items():
        assert plan.key_text(kid) == text, kid
    plan.close()
    inst.close()
    eng.close()


# ------------------------------------------------------------------------------------- 4. capacity
def test_capacity(mxp, eng_inst):
    limits = [{"name": "c", "max_amount": 100, "valid_duration_ns": 0, "key_cap": 3, "overrides": []}]
    units = [("c", [("a", 0)])]
    vals = ["k0", "k1", "k0", "k2", "k3", "k1", "k4", "k3", "k2", "k0"]
    bags = [{"q.a": v} for v in vals]
    rc, ans, want, plan, model = simple_case(mxp, bags, limits, units, eng_inst=eng_inst)
    assert rc == ERR_NOMEM
    same(ans, want, "first call")
    assert want["key"].tolist() == [0, 1, 0, 2, QM.NO_KEY, 1, QM.NO_KEY, QM.NO_KEY, 2, 0]
    assert want["code"].tolist() == [0, 0, 0, 0, -3, 0, -3, -3, 0, 0]
    rc, ans2, want2, _, _ = simple_case(mxp, [{"q.a": v} for v in vals], limits, units, plan=plan, model=model,
                                        eng_inst=eng_inst)
    assert rc == ERR_NOMEM
    same(ans2, want2, "second call")
    assert (ans2["key"] == ans["key"]).all() and (ans2["code"] == ans["code"]).all()
    assert plan.stats()["class_keys"] == [3]
    assert b"ran out of key ids" in eng_inst[0].lib.mxp_last_error(eng_inst[0].h)
    # QuotaPlan.batch hands the complete answers over instead of raising
    b0 = BagBatch.from_bags([{"q.a": "k9", "destination.service": "svc.nsd.svc.cluster.local"}], names=list(MANIFEST))
    _, _, one = plan.batch(b0, 0, [1], [0], BASE_NS)
    assert plan.keys_full and one["code"].tolist() == [QM.KEYS_FULL] and one["key"].tolist() == [QM.NO_KEY]
    plan.close()


# ------------------------------------------------------------------------------------- 5. conflict
def test_conflict(mxp, eng_inst):
    limits = [{"name": "k", "max_amount": 10, "valid_duration_ns": 0, "key_cap": 8,
               "overrides": [{"dimensions": {"a": "x"}, "max_amount": 3, "valid_duration_ns": 0, "key_cap": 8}]}]
    units = [("k", [("a", 0), ("b", 1)])]
    pair = [{"q.a": "x;b=y", "q.b": "z"}, {"q.a": "x", "q.b": "y;b=z"}]
    rc, ans, want, plan, model = simple_case(mxp, [dict(b) for b in pair], limits, units, amounts=[2, 2], eng_inst=eng_inst)
    assert rc == 0
    same(ans, want, "within a call")
    assert want["code"].tolist() == [0, QM.KEY_CONFLICT] and want["granted"].tolist() == [2, 0]
    # across calls: the held text under the other class, then the holder again (no state moved meanwhile)
    rc, ans, want, _, _ = simple_case(mxp, [dict(pair[1]), dict(pair[0])], limits, units, amounts=[2, 9], plan=plan,
                                      model=model, eng_inst=eng_inst)
    same(ans, want, "across calls")
    assert want["code"].tolist() == [QM.KEY_CONFLICT, 0] and want["granted"].tolist() == [0, 0]  # 2 + 9 > 10
    assert plan.stats()["class_keys"] == [1, 0]
    plan.close()


# ------------------------------------------------------------------------------------- 8. the rest
def test_empty_and_skipped(mxp, designed):
    plan = make_plan(mxp, designed["eng"], designed["inst"])
    batch, amounts, be, ids, skip, now = designed["calls"][0]
    st, er, ans = plan.batch(batch.subset(np.arange(0)), 0, amounts[:0], be[:0], now, [], None)
    assert len(st) == 0 and len(ans) == 0
    sub = batch.subset(np.arange(300))
    st, er, ans = plan.batch(sub, 0, amounts[:300], be[:300], now, ids[:300], np.ones(300, dtype=np.uint8))
    assert (ans["code"] == QM.SKIPPED).all() and (ans["key"] == QM.NO_KEY).all() and (ans["granted"] == 0).all()
    assert plan.stats()["keys"] == 0
    plan.close()


def test_plan_validation(mxp, designed):
    eng, inst = designed["eng"], designed["inst"]

    def refused(match, **kw):
        args = dict(limits=LIMITS, units=UNITS, rule_unit=RULE_UNIT)
        args.update(kw)
        with pytest.raises(mxp.MxpError, match=r"failed \(1\): .*" + match):
            make_plan(mxp, eng, inst, **args)

    refused("unit 1: label 'dur': a dimension of type DURATION", units=UNITS[:1] + [("rq2", [("s", 0), ("dur", 6)])] + UNITS[2:])
    refused("no limit named 'nope'", units=[("nope", [])] + UNITS[1:])
    refused("label 'a': twice", units=[("rq", [("a", 0), ("a", 1)])] + UNITS[1:])
    refused("no such value rule", units=[("rq", [("a", len(INST_RULES))])] + UNITS[1:])
    refused("is not a unit", rule_unit=RULE_UNIT[:-1] + [len(UNITS)])
    refused("classes", limits=LIMITS + [{"name": "many", "max_amount": 1, "valid_duration_ns": 0, "key_cap": 1,
                                         "overrides": [{"dimensions": {}, "max_amount": 1, "valid_duration_ns": 0,
                                                        "key_cap": 1}] * 256}])
    sixty_four = LIMITS + [{"name": "m%d" % i, "max_amount": 1, "valid_duration_ns": 0, "key_cap": 1} for i in range(60)]
    make_plan(mxp, eng, inst, limits=sixty_four).close()  # (64 classes work)
    # a rule set compiled after the plan was created
    inst2 = mxp.Engine(0)
    inst2.set_vocabulary(MANIFEST)
    inst2.compile(INST_RULES)
    plan = make_plan(mxp, eng, inst2)
    batch, amounts, be, ids, skip, now = designed["calls"][0]
    sub = batch.subset(np.arange(300))
    assert plan.batch_raw(sub, 0, amounts[:300], be[:300], now, ids[:300], None)[0] == 0
    inst2.compile(INST_RULES)
    assert plan.batch_raw(sub, 0, amounts[:300], be[:300], now, ids[:300], None)[0] == ERR_ARG
    assert b"after the plan was created" in eng.lib.mxp_last_error(eng.h)
    plan.close()
    inst2.close()
