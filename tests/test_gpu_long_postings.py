"""Long posting lists of the guard index (kernels.hip process_slot): a lane whose share of a round
is MXP_COOP_T (16) postings or more hands its list to the whole wave, which expands it 64 postings
per step; shorter lists keep the posting-major loop.  Bar: bit-exact against the oracle (error texts
included), and device outputs -- match bitmap, error bitmap, hit counters, compact flags --
identical with the cooperative path on and off (MXP_DEBUG_FLAGS 16384), over three back-to-back
evaluations, for every kernel instantiation that shares process_slot.

List lengths sit around every boundary of the code: 1, T - 1, T, T + 1, one wave step (63, 64, 65),
the pair queue (255, 256, 257) and ~1000 (several rounds with VM passes between them).  Batches are
333 requests (5 x 64 + 13: a partial last wave)."""
import numpy as np
import pytest

import oracle
from istio_amd import workloads as W
from istio_amd.bags import BagBatch
from test_gpu_dtp import deferred_ran
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu
FORCE = 262144   # value classes (hence deferred pairs) at any batch size
SERIAL = 16384   # the cooperative expansion off
DFA = 67108864   # literal-key regexps keep their DFA templates (the non-lite deferred kernel)
T = 16           # kernels.hip MXP_COOP_T
N = 5 * 64 + 13
LENGTHS = [1, T - 1, T, T + 1, 63, 64, 65, 255, 256, 257, 1000]
MIDDLE = [T + 1, 65, 257]
# every instantiation sharing process_slot: the lite deferred kernel (default), mxp_index_kernel with
# atomics, the non-lite deferred kernel, the overflow list, the gated re-run
INSTANCES = {"lite": ({}, 0), "atomics": ({"MXP_DTP": "0"}, 0), "dfa": ({}, DFA),
             "overflow": ({"MXP_DTP_CAP": "4"}, 0), "rerun": ({"MXP_DTP_CAP": "4", "MXP_DTP_OVF": "8"}, 0)}
# (a regexp rule whose continuation is a DFA template under flag DFA: the rule set is not lite)
DFA_RULE = '"^s9[0-9]x$".matches(destination.service)'


@pytest.fixture(scope="module")
def mxp(libmxp):
    import istio_amd.engine as mxp
    return mxp


def engine_for(mxp, monkeypatch, env, flags, manifest, rules):
    for k in ("MXP_DTP", "MXP_DTP_CAP", "MXP_DTP_OVF"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MXP_DEBUG_FLAGS", str(flags))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = mxp.Engine(0)
    eng.set_vocabulary(manifest)
    assert (eng.compile(rules) == 0).all()
    return eng


def device_outputs(eng, batch, R):
    import torch
    Wd = (R + 31) // 32
    db = eng.upload(batch)
    dm = torch.zeros((Wd, batch.n), dtype=torch.int32, device="cuda:0")
    de = torch.zeros_like(dm)
    cm = torch.zeros_like(dm)
    flags = torch.ones(batch.n, dtype=torch.uint8, device="cuda:0")  # (stale flags must be cleared)
    hits = torch.zeros(R, dtype=torch.int64, device="cuda:0")
    hc = torch.zeros_like(hits)
    for _ in range(3):  # the fused / streamed choice follows the previous evaluation
        db.eval_hits(dm.data_ptr(), de.data_ptr(), hits.data_ptr(), 0)
        db.eval_compact(cm.data_ptr(), flags.data_ptr(), hc.data_ptr(), 0)
    torch.cuda.synchronize()
    out = [x.cpu().numpy() for x in (dm, de, hits, cm, flags, hc)]
    db.free()
    return out


def check(mxp, monkeypatch, manifest, rules, batch, instance="lite"):
    """Oracle parity of the cooperative build of `instance`, then device identity of the cooperative
    and the serial expansion.  Returns the oracle's codes."""
    env, extra = INSTANCES[instance]
    if instance == "dfa" and "destination.service" in manifest:  # (the prefix case has regexps of its own)
        rules = rules + [DFA_RULE]
    R = len(rules)
    eng = engine_for(mxp, monkeypatch, env, FORCE | extra, manifest, rules)
    assert eng.ruleset_info()["indexed"] > 0
    assert deferred_ran(eng, batch, R) == (instance != "atomics")
    got, want = compare(eng, oracle.OracleEvaluator(manifest), rules, batch, sample_msgs=100)
    coop = device_outputs(eng, batch, R)
    ser_eng = engine_for(mxp, monkeypatch, env, FORCE | extra | SERIAL, manifest, rules)
    assert deferred_ran(ser_eng, batch, R) == (instance != "atomics")
    serial = device_outputs(ser_eng, batch, R)
    for a, b in zip(coop, serial):
        assert np.array_equal(a, b)
    # the device bitmaps are the oracle's too (true bits, error bits), and both evaluations agree
    bits = np.zeros(((R + 31) // 32 * 32, batch.n), dtype=np.uint32)
    for plane, code in ((0, 1), (1, 2)):
        bits[:] = 0
        bits[:R] = (np.minimum(want, 2) == code).T
        words = (bits.reshape(-1, 32, batch.n) << np.arange(32, dtype=np.uint32)[None, :, None]).sum(axis=1, dtype=np.uint32)
        assert np.array_equal(coop[plane].view(np.uint32), words)
    assert np.array_equal(coop[3], coop[0]) and np.array_equal(coop[5], coop[2])
    return want


# ------------------------------------------------------------------ C2: composite, equality fallback
def c2_case(length, p_missing_path):
    S = 2  # rule i belongs to service i % S: the service's fallback list holds `length` rules
    return W.c2_workload(n_rules=S * length, n_requests=N, seed=60 + length, n_services=S,
                         p_missing_path=p_missing_path, p_missing_ip=0.05)


@pytest.mark.parametrize("p_missing_path", [0.0, 1.0 / 64, 0.5, 1.0], ids=["none", "one_per_wave", "half", "all"])
@pytest.mark.parametrize("length", LENGTHS)
def test_c2_equality_fallback(mxp, monkeypatch, length, p_missing_path):
    """Requests without request.path take their service's whole list (the composite's equality
    fallback): no such lane, about one per wave, half the lanes, every lane (64 lists compete for
    the 256-entry queue).  Lengths below T keep the posting-major loop covered."""
    manifest, rules, batch = c2_case(length, p_missing_path)
    want = check(mxp, monkeypatch, manifest, rules, batch)
    if p_missing_path > 0.4:  # the fallback's pairs: request.path's lookup error for every rule of the service
        assert (want >= 2).sum() >= length * N // 4


# ------------------------------------------------------------------------------- plain equality index
def eq_case(length, seed=70):
    S = 3
    rng = np.random.default_rng(seed + length)
    rules = ['destination.service == "s%d" && source.ip != ip("10.1.%d.%d")' % (i % S, (i // S) >> 8, (i // S) & 255)
             for i in range(S * length)]
    bags = []
    for _ in range(N):
        b = {"destination.service": "s%d" % rng.integers(0, S + 1)}  # (s3: no rules)
        if rng.random() < 0.7:  # absent for the rest: an error pair for every posting of the list
            b["source.ip"] = bytes([10, 1, int(rng.integers(0, 4)), int(rng.integers(0, 256))])
        bags.append(b)
    manifest = {"destination.service": "STRING", "source.ip": "IP_ADDRESS"}
    return manifest, rules, BagBatch.from_bags(bags, names=list(manifest))


@pytest.mark.parametrize("length", LENGTHS)
def test_equality_index(mxp, monkeypatch, length):
    """`destination.service == K && source.ip != ip(..)`: every request of a service takes a list
    of `length` continuations; source.ip absent for 30% (error pairs out of long lists)."""
    manifest, rules, batch = eq_case(length)
    want = check(mxp, monkeypatch, manifest, rules, batch)
    assert (want == 1).sum() >= length * N // 4 and (want >= 2).sum() >= length * N // 8


# --------------------------------------------------------------- prefix index, mixed codes on one key
def prefix_case(n_cont=300):
    rules = ['request.path.startsWith("/w1") && source.ip != ip("10.0.%d.%d")' % (k >> 8, k & 255) for k in range(n_cont)]
    special = ['"^/w1$".matches(request.path)', '"^/w1(/.*)?$".matches(request.path)', 'request.path.startsWith("/w1")']
    # (the exact key, the tail key and the direct posting in the middle of the list and at its ends)
    rules = special + rules[:n_cont // 2] + special + rules[n_cont // 2:] + special
    subjects = ["/w1", "/w1/x", "/w1\n", "/w1/a\nb", "/w1\udcc3\udca9\udcff", "/w2", None, 7]
    rng = np.random.default_rng(80)
    bags = []
    for i in range(N):
        b = {}
        sub = subjects[i % len(subjects)] if i < 64 else subjects[int(rng.integers(0, len(subjects)))]
        if sub is not None:
            b["request.path"] = sub
        if rng.random() < 0.8:
            b["source.ip"] = bytes([10, 0, int(rng.integers(0, 2)), int(rng.integers(0, 256))])
        bags.append(b)
    manifest = {"request.path": "STRING", "source.ip": "IP_ADDRESS"}
    return manifest, rules, BagBatch.from_bags(bags, names=list(manifest))


@pytest.mark.parametrize("instance", list(INSTANCES))
def test_prefix_index_mixed_codes(mxp, monkeypatch, instance):
    """One prefix key (`/w1`) whose long list mixes continuations with exact (`^/w1$`) and tail
    (`^/w1(/.*)?$`) literal keys and a direct posting: the literal keys are decided from the list
    owner's subject (the prefix alone, a continuation, newlines at and after the key, non-ASCII
    bytes), other paths and absent / non-string paths find nothing or fail the guard."""
    manifest, rules, batch = prefix_case()
    want = check(mxp, monkeypatch, manifest, rules, batch, instance)
    sp = [i for i, r in enumerate(rules) if "source.ip" not in r]
    assert all(0 < (want[:, j] == 1).sum() < batch.n for j in sp)
    assert (want >= 2).sum() > 1000


# ------------------------------------------------------- the other instantiations, middle-sized lists
@pytest.mark.parametrize("instance", [k for k in INSTANCES if k != "lite"])
@pytest.mark.parametrize("length", MIDDLE)
def test_c2_equality_fallback_instances(mxp, monkeypatch, length, instance):
    manifest, rules, batch = c2_case(length, 0.5)
    check(mxp, monkeypatch, manifest, rules, batch, instance)


@pytest.mark.parametrize("instance", [k for k in INSTANCES if k != "lite"])
@pytest.mark.parametrize("length", MIDDLE)
def test_equality_index_instances(mxp, monkeypatch, length, instance):
    manifest, rules, batch = eq_case(length)
    check(mxp, monkeypatch, manifest, rules, batch, instance)
