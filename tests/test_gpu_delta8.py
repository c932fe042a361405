"""MXP_RESOLVE_IDS_DELTA8 (include/mxp.h; delta8.hip): the action lists as a delta-coded byte stream.
The yardstick is always the u16 Resolve of the same engine (itself pinned against the resolver
restatement in test_gpu_resolver.py / test_gpu_pair_resolve.py): the expected byte offsets and
stream are encode_delta8 of its output, compared byte for byte, with status and err_rule equal.

Left out: more than 65536 rules with the flag (MXP_ERR_ARG, the check the u16 flag shares) -- it
needs a compile of 65537 rules, which no test here pays for."""
import ctypes

import numpy as np
import pytest

from istio_amd import workloads as W
from istio_amd.workloads import c2_resolve_case

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_NOMEM = 1, 4
U16, DELTA8 = 1, 2


@pytest.fixture(scope="module")
def mxp(libmxp):
    import istio_amd.engine as mxp
    return mxp


def make_engine(mxp, manifest, rules, conf, cls=None, devices=0):
    eng = (cls or mxp.Engine)(devices)
    eng.set_vocabulary(manifest)
    eng.compile(rules)
    eng.set_resolver(conf["identity_attr"], conf["default_ns"], conf["rule_ns"], conf["variety_mask"],
                     conf["is_tcp"], conf["empty_match"])
    return eng


def expect(mxp, u16):
    """the delta8 outputs a u16 Resolve's outputs stand for"""
    status, err_rule, off, ids = u16
    boff, stream = mxp.encode_delta8(off, ids)
    return status.copy(), err_rule.copy(), boff, stream


def same(got, want, what):
    for name, x, y in zip(("status", "err_rule", "sel_off", "stream"), got, want):
        assert x.dtype == y.dtype and np.array_equal(x, y), (what, name)


def raw_resolve(mxp, eng, batch, variety, flags, cap, pinned):
    """mxp_resolve_batch_ex as called, without the mirror's retry -> (rc, status, err_rule, off, sel u8)"""
    n = batch.n
    if pinned:
        arena = mxp.PinnedArena(n * 13 + 8 + cap + 4 * 64)
        out = (arena.empty(n, np.uint8), arena.empty(n, np.uint32), arena.empty(n + 1, np.uint64),
               arena.empty(cap, np.uint8))
    else:
        arena = None
        out = (np.empty(n, np.uint8), np.empty(n, np.uint32), np.empty(n + 1, np.uint64), np.empty(max(cap, 1), np.uint8))
    rc = eng.lib.mxp_resolve_batch_ex(eng.h, ctypes.byref(batch.c_struct()), variety, flags, out[0].ctypes.data,
                                      out[1].ctypes.data, out[2].ctypes.data, out[3].ctypes.data, cap)
    return (rc,) + tuple(x.copy() for x in out) + (arena,)


# ------------------------------------------------------------------------------ 1. designed lists
BLOCKS = [("ns1", 63), ("ns0", 65), ("ns2", 129), ("ns3", 600), ("ns4", 1), ("ns5", 442)]  # ns0: the default


def designed_case():
    """Every rule has an empty match, so a request's list is fixed by its namespace and the variety:
    the default block (variety 0 only) then the request's own.  In the 600-block variety 0 selects
    positions 0, 255, 511 (a step of d = 254, one byte FE, next to one of d = 255, an escape) and the
    dense run 520..599; variety 1 all 600 (a list above 256 ids that starts with an escape).  The
    442-block selects two rules 300 apart; ns6 / ns7 have no rules."""
    n_rules = sum(k for _, k in BLOCKS)
    manifest, rules, batch = W.c2_workload(n_rules=n_rules, n_requests=4097, seed=51)
    rule_ns, vmask = [], []
    for ns, k in BLOCKS:
        rule_ns += [ns] * k
        if ns == "ns0":
            vmask += [1] * k
        elif ns == "ns3":
            vmask += [3 if p in (0, 255, 511) or p >= 520 else 2 for p in range(k)]
        elif ns == "ns5":
            vmask += [3 if p % 300 == 0 else 0 for p in range(k)]
        else:
            vmask += [3] * k
    conf = dict(rule_ns=rule_ns, variety_mask=vmask, is_tcp=[0] * n_rules, empty_match=[1] * n_rules,
                identity_attr="destination.service", default_ns="ns0")
    return manifest, rules, conf, batch


@pytest.fixture(scope="module")
def designed(mxp):
    manifest, rules, conf, batch = designed_case()
    eng = make_engine(mxp, manifest, rules, conf)
    u16 = {v: [x.copy() for x in eng.resolve_arrays(batch, v, ids16=True)] for v in (0, 1)}
    yield eng, batch, u16
    eng.close()


def test_designed_lists_hold_every_case(designed):
    """(from the u16 output: the test below cannot pass on an input that lost what it is for)"""
    _, _, u16 = designed
    gap = back = first = fe = False
    lens = set()
    for v in (0, 1):
        _, _, off, ids = u16[v]
        off = off.astype(np.int64)
        ids = ids.astype(np.int64)
        cnt = np.diff(off)
        lens |= set(cnt.tolist())
        starts = off[:-1][cnt > 0]
        is_first = np.zeros(len(ids), dtype=bool)
        is_first[starts] = True
        d = np.empty(len(ids), dtype=np.int64)
        d[1:] = ids[1:] - ids[:-1] - 1
        d[is_first] = ids[is_first]
        gap |= bool(np.any((d > 254) & ~is_first))
        back |= bool(np.any((d < 0) & ~is_first))
        first |= bool(np.any(is_first & (ids >= 255)))
        fe |= bool(np.any(d == 254)) and bool(np.any(d == 255))
    assert gap and back and first and fe
    assert 0 in lens and 63 in lens and max(lens) > 256 and any(128 < x <= 256 for x in lens)
    assert {1, 2, 65, 66, 67, 128, 129, 600} <= lens  # (every group width's iteration boundary)


@pytest.mark.parametrize("group", ["", "1", "2", "4", "8", "16", "32", "64"])
def test_designed_lists(mxp, designed, monkeypatch, group):
    """Both varieties, with the lanes per request the host picks and with every width forced."""
    eng, batch, u16 = designed
    if group:
        monkeypatch.setenv("MXP_D8_GROUP", group)
    for v in (0, 1):
        want = expect(mxp, u16[v])
        assert (want[0] == 0).all() and len(want[3]) > len(u16[v][3])  # (escapes: more bytes than ids)
        same(eng.resolve_arrays(batch, v, delta8=True), want, (v, group))
        same(eng.resolve_arrays(batch, v, cap=len(want[3]), delta8=True, pinned=True), want, (v, group, "pinned"))
    sel = eng.resolve(batch, 1, delta8=True)[2]
    off, ids = u16[1][2], u16[1][3]
    assert all(np.array_equal(sel[q], ids[int(off[q]):int(off[q + 1])]) for q in range(0, batch.n, 37))


# ------------------------------------------------------------------------ 2. pair path and errors
@pytest.fixture(scope="module")
def c2case(mxp):
    """case 2's data, and one engine per MXP_RESOLVE_PAIRS setting (read when the engine is made)"""
    manifest, rules, conf, batch = c2_resolve_case(520, 2, 32768)
    mp = pytest.MonkeyPatch()
    engines = {}
    for pairs in ("2", "0"):
        mp.setenv("MXP_RESOLVE_PAIRS", pairs)
        engines[pairs] = make_engine(mxp, manifest, rules, conf)
    mp.undo()
    u16 = [x.copy() for x in engines["0"].resolve_arrays(batch, 1, ids16=True)]
    yield manifest, rules, conf, batch, engines, u16
    for e in engines.values():
        e.close()


@pytest.mark.parametrize("pairs", ["2", "0"])
def test_pair_path_and_errors(mxp, c2case, pairs):
    _, _, _, batch, engines, u16 = c2case
    want = expect(mxp, u16)
    st = want[0]
    assert (st == 0).sum() > 10000 and (st == 3).sum() > 20 and (st == 1).sum() > 20 and len(want[3]) > 100
    got = engines[pairs].resolve_arrays(batch, 1, delta8=True)
    same(got, want, pairs)
    assert (np.diff(got[2].astype(np.int64))[st != 0] == 0).all()  # (not resolved: an empty range)
    same([x.copy() for x in engines[pairs].resolve_arrays(batch, 1, ids16=True)], u16, "u16 after delta8")


# --------------------------------------------------------------------------- 3. long random lists
def test_long_random_lists(mxp):
    n_rules = 4096
    manifest, rules, batch = W.c4_workload(n_rules=n_rules, n_requests=8192)
    conf = dict(rule_ns=["istio-system"] * n_rules, variety_mask=[1] * n_rules, is_tcp=[0] * n_rules,
                empty_match=[0] * n_rules, identity_attr="destination.service", default_ns="istio-system")
    eng = make_engine(mxp, manifest, rules, conf)
    u16 = [x.copy() for x in eng.resolve_arrays(batch, 0, ids16=True)]
    want = expect(mxp, u16)
    n_ids, n_bytes = len(u16[3]), len(want[3])
    print("\nc4 4096 x 8192: %.1f ids per request, delta8 %d B / u16 %d B = %.3f, escapes %.5f of ids"
          % (n_ids / batch.n, n_bytes, 2 * n_ids, n_bytes / (2 * n_ids), (n_bytes - n_ids) / 2 / n_ids))
    assert n_ids / batch.n > 64
    same(eng.resolve_arrays(batch, 0, delta8=True), want, "pageable")
    same(eng.resolve_arrays(batch, 0, cap=n_bytes + 100, delta8=True, pinned=True), want, "pinned")
    eng.close()


# ------------------------------------------------------------------------------------ 4. ragged n
@pytest.mark.parametrize("n", [0, 1, 3, 5, 1025, 4097])
def test_ragged_batches(mxp, c2case, n):
    _, _, _, full, engines, _ = c2case
    batch = full.subset(np.arange(7, 7 + n))
    eng = engines["0"]
    want = expect(mxp, [x.copy() for x in eng.resolve_arrays(batch, 1, ids16=True)])
    got = eng.resolve_arrays(batch, 1, delta8=True)
    same(got, want, n)
    assert len(got[0]) == n and len(got[2]) == n + 1
    if n:
        same(engines["2"].resolve_arrays(batch, 1, delta8=True), want, (n, "pairs"))
        same(eng.resolve_arrays(batch, 1, cap=max(16, len(want[3])), delta8=True, pinned=True), want, (n, "pinned"))


# ------------------------------------------------------------------------- 5. capacities in bytes
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_capacities_in_bytes(mxp, c2case, pinned):
    _, _, _, batch, engines, u16 = c2case
    eng = engines["0"]
    want = expect(mxp, u16)
    total = len(want[3])
    assert total > 100
    for cap in (total, total + 1000, total - 1, 16):
        rc, st, er, off, sel, _keep = raw_resolve(mxp, eng, batch, 1, DELTA8, cap, pinned)
        assert rc == (0 if cap >= total else ERR_NOMEM), cap
        # (too small: status, err_rule and the byte offsets complete, the caller retries with off[n])
        assert np.array_equal(st, want[0]) and np.array_equal(er, want[1]) and np.array_equal(off, want[2]), cap
        if rc == 0:
            assert np.array_equal(sel[:total], want[3]), cap
        else:
            rc, st, er, off2, sel, _keep = raw_resolve(mxp, eng, batch, 1, DELTA8, int(off[-1]), pinned)
            assert rc == 0
            same((st, er, off2, sel[:total]), want, ("retry", cap))
        same(eng.resolve_arrays(batch, 1, cap=cap, delta8=True, pinned=pinned), want, ("mirror", cap))


# --------------------------------------------------------------------------------------- 6. group
def test_group_stream_is_one_engines(mxp, c2case):
    manifest, rules, conf, batch, engines, u16 = c2case
    want = expect(mxp, u16)
    same(engines["0"].resolve_arrays(batch, 1, delta8=True), want, "one engine")
    g = make_engine(mxp, manifest, rules, conf, cls=mxp.Group, devices=[0, 0])
    shards = W.split_batch(batch, 2)
    total, n = len(want[3]), batch.n
    same(g.resolve_arrays(shards, 1, delta8=True), want, "pageable")
    for cap in (total, total + 64):
        arena = mxp.PinnedArena(n * 13 + 8 + cap + 4 * 64)
        out = (arena.empty(n, np.uint8), arena.empty(n, np.uint32), arena.empty(n + 1, np.uint64),
               arena.empty(cap, np.uint8))
        for rep in range(2):
            same(g.resolve_arrays(shards, 1, cap=cap, delta8=True, out=out), want, (cap, rep, "arrays"))
            out[3][:] = 0
            job = g.resolve_submit(g.upload(shards, no_wait=True), 1, delta8=True)
            same(g.resolve_finish(job, cap, out=out), want, (cap, rep, "submit"))
            out[3][:] = 0
    sel = g.resolve(shards, 1, delta8=True)[2]
    off, ids = u16[2], u16[3]
    assert all(np.array_equal(sel[q], ids[int(off[q]):int(off[q + 1])]) for q in range(0, n, 101))
    g.close()


# --------------------------------------------------------------------------------------- 7. flags
def test_both_formats_refused(mxp, c2case):
    manifest, rules, conf, full, engines, _ = c2case
    batch = full.subset(np.arange(64))
    eng = engines["0"]
    rc = raw_resolve(mxp, eng, batch, 1, U16 | DELTA8, 4096, False)[0]
    assert rc == ERR_ARG
    assert raw_resolve(mxp, eng, batch, 1, 4, 4096, False)[0] == ERR_ARG  # (a flag nobody knows)
    with pytest.raises(mxp.MxpError, match=r"failed \(1\)"):
        eng.resolve_arrays(batch, 1, ids16=True, delta8=True)
    with pytest.raises(mxp.MxpError, match=r"failed \(1\)"):
        eng.resolve_uploaded(eng.upload(batch), 1, 4096, ids16=True, delta8=True)
    with pytest.raises(mxp.MxpError, match=r"failed \(1\)"):
        eng.resolve_submit(eng.upload(batch), 1, ids16=True, delta8=True)
    g = make_engine(mxp, manifest, rules, conf, cls=mxp.Group, devices=[0, 0])
    shards = W.split_batch(batch, 2)
    with pytest.raises(mxp.MxpError, match=r"failed \(1\)"):
        g.resolve_arrays(shards, 1, ids16=True, delta8=True)
    with pytest.raises(mxp.MxpError, match=r"failed \(1\)"):
        g.resolve_arrays(None, 1, cap=4096, ids16=True, delta8=True, uploaded=g.upload(shards))
    with pytest.raises(mxp.MxpError, match=r"failed \(1\)"):
        g.resolve_submit(g.upload(shards), 1, ids16=True, delta8=True)
    # (both still work after the refusals)
    want = expect(mxp, [x.copy() for x in eng.resolve_arrays(batch, 1, ids16=True)])
    same(eng.resolve_arrays(batch, 1, delta8=True), want, "engine")
    same(g.resolve_arrays(shards, 1, delta8=True), want, "group")
    g.close()
