"""mxp_fill_tile_kernel, the sparse fill of a retained match bitmap (DESIGN.md §4 "Retained match
bitmap"): one workgroup per sort tile of 1024 requests covers every plain fill chunk of the tile --
thread t checks the kinds of quad t once per guard column, wave w scans the count bytes of chunks
w, w + 4, ... (one u32 = four quads per lane), and the live (chunk, quad) items are compacted into
an LDS queue and stored 256 at a time.  The cases here are the ones that mapping can get wrong:
tile and word edges, chunk counts that leave waves idle or need more than one round, each byte of
a lane's word, rows only the previous / only the current / both evaluations name, the dense
fallback inside the kernel, and the kind check.

Bar (as test_gpu_fill_retain): match bitmap, compact flags and hit counters identical to an engine
with deferred pairs off (MXP_DTP=0) that retains nothing -- never to the retained engine itself --
and fill_retain_stats()["sparse"] == 1 wherever the sparse path is meant.

Error records: no evaluation that writes records (errlog) can reach the sparse fill -- only a
caller's buffer can be retained, and the entry points that evaluate into a caller's buffer
(DeviceBatch.eval_compact / eval_hits, the group) run without records -- so there is no record set
to compare; the kind check is compared through the compact flags."""
import numpy as np
import pytest

from istio_amd import workloads as W
from istio_amd.bags import ABSENT, INT64
from test_gpu_dtp import PATHS, deferred_ran, engine_for
from test_gpu_dtp_handoff import pool  # noqa: F401  (a fixture)
from test_gpu_fill_retain import Out, batches, make_ref, retained, rules4, same

pytestmark = pytest.mark.gpu

N_MAIN = 2048 + 37  # two tiles and a ragged third (37 requests: 9 quads and one request)
EDGE_QUADS = (0, 3, 4, 63, 64, 252, 255)  # first / last byte of a lane's word, of a wave, of the tile


@pytest.fixture(scope="module")
def mxp(libmxp):
    import istio_amd.engine as mxp
    return mxp


def rule_sets(pool):
    """Plain fill chunks hold 16 bitmap words: 1 chunk (waves 1-3 get none), 2 chunks (pool: 600
    rules), 5 chunks (every pool rule four times over: waves get 2, 1, 1, 1)."""
    return {1: pool["rules"][:512], 2: pool["rules"], 5: rules4(pool)}


@pytest.fixture(scope="module")
def refs(mxp, pool):
    """Reference engines (MXP_DTP=0, nothing retained) per rule set, results kept per batch."""
    cache = {}

    def get(chunks):
        if chunks not in cache:
            cache[chunks] = make_ref(mxp, pool["manifest"], rule_sets(pool)[chunks])
        return cache[chunks]
    return get


@pytest.fixture(scope="module")
def engines(mxp, pool):
    """Engines under test per rule set (default paths), compiled once."""
    cache = {}

    def get(chunks):
        if chunks not in cache:
            mp = pytest.MonkeyPatch()
            mp.delenv("MXP_FILL_RETAIN", raising=False)
            cache[chunks] = engine_for(mxp, mp, {}, pool["manifest"], rule_sets(pool)[chunks], flags="0")
            mp.undo()
        return cache[chunks]
    return get


def clean_rich(pool):
    """Pool requests with true pairs and no error pair."""
    true = (pool["want"] == 1).sum(axis=1)
    r = np.flatnonzero((true >= 1) & (pool["cnt"] == true))
    assert len(r) > 500
    return r


def placed(pool, n, is_rich, seed):
    """A batch of n requests: the quads is_rich(quad index) marks hold one rich request four times
    over, every other request has no pair at all."""
    rng = np.random.default_rng(seed)
    q = np.arange(n) // 4
    rich_q = rng.choice(clean_rich(pool), (n + 3) // 4)[q]
    return pool["big"].subset(np.where(is_rich(q), rich_q, rng.choice(pool["zero"], n)))


def has_bits(match):
    """Per request: some bit in some word."""
    return (match != 0).any(axis=0)


def run_sequence(eng, ref, R, n, seq, fallbacks=None):
    """The batches of `seq` in turn into one freshly retained buffer: every step equals the
    reference, every step but the first is sparse; -> the steps' hook values."""
    out = retained(eng, R, n)
    stats = []
    for k, (name, b) in enumerate(seq):
        got, st = out.run(eng, b)
        print(n, k, name, st)
        same(got, ref(b), (n, k, name))
        assert st["sparse"] == (1 if k else 0), (k, name, st)
        assert st["fallbacks"] == (fallbacks[k] if fallbacks else 0), (k, name, st)
        stats.append(st)
    return stats


@pytest.mark.parametrize("chunks", [5, 2, 1])
@pytest.mark.parametrize("n", [1023, 1024, 1028, 2048, 2052])
def test_tile_and_word_edges(pool, refs, engines, n, chunks):
    """P, Z, Q, P at sizes one request short of a tile, a whole tile, a tile and one quad, two
    tiles, two tiles and one quad -- with 5, 2 and 1 plain fill chunks."""
    rules = rule_sets(pool)[chunks]
    R, B, eng, ref = len(rules), batches(pool, n), engines(chunks), refs(chunks)
    if chunks == 1:
        assert (R + 31) // 32 <= 16 and deferred_ran(eng, B["P"], R)
    st = run_sequence(eng, ref, R, n, [(k, B[k]) for k in ("P", "Z", "Q", "P")])
    z = ref(B["Z"])
    assert ref(B["P"])[0].any() and not z[0].any() and not z[1].any()
    assert st[0]["live"] > 0 and st[1]["live"] == 0 and st[1]["live_prev"] == st[0]["live"]
    assert st[2]["live"] > 0 and st[3]["live_prev"] == st[2]["live"]


def test_byte_positions(pool, refs, engines):
    """Rich quads only at tile-quad indices 0, 3, 4, 63, 64, 252 and 255 of every tile: that batch,
    Z, that batch.  From the reference: exactly those quads carry bits."""
    rules = rule_sets(pool)[5]
    R, eng, ref = len(rules), engines(5), refs(5)
    E = placed(pool, N_MAIN, lambda q: np.isin(q % 256, EDGE_QUADS), seed=21)
    Z = batches(pool, N_MAIN)["Z"]
    st = run_sequence(eng, ref, R, N_MAIN, [("E", E), ("Z", Z), ("E", E)])
    tq = np.arange(N_MAIN) // 4 % 256
    bits = has_bits(ref(E)[0])
    assert bits[np.isin(tq, EDGE_QUADS)].all() and not bits[~np.isin(tq, EDGE_QUADS)].any()
    for e in (0, 3, 4):  # (the ragged third tile holds quads 0 .. 9)
        assert bits[(tq == e) & (np.arange(N_MAIN) >= 2048)].all()
    assert st[0]["live"] == st[2]["live"] == st[1]["live_prev"] > 0 and st[1]["live"] == st[2]["live_prev"] == 0


def test_previous_only_current_only_both(pool, refs, engines):
    """A (rich even quads) and B (rich odd quads): A, B, A, A.  After B no bit of A remains (rows
    only the previous evaluation names are stored as zeros); after the second A in a row the rows
    both evaluations name hold the pairs."""
    rules = rule_sets(pool)[5]
    R, eng, ref = len(rules), engines(5), refs(5)
    A = placed(pool, N_MAIN, lambda q: q % 2 == 0, seed=22)
    Bb = placed(pool, N_MAIN, lambda q: q % 2 == 1, seed=23)
    even = np.arange(N_MAIN) // 4 % 2 == 0
    ba, bb = has_bits(ref(A)[0]), has_bits(ref(Bb)[0])
    assert ba[even].all() and not ba[~even].any() and bb[~even].all() and not bb[even].any()
    st = run_sequence(eng, ref, R, N_MAIN, [("A", A), ("B", Bb), ("A", A), ("A", A)])
    assert st[1]["live_prev"] == st[0]["live"] > 0 and st[3]["live"] == st[3]["live_prev"] == st[0]["live"]


def test_more_chunks_than_a_round(mxp, monkeypatch):
    """17k C2 rules: 34 plain fill chunks -- more than the sort's window of 32 and than one round of
    the fill's queue (4 waves x 8 chunks) -- at n = 1029 (a tile and a quad and one request): P, Z, P."""
    manifest, rules, big = W.c2_workload(n_rules=17_000, n_requests=1029, seed=63, n_services=64, p_missing_path=0.1)
    _, _, other = W.c2_workload(n_rules=17_000, n_requests=16 * 1029, seed=64, n_services=128, p_missing_path=0.1)
    svc = other.values[list(other.names).index("destination.service")]
    Z = other.subset(np.flatnonzero(svc >= 64)[:1029])
    assert Z.n == 1029
    R = len(rules)
    assert (R + 31) // 32 > 33 * 16
    ref = make_ref(mxp, manifest, rules)
    monkeypatch.delenv("MXP_FILL_RETAIN", raising=False)
    eng = engine_for(mxp, monkeypatch, {}, manifest, rules, flags="0")
    st = run_sequence(eng, ref, R, 1029, [("P", big), ("Z", Z), ("P", big)])
    z = ref(Z)
    assert ref(big)[0].any() and not z[0].any() and not z[1].any()
    assert st[0]["live"] == st[2]["live"] > 0 and st[1]["live"] == 0


@pytest.mark.parametrize("n", [1028, 2085])
def test_dense_fallback_in_the_tile_kernel(mxp, monkeypatch, pool, refs, n):
    """An overflow list of 8 fills up on P: the next fill (Z) is asked for sparsely and stores every
    row of every chunk on the device; Z overflows nothing, so the third is sparse again."""
    rules = rule_sets(pool)[5]
    B = batches(pool, n)
    monkeypatch.delenv("MXP_FILL_RETAIN", raising=False)
    eng = engine_for(mxp, monkeypatch, PATHS[2], pool["manifest"], rules, flags="0")
    run_sequence(eng, refs(5), len(rules), n, [(k, B[k]) for k in ("P", "Z", "P")], fallbacks=[0, 1, 1])


def test_kind_check(pool, refs, engines):
    """Every seventh request lacks the fills' guard attribute (destination.service) or carries it
    as an INT64, in a batch with no error pair otherwise: the flags of those requests are the
    fill's own.  P, K, Z, K on two chunks and on five: K runs sparse, after and before pairs."""
    n = N_MAIN
    base = placed(pool, n, lambda q: q % 3 == 0, seed=24)
    K = base.subset(np.arange(n))
    c = list(K.names).index("destination.service")
    kinds = K.kinds[c].copy()
    kinds[0::14] = ABSENT
    kinds[7::14] = INT64
    K.kinds[c] = kinds
    seventh = np.arange(n) % 7 == 0
    for chunks in (2, 5):
        rules = rule_sets(pool)[chunks]
        ref = refs(chunks)
        assert not ref(base)[1].any() and ref(K)[1][seventh].all() and not ref(K)[1][~seventh].any()
        B = batches(pool, n)
        run_sequence(engines(chunks), ref, len(rules), n, [("P", B["P"]), ("K", K), ("Z", B["Z"]), ("K", K)])
