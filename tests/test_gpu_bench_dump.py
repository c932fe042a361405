"""bench.py's plain run and --dump-outputs on the GPU, at a size of seconds: the arrays written are
what the last timed step computed -- checked pair by pair against the oracle on the same seeded
workload generated here -- the hit counters show that exactly --steps + --warmup steps ran, and the
result line of a plain run holds the headline's keys and none of the --full blocks."""
import os

import numpy as np
import pytest

import oracle
from istio_amd import workloads as W

pytestmark = pytest.mark.gpu

R, N, STEPS, WARMUP = 100, 3000, 3, 2  # (4 bitmap words with a ragged last one; every request sampled)


def _run(d, *more):
    """A plain run (as bench.main makes it) of R rules / list entries x N requests; (line, arrays)."""
    import bench
    args = bench.headline_only(bench.parse(["--rules", str(R), "--requests", str(N), "--list-entries", str(R),
                                            "--steps", str(STEPS), "--warmup", str(WARMUP), "--gen-procs", "1",
                                            "--dump-outputs", str(d)] + list(more)))
    line = bench.run(args, [0])
    got = {f[:-4]: np.load(os.path.join(str(d), f)) for f in sorted(os.listdir(str(d)))}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 * 10**6
    return line, got


@pytest.fixture(scope="module")
def plain_run(libmxp, tmp_path_factory):
    return _run(tmp_path_factory.mktemp("dump"))


def test_plain_result_line(plain_run):
    line, _ = plain_run
    assert line["metric"] == "request x rule predicate evals/sec at 10k rules" and line["unit"] == "pairs/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u32"
    assert (line["steps"], line["warmup"]) == (STEPS, WARMUP) and line["ms_per_step"] > 0
    # value is pairs per second of the timed steps: N x R pairs every ms_per_step
    assert line["value"] == pytest.approx(N * R / (line["ms_per_step"] * 1e-3), rel=1e-9)
    for k in ("roofline", "kernels_ms", "fresh_batch", "end_to_end", "cpu_baseline", "c3", "c4", "c5"):
        assert k not in line, k


def test_dumped_outputs_against_oracle(plain_run):
    from istio_amd.engine import bits_to_codes
    _, got = plain_run
    assert sorted(got) == ["error_flag_index_0", "error_flags_0", "hits", "match_words_0", "request_index_0"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 * 10**6
    assert np.array_equal(got["request_index_0"], np.arange(N))
    assert np.array_equal(got["error_flag_index_0"], np.arange(N))
    manifest, _, batch = W.c2_workload(n_rules=R, n_requests=N, seed=2)
    rules = W.c2_rules(R, seed=2)[0]
    want = oracle.oracle_matrix(oracle.OracleEvaluator(manifest), rules, batch, threads=4)
    words = got["match_words_0"]
    assert words.shape == ((R + 31) // 32, N)
    match = bits_to_codes(words.astype(np.uint32), np.zeros(words.shape, dtype=np.uint32), R)
    assert np.array_equal(match == 1, want == 1), np.argwhere((match == 1) != (want == 1))[:5].tolist()
    assert np.array_equal(got["error_flags_0"] != 0, (want >= 2).any(axis=1))
    assert (want == 1).sum() > 0 and (want >= 2).any()
    # the counters accumulate over every step since the rules were compiled: warm-up + timed steps
    assert np.array_equal(got["hits"], (STEPS + WARMUP) * (want == 1).sum(axis=0))


def test_dumped_list_codes_against_oracle(libmxp, tmp_path):
    """--workload c3-str: every lookup's HandleListEntry status code of the last step."""
    import lists as L
    line, got = _run(tmp_path, "--workload", "c3-str")
    assert sorted(got) == ["codes_0", "lookup_index_0"] and line["unit"] == "lookups/s" and line["steps"] == STEPS
    assert "cpu_baseline" not in line
    entries, syms = W.c3_string_list(n_entries=R, n_lookups=N, seed=3)
    want = L.codes(L.StringList(entries, case_insensitive=True).found(syms), False)
    assert np.array_equal(got["lookup_index_0"], np.arange(N))
    assert np.array_equal(got["codes_0"], want) and 0 < (want == 0).sum() < N


@pytest.mark.parametrize("wl", ["c5", "c5-quota"])
def test_dumped_quota_outputs_against_oracle(libmxp, tmp_path, wl):
    """The memquota outputs of the C5 step (with the predicates, and alone): the per-key deltas summed
    over every step and the last step's granted amounts, against the sequential replay (oracle/memquota.py)."""
    import bench
    import memquota as M
    line, got = _run(tmp_path, "--workload", wl)
    assert ("match_words_0" in got) == (wl == "c5") and "cpu_baseline" not in line
    K = bench.QUOTA_KEYS
    mx, vd, keys, amounts, be = W.quota_workload(n_keys=K, n_requests=N, seed=5)
    ref = M.CMemquota(mx, vd)
    want_delta = np.zeros(K, dtype=np.int64)
    for s in range(WARMUP + STEPS):
        granted = ref.handle_batch(keys, amounts, be, 1_500_000_000 * 10**9 + s * 10**8, threads=4)
        np.add.at(want_delta, keys.astype(np.int64), np.sign(amounts) * granted)
    assert np.array_equal(got["quota_granted_index"], np.arange(N))
    assert np.array_equal(got["quota_granted"], granted) and (granted != 0).any()
    assert np.array_equal(got["quota_delta"], want_delta) and (want_delta != 0).any()
