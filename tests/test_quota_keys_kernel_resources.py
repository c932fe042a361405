"""Resource budget of quota_keys.hip's kernels (compile-time, no GPU): no scratch anywhere -- the
value formatter of quota_key_fmt.h emits its bytes without per-lane arrays -- and the probe pass
keeps at least the occupancy of mxp_qdd_probe, the pass it is shaped like (read from
quota_dedup.hip's own usage here, not from a constant)."""
from test_kernel_resources import resource_usage

KERNELS = ["mxp_qk_measure", "mxp_qk_write", "mxp_qk_probe", "mxp_qk_rank", "mxp_qk_scan", "mxp_qk_assign",
           "mxp_qk_follow", "mxp_qk_answers"]


def test_quota_keys_kernels():
    usage = resource_usage("quota_keys.hip")
    ours = {k: u for k, u in usage.items() if "mxp_qk_" in k}
    for name in KERNELS:
        assert name in ours, sorted(ours)
    picks = [k for k in ours if "mxp_qk_pick_kernel" in k]
    assert len(picks) == 2 and len(ours) == len(KERNELS) + 2, sorted(ours)  # u16 and u32 ids
    for name, u in ours.items():
        assert u.get("ScratchSize", 0) == 0, (name, u)
    floor = resource_usage("quota_dedup.hip")["mxp_qdd_probe"]["Occupancy"]
    assert ours["mxp_qk_probe"]["Occupancy"] >= floor, (ours["mxp_qk_probe"], floor)
