"""Scalar-register spills of the guard-index kernels (compile-time, no GPU).  The kernels read their
argument block through per-phase views (kernels.hip kargs_view) instead of holding all of it in
scalar registers from entry to exit; a scalar that does not fit is parked in a VGPR lane and costs a
v_readlane (a vector issue slot) at every use.  The bounds are what the build achieves -- a change
that brings the spills back fails here.  (Where the remaining spills sit: DESIGN section 4.)"""
import pytest

from test_kernel_resources import resource_usage

# kernel: most `SGPRs Spill` of -Rpass-analysis=kernel-resource-usage
MAX_SGPR_SPILLS = {
    "mxp_index_dtp_lite_kernel": 54,  # (the whole block held in registers: 171)
    "mxp_index_dtp_kernel": 63,       # (195)
    "mxp_index_kernel": 63,           # (188)
}


@pytest.fixture(scope="module")
def usage():
    return resource_usage("kernels.hip")


@pytest.mark.parametrize("kernel", sorted(MAX_SGPR_SPILLS))
def test_index_kernel_scalar_spills(usage, kernel):
    assert kernel in usage, sorted(usage)
    u = usage[kernel]
    assert "SGPRs Spill" in u, u
    assert u["SGPRs Spill"] <= MAX_SGPR_SPILLS[kernel], (kernel, u)
