"""Resource budget of check.hip's kernels (compile-time, no GPU): no scratch anywhere, and the
one-lane-per-request instantiations -- the ones a rule set with about one id per request runs -- keep
the occupancy of mxp_d8_write_kernel<1>, the precedent they are modelled on (read from delta8.hip's
own usage here, not from a constant)."""
import re

from test_kernel_resources import resource_usage


def _kernels(src, name):
    """{template arguments as mangled: usage} of the instantiations of `name` in src"""
    out = {}
    for k, u in resource_usage(src).items():
        m = re.search(r"\d+%sI((?:L[jb]\d+E)+)EEv" % name, k)
        if m:
            out[m.group(1)] = u
    return out


def test_check_kernels():
    usage = resource_usage("check.hip")
    ours = {k: u for k, u in usage.items() if "mxp_" in k}
    # G = 1, 4, 16, 64 x u16 / u32 ids x (count, count with the 64-bit key, write)
    assert len(ours) == 24 and all("mxp_check_combine_kernel" in k for k in ours), sorted(ours)
    for name, u in ours.items():
        assert u.get("ScratchSize", 0) == 0, (name, u)
    d8 = _kernels("delta8.hip", "mxp_d8_write_kernel")
    assert "Lj1E" in d8, sorted(d8)
    floor = d8["Lj1E"]["Occupancy"]
    g1 = {k: u for k, u in _kernels("check.hip", "mxp_check_combine_kernel").items() if k.startswith("Lj1E")}
    assert len(g1) == 6, sorted(g1)
    for k, u in g1.items():
        assert u["Occupancy"] >= floor, (k, u, floor)
