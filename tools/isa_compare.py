#!/usr/bin/env python3
"""Per-kernel codegen comparison of two builds of kernels.hip.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S kernels.hip -o X.s \
          -Rpass-analysis=kernel-resource-usage 2> X.remarks
    tools/isa_compare.py parent.s parent.remarks tree.s tree.remarks

For every mxp_* kernel: the resource remarks (SGPRs, VGPRs, scratch, occupancy, spills, LDS) and the
instruction stream (label to end of function; comments, directives and blank lines stripped, basic
block labels renumbered) of both builds.  Verdict per kernel: `identical` (same stream), `close`
(same resources, instruction count within CLOSE of the parent's) or `needs A/B`.
"""
import re
import sys

CLOSE = 8
FIELDS = ["TotalSGPRs", "VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]"]


def streams(path):
    out, name, cur = {}, None, None
    for line in open(path):
        s = line.split(";")[0].strip()
        if name is None:
            m = re.match(r"(mxp_\w+):$", s)
            if m:
                name, cur = m.group(1), []
            continue
        if s.startswith(".Lfunc_end"):
            out[name] = cur
            name = None
        elif s and not s.startswith("."):
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return out


def remarks(path):
    out, name = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+Function Name: (\w+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+): (\w+) \[-Rpass", line)
        if m and name:
            out[name][m.group(1).strip()] = m.group(2)
    return out


def main():
    ps, pr, ts, tr = streams(sys.argv[1]), remarks(sys.argv[2]), streams(sys.argv[3]), remarks(sys.argv[4])
    print("# instructions: every line from the kernel's label to .Lfunc_end that is neither blank, a comment, a directive")
    print("# nor a label -- s_endpgm itself and the blocks laid out after the first s_endpgm included, so a count runs 1-7")
    print("# above one that stops before the first s_endpgm (mxp_fill_dtp_kernel 787 against 786, mxp_fill_tile_kernel 2491 against 2484)")
    print("kernel | parent: instructions " + " ".join(f.split(" ")[0] for f in FIELDS) + " | tree: same | verdict")
    worst = 0
    for k in sorted(set(ps) | set(ts)):
        a, b = ps.get(k), ts.get(k)
        ra, rb = [pr.get(k, {}).get(f, "?") for f in FIELDS], [tr.get(k, {}).get(f, "?") for f in FIELDS]
        if a is None or b is None:
            verdict = "MISSING"
        elif a == b and ra == rb:
            verdict = "identical"
        elif ra == rb and abs(len(a) - len(b)) <= CLOSE:
            verdict = "close"
        else:
            verdict = "needs A/B"
        worst = max(worst, {"identical": 0, "close": 1}.get(verdict, 2))
        print(f"{k} | {len(a or [])} {' '.join(ra)} | {len(b or [])} {' '.join(rb)} | {verdict}")
    print(f"{len(set(ps) | set(ts))} kernels")
    return 1 if worst == 2 else 0


if __name__ == "__main__":
    sys.exit(main())
