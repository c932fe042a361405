"""What DeduplicationID handling costs on the C5 batch: mxp_quota_alloc_device (no ids: all the
engine could do before) against mxp_quota_alloc_dedup_device, alternated in one process on
device-resident inputs, then the dedup call's kernels from a rocprofv3 --kernel-trace --stats run
of its own (a child process running this file with --calls-only).

The batch: W.quota_workload(n_keys=1024, n_requests=1 << 20, seed=5); ids of 36 + 12 bytes (a
UUID-shaped prefix and a quota name, as grpcServer.go:200 builds them); 1% of the ids repeat an id
of the batch, 1% are already in `old`.  Before every timed dedup call the state is set up again
(two reaps, the `old` ids stored by a small call, one reap), so each call probes an empty `recent`
and an `old` of ~10k ids and stores ~98% of the batch.

usage: quota_dedup_ab.py [--reps 7] [--no-kernels] [--out DIR]"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from istio_amd import workloads as W  # noqa: E402
from istio_amd.engine import Engine  # noqa: E402

BASE_NS = 1_500_000_000 * 10**9
N, KEYS, ID_LEN = 1 << 20, 1024, 48
NAMES = [b"requestcount", b"quota-name-b", b"ratelimit-00", b"per-user-rpm"]


def make_ids(rng):
    """[N, 48] id bytes: hex digits in the 8-4-4-4-12 shape + a 12-byte name; 1% in-batch repeats;
    the first 1% of the distinct rows are the ones stored in `old`."""
    hexd = np.frombuffer(b"0123456789abcdef", dtype=np.uint8)
    ids = np.empty((N, ID_LEN), dtype=np.uint8)
    ids[:, :36] = hexd[rng.integers(0, 16, size=(N, 36))]
    ids[:, [8, 13, 18, 23]] = ord("-")
    names = np.frombuffer(b"".join(NAMES), dtype=np.uint8).reshape(len(NAMES), 12)
    ids[:, 36:] = names[rng.integers(0, len(NAMES), size=N)]
    rep = rng.choice(N, size=N // 100, replace=False)
    ids[rep] = ids[rng.integers(0, N, size=rep.size)]
    in_old = rng.choice(N, size=N // 100, replace=False)
    return ids, in_old


class Setup:
    def __init__(self):
        self.eng = Engine(0)
        mx, vd, keys, amounts, be = W.quota_workload(n_keys=KEYS, n_requests=N, seed=5)
        self.mx, self.vd = mx, vd
        ids, in_old = make_ids(np.random.default_rng(5))
        cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        self.dk, self.da, self.db = cu(keys.view(np.int32)), cu(amounts), cu(be)
        self.di = cu(np.concatenate([ids.reshape(-1), np.zeros(16, np.uint8)]))
        self.do = cu((np.arange(N + 1, dtype=np.int64) * ID_LEN).astype(np.uint32).view(np.int32))
        # the small call that fills `old`: cells' key 0 ... whatever the key, amount 1
        m = in_old.size
        self.m = m
        self.ok, self.oa, self.ob = cu(keys[in_old].view(np.int32)), cu(np.ones(m, np.int64)), cu(np.zeros(m, np.uint8))
        self.oi = cu(np.concatenate([ids[in_old].reshape(-1), np.zeros(16, np.uint8)]))
        self.oo = cu((np.arange(m + 1, dtype=np.int64) * ID_LEN).astype(np.uint32).view(np.int32))
        self.dg = torch.zeros(N, dtype=torch.int64, device="cuda")
        self.dv = torch.zeros(N, dtype=torch.int64, device="cuda")
        self.dd = torch.zeros(N, dtype=torch.uint8, device="cuda")
        self.qa = self.eng.quota_create(mx, vd)
        self.qb = self.eng.quota_create(mx, vd)
        self.now = BASE_NS

    def plain(self):
        self.qa.alloc_device(N, self.dk.data_ptr(), self.da.data_ptr(), self.db.data_ptr(), self.now, 0, self.dg.data_ptr())

    def prepare_dedup(self):
        q = self.qb
        q.reap()
        q.reap()
        q.alloc_dedup_device(self.m, self.ok.data_ptr(), self.oa.data_ptr(), self.ob.data_ptr(), self.oi.data_ptr(),
                             self.oo.data_ptr(), self.m * ID_LEN, self.now, 0, self.dg.data_ptr())
        q.reap()

    def dedup(self):
        self.qb.alloc_dedup_device(N, self.dk.data_ptr(), self.da.data_ptr(), self.db.data_ptr(), self.di.data_ptr(),
                                   self.do.data_ptr(), N * ID_LEN, self.now, 0, self.dg.data_ptr(), self.dv.data_ptr(),
                                   self.dd.data_ptr())

    def timed(self, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)


def calls_only(reps):
    """For the profiler: warm-up, then `reps` dedup calls, each from the prepared state."""
    S = Setup()
    for _ in range(2 + reps):
        S.prepare_dedup()
        torch.cuda.synchronize()
        S.dedup()
        torch.cuda.synchronize()
        S.now += 300_000_000
    print("dedup_stats", S.qb.dedup_stats(), "dups", int(S.dd.sum()))


def kernel_table(out, reps):
    d = os.path.join(out, "quota_dedup_kt")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "kt", "--",
           sys.executable, os.path.abspath(__file__), "--calls-only", "--reps", str(reps)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=400)
    print(r.stdout.decode(errors="replace")[-600:])
    if r.returncode:
        raise SystemExit("rocprofv3 run failed (%d)" % r.returncode)
    traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    agg = defaultdict(list)
    for row in csv.DictReader(open(traces[0])):
        name = row["Kernel_Name"].split("(")[0]
        if name.startswith(("mxp_qdd_", "mxp_quota_")):
            agg[name].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1000.0)
    # a main call launches each kernel once; so does the small call that fills `old` (its launches are
    # the short half of each name's list)
    calls = 2 + reps
    print("kernels of the dedup call (us; the 1M-request launches of %d calls, median and range):" % calls)
    for name, t in sorted(agg.items(), key=lambda kv: -max(kv[1])):
        big = sorted(t)[-calls:] if name != "mxp_qdd_rehash" else sorted(t)
        print("  %-24s n=%2d  med %8.1f  min %8.1f  max %8.1f" % (name, len(big), big[len(big) // 2], big[0], big[-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls-only", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=None, help="directory for the raw kernel trace (default: a temporary one)")
    args = ap.parse_args()
    if args.calls_only:
        return calls_only(args.reps)
    S = Setup()
    plain, dedup = [], []
    for i in range(2 + args.reps):  # two warm-up rounds: code objects, scratch and table sizes
        tp = S.timed(S.plain)
        S.prepare_dedup()
        td = S.timed(S.dedup)
        S.now += 300_000_000
        if i >= 2:
            plain.append(tp)
            dedup.append(td)
    st = S.qb.dedup_stats()
    print("C5 batch: %d requests, %d keys, ids of %d bytes (%.1f MB)" % (N, KEYS, ID_LEN, N * ID_LEN / 1e6))
    print("dedup state after the last call:", st, " dups in it:", int(S.dd.sum()))
    for name, t in (("mxp_quota_alloc_device      ", plain), ("mxp_quota_alloc_dedup_device", dedup)):
        print("%s ms: min %.3f  range %.3f .. %.3f  (%s)" % (name, min(t), min(t), max(t), " ".join("%.3f" % x for x in t)))
    print("dedup / plain (minima): %.2f" % (min(dedup) / min(plain)))
    del S
    if not args.no_kernels:
        kernel_table(args.out or tempfile.mkdtemp(prefix="quota_dedup_ab_"), 3)


if __name__ == "__main__":
    main()
