"""Lengths of the deferred-pair wave lists (kargs.dtp_n) of one evaluation, downloaded once after it
(DeviceBatch.dtp_lists): p50 / p90 / p99 / max per wave list and per tile of 16 lists, with the fill
chunk counts.  usage: dtp_list_lengths.py [c2|c4|c4p] [rules] [requests]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from istio_amd import workloads as W  # noqa: E402
from istio_amd.engine import Engine  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "c2"
n_rules = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
n_req = int(sys.argv[3]) if len(sys.argv) > 3 else 1 << 20
if wl == "c4":
    manifest, rules, batch = W.c4_workload(n_rules=n_rules, n_requests=n_req, seed=4)
elif wl == "c4p":
    manifest, rules, batch = W.c4_workload(n_rules=n_rules, n_requests=n_req, seed=4, paths_only=True)
else:
    manifest, rules, batch = W.c2_workload(n_rules=n_rules, n_requests=n_req, seed=2)
eng = Engine(0)
eng.set_vocabulary(manifest)
eng.compile(rules)
db = eng.upload(batch)
Wd = (len(rules) + 31) // 32
dm = torch.zeros((Wd, batch.n), dtype=torch.int32, device="cuda:0")
de = torch.zeros_like(dm)
hits = torch.zeros(len(rules), dtype=torch.int64, device="cuda:0")
db.eval_hits(dm.data_ptr(), de.data_ptr(), hits.data_ptr(), 0)
torch.cuda.synchronize()
shape, wave = db.dtp_lists()
wave = wave.astype(np.int64)
tile = np.concatenate([wave, np.zeros((-len(wave)) % 16, dtype=np.int64)]).reshape(-1, 16).sum(axis=1)
print("%s %d rules x %d requests: %d waves, %d plain + %d value-class fill chunks, list capacity %d" % (
    wl, len(rules), batch.n, shape["waves"], shape["fills"], shape["vtfills"], shape["cap"]))
print("%d list entries (%.3f per request), %d lists at the capacity; hit counters sum to %d" % (
    int(wave.sum()), wave.sum() / batch.n, int((wave == shape["cap"]).sum()), int(hits.sum().item())))
for name, v in (("wave list (dtp_n)", wave), ("tile of 16 lists", tile)):
    print("%-18s p50 %d  p90 %d  p99 %d  max %d  mean %.1f  empty %.2f%%" % (
        name, np.percentile(v, 50), np.percentile(v, 90), np.percentile(v, 99), v.max(), v.mean(), 100.0 * (v == 0).mean()))
db.free()
