"""Measures the exact range search (ehx_range_device) on one MI355X: prints one JSON line per workload.

Workloads: 1 M x 768 cosine and 6.25 M x 128 L2 (--workloads rows:dims:metric ...), filled by fill_synthetic, --batch
device-resident queries.  Every figure is the median of --steps timed batches (HIP events around ONE call each, after
--warmup calls), with min / max.  Per workload:
  * ehx_knn_device (k = 10) of the same space in the same run, for comparison;
  * ehx_range_device at radii that admit about 10, 100 and 1000 rows per query — ONE radius per target for the whole batch,
    the median of the exact 10th / 100th / 1000th distance of the first 32 queries — with the members per query it found
    (mean, max) and the share of queries that left the int8 path for the exact one (the counters hook of the library).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import embeddinghub_amd as ehx  # noqa: E402
from embeddinghub_amd import _lib  # noqa: E402

METRICS = {"cosine": ehx.METRIC_COSINE, "l2": ehx.METRIC_L2SQ, "ip": ehx.METRIC_IP}


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def counters(raw, sp):
    out = (C.c_uint64 * 4)()
    raw.ehx_test_range_counters(sp._h, out)
    return list(out)


def run(rows, dims, metric, a):
    L = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    sp = ehx.Space.unique("bench-range", dims, metric=METRICS[metric], initial_capacity=rows)
    sp.fill_synthetic(ehx.SEED_CORPUS, 0, rows, metric == "cosine")
    B = a.batch
    st = torch.cuda.current_stream().cuda_stream
    q = torch.empty((B, dims), dtype=torch.float32, device="cuda")
    _lib.check(L.ehx_gen_rows_device(C.c_void_p(st), ehx.SEED_QUERY, 0, B, dims, 1, C.c_void_p(q.data_ptr())))
    out = {"rows": rows, "dims": dims, "metric": metric, "batch": B, "steps": a.steps, "engine": sp.scan_engine()}
    k_ids = torch.empty((B, 10), dtype=torch.int64, device="cuda")
    k_dist = torch.empty((B, 10), dtype=torch.float32, device="cuda")
    k_cnt = torch.empty((B,), dtype=torch.int32, device="cuda")
    out["knn_device_k10"] = timed(lambda: sp.knn_device(q, 10, k_ids, k_dist, k_cnt, stream=st), a.warmup, a.steps)
    # radii from the exact 1000 nearest of a few queries
    ns = min(32, B)
    s_ids = torch.empty((ns, 1000), dtype=torch.int64, device="cuda")
    s_dist = torch.empty((ns, 1000), dtype=torch.float32, device="cuda")
    s_cnt = torch.empty((ns,), dtype=torch.int32, device="cuda")
    sp.knn_device(q[:ns].contiguous(), 1000, s_ids, s_dist, s_cnt, stream=st)
    torch.cuda.synchronize()
    sd = s_dist.cpu().numpy()
    mr = a.max_results
    o_ids = torch.empty((B, mr), dtype=torch.int64, device="cuda")
    o_dist = torch.empty((B, mr), dtype=torch.float32, device="cuda")
    o_cnt = torch.empty((B,), dtype=torch.int32, device="cuda")
    o_tot = torch.empty((B,), dtype=torch.int64, device="cuda")
    out["range_device"] = []
    for target in (10, 100, 1000):
        radius = float(np.median(sd[:, target - 1]))
        rad = torch.full((B,), radius, dtype=torch.float32, device="cuda")
        c0 = counters(raw, sp)
        r = timed(lambda: sp.range_device(q, rad, mr, o_ids, o_dist, o_cnt, o_tot, stream=st), a.warmup, a.steps)
        c1 = counters(raw, sp)
        tot = o_tot.cpu().numpy()
        calls = a.warmup + a.steps
        r.update({"target_members": target, "radius": radius, "max_results": mr, "members_mean": round(float(tot.mean()), 1),
                  "members_max": int(tot.max()),
                  "exact_path_share": round((c1[1] - c0[1]) / float(B * calls), 5),
                  "pool_overflow_share": round((c1[2] - c0[2]) / float(B * calls), 5),
                  "over_knn_k10": round(r["ms_median"] / out["knn_device_k10"]["ms_median"], 3)})
        out["range_device"].append(r)
    sp.drop()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="*", default=["1000000:768:cosine", "6250000:128:l2"])
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--max-results", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    for w in a.workloads:
        rows, dims, metric = w.split(":")
        run(int(rows), int(dims), metric, a)


if __name__ == "__main__":
    main()
