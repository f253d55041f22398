"""Measures the clustering calls (ehx_assign_device, ehx_centroid_sums_device, ehx_kmeans_device) on one MI355X: one JSON
line per (shape, C).  NOT RUN YET: every figure the README or DESIGN §e.33 would quote has to come from this script.

Shapes: 1 M x 768 cosine and 6.25 M x 128 L2^2, C = 256 / 1024 / 4096 centroids (rows of the space, jittered).  Per line:
  assign_device   ONE call with distances; certified / handed_on: the filter's and the exact kernel's rows (test hook);
                  filter_share_of_fp32_peak: 2 * rows * C * dims flops over the call's time against 157.3 TFLOP/s — a lower
                  bound of the filter kernel's own share, the call also prepares the centroids and walks the handed-on rows;
  centroid_sums   the sums over the labels of that call;
  lloyd_step      kmeans_device with iters = 1 (two assignments, the sums, the divide);
  knn_route       the route the library had before, on --route-rows rows only and scaled: get_by_ids_device of 1024 rows +
                  knn_device at k = 1 on a second space that holds the centroids;
  torch_cdist     torch.cdist + argmin over the same rows in chunks (inexact; for scale only), L2^2 only.
Device figures are the median of --steps timed calls after --warmup calls, with min / max."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import embeddinghub_amd as ehx  # noqa: E402
from embeddinghub_amd import _lib  # noqa: E402

FP32_MATRIX_PEAK = 157.3e12
SHAPES = {"1Mx768-cosine": (1000000, 768, ehx.METRIC_COSINE), "6.25Mx128-l2": (6250000, 128, ehx.METRIC_L2SQ)}


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


def counts(sp):
    out = (C.c_uint64 * 2)()
    assert C.CDLL(_lib.LIB_PATH).ehx_test_assign_counts(sp._h, out) == 0
    return list(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--centroids", type=int, nargs="*", default=[256, 1024, 4096])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--route-rows", type=int, default=65536)
    ap.add_argument("--out", default="profiles/assign_bench.jsonl")
    a = ap.parse_args()
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(20263)
    for name in a.shapes:
        rows, d, metric = SHAPES[name]
        sp = ehx.Space.unique("bench-assign", d, metric=metric, initial_capacity=rows)
        for r0 in range(0, rows, 65536):
            n = min(65536, rows - r0)
            sp.set_batch_device([str(i) for i in range(r0, r0 + n)], torch.randn((n, d), generator=gen, device="cuda"))
        label = torch.empty((rows,), dtype=torch.int32, device="cuda")
        dist = torch.empty((rows,), dtype=torch.float32, device="cuda")
        for n_cent in a.centroids:
            ids = torch.randperm(rows, generator=gen, device="cuda")[:n_cent].to(torch.int64)
            cent = torch.empty((n_cent, d), dtype=torch.float32, device="cuda")
            sp.get_by_ids_device(ids, cent, torch.empty((n_cent,), dtype=torch.int32, device="cuda"), stream=st)
            cent += 0.05 * torch.randn((n_cent, d), generator=gen, device="cuda")
            rec = {"shape": name, "rows": rows, "dims": d, "centroids": n_cent, "steps": a.steps, "warmup": a.warmup}
            before = counts(sp)
            rec["assign_device"] = timed(lambda: sp.assign_device(cent, label, dist, stream=st), a.warmup, a.steps)
            after = counts(sp)
            calls = a.warmup + a.steps
            rec["certified"], rec["handed_on"] = (after[0] - before[0]) // calls, (after[1] - before[1]) // calls
            rec["filter_share_of_fp32_peak"] = round(2.0 * rows * n_cent * d / (rec["assign_device"]["ms_median"] * 1e-3) / FP32_MATRIX_PEAK, 4)
            sums = torch.empty((n_cent, d), dtype=torch.float32, device="cuda")
            cnt = torch.empty((n_cent,), dtype=torch.int32, device="cuda")
            rec["centroid_sums"] = timed(lambda: sp.centroid_sums_device(label, n_cent, sums, cnt, stream=st), a.warmup, a.steps)
            step_cent = cent.clone()
            rec["lloyd_step"] = timed(lambda: sp.kmeans_device(step_cent, 1, label, stream=st), a.warmup, a.steps)
            # the route available before: a centroid space searched at k = 1, 1024 rows per batch
            cs = ehx.Space.unique("bench-assign-cent", d, metric=metric, initial_capacity=n_cent)
            cs.set_batch_device([str(i) for i in range(n_cent)], cent)
            q = torch.empty((1024, d), dtype=torch.float32, device="cuda")
            o = (torch.empty((1024, 1), dtype=torch.int64, device="cuda"), torch.empty((1024, 1), dtype=torch.float32, device="cuda"),
                 torch.empty((1024,), dtype=torch.int32, device="cuda"))
            v = torch.empty((1024,), dtype=torch.int32, device="cuda")

            def route():
                for r0 in range(0, a.route_rows, 1024):
                    sp.get_by_ids_device(torch.arange(r0, r0 + 1024, device="cuda"), q, v, stream=st)
                    cs.knn_device(q, 1, *o, stream=st)
            rec["knn_route"] = timed(route, 1, max(3, a.steps // 3))
            rec["knn_route"]["rows"] = a.route_rows
            rec["knn_route"]["ms_scaled_to_all_rows"] = round(rec["knn_route"]["ms_median"] * rows / a.route_rows, 2)
            cs.drop()
            if metric == ehx.METRIC_L2SQ:
                def cdist():
                    for r0 in range(0, a.route_rows, 1024):
                        sp.get_by_ids_device(torch.arange(r0, r0 + 1024, device="cuda"), q, v, stream=st)
                        torch.cdist(q, cent).argmin(dim=1)
                rec["torch_cdist"] = timed(cdist, 1, max(3, a.steps // 3))
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
        sp.drop()


if __name__ == "__main__":
    main()
