"""Measures the exact kNN under a table of bitmaps, one per query (ehx_knn_masked_multi_device) on one MI355X against what a
caller had to do without it: one JSON line per number of masks.

One flat cosine space of --rows x --dims filled by fill_synthetic, --batch device-resident queries spread evenly over
n_masks random bitmaps of --density, k = --k.  Every figure is the median of --steps timed repeats (HIP events around the
whole work of one batch, after --warmup repeats), with min / max.  Per n_masks, in the same run:
  multi     ONE ehx_knn_masked_multi_device call on the batch as it arrives (mask_of interleaved: query i under mask
            i mod n_masks)
  grouped   the baseline: the queries already grouped by mask in device memory (the grouping itself is not timed), n_masks
            ehx_knn_masked_device calls, one per group, back to back
and whether both gave the same ids, with the library's route counters of the multi calls."""
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
from embeddinghub_amd.space import marshal_mask_table  # noqa: E402


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
    out = (C.c_uint64 * 5)()
    raw.ehx_test_masked_counters(sp._h, out)
    return np.array(list(out), dtype=np.int64)   # scan route, exact route, overflowed, scan passes, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--density", type=float, default=0.1)
    ap.add_argument("--masks", type=int, nargs="*", default=[1, 4, 16, 64])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    L = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)   # the test hook is not part of the bound ABI
    sp = ehx.Space.unique("bench-masked-multi", a.dims, metric=ehx.METRIC_COSINE, initial_capacity=a.rows)
    sp.fill_synthetic(ehx.SEED_CORPUS, 0, a.rows, True)
    B, k = a.batch, a.k
    st = torch.cuda.current_stream().cuda_stream
    q = torch.empty((B, a.dims), dtype=torch.float32, device="cuda")
    _lib.check(L.ehx_gen_rows_device(C.c_void_p(st), ehx.SEED_QUERY, 0, B, a.dims, 1, C.c_void_p(q.data_ptr())))
    o_ids = torch.empty((B, k), dtype=torch.int64, device="cuda")
    o_dist = torch.empty((B, k), dtype=torch.float32, device="cuda")
    o_cnt = torch.empty((B,), dtype=torch.int32, device="cuda")
    g_ids, g_dist, g_cnt = torch.empty_like(o_ids), torch.empty_like(o_dist), torch.empty_like(o_cnt)
    rng = np.random.default_rng(1)
    lines = []
    head = {"rows": a.rows, "dims": a.dims, "metric": "cosine", "batch": B, "k": k, "density": a.density, "steps": a.steps,
            "warmup": a.warmup, "engine": sp.scan_engine()}
    for n_masks in a.masks:
        tab = rng.random((n_masks, a.rows)) < a.density
        words, _, n_bits = marshal_mask_table(tab)
        d_masks = torch.tensor(words.view(np.int32), device="cuda")
        of = (np.arange(B) % n_masks).astype(np.int64)
        d_of = torch.tensor(of.astype(np.int32), device="cuda")
        order = torch.tensor(np.argsort(of, kind="stable"), device="cuda")
        qg = q[order].contiguous()                               # the baseline's queries, grouped by mask
        ends = np.concatenate([[0], np.cumsum(np.bincount(of, minlength=n_masks))])
        rec = dict(head, n_masks=n_masks)
        c0 = counters(raw, sp)
        rec["multi"] = timed(lambda: sp.knn_masked_multi_device(q, k, d_masks, n_masks, n_bits, d_of, o_ids, o_dist, o_cnt,
                                                                stream=st), a.warmup, a.steps)
        dc = counters(raw, sp) - c0
        calls = max(int(dc[4]), 1)
        rec["scan_route_queries_per_call"] = round(int(dc[0]) / calls, 3)
        rec["exact_route_queries_per_call"] = round(int(dc[1]) / calls, 3)
        rec["overflowed_queries_per_call"] = round(int(dc[2]) / calls, 3)
        rec["passes_per_call"] = round(int(dc[3]) / calls, 3)

        def grouped():
            for m in range(n_masks):
                b, e = int(ends[m]), int(ends[m + 1])
                sp.knn_masked_device(qg[b:e], k, d_masks[m], n_bits, g_ids[b:e], g_dist[b:e], g_cnt[b:e], stream=st)
        rec["grouped"] = timed(grouped, a.warmup, a.steps)
        rec["grouped_over_multi"] = round(rec["grouped"]["ms_median"] / rec["multi"]["ms_median"], 3)
        rec["same_ids"] = bool(torch.equal(o_ids[order], g_ids))
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    sp.drop()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
