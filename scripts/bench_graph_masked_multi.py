"""Measures the graph walk under a table of bitmaps, one per query (ehx_graph_knn_masked_multi_device) on one MI355X: one JSON
line per table size.

The GPU-built 1 M x 128 L2 graph space over EHX-MANIFOLD-1 rows (ehx_fill_manifold, 16 latent dimensions) of
scripts/bench_graph_masked.py; --batch device-resident queries from the same generator under the query seed, k = --k,
ef = --ef.  Per n_masks in --masks: that many random bitmaps of density 0.5, device-resident, mask_of interleaved
(query i under bitmap i % n_masks).  In the same run:
  table           ONE ehx_graph_knn_masked_multi_device call, EHX_WALK_GRAPH: ms per call, queries/s
  grouped         what a caller could do before: n_masks ehx_graph_knn_masked_device calls, one per bitmap, over the queries
                  of that bitmap gathered beforehand (the gathering and the scatter back are NOT timed)
  exact_table     the other thing a caller could do: ONE ehx_knn_masked_multi_device call on the same space (exact)
The ids and counts of `table` are asserted equal to the grouped calls'.  A last line adds a MIXED table (bitmaps of density
0.5 and 1 / 50 alternating) under EHX_WALK_AUTO, with the library's split of the batch into walked and exact queries.
Every time is the median of --steps timed calls (HIP events around the call, or around the group of calls, after --warmup
of them), with min / max."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import embeddinghub_amd as ehx  # noqa: E402
from embeddinghub_amd import _lib  # noqa: E402
from embeddinghub_amd.space import marshal_mask_table  # noqa: E402

ROWS, DIMS, LATENT = 1_000_000, 128, 16


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


def counters(sp):
    out = (C.c_uint64 * 4)()
    C.CDLL(_lib.LIB_PATH).ehx_test_graph_masked_counters(sp._h, out)
    return np.array(list(out), dtype=np.int64)   # walked, exact, calls, walked queries at cap


def results(B, k):
    return (torch.empty((B, k), dtype=torch.int64, device="cuda"), torch.empty((B, k), dtype=torch.float32, device="cuda"),
            torch.empty((B,), dtype=torch.int32, device="cuda"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--ef", type=int, default=60)
    ap.add_argument("--masks", type=int, nargs="*", default=[1, 4, 16, 64])
    ap.add_argument("--mixed-masks", type=int, default=16, help="bitmaps of the mixed table (0: skip it)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    L = _lib.load()
    B, k, n, d = a.batch, a.k, ROWS, DIMS
    st = torch.cuda.current_stream().cuda_stream
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    sp = ehx.Space.unique("bench-gmm", d, metric=ehx.METRIC_L2SQ, mode=ehx.MODE_GRAPH, initial_capacity=n, build_batch=4096,
                          ef=a.ef)
    t0 = time.perf_counter()
    sp.fill_manifold(ehx.SEED_CORPUS, 0, n, LATENT, False)
    build_s = time.perf_counter() - t0
    q = torch.empty((B, d), dtype=torch.float32, device="cuda")
    _lib.check(L.ehx_gen_manifold_rows_device(C.c_void_p(st), ehx.SEED_QUERY, 0, B, d, LATENT, 0, C.c_void_p(q.data_ptr())))
    torch.cuda.synchronize()
    head = {"index": "l2_1m128", "rows": n, "dims": d, "metric": "l2", "batch": B, "k": k, "ef": a.ef, "steps": a.steps,
            "warmup": a.warmup, "build_s": round(build_s, 1), "walk_list_factor": _lib.WALK_LIST_FACTOR}
    rng = np.random.default_rng(1)

    def table(densities):
        words, n_masks, n_bits = marshal_mask_table(np.stack([rng.random(n) < p for p in densities]))
        mask_of = (np.arange(B) % n_masks).astype(np.uint32)
        return (torch.tensor(words.view(np.int32), device="cuda"), n_masks, n_bits, mask_of,
                torch.tensor(mask_of.view(np.int32), device="cuda"))

    for n_masks in a.masks:
        d_masks, n_masks, n_bits, mask_of, d_of = table([0.5] * n_masks)
        rec = dict(head, n_masks=n_masks, density=0.5)
        out = results(B, k)
        t = timed(lambda: sp.graph_knn_masked_multi_device(q, k, d_masks, n_masks, n_bits, d_of, *out, route=ehx.WALK_GRAPH,
                                                           stream=st), a.warmup, a.steps)
        rec["table"] = dict(t, qps=round(B / t["ms_median"] * 1e3))
        # the grouped calls: the queries of every bitmap gathered beforehand
        groups = []
        for m in range(n_masks):
            rows = torch.tensor(np.flatnonzero(mask_of == m), device="cuda")
            groups.append((rows, q[rows].contiguous(), d_masks[m], results(len(rows), k)))

        def grouped():
            for rows, gq, gmask, o in groups:
                sp.graph_knn_masked_device(gq, k, gmask, n_bits, *o, route=ehx.WALK_GRAPH, stream=st)

        t = timed(grouped, a.warmup, a.steps)
        rec["grouped"] = dict(t, qps=round(B / t["ms_median"] * 1e3), calls=n_masks)
        torch.cuda.synchronize()
        for rows, gq, gmask, o in groups:
            assert torch.equal(out[0][rows], o[0]) and torch.equal(out[2][rows], o[2]), "the table's ids are the grouped calls'"
        rec["ids_equal_grouped"] = True
        xout = results(B, k)
        t = timed(lambda: sp.knn_masked_multi_device(q, k, d_masks, n_masks, n_bits, d_of, *xout, stream=st), a.warmup, a.steps)
        rec["exact_table"] = dict(t, qps=round(B / t["ms_median"] * 1e3))
        emit(rec)
    if a.mixed_masks:
        d_masks, n_masks, n_bits, mask_of, d_of = table([0.5 if m % 2 == 0 else 1.0 / 50 for m in range(a.mixed_masks)])
        out = results(B, k)
        c0 = counters(sp)
        sp.graph_knn_masked_multi_device(q, k, d_masks, n_masks, n_bits, d_of, *out, stream=st)
        torch.cuda.synchronize()
        dc = counters(sp) - c0
        t = timed(lambda: sp.graph_knn_masked_multi_device(q, k, d_masks, n_masks, n_bits, d_of, *out, stream=st),
                  a.warmup, a.steps)
        emit(dict(head, n_masks=n_masks, density="0.5 | 1/50", route="auto", walked=int(dc[0]), exact=int(dc[1]),
                  mixed=dict(t, qps=round(B / t["ms_median"] * 1e3))))
    sp.drop()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
