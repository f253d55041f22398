"""Measures the exact kNN under a row bitmap (ehx_knn_masked_device) on one MI355X: one JSON line per bitmap density.

One flat cosine space of --rows x --dims filled by fill_synthetic, --batch device-resident queries, k = --k.  Every figure
is the median of --steps timed batches (HIP events around ONE call each, after --warmup calls), with min / max.  Beside
every random bitmap, in the same run: ehx_knn_masked_device under it (the route it took, the scan passes per call and the
queries that overflowed, from the library's counters), the unfiltered ehx_knn_device of the same space, and
ehx_knn_among_device on the bitmap's list of allowed rows — the exact route without the bitmap's compaction.  The last line
gives the crossover: the density at which the list scan costs what the scan route costs (the list scan's time interpolated
between the densities around it, the scan route's taken from the nearest density it was measured at)."""
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
from embeddinghub_amd.space import marshal_mask  # noqa: E402


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
    out = (C.c_uint64 * 5)()
    C.CDLL(_lib.LIB_PATH).ehx_test_masked_counters(sp._h, out)
    return np.array(list(out), dtype=np.int64)   # scan route, exact route, overflowed, scan passes, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--densities", type=float, nargs="*", default=[1.0, 0.5, 0.1, 0.02, 0.01, 0.005])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    L = _lib.load()
    sp = ehx.Space.unique("bench-masked", a.dims, metric=ehx.METRIC_COSINE, initial_capacity=a.rows)
    sp.fill_synthetic(ehx.SEED_CORPUS, 0, a.rows, True)
    B, k = a.batch, a.k
    st = torch.cuda.current_stream().cuda_stream
    q = torch.empty((B, a.dims), dtype=torch.float32, device="cuda")
    _lib.check(L.ehx_gen_rows_device(C.c_void_p(st), ehx.SEED_QUERY, 0, B, a.dims, 1, C.c_void_p(q.data_ptr())))
    o_ids = torch.empty((B, k), dtype=torch.int64, device="cuda")
    o_dist = torch.empty((B, k), dtype=torch.float32, device="cuda")
    o_cnt = torch.empty((B,), dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(1)
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    head = {"rows": a.rows, "dims": a.dims, "metric": "cosine", "batch": B, "k": k, "steps": a.steps, "warmup": a.warmup,
            "engine": sp.scan_engine()}
    for dens in a.densities:
        allowed = np.ones(a.rows, dtype=bool) if dens >= 1.0 else rng.random(a.rows) < dens
        words, n_bits = marshal_mask(allowed)
        d_mask = torch.tensor(words.view(np.int32), device="cuda")
        d_list = torch.tensor(np.nonzero(allowed)[0].astype(np.int64), device="cuda")
        rec = dict(head, density=dens, n_allowed=int(allowed.sum()))
        c0 = counters(sp)
        rec["knn_masked_device"] = timed(
            lambda: sp.knn_masked_device(q, k, d_mask, n_bits, o_ids, o_dist, o_cnt, stream=st), a.warmup, a.steps)
        dc = counters(sp) - c0
        calls = max(int(dc[4]), 1)
        rec["route"] = "scan" if dc[0] else "exact"
        rec["passes_per_call"] = round(int(dc[3]) / calls, 3)
        rec["overflowed_queries_per_call"] = round(int(dc[2]) / calls, 3)
        rec["exact_route_queries_per_call"] = round(int(dc[1]) / calls, 3)
        masked_ids = o_ids.clone()
        rec["knn_device_unfiltered"] = timed(lambda: sp.knn_device(q, k, o_ids, o_dist, o_cnt, stream=st), a.warmup, a.steps)
        rec["knn_among_device"] = timed(
            lambda: sp.knn_among_device(q, k, d_list, None, o_ids, o_dist, o_cnt, stream=st), a.warmup, a.steps)
        rec["same_ids_as_among"] = bool(torch.equal(masked_ids, o_ids))
        emit(rec)
    # crossover of the two routes
    recs = sorted((json.loads(x) for x in lines), key=lambda r: r["n_allowed"])
    scan = [r for r in recs if r["route"] == "scan"]
    if scan and len(recs) >= 2:
        ref = scan[0]["knn_masked_device"]["ms_median"]   # the scan route at the smallest density it was measured at
        cut = None
        for lo, hi in zip(recs, recs[1:]):
            a_lo, a_hi = lo["knn_among_device"]["ms_median"], hi["knn_among_device"]["ms_median"]
            if a_lo <= ref < a_hi:
                cut = lo["n_allowed"] + (ref - a_lo) / (a_hi - a_lo) * (hi["n_allowed"] - lo["n_allowed"])
        if cut is None:   # outside the measured densities: the list scan's per-row cost extrapolated
            r0 = recs[0] if ref < recs[0]["knn_among_device"]["ms_median"] else recs[-1]
            cut = r0["n_allowed"] * ref / r0["knn_among_device"]["ms_median"]
        emit(dict(head, crossover_n_allowed=int(cut), crossover_density=round(cut / a.rows, 5),
                  scan_route_ms_at=scan[0]["density"], routing_cut_n_allowed=max(1024, a.rows // 128)))
    sp.drop()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
