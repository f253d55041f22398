"""Measures the exact kNN among lists of row ids (ehx_knn_among_device) on one MI355X: prints one JSON line.

One flat cosine space of --rows x --dims filled by fill_synthetic, --batch device-resident queries, k = --k.  Every
figure is the median of --steps timed batches (HIP events around ONE call each, after --warmup calls), with min / max.
  (a) per-query lists of --list-len random ids: ms per batch, bytes gathered / time as a fraction of 8 TB/s
  (b) ONE shared list of 4 Ki .. 256 Ki ids: ms per batch, beside the unfiltered ehx_knn_device of the same space in the
      same run; cutoff = the list length (linear interpolation between the two sizes around it) at which the shared-list
      scan costs what scanning everything costs
  (c) the query tiling A/B: the 64 Ki list again as `batch` per-query copies of it, which takes the one-query-per-workgroup
      kernel — every (query, row) pair then makes its own trip through the memory system.  NOT the tile kernel with a
      tile of 1: another kernel, another lane mapping; the ratio mixes tiling with the difference between the two
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--list-len", type=int, default=1024)
    ap.add_argument("--shared", type=int, nargs="*", default=[4096, 16384, 65536, 262144])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    L = _lib.load()
    sp = ehx.Space.unique("bench-among", a.dims, metric=ehx.METRIC_COSINE, initial_capacity=a.rows)
    sp.fill_synthetic(ehx.SEED_CORPUS, 0, a.rows, True)
    B, k = a.batch, a.k
    st = torch.cuda.current_stream().cuda_stream
    q = torch.empty((B, a.dims), dtype=torch.float32, device="cuda")
    _lib.check(L.ehx_gen_rows_device(C.c_void_p(st), ehx.SEED_QUERY, 0, B, a.dims, 1, C.c_void_p(q.data_ptr())))
    o_ids = torch.empty((B, k), dtype=torch.int64, device="cuda")
    o_dist = torch.empty((B, k), dtype=torch.float32, device="cuda")
    o_cnt = torch.empty((B,), dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(1)
    esz = 4
    out = {"rows": a.rows, "dims": a.dims, "batch": B, "k": k, "steps": a.steps}

    full = timed(lambda: sp.knn_device(q, k, o_ids, o_dist, o_cnt, stream=st), a.warmup, a.steps)
    out["unfiltered_knn_device"] = full

    ids = torch.tensor(rng.integers(0, a.rows, size=B * a.list_len, dtype=np.int64), device="cuda")
    off = torch.arange(0, (B + 1) * a.list_len, a.list_len, dtype=torch.int64, device="cuda")
    r = timed(lambda: sp.knn_among_device(q, k, ids, off, o_ids, o_dist, o_cnt, max_list_hint=a.list_len, stream=st),
              a.warmup, a.steps)
    gathered = B * a.list_len * a.dims * esz
    r["list_len"] = a.list_len
    r["gathered_tb_per_s"] = round(gathered / (r["ms_median"] * 1e-3) / 1e12, 3)
    r["fraction_of_8_tb_per_s"] = round(r["gathered_tb_per_s"] / 8.0, 3)
    out["per_query_lists"] = r

    shared = []
    for n_l in a.shared:
        ids_s = torch.tensor(rng.choice(a.rows, size=min(n_l, a.rows), replace=False).astype(np.int64), device="cuda")
        r = timed(lambda: sp.knn_among_device(q, k, ids_s, None, o_ids, o_dist, o_cnt, stream=st), a.warmup, a.steps)
        r["list_len"] = int(ids_s.shape[0])
        r["pairs_per_s"] = round(B * r["list_len"] / (r["ms_median"] * 1e-3), 0)
        shared.append(r)
    out["shared_list"] = shared
    cut = None
    for lo, hi in zip(shared, shared[1:]):
        if lo["ms_median"] <= full["ms_median"] < hi["ms_median"]:
            t = (full["ms_median"] - lo["ms_median"]) / (hi["ms_median"] - lo["ms_median"])
            cut = lo["list_len"] + t * (hi["list_len"] - lo["list_len"])
    if cut is None and shared:   # outside the measured sizes: the first or last size, per-row cost extrapolated
        ref = shared[0] if full["ms_median"] < shared[0]["ms_median"] else shared[-1]
        cut = ref["list_len"] * full["ms_median"] / ref["ms_median"]
    if cut is not None:
        out["cutoff_list_len"] = int(cut)
        out["cutoff_selectivity"] = round(cut / a.rows, 5)

    n_ab = 65536 if 65536 in a.shared or not a.shared else a.shared[-1]
    base = rng.choice(a.rows, size=min(n_ab, a.rows), replace=False).astype(np.int64)
    ids_r = torch.tensor(base, device="cuda").repeat(B)
    off_r = torch.arange(0, (B + 1) * len(base), len(base), dtype=torch.int64, device="cuda")
    r = timed(lambda: sp.knn_among_device(q, k, ids_r, off_r, o_ids, o_dist, o_cnt, max_list_hint=len(base), stream=st),
              max(1, a.warmup // 2), max(3, a.steps // 4))
    r["list_len"] = len(base)
    out["query_tile_1"] = r
    tiled = [s for s in shared if s["list_len"] == len(base)]
    if tiled:
        out["query_tile_8_over_1"] = round(tiled[0]["ms_median"] / r["ms_median"], 3)
    sp.drop()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
