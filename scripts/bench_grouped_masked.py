"""Measures the grouped kNN under row bitmaps (ehx_knn_grouped_masked_device) on one MI355X: one JSON line per (number of
bitmaps, density, labeling, per_group).

One flat cosine space of --rows x --dims filled by fill_synthetic, --batch device-resident queries, k = --k, the labels and
the bitmaps resident on the device, query i under bitmap i % n_masks.  Bitmaps: every row allowed with probability
--densities, one seeded draw per bitmap.  Two labelings: clustered (row // 8: the chunks of a document stored side by side)
and scattered (a multiplicative hash of the row id into rows / 8 labels).  Every figure is the median of --steps timed
batches (HIP events around ONE call each, after --warmup calls), with min / max.  Beside every call, in the same run:
  (a) knn_grouped_device, unfiltered, on the same space: the floor — the filtered call adds the compaction and the per-bitmap
      fixed work;
  (b) what the call replaces: knn_masked_multi_device at --overfetch (48, the largest k its scan route serves) de-duplicated
      on the host to per_group rows per label and cut at k — and how often that answer is wrong or too short;
and the library's counters: the queries on the scan route, the share on the list route, overflows, passes."""
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


def counters(sp):
    out = (C.c_uint64 * 5)()
    C.CDLL(_lib.LIB_PATH).ehx_test_grouped_masked_counters(sp._h, out)
    return np.array(list(out), dtype=np.int64)   # scan route, list route, overflowed, scan passes, calls


def dedup(ids, cnt, labels, k, m):
    """the host-side de-duplication of an over-fetched list: at most m rows per label, the first k"""
    out = []
    for i in range(len(cnt)):
        seen, row = {}, []
        for r in ids[i, :int(cnt[i])]:
            g = int(labels[int(r)])
            if g != _lib.GROUP_NONE:
                if seen.get(g, 0) >= m:
                    continue
                seen[g] = seen.get(g, 0) + 1
            row.append(int(r))
            if len(row) == k:
                break
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--overfetch", type=int, default=48)
    ap.add_argument("--per-group", type=int, nargs="*", default=[1, 3])
    ap.add_argument("--masks", type=int, nargs="*", default=[1, 16, 64])
    ap.add_argument("--densities", type=float, nargs="*", default=[0.5, 0.1, 0.001])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    L = _lib.load()
    sp = ehx.Space.unique("bench-grouped-masked", a.dims, metric=ehx.METRIC_COSINE, initial_capacity=a.rows)
    sp.fill_synthetic(ehx.SEED_CORPUS, 0, a.rows, True)
    B, k, kf = a.batch, a.k, a.overfetch
    st = torch.cuda.current_stream().cuda_stream
    q = torch.empty((B, a.dims), dtype=torch.float32, device="cuda")
    _lib.check(L.ehx_gen_rows_device(C.c_void_p(st), ehx.SEED_QUERY, 0, B, a.dims, 1, C.c_void_p(q.data_ptr())))

    def outputs(width):
        return (torch.empty((B, width), dtype=torch.int64, device="cuda"), torch.empty((B, width), dtype=torch.float32, device="cuda"),
                torch.empty((B,), dtype=torch.int32, device="cuda"))

    o, of = outputs(k), outputs(kf)
    rows = np.arange(a.rows, dtype=np.uint64)
    n_hash = max(a.rows // 8, 1)
    labelings = {"clustered": (rows // np.uint64(8)).astype(np.uint32),
                 "scattered": ((rows * np.uint64(2654435761)) % np.uint64(n_hash)).astype(np.uint32)}
    d_labels = {name: torch.tensor(lb.view(np.int32), device="cuda") for name, lb in labelings.items()}
    lines = []
    head = {"rows": a.rows, "dims": a.dims, "metric": "cosine", "batch": B, "k": k, "overfetch": kf, "steps": a.steps,
            "warmup": a.warmup, "engine": sp.scan_engine(), "device": torch.cuda.get_device_name(0)}
    floor = {(name, m): timed(lambda: sp.knn_grouped_device(q, k, d_labels[name], a.rows, *o, per_group=m, stream=st),
                              a.warmup, a.steps) for name in labelings for m in a.per_group}
    for n_masks in a.masks:
        mask_of = (np.arange(B) % n_masks).astype(np.uint32)
        d_of = torch.tensor(mask_of.view(np.int32), device="cuda")
        for density in a.densities:
            rng = np.random.default_rng(1000 * n_masks + int(density * 1e6))
            allows = np.stack([rng.random(a.rows) < density for _ in range(n_masks)])
            words, _, n_bits = marshal_mask_table(allows)
            d_masks = torch.tensor(words.view(np.int32), device="cuda")
            over = timed(lambda: sp.knn_masked_multi_device(q, kf, d_masks, n_masks, n_bits, d_of, *of, stream=st), a.warmup, a.steps)
            torch.cuda.synchronize()
            f_ids, f_cnt = of[0].cpu().numpy().view(np.uint64), of[2].cpu().numpy().view(np.uint32)
            for name, labels in labelings.items():
                for m in a.per_group:
                    rec = dict(head, n_masks=n_masks, density=density, allowed_min=int(allows.sum(axis=1).min()), labeling=name,
                               per_group=m)
                    c0 = counters(sp)
                    rec["knn_grouped_masked_device"] = timed(
                        lambda: sp.knn_grouped_masked_device(q, k, d_labels[name], a.rows, d_masks, n_masks, n_bits, d_of, *o,
                                                             per_group=m, stream=st), a.warmup, a.steps)
                    dc = counters(sp) - c0
                    calls = max(int(dc[4]), 1)
                    rec["scan_route_queries_per_call"] = round(int(dc[0]) / calls, 3)
                    rec["list_route_share"] = round(int(dc[1]) / (calls * B), 5)
                    rec["overflowed_queries_per_call"] = round(int(dc[2]) / calls, 3)
                    rec["passes_per_call"] = round(int(dc[3]) / calls, 3)
                    rec["knn_grouped_device_unfiltered"] = floor[(name, m)]
                    rec["knn_masked_multi_device_overfetch"] = over
                    torch.cuda.synchronize()
                    g_ids, g_cnt = o[0].cpu().numpy().view(np.uint64), o[2].cpu().numpy().view(np.uint32)
                    guess = dedup(f_ids, f_cnt, labels, k, m)
                    truth = [[int(v) for v in g_ids[i, :int(g_cnt[i])]] for i in range(B)]
                    rec["overfetch_wrong_share"] = round(sum(guess[i] != truth[i] for i in range(B)) / B, 5)
                    rec["overfetch_short_share"] = round(sum(len(guess[i]) < len(truth[i]) for i in range(B)) / B, 5)
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
