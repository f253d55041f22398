"""Measures the exact kNN under a label column (ehx_knn_labeled_device) on one MI355X against what a caller had to do without
it: one JSON line per point.

One flat cosine space of --rows x --dims filled by fill_synthetic, --batch device-resident queries, k = --k.  Every figure is
the median of --steps timed repeats (HIP events around the whole work of one batch, after --warmup repeats), with min / max.
Legs (--legs):
  a  L equal-sized labels, L in 1, 4, 16, 64, the queries spread evenly: the labeled call against ONE
     ehx_knn_masked_multi_device call on the table of bitmaps that says the same
  b  L in 256, 1024, 4096 equal labels, the batch naming min(L, batch) of them: against ceil(distinct / 64)
     ehx_knn_masked_multi_device calls (the queries grouped beforehand, not timed) and against ONE ehx_knn_among_device call
     with per-query lists built beforehand (not timed)
  c  one label of S rows (S around the cut between the routes), the rest of the rows on other labels: the batch on that label
     alone, and on 64 such labels, each under the scan route and under the list route (the test hook
     ehx_test_labeled_route) — where the two cross
The ids of the compared calls are checked against each other at every point."""
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
    raw.ehx_test_labeled_counters(sp._h, out)
    return np.array(list(out), dtype=np.int64)   # scan route, list route, overflowed, scan passes, calls


def u32(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32), device="cuda")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--sizes", type=int, nargs="*", default=[2000, 4000, 6000, 7812, 10000, 16000, 32000])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    L = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)   # the test hooks are not part of the bound ABI
    sp = ehx.Space.unique("bench-labeled", a.dims, metric=ehx.METRIC_COSINE, initial_capacity=a.rows)
    sp.fill_synthetic(ehx.SEED_CORPUS, 0, a.rows, True)
    B, k, n = a.batch, a.k, a.rows
    st = torch.cuda.current_stream().cuda_stream
    q = torch.empty((B, a.dims), dtype=torch.float32, device="cuda")
    _lib.check(L.ehx_gen_rows_device(C.c_void_p(st), ehx.SEED_QUERY, 0, B, a.dims, 1, C.c_void_p(q.data_ptr())))
    outs = lambda: (torch.empty((B, k), dtype=torch.int64, device="cuda"),  # noqa: E731
                    torch.empty((B, k), dtype=torch.float32, device="cuda"), torch.empty((B,), dtype=torch.int32, device="cuda"))
    o, g = outs(), outs()
    rng = np.random.default_rng(1)
    head = {"rows": n, "dims": a.dims, "metric": "cosine", "batch": B, "k": k, "steps": a.steps, "warmup": a.warmup,
            "engine": sp.scan_engine(), "exact_cut": max(1024, n // 128)}
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    def labeled(rec, d_col, d_want, name="labeled"):
        c0 = counters(raw, sp)
        rec[name] = timed(lambda: sp.knn_labeled_device(q, k, d_col, n, d_want, o[0], o[1], o[2], stream=st), a.warmup, a.steps)
        dc = counters(raw, sp) - c0
        calls = max(int(dc[4]), 1)
        rec[name].update(scan_route=round(int(dc[0]) / calls, 2), list_route=round(int(dc[1]) / calls, 2),
                         overflowed=round(int(dc[2]) / calls, 2), passes=round(int(dc[3]) / calls, 2))
        return o[0].clone()

    def masked_calls(col, want):
        """the queries grouped by chunks of 64 wanted labels -> (run(), order): ceil(distinct / 64) masked_multi calls"""
        labs = np.unique(want)
        order = np.argsort(want, kind="stable")
        qg = q[torch.tensor(order, device="cuda")].contiguous()
        parts = []
        for c0 in range(0, len(labs), 64):
            chunk = labs[c0:c0 + 64]
            words, n_masks, n_bits = marshal_mask_table(col[None, :] == chunk[:, None])
            at = np.nonzero(np.isin(want[order], chunk))[0]
            parts.append((int(at[0]), int(at[-1]) + 1, torch.tensor(words.view(np.int32), device="cuda"), n_masks, n_bits,
                          u32(np.searchsorted(chunk, want[order][at]))))

        def run():
            for b, e, dm, n_masks, n_bits, dof in parts:
                sp.knn_masked_multi_device(qg[b:e], k, dm, n_masks, n_bits, dof, g[0][b:e], g[1][b:e], g[2][b:e], stream=st)
        return run, torch.tensor(order, device="cuda"), len(parts)

    if "a" in a.legs:
        for n_lab in (1, 4, 16, 64):
            col = rng.integers(0, n_lab, size=n).astype(np.uint32)
            want = (np.arange(B) % n_lab).astype(np.uint32)
            rec = dict(head, leg="a", labels=n_lab, distinct=n_lab)
            ids = labeled(rec, u32(col), u32(want))
            run, order, _ = masked_calls(col, want)
            rec["masked_multi"] = timed(run, a.warmup, a.steps)
            rec["labeled_over_masked_multi"] = round(rec["labeled"]["ms_median"] / rec["masked_multi"]["ms_median"], 3)
            rec["same_ids"] = bool(torch.equal(ids[order], g[0]))
            emit(rec)
    if "b" in a.legs:
        for n_lab in (256, 1024, 4096):
            col = rng.integers(0, n_lab, size=n).astype(np.uint32)
            distinct = min(n_lab, B)
            want = (np.arange(B) % distinct).astype(np.uint32)
            rec = dict(head, leg="b", labels=n_lab, distinct=distinct)
            ids = labeled(rec, u32(col), u32(want))
            run, order, rec["masked_multi_calls"] = masked_calls(col, want)
            rec["masked_multi"] = timed(run, a.warmup, a.steps)
            rec["same_ids_masked_multi"] = bool(torch.equal(ids[order], g[0]))
            by_label = np.argsort(col, kind="stable")   # per label its ascending rows
            ends = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n_lab))])
            lists = [by_label[ends[w]:ends[w + 1]] for w in want]
            d_cand = torch.tensor(np.concatenate(lists).astype(np.int64), device="cuda")
            d_off = torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64), device="cuda")
            longest = max(len(x) for x in lists)
            rec["among"] = timed(lambda: sp.knn_among_device(q, k, d_cand, d_off, g[0], g[1], g[2], max_list_hint=longest,
                                                             stream=st), a.warmup, a.steps)
            rec["among_list_bytes"] = int(d_cand.numel() * 8)
            rec["same_ids_among"] = bool(torch.equal(ids, g[0]))
            rec["labeled_over_masked_multi"] = round(rec["labeled"]["ms_median"] / rec["masked_multi"]["ms_median"], 3)
            rec["labeled_over_among"] = round(rec["labeled"]["ms_median"] / rec["among"]["ms_median"], 3)
            emit(rec)
    if "c" in a.legs:
        for size in a.sizes:
            for n_on in (1, 64):
                if size * n_on > n:
                    continue
                col = np.full(n, 0x7FFFFFFF, dtype=np.uint32)
                col[rng.permutation(n)[:size * n_on]] = np.repeat(np.arange(n_on, dtype=np.uint32), size)
                d_col, d_want = u32(col), u32(np.arange(B) % n_on)
                rec = dict(head, leg="c", label_rows=size, labels_named=n_on)
                raw.ehx_test_labeled_route(sp._h, 1)
                scan_ids = labeled(rec, d_col, d_want, "scan_route")
                raw.ehx_test_labeled_route(sp._h, 2)
                list_ids = labeled(rec, d_col, d_want, "list_route")
                raw.ehx_test_labeled_route(sp._h, 0)
                rec["scan_over_list"] = round(rec["scan_route"]["ms_median"] / rec["list_route"]["ms_median"], 3)
                rec["same_ids"] = bool(torch.equal(scan_ids, list_ids))
                emit(rec)
    sp.drop()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
