"""Measures the grouped kNN under a label column (ehx_knn_grouped_labeled_device) on one MI355X: one JSON line per (leg,
number of tenants, per_group).

One flat cosine space of --rows x --dims filled by fill_synthetic, --batch device-resident queries, k = --k, both columns
resident on the device.  Groups: clustered (row // 8: the chunks of a document stored side by side).  Tenants: L equal ones,
a multiplicative hash of the document (row // 8) modulo L — a document's chunks belong to one tenant, and every tenant is
spread over the id space; query i wants tenant i % L, so a batch names min(L, batch) tenants.  Every figure is the median
of --steps timed calls (HIP events around the WHOLE call — for a comparison made of several calls, around all of them —
after --warmup calls), with min / max.
  leg a  L = --few (1, 16, 64): against knn_grouped_masked_device on the table of L bitmaps that says the same;
  leg b  L = --many (256, 1024, 4096): against (1) the ceil(distinct / 64) knn_grouped_masked_device calls a caller needs
         to say the same, each on the queries of its 64 tenants, tables resident; and (2) knn_labeled_device at --overfetch
         (48) de-duplicated on the host to per_group rows per group and cut at k — with how many of its answers differ from
         the exact one (the host's de-duplication is not timed).
The library's counters say which route each leg took: queries on the scan route, the share on the list route, overflows,
passes.  Every answer timed is compared with knn_grouped_masked_device's."""
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
    C.CDLL(_lib.LIB_PATH).ehx_test_grouped_labeled_counters(sp._h, out)
    return np.array(list(out), dtype=np.int64)   # scan route, list route, overflowed, scan passes, calls


def dedup(ids, cnt, groups, k, m):
    """the host-side de-duplication of an over-fetched list: at most m rows per group, the first k"""
    out = []
    for i in range(len(cnt)):
        seen, row = {}, []
        for r in ids[i, :int(cnt[i])]:
            g = int(groups[int(r)])
            if g != _lib.GROUP_NONE:
                if seen.get(g, 0) >= m:
                    continue
                seen[g] = seen.get(g, 0) + 1
            row.append(int(r))
            if len(row) == k:
                break
        out.append(row)
    return out


def lists(o):
    ids, cnt = o[0].cpu().numpy().view(np.uint64), o[2].cpu().numpy().view(np.uint32)
    return [[int(v) for v in ids[i, :int(cnt[i])]] for i in range(len(cnt))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--overfetch", type=int, default=48)
    ap.add_argument("--per-group", type=int, nargs="*", default=[1, 3])
    ap.add_argument("--few", type=int, nargs="*", default=[1, 16, 64])
    ap.add_argument("--many", type=int, nargs="*", default=[256, 1024, 4096])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    L = _lib.load()
    sp = ehx.Space.unique("bench-grouped-labeled", a.dims, metric=ehx.METRIC_COSINE, initial_capacity=a.rows)
    sp.fill_synthetic(ehx.SEED_CORPUS, 0, a.rows, True)
    B, k, kf = a.batch, a.k, a.overfetch
    st = torch.cuda.current_stream().cuda_stream
    q = torch.empty((B, a.dims), dtype=torch.float32, device="cuda")
    _lib.check(L.ehx_gen_rows_device(C.c_void_p(st), ehx.SEED_QUERY, 0, B, a.dims, 1, C.c_void_p(q.data_ptr())))

    def outputs(n, width):
        return (torch.empty((n, width), dtype=torch.int64, device="cuda"), torch.empty((n, width), dtype=torch.float32, device="cuda"),
                torch.empty((n,), dtype=torch.int32, device="cuda"))

    o, of = outputs(B, k), outputs(B, kf)
    rows = np.arange(a.rows, dtype=np.uint64)
    groups = (rows // np.uint64(8)).astype(np.uint32)
    d_groups = torch.tensor(groups.view(np.int32), device="cuda")
    head = {"rows": a.rows, "dims": a.dims, "metric": "cosine", "batch": B, "k": k, "overfetch": kf, "steps": a.steps,
            "warmup": a.warmup, "engine": sp.scan_engine(), "device": torch.cuda.get_device_name(0), "grouping": "clustered",
            "cut_rows": max(1024, a.rows // 128)}
    lines = []
    for leg, n_tenants in [("a", t) for t in a.few] + [("b", t) for t in a.many]:
        col = (((rows // np.uint64(8)) * np.uint64(2654435761)) % np.uint64(n_tenants)).astype(np.uint32)
        want = (np.arange(B) % n_tenants).astype(np.uint32)
        d_col = torch.tensor(col.view(np.int32), device="cuda")
        d_want = torch.tensor(want.view(np.int32), device="cuda")
        sizes = np.bincount(col, minlength=n_tenants)
        named = np.unique(want)
        # the tables of at most 64 bitmaps that say the same, and the queries each serves
        chunks = []
        for c0 in range(0, len(named), 64):
            labs = named[c0:c0 + 64]
            words, n_masks, n_bits = marshal_mask_table(col[None, :] == labs[:, None])
            at = np.nonzero(np.isin(want, labs))[0]
            chunks.append({"masks": torch.tensor(words.view(np.int32), device="cuda"), "n_masks": n_masks, "n_bits": n_bits,
                           "at": at, "q": q[torch.tensor(at, device="cuda")].contiguous(),
                           "of": torch.tensor(np.searchsorted(labs, want[at]).astype(np.int32), device="cuda"),
                           "o": outputs(len(at), k)})
        over = None
        if leg == "b":
            over = timed(lambda: sp.knn_labeled_device(q, kf, d_col, a.rows, d_want, *of, stream=st), a.warmup, a.steps)
            torch.cuda.synchronize()
            f_ids, f_cnt = of[0].cpu().numpy().view(np.uint64), of[2].cpu().numpy().view(np.uint32)
        for m in a.per_group:
            rec = dict(head, leg=leg, tenants=n_tenants, tenants_named=int(len(named)), tenant_rows_min=int(sizes.min()),
                       tenant_rows_max=int(sizes.max()), per_group=m)
            c0 = counters(sp)
            rec["knn_grouped_labeled_device"] = timed(
                lambda: sp.knn_grouped_labeled_device(q, k, d_groups, d_col, a.rows, d_want, *o, per_group=m, stream=st),
                a.warmup, a.steps)
            dc = counters(sp) - c0
            calls = max(int(dc[4]), 1)
            rec["scan_route_queries_per_call"] = round(int(dc[0]) / calls, 3)
            rec["list_route_share"] = round(int(dc[1]) / (calls * B), 5)
            rec["overflowed_queries_per_call"] = round(int(dc[2]) / calls, 3)
            rec["passes_per_call"] = round(int(dc[3]) / calls, 3)
            rec["route"] = "scan" if dc[1] == 0 else "list" if dc[0] == 0 else "scan, some queries handed to the list route"

            def tables():
                for c in chunks:
                    sp.knn_grouped_masked_device(c["q"], k, d_groups, a.rows, c["masks"], c["n_masks"], c["n_bits"], c["of"],
                                                 *c["o"], per_group=m, stream=st)
            rec["knn_grouped_masked_device_calls"] = len(chunks)
            rec["knn_grouped_masked_device"] = timed(tables, a.warmup, a.steps)
            torch.cuda.synchronize()
            truth = lists(o)
            table_truth = [None] * B
            for c in chunks:
                for j, row in zip(c["at"], lists(c["o"])):
                    table_truth[int(j)] = row
            rec["differs_from_the_tables"] = sum(truth[i] != table_truth[i] for i in range(B))
            if over is not None:
                rec["knn_labeled_device_overfetch"] = over
                guess = dedup(f_ids, f_cnt, groups, k, m)
                rec["overfetch_wrong_share"] = round(sum(guess[i] != truth[i] for i in range(B)) / B, 5)
                rec["overfetch_short_share"] = round(sum(len(guess[i]) < len(truth[i]) for i in range(B)) / B, 5)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
        del chunks, d_col
    sp.drop()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
