"""Measures the graph walk under per-query exclusion lists (ehx_graph_knn_except_device) on one MI355X: one JSON line per
(shape, list kind, list length).

A GPU-built L2 graph space over EHX-MANIFOLD-1 rows (ehx_fill_manifold, 16 latent dimensions), --rows x each of --dims;
--batch device-resident queries from the same generator under the query seed, k = --k, ef = --ef.  Every query has its own
list of --lens ids: `random` (drawn without replacement) or `nearest` (the query's own nearest rows, ranked with a plain fp32
matrix product over the generated rows — the recommender's case: what a user has seen lies around the user's vector).
In the same run, per line:
  lists           ONE ehx_graph_knn_except_device call, EHX_WALK_GRAPH: ms per call, queries/s
  floor           the plain strict walk at the same ef (ehx_knn_device, no filter).  Measured twice, before and after the
                  others; floor_spread is |second - first| / first of the medians: the noise every comparison is read against
  exact_lists     what the library offered for these lists on this space before: ONE ehx_knn_except_device call (exact)
  bitmap_tables   the other thing a caller could do: batch / 64 ehx_graph_knn_masked_multi_device calls under the complement
                  bitmaps, already packed and on the device (their construction and upload are NOT timed)
and recall@k of `lists` against exact_lists' ids, the queries of the call whose walk list reached its cap (cap_hits), and
whether the ids equal the bitmap walks' (they must).
Every time is the median of --steps timed calls (HIP events around the call, or the group of calls, after --warmup of them),
with min / max."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import embeddinghub_amd as ehx  # noqa: E402
from embeddinghub_amd import _lib  # noqa: E402

LATENT, TABLE = 16, 64


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
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def cap_hits(sp):
    out = (C.c_uint64 * 4)()
    C.CDLL(_lib.LIB_PATH).ehx_test_graph_masked_counters(sp._h, out)
    return int(out[3])


def results(B, k):
    return (torch.empty((B, k), dtype=torch.int64, device="cuda"), torch.empty((B, k), dtype=torch.float32, device="cuda"),
            torch.empty((B,), dtype=torch.int32, device="cuda"))


def complement_words(lists, n):
    """[B, ceil(n / 32)] int32 on the device: bit r of row i clear iff r is in lists[i]"""
    B, words = lists.shape[0], (n + 31) // 32
    w = torch.full((B, words), -1, dtype=torch.int32, device="cuda")
    if n % 32:
        w[:, -1] = (1 << (n % 32)) - 1
    if lists.shape[1]:
        bit = torch.ones_like(lists, dtype=torch.int32) << (lists & 31).to(torch.int32)
        # (ids of one list are distinct: the bits cleared in one word are distinct, so subtracting their sum clears them)
        w.view(-1).index_add_(0, (torch.arange(B, device="cuda")[:, None] * words + (lists >> 5)).view(-1), -bit.view(-1))
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dims", type=int, nargs="*", default=[128, 768])
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--ef", type=int, default=60)
    ap.add_argument("--lens", type=int, nargs="*", default=[0, 100, 1000, 4096])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    L = _lib.load()
    B, k, n = a.batch, a.k, a.rows
    st = torch.cuda.current_stream().cuda_stream
    for d in a.dims:
        sp = ehx.Space.unique("bench-gx", d, metric=ehx.METRIC_L2SQ, mode=ehx.MODE_GRAPH, initial_capacity=n, build_batch=4096,
                              ef=a.ef)
        t0 = time.perf_counter()
        sp.fill_manifold(ehx.SEED_CORPUS, 0, n, LATENT, False)
        build_s = time.perf_counter() - t0
        q = torch.empty((B, d), dtype=torch.float32, device="cuda")
        _lib.check(L.ehx_gen_manifold_rows_device(C.c_void_p(st), ehx.SEED_QUERY, 0, B, d, LATENT, 0, C.c_void_p(q.data_ptr())))
        # every query's nearest max(lens) rows, for the `nearest` lists
        X = torch.empty((n, d), dtype=torch.float32, device="cuda")
        _lib.check(L.ehx_gen_manifold_rows_device(C.c_void_p(st), ehx.SEED_CORPUS, 0, n, d, LATENT, 0, C.c_void_p(X.data_ptr())))
        torch.cuda.synchronize()
        xx = (X * X).sum(1)
        near = torch.cat([(xx[None, :] - 2.0 * (q[i:i + 128] @ X.T)).topk(max(a.lens + [1]), largest=False).indices
                          for i in range(0, B, 128)])
        del X, xx
        gen = torch.Generator(device="cuda").manual_seed(1)
        head = {"index": "l2_%dk%d" % (n // 1000, d), "rows": n, "dims": d, "metric": "l2", "batch": B, "k": k, "ef": a.ef,
                "steps": a.steps, "warmup": a.warmup, "build_s": round(build_s, 1)}
        fout = results(B, k)
        floor = lambda: sp.knn_device(q, k, *fout, stream=st)  # noqa: E731
        for kind in ("random", "nearest"):
            for m in a.lens:
                if kind == "nearest" and m == 0:
                    continue
                lists = (near[:, :m] if kind == "nearest"
                         else torch.rand((B, n), generator=gen, device="cuda").topk(m).indices if m else near[:, :0]).contiguous()
                off = torch.arange(B + 1, dtype=torch.int64, device="cuda") * m
                rec = dict(head, lists=kind, list_len=m)
                f0 = timed(floor, a.warmup, a.steps)
                out = results(B, k)
                h0 = cap_hits(sp)
                sp.graph_knn_except_device(q, k, lists.view(-1), off, *out, route=ehx.WALK_GRAPH, stream=st)
                torch.cuda.synchronize()
                rec["cap_hits"] = cap_hits(sp) - h0
                t = timed(lambda: sp.graph_knn_except_device(q, k, lists.view(-1), off, *out, route=ehx.WALK_GRAPH, stream=st),
                          a.warmup, a.steps)
                rec["lists_call"] = dict(t, qps=round(B / t["ms_median"] * 1e3))
                xout = results(B, k)
                t = timed(lambda: sp.knn_except_device(q, k, lists.view(-1), off, *xout, stream=st), 1, max(3, a.steps // 4))
                rec["exact_lists"] = dict(t, qps=round(B / t["ms_median"] * 1e3))
                words = complement_words(lists, n)
                of = torch.arange(TABLE, dtype=torch.int32, device="cuda")
                bout = results(B, k)

                def tables():
                    for b in range(0, B, TABLE):
                        e = min(B, b + TABLE)
                        sp.graph_knn_masked_multi_device(q[b:e], k, words[b:e], e - b, n, of[:e - b], bout[0][b:e], bout[1][b:e],
                                                         bout[2][b:e], route=ehx.WALK_GRAPH, stream=st)

                t = timed(tables, a.warmup, a.steps)
                rec["bitmap_tables"] = dict(t, qps=round(B / t["ms_median"] * 1e3), calls=(B + TABLE - 1) // TABLE)
                f1 = timed(floor, a.warmup, a.steps)
                rec["floor"] = dict(f0, qps=round(B / f0["ms_median"] * 1e3), ms_median_again=f1["ms_median"])
                rec["floor_spread"] = round(abs(f1["ms_median"] - f0["ms_median"]) / f0["ms_median"], 4)
                torch.cuda.synchronize()
                rec["ids_equal_bitmap_tables"] = bool(torch.equal(out[0], bout[0]) and torch.equal(out[2], bout[2]))
                hit = (out[0][:, :, None] == xout[0][:, None, :]) & (xout[0][:, None, :] >= 0)
                rec["recall_at_k"] = round(float(hit.any(1).sum()) / max(1, int(xout[2].sum())), 4)
                line = json.dumps(rec)
                print(line, flush=True)
                if a.out:    # (line by line: a run cut short keeps what it measured)
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
                del words
        sp.drop()


if __name__ == "__main__":
    main()
