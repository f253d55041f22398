"""Measures the grouped graph walk (ehx_graph_knn_grouped_device) on one MI355X: one JSON line per (shape, label layout,
per_group).

A GPU-built L2 graph space over EHX-MANIFOLD-1 rows (ehx_fill_manifold, 16 latent dimensions), --rows x each of --dims;
--batch device-resident queries from the same generator under the query seed, k = --k, ef = --ef.  Labels, 8 rows a group:
  near        groups of near rows — the leaves of a random-projection tree over the generated rows (17 levels of "split every
              segment at the median of a random direction" at 1 M rows), the chunks-of-a-document case: a query's nearest
              rows share few labels, so the cap bites
  scattered   a random permutation cut into eights: a query's nearest rows hardly ever share a label
In the same run, per line:
  walk        ONE ehx_graph_knn_grouped_device call, EHX_WALK_GRAPH: ms per call, queries/s
  floor       the plain strict walk at the same ef (ehx_knn_device, no cap), measured before and after the others;
              floor_spread is |second - first| / first of the medians: the noise every comparison is read against
  exact       ONE ehx_knn_grouped_device call on the same graph space: the only grouped route it had before
  overfetch   ehx_knn_device at k = --fetch, ids and distances copied to the host, de-duplicated there with numpy
and recall@k of `walk` and of `overfetch` against exact's ids, and the queries whose walk list reached its cap.
Every time is the median of --steps timed calls (HIP events, or the host clock where the host works, after --warmup),
with min / max."""
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

LATENT, GROUP = 16, 8


def timed(fn, warmup, steps, host=False):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        if host:   # (the call ends on the host, behind its own copies)
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
            continue
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def cap_hits(sp):
    out = (C.c_uint64 * 4)()
    C.CDLL(_lib.LIB_PATH).ehx_test_graph_masked_counters(sp._h, out)
    return int(out[3])


def results(B, k):
    return (torch.empty((B, k), dtype=torch.int64, device="cuda"), torch.empty((B, k), dtype=torch.float32, device="cuda"),
            torch.empty((B,), dtype=torch.int32, device="cuda"))


def near_labels(X, gen):
    """[n] int32: the leaf of a random-projection tree with GROUP rows a leaf"""
    n = X.shape[0]
    idx = torch.arange(n, device="cuda")
    pos = torch.arange(n, device="cuda")
    levels = max(0, int(np.ceil(np.log2(max(1, n // GROUP)))))
    for level in range(levels):
        r = torch.randn(X.shape[1], generator=gen, device="cuda")
        by_proj = torch.argsort((X @ r)[idx], stable=True)
        seg = (pos << level) // n   # the segment of a POSITION: equal blocks, halved every level
        idx = idx[by_proj[torch.argsort(seg[by_proj], stable=True)]]   # sorted by (segment, projection): blocks keep their rows
    lab = torch.empty(n, dtype=torch.int32, device="cuda")
    lab[idx] = (pos // GROUP).to(torch.int32)
    return lab


def dedup_host(ids, lab_host, per_group, k):
    """the first k of every row of ids [B, fetch] (nearest first) with fewer than per_group earlier entries of their label"""
    lab = lab_host[np.maximum(ids, 0)]
    earlier = np.tril(lab[:, :, None] == lab[:, None, :], -1).sum(2)
    out = np.full((ids.shape[0], k), -1, dtype=np.int64)
    for i in range(ids.shape[0]):
        keep = ids[i][(earlier[i] < per_group) & (ids[i] >= 0)][:k]
        out[i, :len(keep)] = keep
    return out


def recall(got, want, want_cnt):
    hit = (got[:, :, None] == want[:, None, :]) & (want[:, None, :] >= 0) & (got[:, :, None] >= 0)
    return round(float(hit.any(1).sum()) / max(1, int(want_cnt.sum())), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dims", type=int, nargs="*", default=[128, 768])
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--ef", type=int, default=60)
    ap.add_argument("--fetch", type=int, default=48)
    ap.add_argument("--per-group", type=int, nargs="*", default=[1, 3])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    L = _lib.load()
    B, k, n = a.batch, a.k, a.rows
    st = torch.cuda.current_stream().cuda_stream
    for d in a.dims:
        sp = ehx.Space.unique("bench-gg", d, metric=ehx.METRIC_L2SQ, mode=ehx.MODE_GRAPH, initial_capacity=n, build_batch=4096,
                              ef=a.ef)
        t0 = time.perf_counter()
        sp.fill_manifold(ehx.SEED_CORPUS, 0, n, LATENT, False)
        build_s = time.perf_counter() - t0
        q = torch.empty((B, d), dtype=torch.float32, device="cuda")
        _lib.check(L.ehx_gen_manifold_rows_device(C.c_void_p(st), ehx.SEED_QUERY, 0, B, d, LATENT, 0, C.c_void_p(q.data_ptr())))
        X = torch.empty((n, d), dtype=torch.float32, device="cuda")
        _lib.check(L.ehx_gen_manifold_rows_device(C.c_void_p(st), ehx.SEED_CORPUS, 0, n, d, LATENT, 0, C.c_void_p(X.data_ptr())))
        torch.cuda.synchronize()
        gen = torch.Generator(device="cuda").manual_seed(1)
        layouts = {"near": near_labels(X, gen),
                   "scattered": (torch.argsort(torch.rand(n, generator=gen, device="cuda")) // GROUP).to(torch.int32)}
        del X
        head = {"index": "l2_%dk%d" % (n // 1000, d), "rows": n, "dims": d, "metric": "l2", "batch": B, "k": k, "ef": a.ef,
                "group_rows": GROUP, "fetch": a.fetch, "steps": a.steps, "warmup": a.warmup, "build_s": round(build_s, 1)}
        fout, big = results(B, k), results(B, a.fetch)
        floor = lambda: sp.knn_device(q, k, *fout, stream=st)  # noqa: E731
        for layout, lab in layouts.items():
            lab_host = lab.cpu().numpy()
            for per_group in a.per_group:
                rec = dict(head, labels=layout, per_group=per_group)
                f0 = timed(floor, a.warmup, a.steps)
                out, xout = results(B, k), results(B, k)
                h0 = cap_hits(sp)
                walk = lambda: sp.graph_knn_grouped_device(q, k, per_group, lab, n, *out, route=ehx.WALK_GRAPH, stream=st)  # noqa: E731
                walk()
                torch.cuda.synchronize()
                rec["cap_hits"] = cap_hits(sp) - h0
                t = timed(walk, a.warmup, a.steps)
                rec["walk"] = dict(t, qps=round(B / t["ms_median"] * 1e3))
                t = timed(lambda: sp.knn_grouped_device(q, k, lab, n, *xout, per_group=per_group, stream=st), 1, max(3, a.steps // 6))
                rec["exact"] = dict(t, qps=round(B / t["ms_median"] * 1e3))
                kept = []

                def overfetch():
                    sp.knn_device(q, a.fetch, *big, stream=st)
                    kept[:] = [dedup_host(big[0].cpu().numpy(), lab_host, per_group, k)]

                t = timed(overfetch, a.warmup, a.steps, host=True)
                rec["overfetch"] = dict(t, qps=round(B / t["ms_median"] * 1e3))
                f1 = timed(floor, a.warmup, a.steps)
                rec["floor"] = dict(f0, qps=round(B / f0["ms_median"] * 1e3), ms_median_again=f1["ms_median"])
                rec["floor_spread"] = round(abs(f1["ms_median"] - f0["ms_median"]) / f0["ms_median"], 4)
                torch.cuda.synchronize()
                rec["recall_at_k"] = recall(out[0], xout[0], xout[2])
                rec["overfetch_recall_at_k"] = recall(torch.from_numpy(kept[0]).cuda(), xout[0], xout[2])
                rec["walk_over_floor"] = round(rec["walk"]["ms_median"] / f0["ms_median"], 3)
                rec["exact_over_walk"] = round(rec["exact"]["ms_median"] / rec["walk"]["ms_median"], 1)
                line = json.dumps(rec)
                print(line, flush=True)
                if a.out:    # (line by line: a run cut short keeps what it measured)
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
        sp.drop()


if __name__ == "__main__":
    main()
