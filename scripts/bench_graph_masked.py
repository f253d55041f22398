"""Measures the graph walk under a row bitmap (ehx_graph_knn_masked_device) on one MI355X: one JSON line per index and
allowed share.

Two GPU-built graph spaces over EHX-MANIFOLD-1 rows (ehx_fill_manifold, 16 latent dimensions): 1 M x 128 L2 and
200 k x 768 cosine; --batch device-resident queries from the same generator under the query seed, k = --k, ef = --ef.
Random bitmaps allow shares 1, 1/2, ... 1/64 of the rows.  Per share, in the same run:
  walk            EHX_WALK_GRAPH: queries/s, recall@k against the exact route's answer of the same request, the share of
                  queries whose list reached its cap (from the library's counter), rows fetched per query
  exact           EHX_WALK_EXACT: queries/s — ehx_knn_masked_device's answer, what the request cost before the walk existed
  auto_route      what EHX_WALK_AUTO chose
Every time is the median of --steps timed calls (HIP events around ONE call each, after --warmup calls), with min / max.
The last line of an index gives the crossover: the largest measured share at which the exact route is at least as fast as
the walk (EHX_WALK_LIST_FACTOR is the reciprocal of the share EHX_WALK_AUTO cuts at)."""
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
from embeddinghub_amd.space import marshal_mask  # noqa: E402

INDEXES = {"l2_1m128": (1_000_000, 128, ehx.METRIC_L2SQ, False), "cos_200k768": (200_000, 768, ehx.METRIC_COSINE, True)}
LATENT = 16


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--indexes", nargs="*", default=list(INDEXES), choices=list(INDEXES))
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--ef", type=int, default=60)
    ap.add_argument("--shares", type=int, nargs="*", default=[1, 2, 4, 8, 16, 32, 64], help="allowed share = 1 / this")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    L = _lib.load()
    B, k = a.batch, a.k
    st = torch.cuda.current_stream().cuda_stream
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    for name in a.indexes:
        n, d, metric, norm = INDEXES[name]
        sp = ehx.Space.unique("bench-gm", d, metric=metric, mode=ehx.MODE_GRAPH, initial_capacity=n, build_batch=4096, ef=a.ef)
        t0 = time.perf_counter()
        sp.fill_manifold(ehx.SEED_CORPUS, 0, n, LATENT, norm)
        build_s = time.perf_counter() - t0
        q = torch.empty((B, d), dtype=torch.float32, device="cuda")
        _lib.check(L.ehx_gen_manifold_rows_device(C.c_void_p(st), ehx.SEED_QUERY, 0, B, d, LATENT, int(norm), C.c_void_p(q.data_ptr())))
        torch.cuda.synchronize()
        outs = [(torch.empty((B, k), dtype=torch.int64, device="cuda"), torch.empty((B, k), dtype=torch.float32, device="cuda"),
                 torch.empty((B,), dtype=torch.int32, device="cuda")) for _ in range(2)]
        head = {"index": name, "rows": n, "dims": d, "metric": ("l2", "ip", "cosine")[metric], "batch": B, "k": k, "ef": a.ef,
                "steps": a.steps, "warmup": a.warmup, "build_s": round(build_s, 1), "walk_list_factor": _lib.WALK_LIST_FACTOR}
        rng = np.random.default_rng(1)
        recs = []
        for inv in a.shares:
            allowed = np.ones(n, dtype=bool) if inv <= 1 else rng.random(n) < 1.0 / inv
            words, n_bits = marshal_mask(allowed)
            d_mask = torch.tensor(words.view(np.int32), device="cuda")
            rec = dict(head, share="1/%d" % inv, n_allowed=int(allowed.sum()))

            def run(route, o):
                sp.graph_knn_masked_device(q, k, d_mask, n_bits, o[0], o[1], o[2], route=route, stream=st)

            sp.stats_reset()
            c0 = counters(sp)
            t = timed(lambda: run(ehx.WALK_GRAPH, outs[0]), a.warmup, a.steps)
            dc = counters(sp) - c0
            rec["walk"] = dict(t, qps=round(B / t["ms_median"] * 1e3))
            rec["walk"]["at_cap_share"] = round(int(dc[3]) / max(int(dc[0]), 1), 4)
            rec["walk"]["rows_fetched_per_query"] = round(sp.graph_counters()[0] / max(int(dc[0]), 1), 1)
            t = timed(lambda: run(ehx.WALK_EXACT, outs[1]), a.warmup, a.steps)
            rec["exact"] = dict(t, qps=round(B / t["ms_median"] * 1e3))
            w_ids, w_cnt = outs[0][0].cpu().numpy(), outs[0][2].cpu().numpy()
            x_ids, x_cnt = outs[1][0].cpu().numpy(), outs[1][2].cpu().numpy()
            found = sum(len(set(w_ids[i, :w_cnt[i]].tolist()) & set(x_ids[i, :x_cnt[i]].tolist())) for i in range(B))
            rec["walk"]["recall_at_k"] = round(found / max(int(x_cnt.sum()), 1), 4)
            rec["walk"]["short_answers"] = int((w_cnt < x_cnt).sum())
            c0 = counters(sp)
            run(ehx.WALK_AUTO, outs[0])
            torch.cuda.synchronize()
            rec["auto_route"] = "walk" if (counters(sp) - c0)[0] else "exact"
            emit(rec)
            recs.append((inv, rec))
        slower = [inv for inv, r in recs if r["exact"]["ms_median"] <= r["walk"]["ms_median"]]
        emit(dict(head, crossover_share=("1/%d" % min(slower)) if slower else None,
                  auto_cut_share="1/%d" % _lib.WALK_LIST_FACTOR))
        sp.drop()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
