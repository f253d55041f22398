"""Measures the MaxSim search (ehx_knn_maxsim_device) on one MI355X: one JSON line per (batch, T, fetch_k).

One flat cosine space of --rows x --dims rows; stored column 0 holds the entity of every row, entities of 32 .. 256 rows laid
side by side (the patches of a page, the chunks of a document).  A query is T vectors near rows of one entity.  Per line, in
the same run:
  knn_maxsim_device  ONE call: the candidates of every query vector at fetch_k and the scoring on the device;
  maxsim_select      the scoring alone over those candidates (HIP events around the call: query preparation and the one
                     kernel), the rows it walks (test hook) and their bytes — once per slab from HBM, and once per block of 8
                     query vectors from wherever the cache serves them — per second as a share of 8 TB/s;
  detour             the route the call replaces, for the first --host-queries queries only (every row of every candidate
                     entity leaves the device): knn_grouped_device per query vector, column_read_device, get_by_ids_device of
                     the candidates' rows, the copy out, and the scores in numpy (float32, BLAS products: NOT the canonical
                     arithmetic); a host clock around it all.  detour_ms_per_query against the device call's ms per query is
                     the ratio.
same_top1_share: the share of those queries whose best entity agrees.  Device figures are the median of --steps timed calls
after --warmup calls, with min / max."""
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

HBM_BYTES_PER_S = 8e12
NT = 8   # k_maxsim.hip's block of query vectors


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
    assert C.CDLL(_lib.LIB_PATH).ehx_test_maxsim_counters(sp._h, out) == 0
    return list(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dims", type=int, default=128)
    ap.add_argument("--batch", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--tokens", type=int, nargs="*", default=[8, 32])
    ap.add_argument("--fetch-k", type=int, nargs="*", default=[8, 32])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--host-queries", type=int, default=8)
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    d, k = a.dims, a.k
    rng = np.random.default_rng(29)
    sizes = []
    while sum(sizes) < a.rows:
        sizes.append(int(rng.integers(32, 257)))
    sizes[-1] -= sum(sizes) - a.rows
    first = np.concatenate([[0], np.cumsum(sizes)])
    entity_of = np.repeat(np.arange(len(sizes), dtype=np.uint32), sizes)
    sp = ehx.Space.unique("bench-maxsim", d, metric=ehx.METRIC_COSINE, initial_capacity=a.rows)
    gen = torch.Generator(device="cuda").manual_seed(20262)
    chunk = 65536
    for r0 in range(0, a.rows, chunk):
        n = min(chunk, a.rows - r0)
        sp.set_batch_device([str(i) for i in range(r0, r0 + n)], torch.randn((n, d), generator=gen, device="cuda"))
    d_col = torch.tensor(entity_of.view(np.int32), device="cuda")
    sp.column_load_device(0, 0, d_col)
    st = torch.cuda.current_stream().cuda_stream
    lines = []
    for B in a.batch:
        for T in a.tokens:
            # query i: T vectors near the first T rows of entity i * stride (jittered)
            ent = (np.arange(B) * (len(sizes) // B)).astype(np.int64)
            near = torch.tensor((first[ent][:, None] + np.arange(T)[None, :] % np.asarray(sizes)[ent][:, None]).reshape(-1), device="cuda")
            tok = torch.empty((B * T, d), dtype=torch.float32, device="cuda")
            sp.get_by_ids_device(near, tok, torch.empty((B * T,), dtype=torch.int32, device="cuda"), stream=st)
            tok = (tok + 0.05 * torch.randn((B * T, d), generator=gen, device="cuda")).reshape(B, T, d).contiguous()
            for fk in a.fetch_k:
                if T * fk > _lib.MAXSIM_MAX_CAND:
                    continue
                o = (torch.empty((B, k), dtype=torch.int64, device="cuda"), torch.empty((B, k), dtype=torch.float32, device="cuda"),
                     torch.empty((B,), dtype=torch.int32, device="cuda"))
                g = (torch.empty((B * T, fk), dtype=torch.int64, device="cuda"), torch.empty((B * T, fk), dtype=torch.float32, device="cuda"),
                     torch.empty((B * T,), dtype=torch.int32, device="cuda"))
                rec = {"rows": a.rows, "dims": d, "metric": "cosine", "entities": len(sizes), "batch": B, "tokens": T, "fetch_k": fk,
                       "k": k, "steps": a.steps, "warmup": a.warmup, "engine": sp.scan_engine(), "nt": NT, "slab": 64}
                rec["knn_maxsim_device"] = timed(lambda: sp.knn_maxsim_device(tok, None, 0, k, fk, *o, stream=st), a.warmup, a.steps)
                sp.knn_grouped_device(tok.reshape(B * T, d), fk, d_col, a.rows, *g, stream=st)
                torch.cuda.synchronize()
                cand = d_col[g[0].clamp(0, a.rows - 1)].reshape(B, T * fk).contiguous()   # (every list is full: fk <= entities)
                ccnt = torch.full((B,), T * fk, dtype=torch.int32, device="cuda")
                o2 = tuple(torch.empty_like(x) for x in o)
                rec["maxsim_select"] = timed(lambda: sp.maxsim_select_device(tok, None, 0, cand, ccnt, k, *o2, stream=st), a.warmup, a.steps)
                c0 = counters(sp)
                sp.maxsim_select_device(tok, None, 0, cand, ccnt, k, *o2, stream=st)
                c1 = counters(sp)
                rec["select_candidates"], rec["select_rows_walked"] = c1[1] - c0[1], c1[2] - c0[2]
                once = rec["select_rows_walked"] * ((d + 31) // 32 * 32) * 4
                sec = rec["maxsim_select"]["ms_median"] * 1e-3
                rec["select_row_bytes_once"], rec["select_row_bytes_all_blocks"] = once, once * ((T + NT - 1) // NT)
                rec["select_once_share_of_8TBps"] = round(once / sec / HBM_BYTES_PER_S, 4)
                rec["select_all_blocks_share_of_8TBps"] = round(once * ((T + NT - 1) // NT) / sec / HBM_BYTES_PER_S, 4)
                assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(o, o2)), "the composition differs"
                # ---- the detour, for the first queries ----
                H = min(a.host_queries, B)
                t0 = time.perf_counter()
                hq = tok[:H].reshape(H * T, d)
                hg = tuple(x[:H * T] for x in g)
                sp.knn_grouped_device(hq, fk, d_col, a.rows, *hg, stream=st)
                col = torch.empty((a.rows,), dtype=torch.int32, device="cuda")
                sp.column_read_device(0, 0, col, stream=st)
                h_ids, h_col = hg[0].cpu().numpy(), col.cpu().numpy().view(np.uint32)
                best = []
                for i in range(H):
                    ents = np.unique(h_col[h_ids[i * T:(i + 1) * T].reshape(-1)])
                    ids = np.concatenate([np.arange(first[e], first[e + 1]) for e in ents])
                    rows = torch.empty((len(ids), d), dtype=torch.float32, device="cuda")
                    sp.get_by_ids_device(torch.tensor(ids, device="cuda"), rows, torch.empty((len(ids),), dtype=torch.int32, device="cuda"), stream=st)
                    x, qv = rows.cpu().numpy(), hq[i * T:(i + 1) * T].cpu().numpy()
                    x /= np.sqrt((x * x).sum(1, keepdims=True)) + np.float32(1e-30)
                    qv = qv / (np.sqrt((qv * qv).sum(1, keepdims=True)) + np.float32(1e-30))
                    dist = np.float32(1) - qv @ x.T
                    at = np.concatenate([[0], np.cumsum([first[e + 1] - first[e] for e in ents])])
                    score = [dist[:, at[j]:at[j + 1]].min(1).sum() for j in range(len(ents))]
                    best.append(int(ents[int(np.argmin(score))]))
                ms = (time.perf_counter() - t0) * 1e3
                rec["detour_queries"], rec["detour_ms_per_query"] = H, round(ms / H, 3)
                rec["device_ms_per_query"] = round(rec["knn_maxsim_device"]["ms_median"] / B, 5)
                rec["detour_over_device"] = round(rec["detour_ms_per_query"] / rec["device_ms_per_query"], 1)
                rec["same_top1_share"] = round(float(np.mean(o[0][:H, 0].cpu().numpy() == np.asarray(best))), 4)
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
