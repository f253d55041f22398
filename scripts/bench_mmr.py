"""Measures the MMR search (ehx_knn_mmr_device) on one MI355X: one JSON line per fetch_k.

One flat cosine space of --rows x --dims rows in near-duplicate clusters (8 jittered copies of every centre, stored side by
side — the chunks of a document), --batch device-resident queries near centres, k = --k, lambda = --lam.  Per fetch_k, in the
same run:
  knn_mmr_device   ONE call: the candidates at fetch_k and the selection on the device;
  knn_device       at fetch_k alone, so the difference is the selection;
  mmr_select       the selection alone over those candidates (HIP events around the one launch), and its row bytes — every
                   sweep's unpicked rows and every pivot, computed from the shapes — per second as a share of 8 TB/s;
  host_route       the route the call replaces: knn_device at fetch_k, get_by_ids_device of every candidate, the copy out, and
                   the greedy in numpy (float32, BLAS products: NOT the canonical arithmetic, so near-ties may pick another
                   row); timed with a host clock around it all, --host-steps times.
same_ids_share: the share of queries whose picks agree between knn_mmr_device and the host route; same_bytes: whether ids,
distances and counts agree byte for byte over the whole batch.  Device figures are the median of --steps timed calls after
--warmup calls, with min / max."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import embeddinghub_amd as ehx  # noqa: E402

HBM_BYTES_PER_S = 8e12


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


def host_greedy(rows, dq, cnt, k, lam):
    """rows [nq, fetch_k, dims] as Get returns them, dq [nq, fetch_k], cnt [nq] -> the picked ranks per query (cosine)"""
    lam, mu = np.float32(lam), np.float32(1) - np.float32(lam)
    picks = []
    for x, d, c in zip(rows, dq, cnt):
        x = x[:c] / (np.sqrt((x[:c] * x[:c]).sum(1, keepdims=True)) + np.float32(1e-30))
        near, left, mine = np.full(c, np.inf, dtype=np.float32), np.ones(c, dtype=bool), []
        while len(mine) < min(k, c):
            if mine:
                near = np.minimum(near, np.float32(1) - x @ x[mine[-1]])
                cost = np.where(left, lam * d[:c] - mu * near, np.inf)
                p = int(np.argmin(cost))   # (the first of equal costs: the lowest rank)
            else:
                p = 0
            mine.append(p)
            left[p] = False
        picks.append(mine)
    return picks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--fetch-k", type=int, nargs="*", default=[20, 100, 256])
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    B, k, d = a.batch, a.k, a.dims
    sp = ehx.Space.unique("bench-mmr", d, metric=ehx.METRIC_COSINE, initial_capacity=a.rows)
    gen = torch.Generator(device="cuda").manual_seed(20261)
    chunk = 65536
    for r0 in range(0, a.rows, chunk):   # 8 jittered copies of every centre, side by side
        n = min(chunk, a.rows - r0)
        centres = torch.randn(((n + 7) // 8, d), generator=gen, device="cuda")
        x = centres.repeat_interleave(8, 0)[:n] + 0.05 * torch.randn((n, d), generator=gen, device="cuda")
        sp.set_batch_device([str(i) for i in range(r0, r0 + n)], x.contiguous())
    st = torch.cuda.current_stream().cuda_stream
    near = torch.arange(B, dtype=torch.int64, device="cuda") * (a.rows // B)
    q = torch.empty((B, d), dtype=torch.float32, device="cuda")
    sp.get_by_ids_device(near, q, torch.empty((B,), dtype=torch.int32, device="cuda"), stream=st)
    q += 0.02 * torch.randn((B, d), generator=gen, device="cuda")

    def outputs(width):
        return (torch.empty((B, width), dtype=torch.int64, device="cuda"), torch.empty((B, width), dtype=torch.float32, device="cuda"),
                torch.empty((B,), dtype=torch.int32, device="cuda"))

    o, o2 = outputs(k), outputs(k)
    head = {"rows": a.rows, "dims": d, "metric": "cosine", "batch": B, "k": k, "lambda": a.lam, "steps": a.steps,
            "warmup": a.warmup, "engine": sp.scan_engine()}
    lines = []
    for fk in a.fetch_k:
        c = outputs(fk)
        rec = dict(head, fetch_k=fk)
        rec["knn_mmr_device"] = timed(lambda: sp.knn_mmr_device(q, k, fk, a.lam, *o, stream=st), a.warmup, a.steps)
        rec["knn_device_fetch_k"] = timed(lambda: sp.knn_device(q, fk, *c, stream=st), a.warmup, a.steps)
        rec["mmr_select"] = timed(lambda: sp.mmr_select_device(*c, k, a.lam, *o2, stream=st), a.warmup, a.steps)
        torch.cuda.synchronize()
        cnt = np.minimum(c[2].cpu().numpy().view(np.uint32).astype(np.int64), fk)
        picks = np.minimum(cnt, k)
        # rows a query's sweeps read: before pick t = 1 .. picks - 1 the cnt - t unpicked rows and the pivot
        n_rows_read = int(sum((p - 1) * (n + 1) - p * (p - 1) // 2 for p, n in zip(picks, cnt) if p > 1))
        row_bytes = n_rows_read * ((d + 31) // 32 * 32) * 4
        rec["select_row_bytes"] = row_bytes
        rec["select_row_bytes_per_s"] = round(row_bytes / (rec["mmr_select"]["ms_median"] * 1e-3), 1)
        rec["select_share_of_8TBps"] = round(rec["select_row_bytes_per_s"] / HBM_BYTES_PER_S, 4)
        rows = torch.empty((B * fk, d), dtype=torch.float32, device="cuda")
        valid = torch.empty((B * fk,), dtype=torch.int32, device="cuda")

        def host_route():
            sp.knn_device(q, fk, *c, stream=st)
            sp.get_by_ids_device(c[0].view(-1), rows, valid, stream=st)
            h_rows, h_ids, h_dq = rows.cpu().numpy().reshape(B, fk, d), c[0].cpu().numpy().view(np.uint64), c[1].cpu().numpy()
            h_cnt = np.minimum(c[2].cpu().numpy().view(np.uint32).astype(np.int64), fk)
            r = host_greedy(h_rows, h_dq, h_cnt, k, a.lam)
            return [h_ids[i, p] for i, p in enumerate(r)], [h_dq[i, p] for i, p in enumerate(r)]

        ms = []
        for _ in range(a.host_steps):
            t0 = time.perf_counter()
            h_ids, h_dq = host_route()
            ms.append((time.perf_counter() - t0) * 1e3)
        rec["host_route"] = {"ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}
        g_ids, g_dq, g_cnt = o[0].cpu().numpy().view(np.uint64), o[1].cpu().numpy(), o[2].cpu().numpy().view(np.uint32)
        same = [int(g_cnt[i]) == len(h_ids[i]) and np.array_equal(g_ids[i, :len(h_ids[i])], h_ids[i]) for i in range(B)]
        rec["same_ids_share"] = round(sum(same) / B, 5)
        rec["same_bytes"] = bool(all(same) and all(g_dq[i, :len(h_dq[i])].tobytes() == np.asarray(h_dq[i]).tobytes() for i in range(B)))
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
