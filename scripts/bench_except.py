"""Measures the kNN with per-query exclusion lists (ehx_knn_except_device) on one MI355X: one JSON line per list length and
way of drawing the lists.

One flat cosine space of --rows x --dims Gaussian rows, --batch device-resident queries (stored rows plus noise), k = --k.
Per list length L (--lists) and per draw — "random": L row ids drawn at random per query; "nearest": the query's own L
nearest rows (a float32 product on the device, good enough to draw a workload) — in the same run:
  knn_except_device   ONE call with the lists in CSR form on the device;
  knn_device_k        knn_device at k on the same rows: the floor, it excludes nothing;
  overfetch           the first route the call replaces: knn_device at k + L where the ABI allows it (k + L <= 1024), the ids
                      copied out and filtered in numpy; host clock around it all, --host-steps times;
  masked_multi        the second: ceil(batch / 64) calls of knn_masked_multi_device, 64 complement bitmaps each, the bitmaps
                      already on the device (bitmap_bytes says what a caller would have had to build and upload).
handed_on: queries of the last knn_except_device call the scan route handed to the exact route (ehx_test_except_counters).
Device figures are the median of --steps timed calls after --warmup calls, with min / max."""
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
    C.CDLL(_lib.LIB_PATH).ehx_test_except_counters(sp._h, out)
    return list(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--lists", type=int, nargs="*", default=[0, 100, 1000, 4096])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    B, k, d, n = a.batch, a.k, a.dims, a.rows
    sp = ehx.Space.unique("bench-except", d, metric=ehx.METRIC_COSINE, initial_capacity=n)
    gen = torch.Generator(device="cuda").manual_seed(20262)
    X = torch.empty((n, d), dtype=torch.float32, device="cuda")
    for r0 in range(0, n, 65536):
        m = min(65536, n - r0)
        X[r0:r0 + m] = torch.randn((m, d), generator=gen, device="cuda")
        sp.set_batch_device([str(i) for i in range(r0, r0 + m)], X[r0:r0 + m])
    st = torch.cuda.current_stream().cuda_stream
    q = (X[torch.arange(B, device="cuda") * (n // B)] + 0.3 * torch.randn((B, d), generator=gen, device="cuda")).contiguous()

    def outputs(width):
        return (torch.empty((B, width), dtype=torch.int64, device="cuda"), torch.empty((B, width), dtype=torch.float32, device="cuda"),
                torch.empty((B,), dtype=torch.int32, device="cuda"))

    o = outputs(k)
    head = {"rows": n, "dims": d, "metric": "cosine", "batch": B, "k": k, "steps": a.steps, "warmup": a.warmup,
            "engine": sp.scan_engine()}
    floor = timed(lambda: sp.knn_device(q, k, *o, stream=st), a.warmup, a.steps)
    Lmax = max(a.lists)
    nearest = None
    if Lmax:   # every query's Lmax nearest rows by cosine, in row chunks
        xn, qn = torch.nn.functional.normalize(X, dim=1), torch.nn.functional.normalize(q, dim=1)
        best_s, best_i = torch.full((B, 0), 0.0, device="cuda"), torch.zeros((B, 0), dtype=torch.int64, device="cuda")
        for r0 in range(0, n, 262144):
            s_ = qn @ xn[r0:r0 + 262144].T
            best_s, best_i = torch.cat([best_s, s_], 1), torch.cat([best_i, torch.arange(r0, r0 + s_.shape[1], device="cuda").expand(B, -1)], 1)
            top = torch.topk(best_s, min(Lmax, best_s.shape[1]), dim=1)
            best_s, best_i = top.values, torch.gather(best_i, 1, top.indices)
        nearest = best_i
        del xn, qn, best_s
    lines = []
    for L in a.lists:
        for draw in (("random", "nearest") if L else ("random",)):
            if draw == "random":
                seen = torch.stack([torch.randperm(n, generator=gen, device="cuda")[:L] for _ in range(B)]) if L else torch.zeros((B, 0), dtype=torch.int64, device="cuda")
            else:
                seen = nearest[:, :L]
            ids = seen.reshape(-1).contiguous()
            off = (torch.arange(B + 1, dtype=torch.int64, device="cuda") * L).contiguous()
            rec = dict(head, list_len=L, draw=draw, knn_device_k=floor)
            c0 = counters(sp)
            rec["knn_except_device"] = timed(lambda: sp.knn_except_device(q, k, ids, off, *o, stream=st), a.warmup, a.steps)
            c1 = counters(sp)
            calls = c1[4] - c0[4]
            rec["handed_on"] = round((c1[1] - c0[1]) / calls, 2)
            rec["overflowed"] = round((c1[2] - c0[2]) / calls, 2)
            got = o[0].cpu().numpy().copy()
            if 0 < k + L <= 1024:
                c = outputs(k + L)
                h_seen = seen.cpu().numpy()

                def overfetch():
                    sp.knn_device(q, k + L, *c, stream=st)
                    h = c[0].cpu().numpy()
                    return np.stack([row[~np.isin(row, h_seen[i])][:k] for i, row in enumerate(h)])

                ms = []
                for _ in range(a.host_steps):
                    t0 = time.perf_counter()
                    h_ids = overfetch()
                    ms.append((time.perf_counter() - t0) * 1e3)
                rec["overfetch"] = {"ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}
                rec["overfetch_same_ids"] = bool(np.array_equal(h_ids, got))
            else:
                rec["overfetch"] = None   # k + L is beyond the ABI's largest k
            if L:
                words = (n + 31) // 32
                masks = torch.empty((B, words), dtype=torch.int32, device="cuda")
                weights = (1 << torch.arange(32, dtype=torch.int64, device="cuda"))
                for g0 in range(0, B, 64):
                    allow = torch.ones((min(64, B - g0), words * 32), dtype=torch.bool, device="cuda")
                    allow.scatter_(1, seen[g0:g0 + 64], False)
                    allow[:, n:] = False
                    packed = (allow.view(-1, words, 32).to(torch.int64) * weights).sum(2)
                    masks[g0:g0 + 64] = torch.where(packed >= 2**31, packed - 2**32, packed).to(torch.int32)
                mask_of = torch.arange(64, dtype=torch.int32, device="cuda")
                o2 = outputs(k)

                def masked():
                    for g0 in range(0, B, 64):
                        g = min(64, B - g0)
                        sp.knn_masked_multi_device(q[g0:g0 + g], k, masks[g0:g0 + g], g, n, mask_of[:g], o2[0][g0:g0 + g],
                                                   o2[1][g0:g0 + g], o2[2][g0:g0 + g], stream=st)

                rec["masked_multi"] = timed(masked, a.warmup, a.steps)
                rec["masked_multi_calls"] = (B + 63) // 64
                rec["bitmap_bytes"] = B * words * 4
                rec["masked_same_bytes"] = bool(torch.equal(o2[0], o[0]) and torch.equal(o2[1], o[1]) and torch.equal(o2[2], o[2]))
                del masks
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
