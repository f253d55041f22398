"""Measures the boosted kNN (ehx_knn_boosted_device, ehx_knn_decay_device) on one MI355X: one JSON line per form and weight.

One flat cosine space of --rows x --dims Gaussian rows, --batch device-resident queries (stored rows plus noise), k = --k.
sigma: the standard deviation of one query's distances to the rows (the mean over eight queries).  Per form — "array":
penalties uniform in [0, 1); "column": a stored column uniform in [0, 2^20), origin 2^19, no clipping — and per factor f of
--factors the weight is chosen so that w (p_max - p_min) = f sigma.  In the same run:
  except_floor   knn_except_device with empty lists: the same route without penalties;
  knn_device_k   knn_device at k;
  overfetch      the route the call replaces: knn_device at fetch_k = 256 plus a torch re-score and top-k on the device;
                 overfetch_wrong is the share of queries whose ids differ from the boosted call's (which is exact).
passes: per call; handed_on, overflowed: shares of the queries (ehx_test_boost_counters); rows_per_query: the rows the scan
route re-ranked per query (n_dist without the scan copy's and the exact route's rows).
Device figures are the median of --steps timed calls after --warmup calls, with min / max."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

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
    C.CDLL(_lib.LIB_PATH).ehx_test_boost_counters(sp._h, out)
    return list(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--factors", type=float, nargs="*", default=[0, 0.1, 0.5, 1, 2])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    B, k, d, n = a.batch, a.k, a.dims, a.rows
    sp = ehx.Space.unique("bench-boost", d, metric=ehx.METRIC_COSINE, initial_capacity=n)
    gen = torch.Generator(device="cuda").manual_seed(20263)
    X = torch.empty((n, d), dtype=torch.float32, device="cuda")
    for r0 in range(0, n, 65536):
        m = min(65536, n - r0)
        X[r0:r0 + m] = torch.randn((m, d), generator=gen, device="cuda")
        sp.set_batch_device([str(i) for i in range(r0, r0 + m)], X[r0:r0 + m])
    st = torch.cuda.current_stream().cuda_stream
    q = (X[torch.arange(B, device="cuda") * (n // B)] + 0.3 * torch.randn((B, d), generator=gen, device="cuda")).contiguous()
    sigma = float((1 - torch.nn.functional.normalize(q[:8], dim=1) @ torch.nn.functional.normalize(X, dim=1).T).std(dim=1).mean())
    del X
    pen = torch.rand((n,), generator=gen, device="cuda")
    col = torch.randint(0, 2**20, (n,), generator=gen, device="cuda", dtype=torch.int32)
    sp.column_load_device(0, 0, col)
    origin, span = 2**19, 2**31
    col_pen = (col.to(torch.int64) - origin).abs().to(torch.float32)

    def outputs(width):
        return (torch.empty((B, width), dtype=torch.int64, device="cuda"), torch.empty((B, width), dtype=torch.float32, device="cuda"),
                torch.empty((B,), dtype=torch.int32, device="cuda"))

    o, c = outputs(k), outputs(256)
    no_ids, no_off = torch.zeros((0,), dtype=torch.int64, device="cuda"), torch.zeros((B + 1,), dtype=torch.int64, device="cuda")
    head = {"rows": n, "dims": d, "metric": "cosine", "batch": B, "k": k, "steps": a.steps, "warmup": a.warmup,
            "engine": sp.scan_engine(), "sigma": round(sigma, 6),
            "except_floor": timed(lambda: sp.knn_except_device(q, k, no_ids, no_off, *o, stream=st), a.warmup, a.steps),
            "knn_device_k": timed(lambda: sp.knn_device(q, k, *o, stream=st), a.warmup, a.steps)}
    lines = []
    for form, p in (("array", pen), ("column", col_pen)):
        spread = float(p.max() - p.min())
        for f in a.factors:
            w = torch.full((B,), f * sigma / spread, device="cuda")
            call = ((lambda: sp.knn_boosted_device(q, k, pen, n, *o, d_weight=w, stream=st)) if form == "array" else
                    (lambda: sp.knn_decay_device(q, k, 0, origin, span, *o, d_weight=w, stream=st)))
            rec = dict(head, form=form, factor=f, weight=float(w[0]))
            c0, d0 = counters(sp), sp.stats()["n_dist"]
            rec["boosted"] = timed(call, a.warmup, a.steps)
            c1, calls = counters(sp), a.warmup + a.steps
            rec["passes"] = (c1[3] - c0[3]) / calls
            rec["handed_on"] = round((c1[1] - c0[1]) / calls / B, 4)
            rec["overflowed"] = round((c1[2] - c0[2]) / calls / B, 4)
            # (n_dist counts the scan copy's rows once per query and the exact route's once per handed query besides)
            rec["rows_per_query"] = round((sp.stats()["n_dist"] - d0) / calls / B - n * (1 + rec["handed_on"]), 1)

            def overfetch():
                sp.knn_device(q, 256, *c, stream=st)
                top = torch.topk(c[1] + w[:, None] * p[c[0].clamp(0, n - 1)], k, dim=1, largest=False)
                return torch.gather(c[0], 1, top.indices)

            rec["overfetch"] = timed(overfetch, a.warmup, a.steps)
            rec["overfetch_wrong"] = round(float((overfetch().sort(dim=1).values != o[0].sort(dim=1).values).any(dim=1).float().mean()), 4)
            rec["zero_weight_within_floor"] = (head["except_floor"]["ms_min"] <= rec["boosted"]["ms_median"] <= head["except_floor"]["ms_max"]
                                               if f == 0 else None)
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
