"""Measures the range search under row bitmaps (ehx_range_masked_device) on one MI355X against the two calls a caller had
before it, and finds where its two routes cross: one JSON line per configuration.

One flat cosine space of --rows x --dims filled by fill_synthetic, --batch device-resident queries spread evenly over n_masks
random bitmaps of a density (mask_of interleaved: query i under mask i mod n_masks), max_results = --max-results, the radius
of every query its --rank-th ALLOWED distance (taken from the masked kNN's answer).  Every figure is the median of --steps
timed repeats (HIP events around the whole work of one batch, after --warmup repeats), with min / max.

Sweep 1, per (density, n_masks), in the same run:
  range_masked       ONE ehx_range_masked_device call, with the library's route counters per call
  range              ehx_range_device at the same radii, unfiltered (what a caller then had to filter on the host)
  knn_masked_multi   ehx_knn_masked_multi_device at k = --rank on the same table
Sweep 2, one bitmap per allowed share of --shares: the same call with every query forced onto the scan route and onto the
list route (the library's test hook), and a last line with the share at which the list route costs what the scan route
costs, interpolated between the shares around it, beside the routing cut max(1024, rows / 128)."""
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
    raw.ehx_test_range_masked_counters(sp._h, out)
    return np.array(list(out), dtype=np.int64)   # scan route, list route, pool overflows, truncated, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--max-results", type=int, default=64)
    ap.add_argument("--rank", type=int, default=10)
    ap.add_argument("--densities", type=float, nargs="*", default=[0.5, 0.1, 0.01, 0.001])
    ap.add_argument("--masks", type=int, nargs="*", default=[1, 16, 64])
    ap.add_argument("--shares", type=float, nargs="*", default=[0.002, 0.004, 0.006, 0.008, 0.012, 0.016, 0.02, 0.03])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    L = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)   # the test hooks are not part of the bound ABI
    raw.ehx_test_range_masked_route.argtypes = [C.c_void_p, C.c_uint32]
    sp = ehx.Space.unique("bench-range-masked", a.dims, metric=ehx.METRIC_COSINE, initial_capacity=a.rows)
    sp.fill_synthetic(ehx.SEED_CORPUS, 0, a.rows, True)
    B, mr, k = a.batch, a.max_results, a.rank
    st = torch.cuda.current_stream().cuda_stream
    q = torch.empty((B, a.dims), dtype=torch.float32, device="cuda")
    _lib.check(L.ehx_gen_rows_device(C.c_void_p(st), ehx.SEED_QUERY, 0, B, a.dims, 1, C.c_void_p(q.data_ptr())))
    o_ids = torch.empty((B, mr), dtype=torch.int64, device="cuda")
    o_dist = torch.empty((B, mr), dtype=torch.float32, device="cuda")
    o_cnt = torch.empty((B,), dtype=torch.int32, device="cuda")
    o_tot = torch.empty((B,), dtype=torch.int64, device="cuda")
    u_ids, u_dist, u_cnt, u_tot = (torch.empty_like(t) for t in (o_ids, o_dist, o_cnt, o_tot))
    k_ids = torch.empty((B, k), dtype=torch.int64, device="cuda")
    k_dist = torch.empty((B, k), dtype=torch.float32, device="cuda")
    k_cnt = torch.empty((B,), dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(1)
    lines = []
    head = {"rows": a.rows, "dims": a.dims, "metric": "cosine", "batch": B, "max_results": mr, "rank": k, "steps": a.steps,
            "warmup": a.warmup, "engine": sp.scan_engine(), "device": torch.cuda.get_device_name(0)}

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    def table(n_masks, density):
        tab = rng.random((n_masks, a.rows)) < density
        words, _, n_bits = marshal_mask_table(tab)
        d_masks = torch.tensor(words.view(np.int32), device="cuda")
        d_of = torch.tensor((np.arange(B) % n_masks).astype(np.int32), device="cuda")
        return d_masks, d_of, n_bits, int(tab.sum(axis=1).min()), int(tab.sum(axis=1).max())

    def knn(d_masks, n_masks, n_bits, d_of):
        sp.knn_masked_multi_device(q, k, d_masks, n_masks, n_bits, d_of, k_ids, k_dist, k_cnt, stream=st)

    def rangem(d_masks, n_masks, n_bits, d_of, radius):
        sp.range_masked_device(q, radius, mr, d_masks, n_masks, n_bits, d_of, o_ids, o_dist, o_cnt, o_tot, stream=st)

    def with_counters(rec, name, fn):
        c0 = counters(raw, sp)
        rec[name] = timed(fn, a.warmup, a.steps)
        dc = counters(raw, sp) - c0
        calls = max(int(dc[4]), 1)
        for i, what in enumerate(("scan_route", "list_route", "overflowed", "truncated")):
            rec[name][what + "_queries_per_call"] = round(int(dc[i]) / calls, 3)

    # sweep 1: the call beside the unfiltered range search and the masked kNN
    for density in a.densities:
        for n_masks in a.masks:
            d_masks, d_of, n_bits, lo, hi = table(n_masks, density)
            rec = dict(head, sweep="calls", density=density, n_masks=n_masks, allowed_min=lo, allowed_max=hi)
            knn(d_masks, n_masks, n_bits, d_of)
            torch.cuda.synchronize()
            radius = k_dist[:, k - 1].contiguous()   # every query's rank-th allowed distance
            with_counters(rec, "range_masked", lambda: rangem(d_masks, n_masks, n_bits, d_of, radius))
            torch.cuda.synchronize()
            rec["members_median"] = float(o_tot.median().item())
            rec["range"] = timed(lambda: sp.range_device(q, radius, mr, u_ids, u_dist, u_cnt, u_tot, stream=st), a.warmup, a.steps)
            rec["knn_masked_multi"] = timed(lambda: knn(d_masks, n_masks, n_bits, d_of), a.warmup, a.steps)
            rec["same_ids_as_knn"] = bool(torch.equal(o_ids[:, :k], k_ids))
            emit(rec)

    # sweep 2: both routes forced over one bitmap per share
    sweep = []
    for share in a.shares:
        d_masks, d_of, n_bits, lo, hi = table(1, share)
        rec = dict(head, sweep="routes", share=share, n_masks=1, n_allowed=lo)
        knn(d_masks, 1, n_bits, d_of)
        torch.cuda.synchronize()
        radius = k_dist[:, k - 1].contiguous()
        answers = []
        for name, route in (("forced_scan", 1), ("forced_list", 2)):
            raw.ehx_test_range_masked_route(sp._h, route)
            with_counters(rec, name, lambda: rangem(d_masks, 1, n_bits, d_of, radius))
            torch.cuda.synchronize()
            answers.append((o_ids.clone(), o_tot.clone()))
        raw.ehx_test_range_masked_route(sp._h, 0)
        rec["same_answer"] = bool(torch.equal(answers[0][0], answers[1][0]) and torch.equal(answers[0][1], answers[1][1]))
        sweep.append(rec)
        emit(rec)
    diff = [r["forced_list"]["ms_median"] - r["forced_scan"]["ms_median"] for r in sweep]
    cross = None
    for i in range(1, len(sweep)):
        if diff[i - 1] <= 0 < diff[i]:   # the list route overtakes the scan route's cost between these two shares
            t = -diff[i - 1] / (diff[i] - diff[i - 1])
            cross = sweep[i - 1]["share"] + t * (sweep[i]["share"] - sweep[i - 1]["share"])
    cut = max(1024, a.rows // 128)
    emit(dict(head, sweep="crossover", crossover_share=None if cross is None else round(cross, 5),
              crossover_n_allowed=None if cross is None else int(cross * a.rows), routing_cut_n_allowed=cut,
              routing_cut_share=round(cut / a.rows, 5),
              list_minus_scan_ms={str(r["share"]): round(d, 4) for r, d in zip(sweep, diff)}))
    sp.drop()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
