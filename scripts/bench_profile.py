"""Measures the profile search (ehx_knn_profile_device, ehx_combine_rows_device) on one MI355X: one JSON line per list length
and way of drawing the ids.

One flat cosine space of --rows x --dims Gaussian rows, --batch queries, each a list of L row ids with signed weights, k = --k.
Per list length L (--lists) and per draw — "uniform": ids drawn uniformly from all rows; "popular": from the first 1 % of the
rows, so that rows repeat across the batch and may be served from cache — in the same run:
  knn_profile_device  ONE call: targets summed on the device, then the except route under the same lists;
  combine             combine_rows_device alone; gbytes_per_s = batch x L x row bytes / its median time, against 8 TB/s of HBM;
  floor               knn_except_device on the ready-made targets and the same lists: what the search behind the sum costs;
  replaced            the route the call replaces: get_by_ids_device for every list entry (batch x L row copies, row_copy_bytes),
                      a torch weighted sum (one bmm), knn_except_device.
same_bytes: knn_profile_device's ids, distances and counts equal the floor's on combine's targets.
Device figures are the median of --steps timed calls after --warmup calls, with min / max."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import embeddinghub_amd as ehx  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--lists", type=int, nargs="*", default=[16, 256, 4096])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "profile_bench.jsonl"), help="the JSON lines are appended to this file")
    a = ap.parse_args()
    B, k, d, n = a.batch, a.k, a.dims, a.rows
    sp = ehx.Space.unique("bench-profile", d, metric=ehx.METRIC_COSINE, initial_capacity=n)
    gen = torch.Generator(device="cuda").manual_seed(20263)
    for r0 in range(0, n, 65536):
        m = min(65536, n - r0)
        sp.set_batch_device([str(i) for i in range(r0, r0 + m)], torch.randn((m, d), generator=gen, device="cuda"))
    st = torch.cuda.current_stream().cuda_stream

    def outputs():
        return (torch.empty((B, k), dtype=torch.int64, device="cuda"), torch.empty((B, k), dtype=torch.float32, device="cuda"),
                torch.empty((B,), dtype=torch.int32, device="cuda"))

    o, o2 = outputs(), outputs()
    targets = torch.empty((B, d), dtype=torch.float32, device="cuda")
    valid = torch.empty((B,), dtype=torch.int32, device="cuda")
    head = {"rows": n, "dims": d, "metric": "cosine", "batch": B, "k": k, "steps": a.steps, "warmup": a.warmup,
            "engine": sp.scan_engine()}
    lines = []
    for L in a.lists:
        for draw in ("uniform", "popular"):
            ids = torch.randint(0, n if draw == "uniform" else max(1, n // 100), (B * L,), generator=gen, device="cuda")
            w = torch.randn((B * L,), generator=gen, device="cuda")
            off = (torch.arange(B + 1, dtype=torch.int64, device="cuda") * L).contiguous()
            rec = dict(head, list_len=L, draw=draw, row_copy_bytes=B * L * d * 4)
            rec["knn_profile_device"] = timed(lambda: sp.knn_profile_device(k, ids, off, w, *o, stream=st), a.warmup, a.steps)
            rec["combine"] = timed(lambda: sp.combine_rows_device(ids, off, w, targets, valid, stream=st), a.warmup, a.steps)
            rec["combine"]["gbytes_per_s"] = round(B * L * d * 4 / rec["combine"]["ms_median"] / 1e6, 1)
            rec["floor"] = timed(lambda: sp.knn_except_device(targets, k, ids, off, *o2, stream=st), a.warmup, a.steps)
            rec["same_bytes"] = bool(torch.equal(o2[0], o[0]) and torch.equal(o2[1], o[1]) and torch.equal(o2[2], o[2]))
            rows = torch.empty((B * L, d), dtype=torch.float32, device="cuda")
            rvalid = torch.empty((B * L,), dtype=torch.int32, device="cuda")
            t2 = torch.empty((B, 1, d), dtype=torch.float32, device="cuda")

            def replaced():
                sp.get_by_ids_device(ids, rows, rvalid, stream=st)
                torch.bmm(w.view(B, 1, L), rows.view(B, L, d), out=t2)
                sp.knn_except_device(t2.view(B, d), k, ids, off, *o2, stream=st)

            rec["replaced"] = timed(replaced, a.warmup, a.steps)
            del rows, rvalid
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    sp.drop()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
