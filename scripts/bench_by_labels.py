"""Measures the multi-probe label search (ehx_knn_by_labels_device, k_probe.hip) as an IVF search on one MI355X against the
composed route it replaces and the exact floor: one JSON line per n_probe, appended to --out (default
profiles/by_labels_bench.jsonl).

One flat cosine space of --rows x --dims filled by fill_synthetic; --centroids centroids from kmeans_device (seeded from
stored rows, --iters Lloyd steps), the labels loaded as column 0; the centroids set into a second small space, whose
knn_device(k = n_probe) gives every query's probe labels and — its count — want_count.  --batch device-resident queries,
k = --k, n_probe in --probes.
  probe      knn_by_labels_device
  composed   the queries replicated n_probe times, knn_by_label_device on the replicas, ehx_merge_topk_device
  exact      knn_device over all rows (once per run: the recall's truth and the floor)
probe and composed alternate A B A B ... after --warmup rounds, HIP events around each call; the A leg is reported as two
interleaved halves, whose medians' difference is the spread a B - A difference is judged against.  Their outputs must be
byte-equal or the script fails.  recall@k is against knn_device's ids.  row_bytes_staged comes from the search's own
counters (rows staged x dims x element size); over the CALL's time it is a lower bound of the kernel's rate — the kernel's
own time comes from a rocprofv3 --kernel-trace --stats run of `--only probe`, not from here."""
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
from embeddinghub_amd.space import _ptr, check  # noqa: E402


def med(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def outs(nq, k):
    return (torch.empty((nq, k), dtype=torch.int64, device="cuda"), torch.empty((nq, k), dtype=torch.float32, device="cuda"),
            torch.empty((nq,), dtype=torch.int32, device="cuda"))


def same(x, y):
    torch.cuda.synchronize()
    return all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(x, y))


def probe_counters(raw, sp):
    out = (C.c_uint64 * 4)()
    raw.ehx_test_probe_counters(sp._h, out)
    return list(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--centroids", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--probes", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", choices=["probe"], default=None, help="the probe call alone, --steps times: for a profiler run")
    ap.add_argument("--out", default=os.path.join("profiles", "by_labels_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    raw = C.CDLL(_lib.LIB_PATH)
    n, d, nc, nq, k = args.rows, args.dims, args.centroids, args.batch, args.k
    sp = ehx.Space.unique("bench-probe", d, metric=ehx.METRIC_COSINE, initial_capacity=n)
    sp.fill_synthetic(ehx.SEED_CORPUS, 0, n, True)
    g = torch.Generator(device="cuda").manual_seed(1)
    seeds = torch.randperm(n, generator=g, device="cuda")[:nc].contiguous()
    cent = torch.empty((nc, d), dtype=torch.float32, device="cuda")
    sp.get_by_ids_device(seeds, cent, torch.empty((nc,), dtype=torch.int32, device="cuda"))
    labels = torch.empty((n,), dtype=torch.int32, device="cuda")
    sp.kmeans_device(cent, args.iters, labels)
    sp.column_load_device(0, 0, labels)
    sizes = torch.bincount(labels.long(), minlength=nc)
    cs = ehx.Space.unique("bench-probe-centroids", d, metric=ehx.METRIC_COSINE, initial_capacity=nc)
    cs.set_batch_device(["%d" % i for i in range(nc)], cent)   # row id c is label c
    dq = torch.empty((nq, d), dtype=torch.float32, device="cuda").normal_(generator=g)
    truth = outs(nq, k)
    exact = lambda: sp.knn_device(dq, k, *truth)  # noqa: E731
    exact()
    t_exact = med([event_ms(exact) for _ in range(args.steps)])
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    f = open(args.out, "a")
    for n_probe in args.probes:
        p_ids, p_dist, p_cnt = outs(nq, n_probe)
        cs.knn_device(dq, n_probe, p_ids, p_dist, p_cnt)
        torch.cuda.synchronize()
        want = p_ids.to(torch.int32).contiguous()           # [nq, n_probe]; entries behind the count are never read
        assert bool((p_cnt == n_probe).all())               # (the composed route has no count to honour)
        o_a, o_b = outs(nq, k), outs(nq, k)
        rq = dq.repeat(n_probe, 1).contiguous()             # list-major replicas: [n_probe][nq]
        rw = want.t().contiguous().view(-1)
        r_out = outs(nq * n_probe, k)

        def probe():
            sp.knn_by_labels_device(dq, k, 0, want, *o_a, d_want_count=p_cnt)

        def composed():
            sp.knn_by_label_device(rq, k, 0, rw, *r_out)
            check(sp._L.ehx_merge_topk_device(None, nq, k, n_probe, _ptr(r_out[0]), _ptr(r_out[1]), _ptr(r_out[2]),
                                              _ptr(o_b[0]), _ptr(o_b[1]), _ptr(o_b[2])))

        if args.only == "probe":
            for _ in range(args.warmup + args.steps):
                probe()
            torch.cuda.synchronize()
            continue
        for _ in range(args.warmup):
            probe()
            composed()
        torch.cuda.synchronize()
        c0 = probe_counters(raw, sp)
        ta, tb = [], []
        for _ in range(args.steps):
            ta.append(event_ms(probe))
            tb.append(event_ms(composed))
        c1 = probe_counters(raw, sp)
        if not same(o_a, o_b):
            raise SystemExit("n_probe = %d: the two label routes differ" % n_probe)
        staged = (c1[2] - c0[2]) // args.steps * d * 4
        a = med(ta)
        hit = (o_a[0].unsqueeze(2) == truth[0].unsqueeze(1)).any(dim=2).float().sum(dim=1) / k
        rec = {"rows": n, "dims": d, "centroids": nc, "kmeans_iters": args.iters, "batch": nq, "k": k, "n_probe": n_probe,
               "list_rows_min_mean_max": [int(sizes.min()), round(float(sizes.float().mean()), 1), int(sizes.max())],
               "probe": a, "composed": med(tb), "exact_knn_device": t_exact,
               "a_spread_ms": round(abs(statistics.median(ta[0::2]) - statistics.median(ta[1::2])), 4),
               "byte_equal": True, "work_items_per_call": (c1[1] - c0[1]) // args.steps,
               "pairs_per_call": (c1[3] - c0[3]) // args.steps, "row_bytes_staged_per_call": staged,
               "row_bytes_staged_per_s_over_call_time": round(staged / (a["ms_median"] * 1e-3), 1),
               "row_bytes_composed_per_call": (c1[3] - c0[3]) // args.steps * d * 4,
               "recall_at_k": round(float(hit.mean()), 4)}
        line = json.dumps(rec)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()
    sp.drop()
    cs.drop()


if __name__ == "__main__":
    main()
