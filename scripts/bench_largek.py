"""Measures flat kNN at large k (ehx_knn_device, EHX_MAX_K < k <= 256: the large-k scan route) on one MI355X
against ANOTHER build of the library — the parent commit's, given as --parent-lib — in the same session.

One flat space of --rows x --dims (fill_synthetic, normalised rows), --batch device-resident queries.  Every figure is the
median of --steps timed batches (HIP events around ONE call each, after --warmup calls), with min / max.  The library and
the knobs (EHX_LIB, EHX_LARGEK, EHX_LARGEK_GROWTH) are read once per process, so every configuration runs in a fresh child
process of this script (--worker), parent and new alternating, --repeats times each:
  columns   k in --ks at the full batch, parent and new (growth 4); k > 48 once more for the new library at every other
            growth of --growths
  gate      k = 100 at every batch size of --gate-batches, the new library with EHX_LARGEK=0 and with EHX_LARGEK=1 and the
            batch-size gate opened (EHX_LARGEK_MIN_QUERIES=1): where the route's crossover against the paged pass lies
For the route the worker also records, per call: scan passes, the share of queries handed to the exhaustive pass, the rows
re-ranked per query (n_dist beyond queries x rows).  One JSON line per (configuration, k, batch)."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def worker(a):
    import numpy as np
    import torch
    import embeddinghub_amd as ehx
    from embeddinghub_amd import _lib
    L = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    has_hook = hasattr(raw, "ehx_test_largek_counters")

    def counters(sp):
        out = (C.c_uint64 * 5)()
        if has_hook:
            raw.ehx_test_largek_counters(sp._h, out)
        return np.array(list(out), dtype=np.int64)   # on the route, handed on, overflowed, scan passes, calls

    metric = {"cosine": ehx.METRIC_COSINE, "l2": ehx.METRIC_L2SQ}[a.metric]
    sp = ehx.Space.unique("bench-largek", a.dims, metric=metric, initial_capacity=a.rows)
    sp.fill_synthetic(ehx.SEED_CORPUS, 0, a.rows, True)
    st = torch.cuda.current_stream().cuda_stream
    qmax = max(b for _, b in a.points)
    q = torch.empty((qmax, a.dims), dtype=torch.float32, device="cuda")
    _lib.check(L.ehx_gen_rows_device(C.c_void_p(st), ehx.SEED_QUERY, 0, qmax, a.dims, 1, C.c_void_p(q.data_ptr())))
    head = {"label": a.label, "lib": os.path.basename(_lib.LIB_PATH), "largek": os.environ.get("EHX_LARGEK", "1"), "min_queries": int(os.environ.get("EHX_LARGEK_MIN_QUERIES", "64")),
            "growth": int(os.environ.get("EHX_LARGEK_GROWTH", "4")), "rows": a.rows, "dims": a.dims, "metric": a.metric,
            "steps": a.steps, "warmup": a.warmup, "engine": sp.scan_engine()}
    for k, B in a.points:
        o_ids = torch.empty((B, k), dtype=torch.int64, device="cuda")
        o_dist = torch.empty((B, k), dtype=torch.float32, device="cuda")
        o_cnt = torch.empty((B,), dtype=torch.int32, device="cuda")
        qb = q[:B]

        def call():
            sp.knn_device(qb, k, o_ids, o_dist, o_cnt, stream=st)
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        c0, s0 = counters(sp), sp.stats()
        ms = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        dc, s1 = counters(sp) - c0, sp.stats()
        rec = dict(head, k=k, batch=B, ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4),
                   ms_max=round(max(ms), 4), exhaustive_queries_per_call=(s1["n_exhaustive"] - s0["n_exhaustive"]) / a.steps,
                   ids_checksum=int(o_ids.sum().item()), dist_checksum=float(o_dist.double().sum().item()))
        if dc[4]:
            calls = int(dc[4])
            rec.update(route="largek", passes_per_call=round(int(dc[3]) / calls, 3),
                       handed_on_share=round(int(dc[1]) / (calls * B), 5), overflowed_per_call=round(int(dc[2]) / calls, 3),
                       reranked_rows_per_query=round((s1["n_dist"] - s0["n_dist"]) / (a.steps * B) - a.rows, 1))
        else:
            rec.update(route="paged" if k > 48 else "chain")
        print(json.dumps(rec), flush=True)
    sp.drop()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--metric", default="cosine", choices=["cosine", "l2"])
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--ks", type=int, nargs="*", default=[10, 48, 49, 100, 256])
    ap.add_argument("--growths", type=int, nargs="*", default=[2, 4, 8, 16])
    ap.add_argument("--gate-batches", type=int, nargs="*", default=[16, 32, 64, 128])
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--parent-lib", default="", help="the parent commit's libehx.so (the yardstick); none: new library only")
    ap.add_argument("--child-timeout", type=int, default=420)
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--points", default="", help="worker: k:batch,k:batch,...")
    a = ap.parse_args()
    if a.worker:
        a.points = [tuple(int(v) for v in p.split(":")) for p in a.points.split(",")]
        return worker(a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def child(label, points, lib=None, **env):
        e = dict(os.environ)
        for name in ("EHX_LIB", "EHX_LARGEK", "EHX_LARGEK_GROWTH", "EHX_LARGEK_MIN_QUERIES"):
            e.pop(name, None)
        if lib:
            e["EHX_LIB"] = lib
        e.update({k: str(v) for k, v in env.items()})
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--label", label, "--rows", str(a.rows), "--dims",
               str(a.dims), "--metric", a.metric, "--warmup", str(a.warmup), "--steps", str(a.steps), "--points",
               ",".join("%d:%d" % p for p in points)]
        r = subprocess.run(cmd, env=e, cwd=ROOT, timeout=a.child_timeout, stdout=subprocess.PIPE, text=True)
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                if a.out:   # (as they come: a later worker's failure loses nothing)
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
        if r.returncode != 0:   # (a fault, an abort or a time limit: nothing more is started on the device)
            raise SystemExit("worker %s ended with status %d" % (label, r.returncode))

    cols = [(k, a.batch) for k in a.ks]
    for rep in range(a.repeats if cols else 0):
        if a.parent_lib:
            child("parent r%d" % rep, cols, lib=os.path.abspath(a.parent_lib))
        child("new r%d" % rep, cols)
    big = [(k, a.batch) for k in a.ks if k > 48]
    for g in a.growths:
        if g != 4 and big:
            child("new g%d" % g, big, EHX_LARGEK_GROWTH=g)
    gate = [(100, b) for b in a.gate_batches]
    if gate:
        child("gate largek=0", gate, EHX_LARGEK=0)
        child("gate largek=1 min_queries=1", gate, EHX_LARGEK=1, EHX_LARGEK_MIN_QUERIES=1)


if __name__ == "__main__":
    main()
