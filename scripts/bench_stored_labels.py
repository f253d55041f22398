"""Measures the label searches on STORED columns (ehx_knn_by_label_device, ehx_knn_grouped_by_label_device) on one MI355X
against the column forms given the same column (ehx_knn_labeled_device, ehx_knn_grouped_labeled_device), and the cost of the
column index: one JSON line per point, appended to --out (default profiles/stored_labels_bench.jsonl).

Search legs (--legs s): one flat cosine space of --rows x --dims filled by fill_synthetic, --batch device-resident queries,
k = --k; T equal tenants (row r on tenant r % T), T in --tenants, the batch naming min(T, batch) of them.  The stored form
with a FRESH index and the column form alternate A B A B ... after --warmup rounds (HIP events around each call); the A leg
is reported as two interleaved halves, whose medians' difference is the spread a B - A difference is judged against.  The
outputs of the two forms are checked byte for byte at the timed size.  The same pair for the grouped searches (group of
row r: r // 4, per_group 1).
Build legs (--legs b): spaces of --build-rows x --build-dims; the index build alone (a relabel of one row by key leaves it
stale, the next search of ONE query rebuilds it; the search itself is timed on the fresh index and subtracted) for a
16-tenant column (one digit pass) and a random 32-bit column (four passes); and the every-call-stale case: one
set_batch_cols append of 8192 rows between searches of --batch queries.
Kernel times and bytes per pass come from a rocprofv3 --kernel-trace --stats run of `--legs b` of its own, not from here."""
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


def u32(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32), device="cuda")


def med(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def abab(a, b, warmup, steps):
    for _ in range(warmup):
        a()
        b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(steps):
        ta.append(event_ms(a))
        tb.append(event_ms(b))
    a0, a1 = ta[0::2], ta[1::2]
    spread = abs(statistics.median(a0) - statistics.median(a1)) if a1 else None
    return med(ta), med(tb), None if spread is None else round(spread, 4)


def col_counters(raw, sp, col):
    out = (C.c_uint64 * 3)()
    raw.ehx_test_column_counters(sp._h, C.c_uint32(col), out)
    return list(out)


def outs(nq, k):
    return (torch.empty((nq, k), dtype=torch.int64, device="cuda"), torch.empty((nq, k), dtype=torch.float32, device="cuda"),
            torch.empty((nq,), dtype=torch.int32, device="cuda"))


def same(x, y):
    torch.cuda.synchronize()
    return all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(x, y))


def search_legs(args, emit):
    raw = C.CDLL(_lib.LIB_PATH)
    n, d, nq, k = args.rows, args.dims, args.batch, args.k
    sp = ehx.Space.unique("bench-stored", d, metric=ehx.METRIC_COSINE, initial_capacity=n)
    sp.fill_synthetic(ehx.SEED_CORPUS, 0, n, True)
    dq = torch.empty((nq, d), dtype=torch.float32, device="cuda")
    dq.normal_()
    groups = u32(np.arange(n, dtype=np.uint32) // 4)
    sp.column_load_device(0, 0, groups)
    for T in args.tenants:
        col = u32(np.arange(n, dtype=np.uint32) % T)
        sp.column_load_device(1, 0, col)
        want = u32((np.arange(nq, dtype=np.uint32) * 7919) % T)
        o_a, o_b = outs(nq, k), outs(nq, k)
        stored = lambda: sp.knn_by_label_device(dq, k, 1, want, *o_a)  # noqa: E731
        column = lambda: sp.knn_labeled_device(dq, k, col, n, want, *o_b)  # noqa: E731
        stored()
        c0 = col_counters(raw, sp, 1)
        a, b, spread = abab(stored, column, args.warmup, args.steps)
        c1 = col_counters(raw, sp, 1)
        emit({"leg": "knn", "rows": n, "dims": d, "batch": nq, "k": k, "tenants": T, "stored": a, "column": b,
              "a_spread_ms": spread, "byte_equal": same(o_a, o_b), "index_builds_while_timed": c1[0] - c0[0]})
        g_a, g_b = outs(nq, k), outs(nq, k)
        gstored = lambda: sp.knn_grouped_by_label_device(dq, k, 0, 1, want, *g_a, per_group=1)  # noqa: E731
        gcolumn = lambda: sp.knn_grouped_labeled_device(dq, k, groups, col, n, want, *g_b, per_group=1)  # noqa: E731
        a, b, spread = abab(gstored, gcolumn, args.warmup, args.steps)
        emit({"leg": "grouped", "rows": n, "dims": d, "batch": nq, "k": k, "tenants": T, "stored": a, "column": b,
              "a_spread_ms": spread, "byte_equal": same(g_a, g_b)})
    sp.drop()


def build_legs(args, emit):
    raw = C.CDLL(_lib.LIB_PATH)
    d, k = args.build_dims, args.k
    for n in args.build_rows:
        sp = ehx.Space.unique("bench-build", d, metric=ehx.METRIC_COSINE, initial_capacity=n + 64 * 8192)
        sp.fill_synthetic(ehx.SEED_CORPUS, 0, n, True)
        q1 = torch.randn((1, d), dtype=torch.float32, device="cuda")
        o1 = outs(1, k)
        w1 = u32([3])
        rng = np.random.default_rng(1)
        for name, colv in (("16_tenants", np.arange(n, dtype=np.uint32) % 16),
                           ("random32", rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32))):
            sp.column_load_device(0, 0, u32(colv))
            search = lambda: sp.knn_by_label_device(q1, k, 0, w1, *o1)  # noqa: E731
            search()
            fresh = med([event_ms(search) for _ in range(args.steps)])
            stale = []
            for i in range(args.steps):
                sp.column_set(0, ["%d" % i], [int(colv[i])])   # the same value: the generation moves, the answer does not
                stale.append(event_ms(search))
            c = col_counters(raw, sp, 0)
            emit({"leg": "build", "rows": n, "dims": d, "column": name, "digit_passes": c[2], "search_fresh": fresh,
                  "search_stale": med(stale), "build_ms_median": round(statistics.median(stale) - fresh["ms_median"], 4)})
        # every call stale: an append of 8192 labelled rows between searches of a whole batch
        nq = args.batch
        dq = torch.randn((nq, d), dtype=torch.float32, device="cuda")
        want = u32(np.arange(nq, dtype=np.uint32) % 16)
        ob = outs(nq, k)
        sp.column_load_device(0, 0, u32(np.arange(n, dtype=np.uint32) % 16))
        batch = lambda: sp.knn_by_label_device(dq, k, 0, want, *ob)  # noqa: E731
        batch()
        fresh = med([event_ms(batch) for _ in range(args.steps)])
        rows = np.random.default_rng(2).standard_normal((8192, d)).astype(np.float32)
        labels = (np.arange(8192, dtype=np.uint32) % 16)
        stale, write = [], []
        for i in range(min(args.steps, 32)):
            t0 = time.perf_counter()
            sp.set_batch_cols(["a%d_%d" % (i, j) for j in range(8192)], rows, {0: labels})
            write.append((time.perf_counter() - t0) * 1e3)
            stale.append(event_ms(batch))
        emit({"leg": "append_between_searches", "rows": n, "dims": d, "batch": nq, "appended": 8192, "search_fresh": fresh,
              "search_stale": med(stale), "set_batch_cols_host_ms": med(write)})
        sp.drop()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--tenants", type=int, nargs="+", default=[16, 1024, 4096])
    ap.add_argument("--build-rows", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--build-dims", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--legs", default="sb")
    ap.add_argument("--out", default=os.path.join("profiles", "stored_labels_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    f = open(args.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    if "s" in args.legs:
        search_legs(args, emit)
    if "b" in args.legs:
        build_legs(args, emit)


if __name__ == "__main__":
    main()
