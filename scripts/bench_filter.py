"""Measures the Boolean filter search on stored columns (ehx_knn_filter_device) on one MI355X against its floor and against
the workflow it replaces, and the kernel that builds its bitmaps alone: one JSON line per point, appended to --out (default
profiles/filter_bench.jsonl).

One flat cosine space of --rows x --dims filled by fill_synthetic, --batch device-resident queries, k = --k.  Two stored
columns: column 0 holds a seeded random group id below --groups, column 1 a seeded random 32-bit value.

1. Calls ("what": "call").  F filters (--filters), query i under filter i % F, two shapes per F and share:
     in   ONE clause: column 0 IN a set of 32 group ids that moves with the filter, AND column 1 inside a window sized so that
          the filter allows about `share` of the rows;
     or   TWO clauses ORed: column 0 in one half of the group ids AND column 1 inside a window — once per half, each
          window sized so that its clause allows share / 2.
   Three timings per point (HIP events around each call, median / min / max of --steps after --warmup):
     filter     knn_filter_device: the bitmaps built on the device from the columns
     resident   knn_masked_multi_device on the SAME table (numpy's bitmaps of the filters) already resident on the device —
                the floor: only the build differs
     host       knn_masked_multi from host bitmaps (packed words): what a caller must do today for an OR or an IN-list (wall
                clock of the whole call; the resolution of the filter on the host is NOT included)
   The filter call's outputs are asserted byte-equal to the resident-table call's before anything is timed.
2. The build kernel alone ("what": "build"; the hooks ehx_test_filter_build_ms / ehx_test_where_build_ms: --build-reps
   launches back to back between two events), with its algorithmic traffic — 4 bytes per row and column named, F / 8 bytes per
   row out — as bytes per second and as a share of --hbm-gbs:
     plain      F one-clause filters without IN terms (bench_where.py's predicates) against where_bitmaps_kernel on the same
                predicates: the cost of the generality
     clauses    ONE filter of C range clauses, C in --clauses: the cost per added clause
     in         ONE filter of one IN term, set lengths in --set-lengths: the cost per IN term and binary-search step
     shared     8 filters over the same 16 clauses against ("own") 8 filters of 16 clauses of their own: what evaluating a
                clause once saves"""
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
from embeddinghub_amd.space import marshal_filter_table, marshal_filters, marshal_preds  # noqa: E402


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


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def outs(nq, k):
    return (torch.empty((nq, k), dtype=torch.int64, device="cuda"), torch.empty((nq, k), dtype=torch.float32, device="cuda"),
            torch.empty((nq,), dtype=torch.int32, device="cuda"))


def same(x, y):
    torch.cuda.synchronize()
    return all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(x, y))


def window(width, salt):
    width = max(1, min(int(width), 2 ** 32))
    lo = (salt * 0x9E3779B1) % (2 ** 32 - width + 1)
    return lo, lo + width - 1


def filters_of(shape, F, share, groups):
    out = []
    for f in range(F):
        if shape == "in":   # 32 of `groups` ids AND a window: share = 32 / groups x width / 2^32
            ids = [(f * 7 + 3 * j) % groups for j in range(32)]
            assert len(set(ids)) == 32
            lo, hi = window(share * groups / 32 * 2 ** 32, f)
            out.append([[(0, "in", ids), (1, lo, hi)]])
        else:               # the halves of the group ids are disjoint: share = 2 x 1 / 2 x width / 2^32
            lo0, hi0 = window(share * 2 ** 32, 2 * f)
            lo1, hi1 = window(share * 2 ** 32, 2 * f + 1)
            out.append([[(0, 0, groups // 2 - 1), (1, lo0, hi0)], [(0, groups // 2, groups - 1), (1, lo1, hi1)]])
    return out


def term_truth(term, cols):
    v = cols[term[0]].astype(np.uint64)
    if isinstance(term[1], str):
        ok = np.isin(v, np.asarray(term[2], dtype=np.uint64))
    else:
        ok = (v >= term[1]) & (v <= term[2])
    return ~ok if len(term) == 4 and term[3] else ok


def truth_words(filters, cols):
    """numpy's bitmaps of the filters, packed: u32 [F, ceil(n / 32)]"""
    n = len(cols[0])
    tab = np.zeros((len(filters), n), dtype=bool)
    for f, flt in enumerate(filters):
        for clause in flt:
            ok = np.ones(n, dtype=bool)
            for term in clause:
                ok &= term_truth(term, cols)
            tab[f] |= ok
    bits = np.zeros((len(filters), (n + 31) // 32 * 32), dtype=np.uint8)
    bits[:, :n] = tab
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little").view("<u4").astype(np.uint32)), tab.sum(axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--filters", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--shares", type=float, nargs="+", default=[0.5, 0.001])
    ap.add_argument("--shapes", nargs="+", default=["in", "or"])
    ap.add_argument("--clauses", type=int, nargs="+", default=[1, 2, 8, 32, 128])
    ap.add_argument("--set-lengths", type=int, nargs="+", default=[1, 2, 4, 8, 32, 1024])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--build-reps", type=int, default=50)
    ap.add_argument("--skip-calls", action="store_true")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM bandwidth the build kernel's rate is stated against")
    ap.add_argument("--out", default=os.path.join("profiles", "filter_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    f = open(args.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    raw = C.CDLL(_lib.LIB_PATH)
    raw.ehx_test_filter_build_ms.restype = C.c_int
    raw.ehx_test_where_build_ms.restype = C.c_int
    n, d, nq, k = args.rows, args.dims, args.batch, args.k
    sp = ehx.Space.unique("bench-filter", d, metric=ehx.METRIC_COSINE, initial_capacity=n)
    sp.fill_synthetic(ehx.SEED_CORPUS, 0, n, True)
    rng = np.random.default_rng(11)
    cols = {0: rng.integers(0, args.groups, size=n).astype(np.uint32),
            1: rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)}
    sp.column_load_device(0, 0, u32(cols[0]))
    sp.column_load_device(1, 0, u32(cols[1]))
    base = {"rows": n, "dims": d, "batch": nq, "k": k}

    def build_ms(ft):
        ms, got_n = C.c_float(0), C.c_uint64(0)
        rc = raw.ehx_test_filter_build_ms(sp._h, C.byref(ft.struct), C.c_uint32(args.build_reps), C.byref(ms), C.byref(got_n))
        assert rc == 0 and got_n.value == n, rc
        return ms.value

    def rate(ms, n_cols, n_maps):
        traffic = 4 * n_cols * n + n_maps * n // 8
        gbs = traffic / (ms * 1e-3) / 1e9 if ms > 0 else None
        return {"ms": round(ms, 5), "reps": args.build_reps, "algorithmic_bytes": traffic,
                "gb_per_s": None if gbs is None else round(gbs, 1),
                "share_of_hbm": None if gbs is None else round(gbs / args.hbm_gbs, 4), "hbm_gb_per_s": args.hbm_gbs}

    # ---- 1. the calls ----
    if not args.skip_calls:
        dq = torch.empty((nq, d), dtype=torch.float32, device="cuda")
        dq.normal_()
        hq = dq.cpu().numpy()
        for F in args.filters:
            of = (np.arange(nq) % F).astype(np.uint32)
            dof = u32(of)
            for shape in args.shapes:
                for share in args.shares:
                    filters = filters_of(shape, F, share, args.groups)
                    ft = marshal_filters(filters)
                    words, allowed = truth_words(filters, cols)
                    dm = u32(words)
                    o_f, o_r = outs(nq, k), outs(nq, k)
                    call = lambda: sp.knn_filter_device(dq, k, ft, dof, *o_f)  # noqa: E731
                    resident = lambda: sp.knn_masked_multi_device(dq, k, dm, F, n, dof, *o_r)  # noqa: E731
                    host = lambda: sp.knn_masked_multi(hq, k, words, of, n_bits=n)  # noqa: E731
                    call()
                    resident()
                    assert same(o_f, o_r), "the filter call differs from the resident-table call (F=%d %s share=%g)" % (F, shape, share)
                    for _ in range(args.warmup):
                        call()
                        resident()
                        host()
                    tf, tr, th = [], [], []
                    for _ in range(args.steps):
                        tf.append(event_ms(call))
                        tr.append(event_ms(resident))
                        th.append(wall_ms(host))
                    emit(dict(base, what="call", filters=F, shape=shape, share=share, allowed_min=int(allowed.min()),
                              allowed_max=int(allowed.max()), byte_equal=True, filter=med(tf), resident=med(tr), host=med(th),
                              filter_minus_resident_ms=round(statistics.median(tf) - statistics.median(tr), 4),
                              table_bytes=int(words.nbytes), build=rate(build_ms(ft), 2, F)))

    # ---- 2. the build kernel alone ----
    for F in args.filters:   # plain conjunctions: against where_bitmaps_kernel on the same predicates
        preds = []
        for p in range(F):
            lo, hi = window(2 * 0.1 * 2 ** 32, p)
            preds.append([(0, 0, args.groups // 2 - 1), (1, lo, hi)])
        table, n_preds = marshal_preds(preds)
        ms, got_n = C.c_float(0), C.c_uint64(0)
        rc = raw.ehx_test_where_build_ms(sp._h, table, C.c_uint32(n_preds), C.c_uint32(args.build_reps), C.byref(ms), C.byref(got_n))
        assert rc == 0 and got_n.value == n, rc
        emit(dict(base, what="build", kind="plain", filters=F, clauses=F, filter_kernel=rate(build_ms(marshal_filters([[p] for p in preds])), 2, F),
                  where_kernel=rate(ms.value, 2, F)))
    for Cn in args.clauses:   # ONE filter of Cn range clauses over column 1
        clauses = [[(1,) + window(2 ** 32 / 256, j)] for j in range(Cn)]
        emit(dict(base, what="build", kind="clauses", filters=1, clauses=Cn, filter_kernel=rate(build_ms(marshal_filters([clauses])), 1, 1)))
    for L in args.set_lengths:   # ONE filter of one IN term over column 1
        vals = [int(v) for v in np.unique(np.concatenate([cols[1][:L // 2], rng.integers(0, 2 ** 32, size=2 * L + 2, dtype=np.uint64)]))[:L]]
        assert len(vals) == L
        emit(dict(base, what="build", kind="in", filters=1, clauses=1, set_length=L,
                  filter_kernel=rate(build_ms(marshal_filters([[[(1, "in", vals)]]])), 1, 1)))
    sixteen = [[(1,) + window(2 ** 32 / 256, j), (0, 0, args.groups // 2 - 1)] for j in range(16)]
    own = [[(1,) + window(2 ** 32 / 256, 16 * f + j), (0, 0, args.groups // 2 - 1)] for f in range(8) for j in range(16)]
    emit(dict(base, what="build", kind="shared", filters=8, clauses=16,
              filter_kernel=rate(build_ms(marshal_filter_table(sixteen, [(0, 16)] * 8)), 2, 8)))
    emit(dict(base, what="build", kind="own", filters=8, clauses=128,
              filter_kernel=rate(build_ms(marshal_filter_table(own, [(16 * f, 16) for f in range(8)])), 2, 8)))
    sp.drop()


if __name__ == "__main__":
    main()
