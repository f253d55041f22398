"""Measures the predicate search on stored columns (ehx_knn_where_device) on one MI355X against the workflow it replaces:
one JSON line per point, appended to --out (default profiles/where_bench.jsonl).

One flat cosine space of --rows x --dims filled by fill_synthetic, --batch device-resident queries, k = --k.  Two stored
columns: column 0 holds row % 2, column 1 a seeded random 32-bit value.  Predicate p of P is ONE equality and ONE range over
the two columns — column 0 == p % 2 AND column 1 inside a window of 2 * share * 2^32 values whose start moves with p — so it
allows about `share` of the rows; P in --preds, share in --shares, query i under predicate i % P.  Three timings per point
(HIP events around each call, median / min / max of --steps after --warmup):
  where      knn_where_device: the bitmaps built on the device from the columns
  resident   knn_masked_multi_device on the SAME table (numpy's bitmaps of the predicates) already resident on the device —
             the reference point: the where call is expected to differ from it by the build kernel's time minus the table's
             device-to-device copy
  host       knn_masked_multi from host bitmaps (packed words): the workflow this replaces, P * rows / 8 bytes uploaded per
             call (wall clock of the whole call; the resolution of the predicate on the host is NOT included)
The where call's outputs are asserted byte-equal to the resident-table call's before anything is timed.  The build kernel alone
(the hook ehx_test_where_build_ms: --build-reps launches back to back between two events) is reported with its algorithmic
traffic, 4 * 2 * rows bytes in and P * rows / 8 out, as bytes per second and as a share of --hbm-gbs."""
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
from embeddinghub_amd.space import marshal_preds  # noqa: E402


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


def predicates(P, share):
    width = min(int(2 * share * 2 ** 32), 2 ** 32)
    out = []
    for p in range(P):
        lo = (p * 0x9E3779B1) % (2 ** 32 - width + 1)
        out.append([(0, p % 2, p % 2), (1, lo, lo + width - 1)])
    return out


def truth_words(preds, c0, c1):
    """numpy's bitmaps of the predicates, packed: u32 [P, ceil(n / 32)]"""
    n = len(c0)
    v1 = c1.astype(np.uint64)
    tab = np.stack([(c0 == p[0][1]) & (v1 >= p[1][1]) & (v1 <= p[1][2]) for p in preds])
    bits = np.zeros((len(preds), (n + 31) // 32 * 32), dtype=np.uint8)
    bits[:, :n] = tab
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little").view("<u4").astype(np.uint32)), tab.sum(axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--preds", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--shares", type=float, nargs="+", default=[0.5, 0.1, 0.001])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--build-reps", type=int, default=50)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM bandwidth the build kernel's rate is stated against")
    ap.add_argument("--out", default=os.path.join("profiles", "where_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    f = open(args.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    raw = C.CDLL(_lib.LIB_PATH)
    raw.ehx_test_where_build_ms.restype = C.c_int
    n, d, nq, k = args.rows, args.dims, args.batch, args.k
    sp = ehx.Space.unique("bench-where", d, metric=ehx.METRIC_COSINE, initial_capacity=n)
    sp.fill_synthetic(ehx.SEED_CORPUS, 0, n, True)
    c0 = (np.arange(n) % 2).astype(np.uint32)
    c1 = np.random.default_rng(11).integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    sp.column_load_device(0, 0, u32(c0))
    sp.column_load_device(1, 0, u32(c1))
    dq = torch.empty((nq, d), dtype=torch.float32, device="cuda")
    dq.normal_()
    hq = dq.cpu().numpy()
    for P in args.preds:
        of = (np.arange(nq) % P).astype(np.uint32)
        dof = u32(of)
        for share in args.shares:
            preds = predicates(P, share)
            words, allowed = truth_words(preds, c0, c1)
            dm = u32(words)
            o_w, o_r = outs(nq, k), outs(nq, k)
            where = lambda: sp.knn_where_device(dq, k, preds, dof, *o_w)  # noqa: E731
            resident = lambda: sp.knn_masked_multi_device(dq, k, dm, P, n, dof, *o_r)  # noqa: E731
            host = lambda: sp.knn_masked_multi(hq, k, words, of, n_bits=n)  # noqa: E731
            where()
            resident()
            assert same(o_w, o_r), "the where call differs from the resident-table call (P=%d share=%g)" % (P, share)
            for _ in range(args.warmup):
                where()
                resident()
                host()
            tw, tr, th = [], [], []
            for _ in range(args.steps):
                tw.append(event_ms(where))
                tr.append(event_ms(resident))
                th.append(wall_ms(host))
            table, n_preds = marshal_preds(preds)
            ms, got_n = C.c_float(0), C.c_uint64(0)
            rc = raw.ehx_test_where_build_ms(sp._h, table, C.c_uint32(n_preds), C.c_uint32(args.build_reps), C.byref(ms),
                                             C.byref(got_n))
            assert rc == 0 and got_n.value == n, rc
            traffic = 4 * 2 * n + P * n // 8
            gbs = traffic / (ms.value * 1e-3) / 1e9 if ms.value > 0 else None
            emit({"rows": n, "dims": d, "batch": nq, "k": k, "preds": P, "share": share,
                  "allowed_min": int(allowed.min()), "allowed_max": int(allowed.max()), "byte_equal": True,
                  "where": med(tw), "resident": med(tr), "host": med(th),
                  "where_minus_resident_ms": round(statistics.median(tw) - statistics.median(tr), 4),
                  "table_bytes": int(words.nbytes),
                  "build": {"ms": round(ms.value, 5), "reps": args.build_reps, "algorithmic_bytes": traffic,
                            "gb_per_s": None if gbs is None else round(gbs, 1),
                            "share_of_hbm": None if gbs is None else round(gbs / args.hbm_gbs, 4), "hbm_gb_per_s": args.hbm_gbs}})
    sp.drop()


if __name__ == "__main__":
    main()
