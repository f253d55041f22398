"""Measures how evenly the eight XCDs finish the int8 scan's last pass (csrc/ehx_balance.h), in one process.

Every workgroup of a long pass stamps wall_clock64() before its prologue and after its last flush; the stamps ride home
with the batch's verdict and the test hook ehx_test_i8_balance_read hands out those of the last batch's final pass.  On
--rows x --dims cosine rows (EHX-GAUSS-1, as bench.py fills them), --batch queries, k = 10, after --warmup batches, for each
of --batches batches (one caller; EHX_STATS_EVERY=1 so that every batch has a HIP-event scan window):

  finish_ms[8]   latest finish of every XCD's workgroups, from the earliest start of the pass
  pass_ms        latest finish - earliest start;  skew = (latest - mean of the eight) / pass_ms
  start_spread_us  latest - earliest of the XCDs' own earliest starts (one time base: microseconds, not an XCD's offset)
  scan_ms        the HIP-event window of the batch's whole scan phase (it must bracket the pass: pass_ms < scan_ms)
  tiles[8], rates[8], factors[8], table   the split the pass ran with, the batch's relative rates, the shape's factors

EHX_I8_BALANCE is read once per process: run once with it 0 (the skew of the uniform split = the gain a perfect split
could bring on that pass) and once with the default (what is left after balancing).  One JSON line per batch and a summary
line, appended to --out."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "logs", "i8_xcd_finish_skew.jsonl"))
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    os.environ.setdefault("EHX_STATS_EVERY", "1")
    import numpy as np
    import embeddinghub_amd as ehx
    from embeddinghub_amd import _lib

    raw = C.CDLL(_lib.LIB_PATH)
    raw.ehx_test_i8_balance_read.argtypes = [C.c_void_p] * 6
    raw.ehx_test_i8_balance_read.restype = C.c_int
    s = ehx.Space.unique("xcd-skew", args.dims, metric=ehx.METRIC_COSINE, initial_capacity=args.rows)
    s.fill_synthetic(ehx.SEED_CORPUS, 0, args.rows, True)
    assert s.scan_engine() == "i8"
    rng = np.random.default_rng(20250212)
    n_q = args.warmup + args.batches
    Q = rng.standard_normal((n_q, args.batch, args.dims)).astype(np.float32)
    Q /= np.linalg.norm(Q, axis=2, keepdims=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a")
    switch = os.environ.get("EHX_I8_BALANCE", "default")
    recs = []
    for i in range(n_q):
        s.knn(np.ascontiguousarray(Q[i]), args.k)
        info = np.zeros(8, dtype=np.uint64)
        bounds = np.zeros(257, dtype=np.uint32)
        stamps = np.zeros(1024, dtype=np.uint64)
        factors, rates = np.zeros(8), np.zeros(8)
        rc = raw.ehx_test_i8_balance_read(s._h, info.ctypes.data, bounds.ctypes.data, stamps.ctypes.data, factors.ctypes.data,
                                          rates.ctypes.data)
        assert rc == 0, (rc, _lib.load().ehx_last_error())
        _, grid, q_tiles, n_tiles, n_chunks, tile0, table, khz = (int(v) for v in info)
        st = stamps[:2 * grid].reshape(grid, 2).astype(np.int64)
        xcd = np.arange(grid) & 7
        t0 = int(st[:, 0].min())
        to_ms = 1.0 / khz
        finish = np.array([(st[xcd == x, 1].max() - t0) * to_ms for x in range(8)])
        first = np.array([(st[xcd == x, 0].min() - t0) * to_ms for x in range(8)])
        pass_ms = float(finish.max())
        cpx = n_chunks // 8
        rec = {"what": "batch", "tag": args.tag, "EHX_I8_BALANCE": switch, "batch": i - args.warmup, "rows": args.rows,
               "dims": args.dims, "queries": args.batch, "tile0": tile0, "n_tiles": n_tiles, "n_chunks": n_chunks, "grid": grid,
               "table": table, "finish_ms": [round(float(v), 4) for v in finish], "pass_ms": round(pass_ms, 4),
               "skew": round(float((finish.max() - finish.mean()) / pass_ms), 5),
               "spread": round(float((finish.max() - finish.min()) / pass_ms), 5),
               "start_spread_us": round(float(first.max() - first.min()) * 1e3, 2),
               "scan_ms": round(float(s.stats()["last_scan_ms"]), 4),
               "tiles": [int(bounds[(x + 1) * cpx]) - int(bounds[x * cpx]) for x in range(8)],
               "rates": [round(float(v), 4) for v in rates], "factors": [round(float(v), 4) for v in factors]}
        if i >= args.warmup:
            recs.append(rec)
            out.write(json.dumps(rec) + "\n")
    summary = {"what": "summary", "tag": args.tag, "EHX_I8_BALANCE": switch, "rows": args.rows, "dims": args.dims,
               "queries": args.batch, "batches": len(recs), "table": recs[-1]["table"],
               "pass_ms_mean": round(float(np.mean([r["pass_ms"] for r in recs])), 4),
               "pass_ms_min": min(r["pass_ms"] for r in recs), "pass_ms_max": max(r["pass_ms"] for r in recs),
               "scan_ms_mean": round(float(np.mean([r["scan_ms"] for r in recs])), 4),
               "skew_mean": round(float(np.mean([r["skew"] for r in recs])), 5),
               "skew_min": min(r["skew"] for r in recs), "skew_max": max(r["skew"] for r in recs),
               "spread_mean": round(float(np.mean([r["spread"] for r in recs])), 5),
               "finish_ms_mean": [round(float(v), 4) for v in np.mean([r["finish_ms"] for r in recs], axis=0)],
               "start_spread_us_max": max(r["start_spread_us"] for r in recs),
               "pass_inside_scan_window": all(r["pass_ms"] < r["scan_ms"] for r in recs),
               "tiles_last": recs[-1]["tiles"], "factors_last": recs[-1]["factors"]}
    out.write(json.dumps(summary) + "\n")
    out.close()
    print(json.dumps(summary))
    s.drop()


if __name__ == "__main__":
    main()
