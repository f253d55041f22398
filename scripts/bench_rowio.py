"""Measures row I/O on one MI355X, in one process:

  ingest  --rows x --dims cosine rows in chunks of --chunk into a space reserved for them, F32 and F16 spaces: the host path
          (set_prepared: ehx_set_batch from pageable host floats, the code of every earlier revision) against
          ehx_set_batch_device from a resident fp32 tensor (F16 spaces: from a resident binary16 tensor as well), each on a
          fresh space, alternating host, device, host, device (--repeats rounds).  Keys are marshalled before the clock starts
          on both paths.  Per path and round: rows/s as median, min and max over the chunks behind the first (a host clock
          around one call, which returns after the rows are published), and the writers' stream's time per chunk split into
          the rows (staging + upload, or wait + scatter) and what follows (row statistics, scan copies): the test hook
          ehx_test_write_times.
  fill    wall time of ONE fill_synthetic of --fill-rows x --dims rows into a space reserved for them, F32 and F16, on a fresh
          space per repeat (--fill-repeats): the generator's lander and the tail it shares with the Sets.
  get     --get-rows rows of the last F32 space by a loop of get, by ONE get_batch, and by get_by_ids_device (HIP events
          around one call, median of --steps after --warmup): bytes read + written over time, beside 8 TB/s.

One JSON line per figure, appended to --out as well."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--chunk", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--fill-rows", type=int, default=1048576)
    ap.add_argument("--fill-repeats", type=int, default=3)
    ap.add_argument("--get-rows", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rowio_bench.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import embeddinghub_amd as ehx
    from embeddinghub_amd import _lib
    from embeddinghub_amd.space import marshal_keys
    L = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    raw.ehx_test_write_times.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(**rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    st = torch.cuda.current_stream().cuda_stream
    d32 = torch.empty((a.rows, a.dims), dtype=torch.float32, device="cuda")
    _lib.check(L.ehx_gen_rows_device(C.c_void_p(st), ehx.SEED_CORPUS, 0, a.rows, a.dims, 1, C.c_void_p(d32.data_ptr())))
    torch.cuda.synchronize()
    d16 = d32.half()
    h32 = d32.cpu().numpy()
    cuts = [(r0, min(r0 + a.chunk, a.rows)) for r0 in range(0, a.rows, a.chunk)]
    keys = ["k%d" % i for i in range(a.rows)]
    head = dict(rows=a.rows, dims=a.dims, chunk=a.chunk, metric="cosine", warmup_chunks=1)

    def ingest(path, dtype):
        sp = ehx.Space.unique("bench-rowio", a.dims, metric=ehx.METRIC_COSINE, dtype=dtype, initial_capacity=a.rows)
        out2 = (C.c_float * 2)()
        raw.ehx_test_write_times(sp._h, out2)   # (arms the events)
        if path == "host":
            preps = [sp.prepare_batch(keys[r0:r1], h32[r0:r1]) for r0, r1 in cuts]
        else:
            src = d16 if path == "device_f16src" else d32
            code = _lib.DTYPE_F16 if path == "device_f16src" else _lib.DTYPE_F32
            preps = [marshal_keys(keys[r0:r1]) + (src[r0:r1].data_ptr(),) for r0, r1 in cuts]
        rate, up, derived = [], [], []
        for (r0, r1), p in zip(cuts, preps):
            t0 = time.perf_counter()
            if path == "host":
                sp.set_prepared(p)
            else:
                _lib.check(L.ehx_set_batch_device(sp._h, C.c_void_p(st), p[0], p[1], p[2], C.c_void_p(p[4]), code))
            dt = time.perf_counter() - t0
            if raw.ehx_test_write_times(sp._h, out2) == 0:
                up.append(out2[0])
                derived.append(out2[1])
            rate.append((r1 - r0) / dt)
        assert len(sp) == a.rows
        rate, up, derived = rate[1:], up[1:], derived[1:]
        return sp, dict(rows_per_s_median=round(statistics.median(rate)), rows_per_s_min=round(min(rate)),
                        rows_per_s_max=round(max(rate)), rows_ms_median=round(statistics.median(up), 4),
                        derived_ms_median=round(statistics.median(derived), 4), engine=sp.scan_engine())

    kept = None
    for dtype, name in ((ehx.DTYPE_F32, "F32"), (ehx.DTYPE_F16, "F16")):
        paths = ["host", "device"] + (["device_f16src"] if dtype == ehx.DTYPE_F16 else [])
        for rep in range(a.repeats):
            for path in paths:
                sp, rec = ingest(path, dtype)
                emit(leg="ingest", space=name, path=path, round=rep, **head, **rec)
                if dtype == ehx.DTYPE_F32 and path == "device" and kept is None:
                    kept = sp
                else:
                    sp.drop()

    # ---- fill ----
    for dtype, name in ((ehx.DTYPE_F32, "F32"), (ehx.DTYPE_F16, "F16")):
        secs = []
        for _ in range(a.fill_repeats):
            sp = ehx.Space.unique("bench-fill", a.dims, metric=ehx.METRIC_COSINE, dtype=dtype, initial_capacity=a.fill_rows)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sp.fill_synthetic(ehx.SEED_CORPUS, 0, a.fill_rows, True)
            secs.append(time.perf_counter() - t0)
            assert len(sp) == a.fill_rows
            sp.drop()
        emit(leg="fill", space=name, rows=a.fill_rows, dims=a.dims, metric="cosine", fill_s_median=round(statistics.median(secs), 5),
             fill_s_min=round(min(secs), 5), fill_s_max=round(max(secs), 5), rows_per_s_median=round(a.fill_rows / statistics.median(secs)))

    # ---- Gets ----
    sp = kept
    n = min(a.get_rows, a.rows)
    pick = np.random.default_rng(1).integers(0, a.rows, n)
    ask = [keys[i] for i in pick]
    t0 = time.perf_counter()
    loop = np.stack([sp.get(k) for k in ask])
    t_loop = time.perf_counter() - t0
    sp.get_batch(ask[:1024])   # (warm-up: the scratch)
    sp.get_batch(ask)
    t0 = time.perf_counter()
    got = sp.get_batch(ask)
    t_batch = time.perf_counter() - t0
    assert np.array_equal(got.view(np.uint32), loop.view(np.uint32))
    emit(leg="get", rows=n, dims=a.dims, loop_s=round(t_loop, 4), loop_rows_per_s=round(n / t_loop), get_batch_s=round(t_batch, 4),
         get_batch_rows_per_s=round(n / t_batch))
    d_ids = torch.from_numpy(pick.astype(np.int64)).cuda()
    d_out = torch.empty((n, a.dims), dtype=torch.float32, device="cuda")
    d_valid = torch.empty((n,), dtype=torch.int32, device="cuda")
    for _ in range(a.warmup):
        sp.get_by_ids_device(d_ids, d_out, d_valid, stream=st)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sp.get_by_ids_device(d_ids, d_out, d_valid, stream=st)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), loop.view(np.uint32))
    moved = n * (2 * a.dims * 4 + 8 + 4)   # every row read and written once, its id, its flag
    med = statistics.median(ms)
    emit(leg="get_by_ids_device", rows=n, dims=a.dims, ms_median=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
         bytes_moved=moved, bytes_per_s=round(moved / (med * 1e-3)), share_of_8TBps=round(moved / (med * 1e-3) / HBM_BYTES_PER_S, 4))
    sp.drop()


if __name__ == "__main__":
    main()
