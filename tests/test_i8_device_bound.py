"""GPU: the int8 filter scan's copy, its lower bound and its hit path, checked on what the DEVICE wrote and collected.

Two test hooks (csrc/ehx_testhooks.cpp) read the scan copy back raw and run single launches of flat_scan_i8_kernel with a
search's arguments: the sample form (every lower bound of an eight-tile window) and collect passes under thresholds drawn
from those scores.  tests/i8_checks.py then applies, in float64 against the original rows and queries:
  C1 perm8 is a permutation per tile, the identity where the tile was not full when written
  C2 the codes and the stored steps / error bounds of rows and queries (|x^ - s xi| <= e)
  C3 rows the filter cannot bound, padding rows and unwritten tiles hold the never-alarm parameters
  C4 tile and lane-group extremes to the bit; ordered tiles: one |A| per group, groups in rank order
  C5 the kernel's score is the stated expression of the stored parameters and the exact integer dot product
  C6 u S + v never exceeds the true distance
  C7 a pass collects exactly the published rows at or below its thresholds, scores bit-equal to the dump's.
tests/test_i8_checks_cpu.py shows that each of them can fail."""
import ctypes as C

import numpy as np
import pytest

import i8_checks as ck
import i8_layout as L
from i8_model import _datasets, _true_distance

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402

f32 = np.float32
METRICS = {"l2": ehx.METRIC_L2SQ, "ip": ehx.METRIC_IP, "cosine": ehx.METRIC_COSINE}
N_ROWS = 9 * 256 + 168          # nine full tiles and a straddling tail
N_APPEND = 200                  # ... crossed by the append
CAP = 12 * 256

_RAW = []


def _raw():
    if not _RAW:
        lib = C.CDLL(_lib.LIB_PATH)
        lib.ehx_test_i8_array.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]
        lib.ehx_test_i8_array.restype = C.c_int
        lib.ehx_test_i8_pass.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 9
        lib.ehx_test_i8_pass.restype = C.c_int
        _RAW.append(lib)
    return _RAW[0]


def _ok(rc):
    assert rc == 0, (rc, _lib.load().ehx_last_error())


def _array(s, which, n, dtype):
    out = np.zeros(n, dtype=dtype)
    _ok(_raw().ehx_test_i8_array(s._h, which, 0, n, out.ctypes.data))
    return out


def snapshot(s):
    ld8 = int(_array(s, 6, 1, np.uint64)[0])
    cap = int(_array(s, 7, 1, np.uint64)[0])
    T = cap // 256
    return ck.Snapshot(_array(s, 0, cap * ld8, np.int8), _array(s, 1, (cap + 512) * 4, f32), _array(s, 2, (T + 2) * 4, f32),
                       _array(s, 3, (T + 2) * 16, f32), _array(s, 4, cap, np.uint8), _array(s, 5, 2, np.uint64), ld8, cap)


def run_pass(s, Q, thr, tile0, n_tiles, ld8):
    """-> dict: dump (sample form) or pool (count, overflow, ids, scores), qparams, quv, q8 raw, q_rows, info"""
    nq = len(Q)
    q_rows = (nq + 255) // 256 * 256
    Qc = np.ascontiguousarray(Q, dtype=f32)
    qparams = np.zeros((nq, 4), dtype=f32)
    quv = np.zeros((nq, 2), dtype=f32)
    q8 = np.zeros(L.scanq8_bytes(q_rows, ld8), dtype=np.int8)
    info = np.zeros(8, dtype=np.uint32)
    out = {"qparams": qparams, "quv": quv, "q8": q8, "q_rows": q_rows, "info": info}
    if thr is None:
        dump = np.zeros(q_rows * n_tiles * 256, dtype=f32)
        _ok(_raw().ehx_test_i8_pass(s._h, nq, Qc.ctypes.data, None, tile0, n_tiles, dump.ctypes.data, None, None, None, None,
                                    qparams.ctypes.data, quv.ctypes.data, q8.ctypes.data, info.ctypes.data))
        out["dump"] = dump
    else:
        th = np.ascontiguousarray(thr, dtype=f32)
        cnt, ovf = np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint32)
        ids = np.zeros((nq, L.POOL_CAP), dtype=np.uint32)
        sc = np.zeros((nq, L.POOL_CAP), dtype=f32)
        _ok(_raw().ehx_test_i8_pass(s._h, nq, Qc.ctypes.data, th.ctypes.data, tile0, n_tiles, None, cnt.ctypes.data,
                                    ovf.ctypes.data, ids.ctypes.data, sc.ctypes.data, qparams.ctypes.data, quv.ctypes.data,
                                    q8.ctypes.data, info.ctypes.data))
        out["pool"] = (cnt, ovf, ids, sc)
    return out


# ---- data ----------------------------------------------------------------------------------------------------------
def _rows(rng, d, metric, kind, n):
    if kind == "mixed-norms":       # L2^2: norms of 0.4x and 1x inside every tile -> group B margins matter
        X = rng.standard_normal((n, d)).astype(f32) * rng.uniform(0.9, 1.1, (n, 1)).astype(f32)
        X[rng.random(n) < 0.5] *= f32(0.4)
        return X
    if kind == "normalised":        # L2^2 on unit rows: no margin anywhere
        X = rng.standard_normal((n, d))
        return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(f32)
    per = ((n + 9) // 10 + 31) // 16 * 16     # (the near-duplicates set repeats 16 rows: a multiple of 16)
    sets = [X for _, X in _datasets(rng, d, n=per)]
    if metric == "l2":
        sets.append(rng.standard_normal((per, d)).astype(f32))
    pool = np.concatenate(sets)
    return np.ascontiguousarray(pool[rng.permutation(len(pool))[:n]])


def _queries(rng, X, nq):
    d = X.shape[1]
    near = X[:12] + f32(1e-3) * rng.standard_normal((12, d)).astype(f32)
    exact = X[[300, 700, 1500, len(X) - 5]]
    rest = rng.standard_normal((nq - 17, d)).astype(f32)
    return np.ascontiguousarray(np.concatenate([near, exact, np.zeros((1, d), dtype=f32), rest]), dtype=f32)


def _keys(a, b):
    return ["r%d" % i for i in range(a, b)]


def _write(s, X, how, rng, d):
    """-> (rows as written [n][d], tiles that were not full when written, tiles written full)"""
    n = len(X)
    full = list(range(n // 256))
    if how == "pieces":             # no tile is ever full when written
        for i in range(0, n, 100):
            s.set_batch(_keys(i, min(i + 100, n)), X[i:i + 100])
        return X, full, []
    if how == "grow":               # default capacity: the copies move through several grow calls
        for i in range(0, n, 700):
            s.set_batch(_keys(i, min(i + 700, n)), X[i:i + 700])
        straddled = sorted({i // 256 for i in range(700, n, 700)})
        return X, straddled, [t for t in full if t not in straddled]
    s.set_batch(_keys(0, n), X)
    if how == "rewrite":            # 300 rows in place, from the middle of one ordered tile into the next
        X = X.copy()
        X[400:700] = _rows(rng, d, "l2", "datasets", 300)
        s.set_batch(_keys(400, 700), X[400:700])
    elif how == "dominant":         # one tile mixes rows of a 50x dominant coordinate with ordinary rows
        X = X.copy()
        heavy = rng.standard_normal((96, d)).astype(f32)
        heavy[:, 0] *= f32(50)
        X[576:672] = heavy
        s.set_batch(_keys(576, 672), heavy)
    return X, [], full


def _unsafe_rows(X):
    X = X.copy()
    d = X.shape[1]
    ramp = (1.0 + np.arange(d) / d).astype(f32)
    X[5] = f32(1e-16) * ramp        # |x|^2 far below 1e-24
    X[300] = f32(1e17) * ramp       # ... far above 1e30
    X[1000] = f32(-1e-15) * ramp
    X[1300] = ramp
    X[1300, 3] = np.nan
    X[2000] = 0
    return X


CASES = []
for _d in (128, 384, 768):
    for _m in ("cosine", "ip", "l2"):
        CASES.append((_d, _m, "datasets", "batch", 40))
for _d in (64, 192, 200, 320, 2048):
    for _m in ("cosine", "l2"):
        CASES.append((_d, _m, "datasets", "batch", 40))
CASES += [(128, "l2", "mixed-norms", "batch", 40), (128, "l2", "normalised", "batch", 40), (300, "cosine", "datasets", "batch", 300)]
for _d, _m in ((128, "l2"), (384, "cosine")):
    for _how in ("pieces", "grow", "rewrite", "dominant", "f16", "unsafe"):
        CASES.append((_d, _m, "datasets", _how, 40))


def _check_space(s, X, Q, metric, d, n_pub, identity, ordered, passes, written_once=True):
    snap = snapshot(s)
    assert snap.ld8 == (d + 63) // 64 * 64 and snap.cap % 256 == 0
    ck.check_c1(snap, n_pub, identity_tiles=identity, expect_ordered=ordered)
    ck.check_c2_rows(snap, X, metric, d, n_pub)
    ck.check_c3(snap, X, n_pub, written_once=written_once)
    ck.check_c4(snap, X, metric, n_pub)
    if not passes:
        return None
    T = (n_pub + 255) // 256
    lo = run_pass(s, Q, None, 0, L.SAMPLE_TILES, snap.ld8)
    hi = run_pass(s, Q, None, T - L.SAMPLE_TILES, L.SAMPLE_TILES, snap.ld8)
    nq = len(Q)
    assert int(lo["info"][6]) == n_pub
    for k in ("qparams", "quv", "q8"):
        assert lo[k].tobytes() == hi[k].tobytes()
    qi = ck.check_c2_queries(Q, d, lo["qparams"], lo["q8"], lo["q_rows"], snap.ld8)
    S_lo = ck.dump_scores(lo["dump"], lo["q_rows"], nq)
    S_hi = ck.dump_scores(hi["dump"], hi["q_rows"], nq)
    ck.check_c5(snap, S_lo, 0, qi, lo["qparams"])
    ck.check_c5(snap, S_hi, T - L.SAMPLE_TILES, qi, lo["qparams"])
    t_hi = T - L.SAMPLE_TILES
    both = slice(t_hi * 256, L.SAMPLE_TILES * 256)
    assert S_lo[both].tobytes() == S_hi[:(L.SAMPLE_TILES - t_hi) * 256].tobytes(), "the two windows disagree where they overlap"
    S = np.concatenate([S_lo, S_hi[(L.SAMPLE_TILES - t_hi) * 256:]])
    ck.check_c6(snap, S, X, Q, metric, lo["quv"], n_pub, _true_distance)
    S_row = S[snap.pos_of_row()[:n_pub]]
    for case in range(ck.N_THRESHOLD_CASES):
        thr = ck.thresholds(S_row, case)
        got = run_pass(s, Q, thr, 0, T, snap.ld8)
        assert got["qparams"].tobytes() == lo["qparams"].tobytes()
        ck.check_c7(snap, S, thr, got["pool"], n_pub)
    return lo["info"]


@pytest.mark.parametrize("d,metric,kind,how,nq", CASES, ids=["%d-%s-%s-%s-q%d" % c for c in CASES])
def test_device_scan_copy_bound_and_hit_path(d, metric, kind, how, nq):
    rng = np.random.default_rng(1000 * d + len(metric) + 7 * len(how) + len(kind))
    X = _rows(rng, d, metric, kind, N_ROWS)
    if how == "unsafe":
        X = _unsafe_rows(X)
    dtype = ehx.DTYPE_F16 if how == "f16" else ehx.DTYPE_F32
    if how == "f16":
        X = X.astype(np.float16).astype(f32)      # the rows as stored
    s = ehx.Space.unique("i8-bound", d, metric=METRICS[metric], dtype=dtype, initial_capacity=0 if how == "grow" else CAP)
    try:
        X, identity, ordered = _write(s, X, how, rng, d)
        if how == "f16":
            X = X.astype(np.float16).astype(f32)
        assert len(s) == N_ROWS
        Q = _queries(rng, X, nq)
        once = how not in ("rewrite", "dominant")
        info = _check_space(s, X, Q, metric, d, N_ROWS, identity, ordered, passes=how != "unsafe", written_once=once)
        if kind == "mixed-norms":
            assert int(info[2]) == 1, "group B margins should be in use"
        if kind == "normalised" or metric != "l2":
            assert info is None or int(info[2]) == 0
        # the append: 200 rows of 0.4x norm across the straddling tile, then everything again from the start
        add = f32(0.4) * _rows(rng, d, metric, kind if kind != "datasets" else "mixed-norms", N_APPEND) if how != "unsafe" \
            else rng.standard_normal((N_APPEND, d)).astype(f32)
        if how == "f16":
            add = add.astype(np.float16).astype(f32)
        s.set_batch(_keys(N_ROWS, N_ROWS + N_APPEND), add)
        X2 = np.concatenate([X, add])
        _check_space(s, X2, Q, metric, d, N_ROWS + N_APPEND, list(identity) + [N_ROWS // 256], ordered, passes=how != "unsafe",
                     written_once=once)
    finally:
        s.drop()
