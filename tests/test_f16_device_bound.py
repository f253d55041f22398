"""GPU: the fp16 filter scan's copy, its lower bound and its candidate lists, checked on what the DEVICE wrote and collected;
the list path of the fp32 scan with it.

Three test hooks (csrc/ehx_testhooks.cpp) read the scan copy back raw and run single launches of flat_scan16_kernel /
flat_scan8_kernel with a search's arguments: the sample form (every score of an eight-tile window, and sample select's
thresholds) and collect passes under 64-bit threshold keys drawn from those scores.  tests/f16_checks.py then applies, in
float64 against the original rows and queries:
  H1 the stored halves are the correctly rounded unit rows, padding zero           H5 u S + v never exceeds the true distance
  H2 the row parameters per metric, never-alarm parameters where nothing is bound  H6 sample select's threshold to the bit
  H3 the query tiles, their repeated stages, gamma and (u, v)                      H7 what a collect pass publishes
  H4 the score is the stated expression of the stored halves                      H8 what the merge makes of it
and for the fp32 scan, which has no dump, the weaker list check of f16_checks.check_f32_lists.
tests/test_f16_checks_cpu.py shows that each of them can fail.  Every case prints the largest H4 error / tolerance and the
largest (u S + v - D_true) / scale it saw: how close the device runs to the bound."""
import ctypes as C

import numpy as np
import pytest

import f16_checks as ck
import f16_layout as L
import f16_model as M
from i8_model import _true_distance
from test_i8_device_bound import CAP, METRICS, N_APPEND, N_ROWS, _keys, _queries, _rows, _unsafe_rows, _write

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402

f32 = np.float32
KPRIMES = (9, 30, 56)
N_ALIGNED = 48                  # rows of the aligned kind per case, half below and half above the midpoints
ALIGNED_AT = 2280               # ... stored across the boundary of tiles 8 and 9

_RAW = []


def _raw():
    if not _RAW:
        lib = C.CDLL(_lib.LIB_PATH)
        lib.ehx_test_f16_array.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]
        lib.ehx_test_f16_array.restype = C.c_int
        lib.ehx_test_f16_pass.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 9
        lib.ehx_test_f16_pass.restype = C.c_int
        lib.ehx_test_f32_pass.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 5
        lib.ehx_test_f32_pass.restype = C.c_int
        _RAW.append(lib)
    return _RAW[0]


def _ok(rc):
    assert rc == 0, (rc, _lib.load().ehx_last_error())


def _array(s, which, n, dtype):
    out = np.zeros(n, dtype=dtype)
    _ok(_raw().ehx_test_f16_array(s._h, which, 0, n, out.ctypes.data))
    return out


def snapshot(s):
    ld16 = int(_array(s, 3, 1, np.uint64)[0])
    cap = int(_array(s, 4, 1, np.uint64)[0])
    return ck.Snapshot16(_array(s, 0, L.x16_halves(cap, ld16), np.uint16), _array(s, 1, (cap + L.ROWP_PAD) * 2, f32),
                         _array(s, 2, 1, np.uint64), ld16, cap)


def _p(a):
    return None if a is None else a.ctypes.data


def run_f16(s, Q, kprime, keys, tile0, n_tiles, ld16):
    """one launch of the fp16 scan -> dict: dump + gthr (sample form) or part, err, merged, gthr (collect form); q16, gamma,
    quv, q_rows, info"""
    nq = len(Q)
    q_rows = (nq + 255) // 256 * 256
    Qc = np.ascontiguousarray(Q, dtype=f32)
    out = {"q16": np.zeros(L.scanq16_halves(q_rows, ld16), dtype=np.uint16), "gamma": np.zeros(q_rows, dtype=f32),
           "quv": np.zeros((q_rows, 2), dtype=f32), "info": np.zeros(8, dtype=np.uint32), "gthr": np.zeros(nq, dtype=np.uint64),
           "q_rows": q_rows}
    dump = part = err = merged = kk = None
    if keys is None:
        dump = out["dump"] = np.zeros((n_tiles * L.TILE, q_rows), dtype=f32)
    else:
        kk = np.ascontiguousarray(keys, dtype=np.uint64)
        part = np.zeros(nq * 2 * n_tiles * kprime, dtype=np.uint64)
        err = out["err"] = np.zeros(1, dtype=np.uint32)
        merged = out["merged"] = np.zeros((nq, 64), dtype=np.uint64)
    _ok(_raw().ehx_test_f16_pass(s._h, nq, Qc.ctypes.data, kprime, _p(kk), tile0, n_tiles, _p(dump), out["gthr"].ctypes.data,
                                 _p(part), _p(err), _p(merged), out["q16"].ctypes.data, out["gamma"].ctypes.data,
                                 out["quv"].ctypes.data, out["info"].ctypes.data))
    if part is not None:
        lists = int(out["info"][7])
        assert lists == 2 * int(out["info"][2]) <= 2 * n_tiles
        out["part"] = part[:nq * lists * kprime].reshape(nq, lists, kprime)
    return out


def run_f32(s, Q, kprime, keys, tile0, n_tiles):
    nq = len(Q)
    Qc = np.ascontiguousarray(Q, dtype=f32)
    kk = np.ascontiguousarray(keys, dtype=np.uint64)
    part = np.zeros(nq * 2 * n_tiles * kprime, dtype=np.uint64)
    out = {"err": np.zeros(1, dtype=np.uint32), "merged": np.zeros((nq, 64), dtype=np.uint64), "info": np.zeros(8, dtype=np.uint32),
           "gthr": np.zeros(nq, dtype=np.uint64)}
    _ok(_raw().ehx_test_f32_pass(s._h, nq, Qc.ctypes.data, kprime, kk.ctypes.data, tile0, n_tiles, out["gthr"].ctypes.data,
                                 part.ctypes.data, out["err"].ctypes.data, out["merged"].ctypes.data, out["info"].ctypes.data))
    lists = int(out["info"][7])
    assert lists == 2 * int(out["info"][2]) <= 2 * n_tiles
    out["part"] = part[:nq * lists * kprime].reshape(nq, lists, kprime)
    return out


def full_dump(s, Q, T, ld16):
    """the sample form over windows of eight tiles that cover tiles [0, T) -> (S [T * 256][nq], the first window's result);
    where two windows overlap they must agree to the bit, and the prepared queries are the same bytes every time"""
    nq = len(Q)
    starts = list(range(0, T - L.SAMPLE_TILES, L.SAMPLE_TILES)) + [T - L.SAMPLE_TILES]
    S = np.zeros((T * L.TILE, nq), dtype=f32)
    seen = 0
    first = None
    for t0 in starts:
        r = run_f16(s, Q, 30, None, t0, L.SAMPLE_TILES, ld16)
        d = r["dump"][:, :nq]
        if first is None:
            first = r
        else:
            for k in ("q16", "gamma", "quv"):
                assert r[k].tobytes() == first[k].tobytes()
        lo = t0 * L.TILE
        assert S[lo:seen].tobytes() == d[:max(seen - lo, 0)].tobytes(), "two windows disagree where they overlap"
        S[lo:lo + len(d)] = d
        seen = lo + len(d)
    return S, first


# ---- data ----------------------------------------------------------------------------------------------------------
def _norms(rng, n, metric):
    return np.ones(n, dtype=f32) if metric == "cosine" else (10.0 ** rng.uniform(-3, 3, n)).astype(f32)


def _aligned(rng, d, metric):
    """-> (rows of the aligned kind, the queries made of them: some as they are, some negated), both scaled by norms of
    1e-3 .. 1e3 for IP and L2^2.  A row below the midpoints queried by itself, and a row above them queried by its negative,
    lose almost 2^-10 of the dot product in the direction that raises the score."""
    h = N_ALIGNED // 2
    A = np.concatenate([M.aligned_rows(rng, d, h), M.aligned_rows(rng, d, h, above=True)])
    qa = np.concatenate([A[0:6], -A[6:10], A[h:h + 4], -A[h + 4:h + 10]])
    return A * _norms(rng, len(A), metric)[:, None], qa * _norms(rng, len(qa), metric)[:, None]


def _data(rng, d, metric, how, nq_base=24):
    X = _rows(rng, d, metric, "datasets", N_ROWS)
    A, qa = _aligned(rng, d, metric)
    X[ALIGNED_AT:ALIGNED_AT + len(A)] = A
    X[ALIGNED_AT - 8:ALIGNED_AT] = X[ALIGNED_AT - 8]           # eight equal rows: ties at the thresholds
    if how == "unsafe":
        X = _unsafe_rows(X)
    band = f32(1e-16) * (1.0 + np.arange(d) / d).astype(f32)       # a query the filter cannot bound
    return X, lambda Xw: np.ascontiguousarray(np.concatenate([_queries(rng, Xw, nq_base), Xw[ALIGNED_AT - 8:ALIGNED_AT - 7], qa,
                                                              band[None, :]]), dtype=f32)


CASES = []
for _d in (20, 64, 128, 200, 768, 1024):
    for _m in ("cosine", "ip", "l2"):
        CASES.append((_d, _m, "batch"))
for _d in (2304, 4096):
    for _m in ("cosine", "l2"):
        CASES.append((_d, _m, "batch"))
for _d, _m in ((128, "l2"), (200, "cosine")):
    for _how in ("pieces", "grow", "rewrite", "f16", "unsafe"):
        CASES.append((_d, _m, _how))

WORST = {}


def _report(name, h4, h5, loss, eps):
    WORST[name] = (h4, h5, loss)
    print("\n[f16 bound] %-28s largest H4 error / tolerance %.4f   largest (u S + v - D_true) / scale %+.4e   largest <q^, x^> - dot16 "
          "%.4e = %.3f of 2^-10 = %.3f of eps" % (name, h4, h5, loss, loss * 1024.0, loss / float(eps)))


def _check_lists_f16(s, Q, S, n_pub, ld16, kprimes, cases, dump0):
    T = (n_pub + L.TILE - 1) // L.TILE
    info = None
    for kprime in kprimes:
        smp = run_f16(s, Q, kprime, None, 0, L.SAMPLE_TILES, ld16)
        assert smp["dump"].tobytes() == dump0.tobytes()
        ck.check_h6(smp["dump"][:, :len(Q)], kprime, smp["gthr"])
        for case in cases:
            g = ck.h7_thresholds(S, n_pub, case, kprime, smp["gthr"])
            got = run_f16(s, Q, kprime, g, 0, T, ld16)
            info = got["info"]
            ck.check_h7(S, g, got["part"], got["err"][0], kprime, 0, T, int(info[3]), n_pub)
            ck.check_h8(got["part"], got["merged"], g, got["gthr"], kprime)
            if case == 2:
                assert (got["part"] == L.KEY_INF).all()
    return info


def _check_lists_f32(s, X, Q, metric, d, n_pub, kprimes):
    fin = ~ck.unbounded_rows(Q)
    Qf = np.ascontiguousarray(Q[fin])
    S64 = ck.f32_scores(X[:n_pub], Qf, metric)
    T = (n_pub + L.TILE_F32 - 1) // L.TILE_F32
    srt = np.sort(S64.astype(f32), axis=0)
    for kprime in kprimes:
        for g in (np.full(len(Qf), L.KEY_INF, dtype=np.uint64), L.make_key(srt[2 * kprime], 0xFFFFFFFF),
                  L.make_key((srt[0] - np.abs(srt[0]) - f32(1)).astype(f32), 0)):
            got = run_f32(s, Qf, kprime, g, 0, T)
            ck.check_f32_lists(S64, X, Qf, metric, d, g, got["part"], got["err"][0], kprime, 0, T, int(got["info"][3]), n_pub)
            ck.check_h8(got["part"], got["merged"], g, got["gthr"], kprime)


def _check_space(name, s, X, Q, metric, d, n_pub, passes, written_once=True, kprimes=KPRIMES, cases=range(ck.N_THRESHOLD_CASES),
                 h4_windows=None, h5_queries=None, f32_queries=None, aligned_reach=None):
    snap = snapshot(s)
    assert snap.ld16 == L.ld16_of(d)
    ck.check_h1(snap, X, d, n_pub)
    ck.check_h2(snap, X, metric, d, n_pub, written_once=written_once)
    if not passes:
        return None
    T = (n_pub + L.TILE - 1) // L.TILE
    nq = len(Q)
    S, first = full_dump(s, Q, T, snap.ld16)
    info = first["info"]
    eps = M.scan16_eps(d)
    assert int(info[5]) == n_pub and int(info[1]) == snap.ld16 and info[6:7].view(f32)[0] == eps
    Hq = ck.check_h3(Q, d, metric, first["q16"], first["gamma"], first["quv"], first["q_rows"])
    h4 = 0.0
    for t0 in (h4_windows if h4_windows is not None else range(0, T, L.SAMPLE_TILES)):
        h4 = max(h4, ck.check_h4(snap, S[t0 * L.TILE:(t0 + L.SAMPLE_TILES) * L.TILE], t0 * L.TILE, Hq, first["gamma"], eps))
    if n_pub < T * L.TILE:
        assert np.isposinf(S[n_pub:]).all(), "a row behind the published ones does not score +inf"
    qs = slice(None) if h5_queries is None else h5_queries
    h5 = ck.check_h5(snap, S[:, qs], X, Q[qs], metric, first["quv"][:nq][qs], n_pub, _true_distance)
    loss = ck.rounding_loss(snap, Hq, X, Q, n_pub)
    _report(name, h4, h5, loss, eps)
    # Cauchy-Schwarz on two unit vectors rounded with relative error 2^-11 each, their norms' own t(d), and 2^-25 absolute per
    # subnormal half against |q^|_1 <= sqrt(d)
    assert loss <= 2.0 ** -10 + 2.0 ** -22 + 2 * ck.t_of(d) + np.sqrt(d) * 2.0 ** -25, loss * 1024.0
    if aligned_reach is not None:     # the aligned rows do what they are there for, on the halves the device stored
        assert loss >= aligned_reach * 2.0 ** -10, loss * 1024.0
    info = _check_lists_f16(s, Q, S, n_pub, snap.ld16, kprimes, cases, first["dump"])
    _check_lists_f32(s, X, Q if f32_queries is None else Q[f32_queries], metric, d, n_pub, kprimes[-1:])
    return info


@pytest.mark.parametrize("d,metric,how", CASES, ids=["%d-%s-%s" % c for c in CASES])
def test_device_fp16_copy_bound_and_lists(d, metric, how):
    rng = np.random.default_rng(1000 * d + len(metric) + 7 * len(how))
    X, make_queries = _data(rng, d, metric, how)
    dtype = ehx.DTYPE_F16 if how == "f16" else ehx.DTYPE_F32
    if how == "f16":
        X = X.astype(np.float16).astype(f32)      # the rows as stored
    s = ehx.Space.unique("f16-bound", d, metric=METRICS[metric], dtype=dtype, initial_capacity=0 if how == "grow" else CAP)
    name = "%d-%s-%s" % (d, metric, how)
    try:
        X, _, _ = _write(s, X, how, rng, d)
        if how == "f16":
            X = X.astype(np.float16).astype(f32)
        assert len(s) == N_ROWS
        Q = make_queries(X)
        once = how != "rewrite"
        reach = 0.85 if d in (64, 1024, 4096) and how != "f16" else None    # (the sizes tests/test_f16_checks_cpu.py pins)
        _check_space(name, s, X, Q, metric, d, N_ROWS, passes=how != "unsafe", written_once=once, aligned_reach=reach)
        # the append: 200 rows across the straddling tile, then everything again from the start
        add = f32(0.4) * _rows(rng, d, metric, "mixed-norms", N_APPEND) if how != "unsafe" else rng.standard_normal((N_APPEND, d)).astype(f32)
        if how == "f16":
            add = add.astype(np.float16).astype(f32)
        s.set_batch(_keys(N_ROWS, N_ROWS + N_APPEND), add)
        X2 = np.concatenate([X, add])
        _check_space(name + "+append", s, X2, Q, metric, d, N_ROWS + N_APPEND, passes=how != "unsafe", written_once=once)
    finally:
        s.drop()


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_device_fp16_lists_at_300_tiles(metric):
    """two query tiles, chunks that share an XCD, several tiles per chunk and chunks with no tiles; the sample-pass regime, so
    an ordinary search of the same space is held to the oracle's exhaustive scan at the end"""
    from oracle import pyoracle
    d, T, nq = 128, 300, 300
    n = T * L.TILE - 88
    rng = np.random.default_rng(300 + len(metric))
    X = rng.standard_normal((n, d)).astype(f32)
    if metric == "l2":
        X *= rng.uniform(0.5, 2.0, (n, 1)).astype(f32)
    A, qa = _aligned(rng, d, metric)
    X[ALIGNED_AT:ALIGNED_AT + len(A)] = A
    X[50000:50008] = X[50000]
    Q = np.concatenate([X[:40] + f32(1e-3) * rng.standard_normal((40, d)).astype(f32), X[50000:50001], qa,
                        rng.standard_normal((nq - 41 - len(qa), d)).astype(f32)]).astype(f32)
    s = ehx.Space.unique("f16-bound-300", d, metric=METRICS[metric], scan=_lib.SCAN_F16, initial_capacity=T * L.TILE)
    try:
        for i in range(0, n, 19200):
            s.set_batch(_keys(i, min(i + 19200, n)), X[i:i + 19200])
        info = _check_space("128-%s-300-tiles" % metric, s, X, Q, metric, d, n, passes=True, kprimes=(30,), cases=(0, 1, 4),
                            h4_windows=(0, T - L.SAMPLE_TILES), h5_queries=slice(38, 50), f32_queries=slice(0, 64))
        q_rows, n_chunks, tpc, xcd_map = int(info[0]), int(info[2]), int(info[3]), int(info[4])
        assert q_rows == 512 and xcd_map == 1 and tpc >= 2 and n_chunks * tpc >= T + tpc, (q_rows, n_chunks, tpc, xcd_map)
        om = pyoracle.METRIC_COSINE if metric == "cosine" else pyoracle.METRIC_L2
        ids, dist, cnt = s.knn(Q[:64], 10)
        oids, odist, ocnt = pyoracle.exhaustive(X, Q[:64], 10, om)
        np.testing.assert_array_equal(cnt, ocnt)
        assert ids.tolist() == oids.tolist() and dist.tobytes() == odist.tobytes()
    finally:
        s.drop()
