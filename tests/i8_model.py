"""numpy float32 restatement of what make_scan8 / prep_queries8 (k_misc.hip) store and i8_score / i8_alarm_k (k_flati8.hip)
evaluate: shared by tests/test_i8_model.py (the model against float64 distances) and tests/test_i8_checks_cpu.py (the model
in the device layout, as the baseline the checker of tests/i8_checks.py must pass).  The constants are the kernels'."""
import numpy as np

f32 = np.float32


def _slack(d):
    return f32(4e-6) + f32(1.5e-7) * f32(d)          # i8_slack


def _err_up(e2):
    return np.sqrt(e2).astype(f32) * f32(1.0 + 1e-4) + f32(3e-7)   # i8_err_up


def _quantise(V):
    """rows V (fp32) -> (n_f, ss, xi, s, e) as make_scan8 / prep_queries8 compute them"""
    ss = (V.astype(f32) ** 2).sum(axis=1, dtype=f32)
    nr = np.sqrt(ss).astype(f32)
    inv = np.where(nr > 0, f32(1) / np.where(nr > 0, nr, f32(1)), f32(0)).astype(f32)
    xh = (V * inv[:, None]).astype(f32)
    amax = np.abs(xh).max(axis=1).astype(f32)
    s = (amax / f32(127)).astype(f32)
    rs = np.where(amax > 0, f32(127) / np.where(amax > 0, amax, f32(1)), f32(0)).astype(f32)
    qf = np.clip(np.rint((xh * rs[:, None]).astype(f32)), -127, 127).astype(f32)
    res = (xh - (s[:, None] * qf).astype(f32)).astype(f32)
    e = _err_up((res ** 2).sum(axis=1, dtype=f32))
    return nr, ss, qf.astype(np.int32), s, e


def _row_params(X, metric, d):
    nr, ss, xi, s, e = _quantise(X)
    a = -np.ones_like(nr)
    b = np.ones_like(nr)
    if metric in ("ip", "l2"):
        a = -nr
    if metric == "l2":
        b = (ss * f32(1.0 - 1e-6 - 7e-8 * ((d >> 6) + 8.0))).astype(f32)
    A = (a * s).astype(f32)
    B = (b * f32(1.0 - 1e-6)).astype(f32)
    C = (a * (f32(1.0001) + e)).astype(f32)
    D = (a * (f32(1.0001) * e + _slack(d))).astype(f32)
    return xi, A, B, C, D


def _row_params_raised(X, metric, d, tgtA=None):
    """make_scan8_kernel with tgtA: the row's step raised so that |a_r| s reaches its lane group's |A|, the codes and the
    residual bound taken with the RAISED step; tgtA None: the rows' own steps.  -> xi, A, B, C, D, e"""
    V = X.astype(f32)
    ss = (V ** 2).sum(axis=1, dtype=f32)
    nr = np.sqrt(ss).astype(f32)
    inv = np.where(nr > 0, f32(1) / np.where(nr > 0, nr, f32(1)), f32(0)).astype(f32)
    xh = (V * inv[:, None]).astype(f32)
    amax = np.abs(xh).max(axis=1).astype(f32)
    a_abs = np.ones_like(nr) if metric == "cosine" else nr
    s = (amax / f32(127)).astype(f32)
    if tgtA is not None:
        want = np.where(a_abs > 0, tgtA.astype(f32) / np.where(a_abs > 0, a_abs, f32(1)), s).astype(f32)
        s = np.maximum(s, want)
    rs = np.where(s > 0, f32(1) / np.where(s > 0, s, f32(1)), f32(0)).astype(f32)
    qf = np.clip(np.rint((xh * rs[:, None]).astype(f32)), -127, 127).astype(f32)
    res = (xh - (s[:, None] * qf).astype(f32)).astype(f32)
    e = _err_up((res ** 2).sum(axis=1, dtype=f32))
    a = -a_abs
    b = np.ones_like(nr)
    if metric == "l2":
        b = (ss * f32(1.0 - 1e-6 - 7e-8 * ((d >> 6) + 8.0))).astype(f32)
    A = (a * s).astype(f32) if tgtA is None else (-tgtA).astype(f32)   # (an ordered tile stores the group's |A| itself)
    B = (b * f32(1.0 - 1e-6)).astype(f32)
    C = (a * (f32(1.0001) + e)).astype(f32)
    D = (a * (f32(1.0001) * e + _slack(d))).astype(f32)
    return qf.astype(np.int32), A, B, C, D, e


def _norm_ok(ss):
    """norm_ok (k_misc.hip): the norms the filter's error analysis covers (a NaN sumsq compares false)"""
    with np.errstate(invalid="ignore"):
        return (ss == 0) | ((ss > f32(1e-24)) & (ss < f32(1e30)))


def _query_params(Q, metric, d, band=False):
    """band=True restates what prep_queries8 does besides: a query whose sumsq fails norm_ok takes beta = 0 (its codes
    are then whatever 0 * x gives; the model stores zeros) and u = NaN, the value that makes range_thr_kernel hand it to an
    exact path; a zero query passes norm_ok and keeps (g, u, v) = (1, 1, 0) under every metric."""
    if band:
        with np.errstate(all="ignore"):
            ok = _norm_ok((Q.astype(f32) ** 2).sum(axis=1, dtype=f32))
        qi, s, e, g, u, v = _query_params(np.where(ok[:, None], Q, f32(0)).astype(f32), metric, d)
        return qi, s, e, g, np.where(ok, u, f32(np.nan)).astype(f32), v
    beta, ss, qi, s, e = _quantise(Q)
    g = np.ones_like(beta)
    u = np.ones_like(beta)
    v = np.zeros_like(beta)
    pos = beta > 0
    if metric == "ip":
        g[pos] = f32(1) / beta[pos]
        u[pos] = beta[pos]
    elif metric == "l2":
        g[pos] = f32(0.5) / beta[pos]
        u[pos] = f32(2) * beta[pos]
        v[pos] = (ss[pos] * f32(1.0 - 1e-6 - 7e-8 * ((d >> 6) + 8.0))).astype(f32)
    return qi, s, e, g, u, v


def _true_distance(X, Q, metric):
    X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
    if metric == "cosine":
        nx = np.maximum(np.linalg.norm(X64, axis=1), 1e-300)
        nq = np.maximum(np.linalg.norm(Q64, axis=1), 1e-300)
        return 1.0 - (X64 / nx[:, None]) @ (Q64 / nq[:, None]).T
    if metric == "ip":
        return 1.0 - X64 @ Q64.T
    # (|x|^2 + |q|^2 - 2 <x, q> would cancel: the differences, a block of queries at a time)
    out = np.empty((X64.shape[0], Q64.shape[0]))
    for j in range(Q64.shape[0]):
        out[:, j] = ((X64 - Q64[j][None, :]) ** 2).sum(axis=1)
    return out


def _datasets(rng, d, n=320):
    g = rng.standard_normal((n, d)).astype(f32)
    yield "gaussian", g
    yield "scaled 1e3", g * f32(1e3)
    yield "scaled 1e-3", g * f32(1e-3)
    yield "near-duplicates", np.repeat(g[:16], n // 16, axis=0) + f32(1e-4) * rng.standard_normal((n, d)).astype(f32)
    sparse = np.zeros((n, d), dtype=f32)
    sparse[np.arange(n)[:, None], rng.integers(0, d, size=(n, 3))] = rng.standard_normal((n, 3)).astype(f32)
    yield "3-sparse", sparse
    yield "one-hot-ish", np.eye(d, dtype=f32)[rng.integers(0, d, n)] + f32(1e-3) * g
    yield "constant", np.ones((n, d), dtype=f32) * rng.uniform(0.5, 2, size=(n, 1)).astype(f32)
    heavy = g.copy()
    heavy[:, 0] *= f32(50)
    yield "dominant coordinate", heavy
    mixed = g * (10.0 ** rng.uniform(-1, 1, size=(n, 1))).astype(f32)
    mixed[:8] = 0
    yield "mixed norms + zero rows", mixed
    yield "all positive", np.abs(g)


def _alarm_k(Bmin, Cmax, Dmax, g, eq, sq, thr):
    with np.errstate(invalid="ignore", over="ignore"):
        bg, ce = f32(Bmin * g), f32(Cmax * eq)
        num = f32(f32(f32(bg - Dmax) - ce) - thr)
        num = f32(num - f32(1e-5) * f32(abs(bg) + Dmax + ce + abs(thr))) if np.isfinite(thr) else f32(-np.inf)
    if not (num > 0):
        return f32(-np.inf)
    if not (sq > 0):
        return f32(np.inf)
    return f32(f32(num / sq) * f32(1.0 - 1e-5))


def _kernel_order(A, norms):
    """rank_tiles8_kernel (k_misc.hip, round 6): the positions of a FULL tile's 256 rows — pure step order when the norms
    spread by less than 0.1 %, else four norm bands of 64 rows, each by step; returns the rows in rank order (rank r sits in
    lane group r // 32)"""
    idx = np.arange(256)
    if norms.max() <= norms.min() * f32(1.001):
        return idx[np.argsort(np.abs(A), kind="stable")]
    by_norm = idx[np.argsort(norms, kind="stable")]
    return np.concatenate([b[np.argsort(np.abs(A[b]), kind="stable")] for b in (by_norm[i * 64:(i + 1) * 64] for i in range(4))])


def _group_b_margin(bg, bt):
    """i8_group_b_margin (ehx_kernels.h): (bg - bt) rounded down, never negative; bt = +inf: 0"""
    if not bt < np.inf:
        return f32(0)
    m = f32(f32(bg - bt) * f32(1.0 - 1e-6)) if bg < np.inf else f32(np.inf)
    return m if m > 0 else f32(0)
