"""Helper of the range-search tests (no test here): the data of the int8 cases, shared by the CPU model
(tests/test_range_model.py) and the GPU tests (tests/test_range.py), the oracle's answers cut at a radius, and a numpy
restatement of range_thr_kernel (k_range.hip) on top of the bound restated in tests/test_i8_model.py."""
import functools

import numpy as np

from oracle import pyoracle

f32 = np.float32
I8_ROWS = 20000                       # >= i8_min_rows (16384); 78 full tiles of 256 rows and a partial one
I8_QUERIES = 257                      # two query tiles
I8_DIMS = (128, 192, 384, 768)        # the HALF, resident-query, PAIR and general instantiations of the scan
I8_RANKS = (1, 10, 100, 300)          # radii at the oracle's j-th distance
I8_MAX_RESULTS = 256
OM = {"cosine": pyoracle.METRIC_COSINE, "l2": pyoracle.METRIC_L2, "ip": pyoracle.METRIC_IP}


@functools.lru_cache(maxsize=None)
def i8_data(d):
    """rows near a 24-dimensional subspace (distances spread widely, as embeddings' do) and queries near stored rows"""
    rng = np.random.default_rng(9000 + d)
    W = rng.standard_normal((24, d)).astype(f32)
    X = (rng.standard_normal((I8_ROWS, 24)).astype(f32) @ W / f32(np.sqrt(24.0))
         + f32(0.3) * rng.standard_normal((I8_ROWS, d)).astype(f32)).astype(f32)
    Q = (X[rng.choice(I8_ROWS, size=I8_QUERIES, replace=False)]
         + f32(0.2) * rng.standard_normal((I8_QUERIES, d)).astype(f32)).astype(f32)
    X.setflags(write=False)
    Q.setflags(write=False)
    return X, Q


@functools.lru_cache(maxsize=None)
def i8_oracle(d, metric, depth=6000):
    """the oracle's `depth` nearest of every query of i8_data(d): ids [nq, depth], distances [nq, depth]"""
    X, Q = i8_data(d)
    ids, dist, cnt = pyoracle.exhaustive(X, Q, depth, OM[metric])
    assert (cnt == depth).all()
    ids.setflags(write=False)
    dist.setflags(write=False)
    return ids, dist


def cut(ids, dist, cnt, radius, max_results):
    """the oracle's sorted lists (every row: k = n) cut at `radius` -> [(ids, dist bytes, total)] per query"""
    out = []
    for i in range(len(cnt)):
        c = int(cnt[i])
        r = f32(radius[i])
        total = 0 if np.isnan(r) else int((dist[i, :c] <= r).sum())   # (sorted, NaN never listed: a prefix)
        m = min(total, max_results)
        out.append(([int(v) for v in ids[i, :m]], dist[i, :m].copy(), total))
    return out


def cert_margin(metric, dims, qn, max_sumsq, scale):
    """cert_margin (ehx_kernels.h) in float32"""
    eps_d = f32(1.3) * (f32(dims) + f32(16.0)) * f32(5.9604645e-8)
    if metric == "cosine":
        base = eps_d * f32(1.01) * np.ones_like(qn)
    else:
        qb, mx = np.sqrt(qn).astype(f32), np.sqrt(f32(max_sumsq))
        base = eps_d * f32(1.01) * qb * mx if metric == "ip" else eps_d * f32(1.01) * (qb + mx) * (qb + mx)
    return (base + f32(2e-6) * np.maximum(scale, np.maximum(qn, f32(1.0)))).astype(f32)


def range_thr(radius, u, v, metric, dims, max_sumsq):
    """range_thr_kernel: radius [nq] -> (thr [nq], marked [nq]), float32 operation by operation"""
    r = np.asarray(radius, dtype=f32)
    with np.errstate(all="ignore"):
        qn = v if metric == "l2" else ((u * u).astype(f32) if metric == "ip" else np.ones_like(u))
        m = cert_margin(metric, dims, qn.astype(f32), max_sumsq, np.abs(r))
        L = (r + (f32(1.001) * m).astype(f32)).astype(f32)
        L = (L + (np.abs(L) * f32(2.4e-7)).astype(f32)).astype(f32)
        t = ((L - v).astype(f32) / u).astype(f32)
        t = (t + (np.abs(t) * f32(4.8e-7)).astype(f32)).astype(f32)
    unbounded = np.isinf(r) | ~(u > 0) | np.isinf(u) | np.isnan(t) | np.isinf(t) | np.isnan(m)
    marked = ~np.isnan(r) & unbounded
    thr = np.where(np.isnan(r) | marked, f32(-np.inf), t).astype(f32)
    return thr, marked
