"""Helper of the large-k tests (no test here): the data of the GPU cases of tests/test_knn_largek.py, shared with the CPU
model (tests/test_largek_model.py), a Python mirror of the route's pass planner (largek_passes, ehx_largek.cpp) and a numpy
restatement of its cascade — seed, pass cuts, radius updates — on top of range_thr (tests/range_cases.py) and the int8
lower bound of tests/i8_model.py."""
import functools

import numpy as np

import i8_model as m8
import range_cases as rc
from oracle import pyoracle

f32 = np.float32
TILE = 256
SAMPLE = 1024            # kLargeKSample
POOL_CAP = 4096          # kPoolCap
K_MIN, K_MAX = 49, 256   # EHX_MAX_K + 1, kLargeKScanMax
MIN_QUERIES = 64         # kLargeKMinQueries
GROWTH = 4               # EHX_LARGEK_GROWTH's default
KS = (49, 64, 65, 100, 255, 256)
OM = rc.OM


def passes(n, growth=GROWTH):
    """largek_passes: [(tile0, n_tiles)]"""
    n_tiles = -(-n // TILE)
    out, t0, want = [], 0, SAMPLE * growth
    while t0 < n_tiles:
        t1 = n_tiles if want >= n else -(-want // TILE)
        out.append((t0, t1 - t0))
        t0, want = t1, want * growth
    return out


def sample_ids(n):
    stride = -(-n // SAMPLE)
    return np.arange(0, n, stride, dtype=np.int64)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def gauss(n, d, nq, seed):
    """Gaussian rows and queries"""
    rng = np.random.default_rng(seed)
    return _frozen(rng.standard_normal((n, d)).astype(f32), rng.standard_normal((nq, d)).astype(f32))


@functools.lru_cache(maxsize=None)
def ties():
    """gauss(20000, 64) with 300 copies of row 5 spread over the ids of all three passes; query 0 is that row"""
    X0, Q0 = gauss(20000, 64, 64, 1)
    X, Q = X0.copy(), Q0.copy()
    at = np.unique(np.linspace(5, 19990, 300).astype(np.int64))
    assert len(at) == 300 and (at < 4096).sum() > 10 and ((at >= 4096) & (at < 16384)).sum() > 10 and (at >= 16384).sum() > 10
    X[at] = X[5]
    Q[0] = X[5]
    return _frozen(X, Q, at)


@functools.lru_cache(maxsize=None)
def f16_rows():
    """20 000 x 96, rounded to binary16 as an EHX_DTYPE_F16 space stores them"""
    X, Q = gauss(20000, 96, 64, 4)
    return _frozen(X.astype(np.float16).astype(f32), Q.copy())


# name -> (rows, queries, metric, the k the GPU test runs); every one of them must pass tests/test_largek_model.py before the
# GPU test may assert "no query handed on" for it
def model_cases():
    out = {}
    X, Q = gauss(20000, 64, 64, 1)
    for metric in ("l2", "ip", "cosine"):
        out["gauss64-" + metric] = (X, Q, metric, KS)
    Xt, Qt, _ = ties()
    out["ties"] = (Xt, Qt, "l2", (100, 256))
    X, Q = gauss(20000, 200, 64, 2)
    out["d200"] = (X, Q, "l2", (100,))
    X, Q = gauss(17000, 768, 100, 3)
    out["d768"] = (X, Q, "cosine", (100,))
    X, Q = f16_rows()
    out["f16"] = (X, Q, "cosine", (100,))
    X, Q = gauss(20000, 32, 2100, 5)
    out["chunks"] = (X, Q, "l2", (100,))
    X, Q = gauss(20000, 64, 64, 1)
    out["bykeys"] = (X, X[:64 * 300:300].copy(), "l2", (49,))     # the queries are stored rows, k + 1 = 49
    X, Q = gauss(40000, 64, 64, 6)
    for i in range(2):                                               # shard i of two holds rows i, i + 2, ...
        out["shard%d" % i] = (np.ascontiguousarray(X[i::2]), Q, "l2", (100,))
    return out


def _s_lower(X, Q, metric, d):
    """S_lower [rows, queries] and the queries' (u, v) (tests/test_range_model.py's, restated: importing a test module from a
    helper would collect its tests twice)"""
    xi, A, B, C, D = m8._row_params(X, metric, d)
    qi, sq, eq, g, u, v = m8._query_params(Q, metric, d)
    I = (xi.astype(np.float64) @ qi.astype(np.float64).T)
    t = (sq[None, :] * I.astype(f32)).astype(f32)
    K = (B[:, None] * g[None, :] + (C[:, None] * eq[None, :] + D[:, None]).astype(f32)).astype(f32)
    return (A[:, None] * t + K).astype(f32), u, v


def cascade(X, Q, metric, ks, growth=GROWTH, depth=8000, block=256):
    """The route in numpy for every k of `ks`.  -> {k: (answer ids per query, worst pool fill per pass)}.  Asserts, at every
    pass, that no row within the radius lies above the threshold and that no query is marked; the oracle's `depth` nearest
    are enough (every radius met lies below the depth-th distance, asserted)."""
    n, d = X.shape
    depth = n if len(Q) <= 128 else min(depth, n)   # (a small batch: every distance)
    plan = passes(n, growth)
    smp = sample_ids(n)
    max_sumsq = f32((X ** 2).sum(axis=1, dtype=f32).max())
    out = {k: ([], [0] * len(plan)) for k in ks}
    for q0 in range(0, len(Q), block):
        Qb = np.ascontiguousarray(Q[q0:q0 + block])
        nq = len(Qb)
        oids, odist, ocnt = pyoracle.exhaustive(X, Qb, depth, OM[metric])
        assert (ocnt == depth).all()
        D = np.full((n, nq), np.inf, dtype=f32)
        for q in range(nq):
            D[oids[q].astype(np.int64), q] = odist[q]
        floor = odist[:, -1] if depth < n else np.full(nq, np.inf, dtype=f32)
        S, u, v = _s_lower(X, Qb, metric, d)
        for k in ks:
            assert k <= len(smp)
            radius = np.sort(D[smp], axis=0)[k - 1].astype(f32)      # the seed: the sample's exact k-th distance, nothing carried
            assert (radius < floor).all() or depth == n, "a radius beyond the oracle's depth: deepen it"
            carried = [np.zeros(0, dtype=np.int64) for _ in range(nq)]
            for j, (t0, nt) in enumerate(plan):
                lo, hi = t0 * TILE, min((t0 + nt) * TILE, n)
                thr, marked = rc.range_thr(radius, u, v, metric, d, max_sumsq)
                assert not marked.any(), "a query the bound does not serve"
                through = S[lo:hi] <= thr[None, :]
                member = D[lo:hi] <= radius[None, :]
                assert not (member & ~through).any(), "the threshold hides a row within the radius"
                out[k][1][j] = max(out[k][1][j], int(through.sum(axis=0).max()))
                for q in range(nq):                                   # radius_rerank_kernel
                    hits = lo + np.nonzero(through[:, q])[0]
                    hits = hits[D[hits, q] <= radius[q]]
                    pool = np.concatenate([carried[q], hits])
                    pool = pool[np.lexsort((pool, D[pool, q]))][:k]
                    if len(pool) == k:
                        assert D[pool[-1], q] <= radius[q]            # the radius only falls
                        radius[q] = D[pool[-1], q]
                    carried[q] = pool
            for q in range(nq):
                assert np.array_equal(carried[q], oids[q, :k].astype(np.int64)), (k, q0 + q)
            out[k][0].extend(carried)
    return out
