"""CPU model of the range search's int8 threshold (host logic, no GPU): range_thr_kernel (k_range.hip) restated in numpy
float32 (tests/range_cases.py) on top of the int8 bound restated in tests/test_i8_model.py, imported as it is.

  * soundness: every row whose CANONICAL distance (the oracle's arithmetic) is <= r has S_lower <= thr — on that file's
    adversarial data and on rows of spread norms, at radii that equal a distance exactly, lie just below one, and more;
  * the int8 GPU cases of tests/test_range.py: the candidates per query the bound lets through stay within half a pool
    (2048 of kPoolCap = 4096) at the radii that must not overflow, and exceed the pool where the test expects an overflow."""
import numpy as np
import pytest

import range_cases as rc
import test_i8_model as m8
from oracle import pyoracle

f32 = np.float32


def _s_lower(X, Q, metric, d):
    """S_lower [rows, queries] and the queries' (u, v), as test_i8_model evaluates them (integer dots exact in float64)"""
    xi, A, B, C, D = m8._row_params(X, metric, d)
    qi, sq, eq, g, u, v = m8._query_params(Q, metric, d)
    I = (xi.astype(np.float64) @ qi.astype(np.float64).T)
    t = (sq[None, :] * I.astype(f32)).astype(f32)
    K = (B[:, None] * g[None, :] + (C[:, None] * eq[None, :] + D[:, None]).astype(f32)).astype(f32)
    return (A[:, None] * t + K).astype(f32), u, v


def _canonical(X, Q, metric):
    """the oracle's distance of every (row, query) pair [rows, queries] (NaN where the oracle lists no neighbour)"""
    n = X.shape[0]
    ids, dist, cnt = pyoracle.exhaustive(X, Q, n, rc.OM[metric])
    Dm = np.full((n, Q.shape[0]), np.nan, dtype=f32)
    for q in range(Q.shape[0]):
        c = int(cnt[q])
        Dm[ids[q, :c].astype(np.int64), q] = dist[q, :c]
    return Dm


def _check_sound(X, Q, metric, d, what):
    keep = np.linalg.norm(X.astype(np.float64), axis=1) > 0     # (zero rows: the filter does not bound them, h_unsafe8)
    X = X[keep]
    S, u, v = _s_lower(X, Q, metric, d)
    Dm = _canonical(X, Q, metric)
    max_sumsq = f32((X.astype(f32) ** 2).sum(axis=1, dtype=f32).max())
    order = np.sort(np.where(np.isnan(Dm), np.inf, Dm), axis=0)
    n = X.shape[0]
    radii = []
    for j in (0, 1, n // 3, n - 1):
        radii.append(order[j])                                   # exactly the (j + 1)-th distance
        radii.append(np.nextafter(order[j], f32(-np.inf)))       # just below it
    radii.append((order[n // 2] * f32(1.5)).astype(f32))
    for r in radii:
        r = r.astype(f32)
        thr, marked = rc.range_thr(r, u, v, metric, d, max_sumsq)
        member = Dm <= r[None, :]                                # (NaN: no member)
        hidden = member & ~(S <= thr[None, :]) & ~marked[None, :]
        assert not hidden.any(), (what, metric, d, int(hidden.sum()))


@pytest.mark.parametrize("d", [8, 100, 768])
@pytest.mark.parametrize("metric", ["cosine", "ip", "l2"])
def test_threshold_never_hides_a_member_on_adversarial_data(d, metric):
    rng = np.random.default_rng(50 + d)
    for name, X in m8._datasets(rng, d, n=160):
        Q = np.concatenate([X[:6] + f32(1e-3) * rng.standard_normal((6, d)).astype(f32),
                            rng.standard_normal((6, d)).astype(f32), X[:3]]).astype(f32)
        _check_sound(X, Q, metric, d, name)


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_threshold_never_hides_a_member_on_rows_of_spread_norms(metric):
    rng = np.random.default_rng(77)
    d = 192
    X = (rng.standard_normal((400, d)) * 10.0 ** rng.uniform(-2, 2, size=(400, 1))).astype(f32)
    Q = (rng.standard_normal((16, d)) * 10.0 ** rng.uniform(-2, 2, size=(16, 1))).astype(f32)
    _check_sound(X, Q, metric, d, "spread norms")


def test_unbounded_radii_and_queries_are_marked():
    u = np.array([1.0, 1.0, 1.0, 1.0, np.nan, 0.0], dtype=f32)
    v = np.zeros(6, dtype=f32)
    r = np.array([0.5, np.nan, np.inf, -np.inf, 0.5, 0.5], dtype=f32)
    thr, marked = rc.range_thr(r, u, v, "cosine", 128, f32(1.0))
    assert marked.tolist() == [False, False, True, True, True, True]
    assert np.isfinite(thr[0]) and thr[0] > 0.5 and np.isneginf(thr[1:]).all()
    thr, marked = rc.range_thr(r[:1], u[:1], v[:1], "l2", 128, f32(np.inf))   # a row norm that overflowed
    assert marked.all() and np.isneginf(thr).all()


@pytest.mark.parametrize("d", rc.I8_DIMS)
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_gpu_cases_stay_within_the_pool(d, metric):
    X, Q = rc.i8_data(d)
    ids, dist = rc.i8_oracle(d, metric)
    S, u, v = _s_lower(X, Q, metric, d)
    max_sumsq = f32((X ** 2).sum(axis=1, dtype=f32).max())
    for rank in rc.I8_RANKS:
        thr, marked = rc.range_thr(dist[:, rank - 1], u, v, metric, d, max_sumsq)
        assert not marked.any()
        through = (S <= thr[None, :]).sum(axis=0)
        assert (through >= rank).all()
        assert through.max() <= 2048, (d, metric, rank, int(through.max()))
    # the overflow case: a radius at the 5 000th distance lets more than a pool through
    thr, marked = rc.range_thr(dist[:64, 4999], u[:64], v[:64], metric, d, max_sumsq)
    assert ((S[:, :64] <= thr[None, :]).sum(axis=0) > 4096).all()
