"""The oracle's exhaustive answer on non-finite and extreme values (CPU only).

The reference rule every engine is held to: the first k (query, row) pairs in (canonical distance, id) order, where a
pair whose distance is NaN is no neighbour (counts may then be < k) and +-Inf distances are ordinary keys.  Checked here
against a brute force built pair by pair from pyoracle.dist / pyoracle.normalize.
"""
import numpy as np
import pytest

from oracle import pyoracle

NEG_NAN = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]
POS_NAN = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]


def _odd_rows(rng, n, d):
    """n Gaussian rows with every kind of odd row at fixed places"""
    X = rng.standard_normal((n, d)).astype(np.float32)
    X[1, 3] = POS_NAN
    X[2, 0] = NEG_NAN
    X[3, d - 1] = np.inf
    X[4, 2] = -np.inf
    X[5] = 0.0
    X[6] = 0.0
    X[7] = rng.standard_normal(d).astype(np.float32) * np.float32(1e19)   # finite, L2 distances overflow
    X[8] = np.float32(3e38)                                                 # sumsq overflows: cosine -> zero row
    X[9] = np.float32(1e-21)                                                # subnormal products
    X[10, :] = POS_NAN
    X[11] = X[12]                                                           # an exact tie
    return X


def _brute(X, Q, k, metric):
    if metric == pyoracle.METRIC_COSINE:
        X = np.stack([pyoracle.normalize(x) for x in X])
        Q = np.stack([pyoracle.normalize(q) for q in Q])
        metric = pyoracle.METRIC_IP
    out = []
    for q in Q:
        pairs = []
        for i, x in enumerate(X):
            d = np.float32(pyoracle.dist(metric, q, x))
            if not np.isnan(d):
                pairs.append((float(d), i))
        out.append(sorted(pairs)[:k])
    return out


@pytest.mark.parametrize("metric", [pyoracle.METRIC_L2, pyoracle.METRIC_IP, pyoracle.METRIC_COSINE])
@pytest.mark.parametrize("d", [16, 19])
@pytest.mark.parametrize("k", [3, 40, 100])
def test_exhaustive_skips_nan_pairs_and_orders_inf(metric, d, k):
    rng = np.random.default_rng(d * 7 + metric)
    n = 64
    X = _odd_rows(rng, n, d)
    Q = rng.standard_normal((10, d)).astype(np.float32)
    Q[1] = 0.0
    Q[2, 1] = POS_NAN
    Q[3, 4] = NEG_NAN
    Q[4, 0] = np.inf
    Q[5, 2] = -np.inf
    Q[6] = X[7]
    Q[7] = np.float32(1e-21)
    Q[8] = X[8]
    ids, dist, cnt = pyoracle.exhaustive(X, Q, k, metric, threads=3)
    want = _brute(X, Q, k, metric)
    for i, w in enumerate(want):
        c = int(cnt[i])
        assert c == len(w), (i, c, len(w))
        assert ids[i, :c].tolist() == [p[1] for p in w], i
        assert dist[i, :c].tobytes() == np.array([p[0] for p in w], dtype=np.float32).tobytes(), i
    # the rule at work: a NaN query has no neighbour, NaN rows are never one, Inf distances are
    assert cnt[2] == 0 and cnt[3] == 0
    for r in (1, 2, 10):
        assert r not in ids[cnt[:, None] > np.arange(k)[None, :]].tolist()
    if metric == pyoracle.METRIC_L2 and k == 100:
        assert np.isposinf(dist[0, :cnt[0]]).any() and cnt[0] < n   # row 7 at +Inf; NaN rows missing
    if metric == pyoracle.METRIC_COSINE and k == 100:   # the sumsq-overflow row normalises to zero: distance 1
        row = ids[0, :cnt[0]].tolist()
        assert 8 in row and dist[0, row.index(8)] == np.float32(1.0)


def test_exhaustive_is_unchanged_on_finite_rows():
    """NaN-free input: the (dist, id) answer of the row-blocked scan equals the pairwise brute force"""
    rng = np.random.default_rng(3)
    X = rng.standard_normal((300, 24)).astype(np.float32)
    X[100:110] = X[5]
    Q = rng.standard_normal((6, 24)).astype(np.float32)
    for metric in (pyoracle.METRIC_L2, pyoracle.METRIC_IP, pyoracle.METRIC_COSINE):
        ids, dist, cnt = pyoracle.exhaustive(X, Q, 20, metric, threads=4)
        want = _brute(X, Q, 20, metric)
        assert (cnt == 20).all()
        for i, w in enumerate(want):
            assert ids[i].tolist() == [p[1] for p in w]
            assert dist[i].tobytes() == np.array([p[0] for p in w], dtype=np.float32).tobytes()
