"""CPU tests of tests/prefix_oracle.py: the merged prefix answers are the oracle's own, and an answer torn between two
prefixes — page 1 of one, page 2 of another — is rejected."""
import numpy as np
import pytest

from oracle import pyoracle
from prefix_oracle import PrefixOracle


def _data(metric, d=32, n=3000, nq=24, seed=3):
    r = np.random.default_rng(seed)
    X = r.standard_normal((n, d)).astype(np.float32)
    Q = X[r.integers(0, 400, nq)] + np.float32(0.05) * r.standard_normal((nq, d)).astype(np.float32)
    if metric == pyoracle.METRIC_COSINE:
        X[n - 700:] = X[r.integers(0, 400, 700)] * np.float32(1.5)   # late rows that change the early answers
    else:
        X[n - 700:] = X[r.integers(0, 400, 700)] + np.float32(0.02) * r.standard_normal((700, d)).astype(np.float32)
    return X, Q


@pytest.mark.parametrize("metric", [pyoracle.METRIC_L2, pyoracle.METRIC_COSINE])
@pytest.mark.parametrize("k", [10, 128])
def test_merged_prefix_answers_are_the_oracles_own(metric, k):
    X, Q = _data(metric)
    bounds = [1000, 1001, 1700, 2333, 2999, 3000]
    po = PrefixOracle(X, Q, k, metric, bounds)
    for b in bounds:
        oids, odist, ocnt = pyoracle.exhaustive(X[:b], Q, k, metric)
        ids, dist, cnt = po.answer(b)
        np.testing.assert_array_equal(cnt, ocnt)
        np.testing.assert_array_equal(ids, oids)
        assert dist.tobytes() == odist.tobytes()
        assert po.assert_is_some_prefix(oids, odist, ocnt, b, b) == b
        assert po.assert_is_some_prefix(oids, odist, ocnt, bounds[0], bounds[-1]) in bounds


def test_short_prefixes_merge_with_partial_counts():
    X, Q = _data(pyoracle.METRIC_L2)
    X = X[:40]
    po = PrefixOracle(X, Q, 16, pyoracle.METRIC_L2, [5, 12, 40])
    for b in (5, 12, 40):
        oids, odist, ocnt = pyoracle.exhaustive(X[:b], Q, 16, pyoracle.METRIC_L2)
        ids, dist, cnt = po.answer(b)
        np.testing.assert_array_equal(cnt, ocnt)
        for q in range(len(Q)):
            np.testing.assert_array_equal(ids[q, :cnt[q]], oids[q, :ocnt[q]])
            assert dist[q, :cnt[q]].tobytes() == odist[q, :ocnt[q]].tobytes()


def test_a_torn_answer_is_rejected():
    """page 1 (results 0..63) from X[:b1], page 2 (64..127) from X[:b2]: the top-128 of no prefix"""
    metric, k = pyoracle.METRIC_L2, 128
    X, Q = _data(metric)
    b1, b2 = 2333, 3000
    po = PrefixOracle(X, Q, k, metric, [1000, b1, b2])
    i1, d1, c1 = po.answer(b1)
    i2, d2, c2 = po.answer(b2)
    assert not np.array_equal(i1[:, 64:], i2[:, 64:]), "the data must make the pages differ"
    ids, dist = i1.copy(), d1.copy()
    ids[:, 64:], dist[:, 64:] = i2[:, 64:], d2[:, 64:]
    with pytest.raises(AssertionError, match="no published prefix"):
        po.assert_is_some_prefix(ids, dist, c1, 1000, b2)
    # one query from another prefix is a tear too
    ids, dist = i1.copy(), d1.copy()
    q = int(np.nonzero((i1 != i2).any(axis=1))[0][0])
    ids[q], dist[q] = i2[q], d2[q]
    with pytest.raises(AssertionError, match="no published prefix"):
        po.assert_is_some_prefix(ids, dist, c1, 1000, b2)
    # the same distances with one id changed, and the same ids with one distance a bit off: rejected
    ids = i2.copy()
    ids[0, 5] = ids[0, 6]
    with pytest.raises(AssertionError):
        po.assert_is_some_prefix(ids, d2, c2, b2, b2)
    dist = d2.copy()
    dist[3, 7] = np.nextafter(dist[3, 7], np.float32(np.inf))
    with pytest.raises(AssertionError):
        po.assert_is_some_prefix(i2, dist, c2, b2, b2)
    # a correct answer outside [lo, hi] is rejected as well
    with pytest.raises(AssertionError):
        po.assert_is_some_prefix(i1, d1, c1, b2, b2)
