"""CPU model of the grouped kNN under row bitmaps (no GPU): the contract — the oracle's order with the rows that are not
allowed dropped, then tests/grouped_model.py's capped greedy — against the pass-by-pass model of the scan route
(tests/grouped_masked_model.py: the sample of the allowed rows by rank, the unfiltered passes, a `through` that lets only
allowed rows take a pool slot), for every scan case tests/test_knn_grouped_masked.py asserts "none handed on" for: no query
the bound does not serve and at most kPoolCap / 2 rows through at every pass."""
import numpy as np
import pytest

import grouped_masked_model as gmm
import grouped_model as gm
import largek_cases as lc

f32 = np.float32


def test_filter_first_then_cap_on_a_hand_made_case():
    # group 5: rows 0 (nearest, forbidden), 1, 2; group 6: row 3; row 4 a group of its own, forbidden
    full = (np.array([[0, 1, 3, 4, 2]], dtype=np.uint64), np.array([[1, 2, 3, 4, 5]], dtype=f32), np.array([5], dtype=np.uint32))
    labels = np.array([5, 5, 5, 6, gm.NONE], dtype=np.uint32)
    allow = np.array([False, True, True, True, False])
    (ids, dist), = gmm.expected(full, labels, allow, None, 4, 1)
    assert ids.tolist() == [1, 3] and dist.tolist() == [2, 3]           # the group's nearest ALLOWED row, not row 0
    (ids, _), = gmm.expected(full, labels, allow, None, 4, 2)
    assert ids.tolist() == [1, 3, 2]                                     # the forbidden row 0 does not use up the cap
    (ids, _), = gmm.expected(full, labels, [allow, ~allow], [1], 4, 2)
    assert ids.tolist() == [0, 4]                                        # query 0 under the other bitmap
    (ids, _), = gmm.expected(full, labels, np.ones(5, dtype=bool), None, 4, 1, n_eff=3)
    assert ids.tolist() == [0]                                           # rows at or above n_eff are not allowed
    (ids, _), = gmm.expected(full, labels, np.zeros(5, dtype=bool), None, 4, 1)
    assert ids.tolist() == []


def test_the_sample_is_strided_by_rank():
    a = np.zeros(20000, dtype=bool)
    a[::3] = True                                                        # 6667 allowed rows: stride 7
    s = gmm.sample_of(a)
    assert len(s) == 953 and s[0] == 0 and s[1] == 21 and a[s].all() and len(s) <= gmm.SAMPLE
    assert gmm.sample_of(np.zeros(10, dtype=bool)).tolist() == []
    assert gmm.sample_of(np.ones(1024, dtype=bool)).tolist() == list(range(1024))
    assert len(gmm.sample_of(np.ones(1025, dtype=bool))) == 513


@pytest.mark.parametrize("density", gmm.SCAN_DENSITIES)
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_the_scan_cases_that_assert_none_handed_on_clear_the_model(metric, density):
    X, Q = lc.gauss(20000, 64, 64, 1)
    full = gm.scan_oracle(metric)
    allows, mask_of = gmm.scan_bitmaps(density), gmm.scan_mask_of(len(Q))
    worst = 0
    for _, lab, k, m in (c for c in gmm.scan_cases() if c[0] == density):
        labels = gm.LABELINGS[lab](len(X))
        answers, fills, unserved = gmm.scan_cascade(metric, labels, allows, mask_of, k, m)
        print("%s density %g %s k=%d m=%d: worst pool fill per pass %s, unserved %d" % (metric, density, lab, k, m, fills, unserved))
        want = gmm.expected(full, labels, allows, mask_of, k, m)
        for q in range(len(Q)):   # the algorithm is exact whether the case is cleared or not
            assert answers[q] == [int(v) for v in want[q][0]], (density, lab, k, m, q)
        assert unserved == 0, (metric, density, lab, k, m)
        assert max(fills) <= gm.POOL_CAP // 2, (metric, density, lab, k, m, fills)
        assert gmm.cleared(density, lab, k, m)
        worst = max(worst, max(fills))
    print("%s density %g: worst pool fill %d of %d" % (metric, density, worst, gm.POOL_CAP))
