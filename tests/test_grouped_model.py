"""CPU model of the grouped kNN (no GPU): the contract — a plain-Python capped greedy — against a plain-Python model of the
pass-by-pass algorithm of k_grouped.hip (tests/grouped_model.py), on seeded random inputs and on adversarial ones; and, for
every scan case tests/test_knn_grouped.py asserts "none handed on" for, the cascade under the int8 threshold: no query the
bound does not serve and at most kPoolCap / 2 rows through the threshold at every pass — the condition that keeps a GPU test
from hiding a fall-back."""
import numpy as np
import pytest

import grouped_model as gm
import largek_cases as lc

f32 = np.float32


def _both(dist, labels, k, m, ranges, sample=None):
    want = gm.capped_greedy(gm.ordered_rows(dist), labels, k, m)
    got, radii, _ = gm.passes_model(dist, labels, k, m, ranges, sample=sample)
    assert got == want, (k, m)
    assert all(a >= b for a, b in zip(radii, radii[1:]))   # the radius only falls
    return want


@pytest.mark.parametrize("seed", range(6))
def test_passes_agree_with_the_greedy_on_random_inputs(seed):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(1, 900))
    dist = rng.standard_normal(n).astype(f32)
    dist[rng.integers(0, n, size=n // 5)] = dist[0]                       # ties
    dist[rng.integers(0, n, size=n // 20)] = np.nan                       # never neighbours
    dist[rng.integers(0, n, size=3)] = np.inf
    labels = rng.integers(0, max(2, n // int(rng.integers(1, 30))), size=n).astype(np.uint32)
    labels[rng.integers(0, n, size=n // 7)] = gm.NONE
    step = int(rng.integers(1, 200))
    ranges = [(lo, min(lo + step, n)) for lo in range(0, n, step)]
    for k in (1, 2, 7, 50, 256):
        for m in (1, 2, 5, 256, 2 ** 32 - 1):
            _both(dist, labels, k, m, ranges)
            _both(dist, labels, k, m, ranges, sample=np.arange(0, n, 3))


def test_consequences_of_the_contract():
    rng = np.random.default_rng(7)
    dist = rng.standard_normal(500).astype(f32)
    order = gm.ordered_rows(dist)
    labels = (np.arange(500) % 9).astype(np.uint32)
    for k in (1, 10, 100):
        assert gm.capped_greedy(order, labels, k, k) == order[:k]                         # per_group >= k: plain kNN
        assert gm.capped_greedy(order, np.full(500, gm.NONE, np.uint32), k, 1) == order[:k]
    best = gm.capped_greedy(order, labels, 100, 1)                                        # collapse: 9 groups exist
    assert len(best) == 9 and sorted(int(labels[r]) for r in best) == list(range(9))
    for g in range(9):
        assert best[[int(labels[r]) for r in best].index(g)] == min((r for r in order if labels[r] == g), key=order.index)


def test_adversarial_a_carried_key_is_displaced_by_a_later_pass():
    # rows 0..9: group 5 at distances 10..19, carried after pass 0 at m = 2; pass 1 brings two nearer rows of group 5
    dist = np.array([10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 1, 2, 30, 31], dtype=f32)
    labels = np.array([5] * 10 + [5, 5, 6, 7], dtype=np.uint32)
    want = _both(dist, labels, 3, 2, [(0, 10), (10, 14)])
    assert want == [10, 11, 12]                       # rows 0 and 1, carried, are displaced; 12 (group 6) enters
    # the first m of a group straddle a range edge
    want = _both(dist, labels, 4, 3, [(0, 11), (11, 14)])
    assert want == [10, 11, 0, 12]
    # a giant group: fewer than k groups exist
    labels = np.array([1] * 13 + [2], dtype=np.uint32)
    assert _both(dist, labels, 10, 1, [(0, 5), (5, 14)]) == [10, 13]
    # ties fall by id, within a group and across groups, across ranges
    dist = np.zeros(12, dtype=f32)
    labels = np.array([3, 3, 4, 4, 3, 4, 8, 8, 8, gm.NONE, gm.NONE, 3], dtype=np.uint32)
    assert _both(dist, labels, 6, 1, [(0, 4), (4, 8), (8, 12)]) == [0, 2, 6, 9, 10]
    assert _both(dist, labels, 6, 2, [(0, 4), (4, 8), (8, 12)]) == [0, 1, 2, 3, 6, 7]


def test_slabs_and_scan_ranges_cover_the_prefix():
    for n in (0, 1, 4095, 4096, 4097, 8193, 20000):
        s = gm.slabs(n)
        assert s[0][0] == 0 and s[-1][1] == n and all(a[1] == b[0] for a, b in zip(s, s[1:]))
        assert all(hi - lo <= gm.POOL_CAP for lo, hi in s)
    r = gm.scan_ranges(20000)
    assert len(r) == 3 and r[0][0] == 0 and r[-1][1] == 20000 and all(a[1] == b[0] for a, b in zip(r, r[1:]))


@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_the_scan_cases_that_assert_none_handed_on_clear_the_model(metric):
    X, Q = lc.gauss(20000, 64, 64, 1)
    _, _, full, D, _, _, _, _ = gm._scan_inputs(metric)
    for lab, k, m in gm.scan_cases():
        labels = gm.LABELINGS[lab](len(X))
        answers, fills, unserved = gm.scan_cascade(metric, labels, k, m)
        print("%s %s k=%d m=%d: worst pool fill per pass %s, unserved %d" % (metric, lab, k, m, fills, unserved))
        for q in range(len(Q)):   # the algorithm is exact whether the case is cleared or not
            assert answers[q] == gm.capped_greedy([int(v) for v in full[0][q]], labels, k, m), (lab, k, m, q)
        clear = unserved == 0 and max(fills) <= gm.POOL_CAP // 2
        assert clear == gm.cleared(lab, k, m), (metric, lab, k, m, fills, unserved)
