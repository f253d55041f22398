"""CPU model of the large-k scan route (host logic, no GPU): the cascade of ehx_largek.cpp / k_radius.hip restated in numpy
(tests/largek_cases.py) on the lower-bound model of tests/i8_model.py and range_thr (tests/range_cases.py), for every case
tests/test_knn_largek.py asserts "no query handed on" for.  At every pass of every case:

  (a) no row within the radius lies above the threshold, and no query is one the bound does not serve;
  (b) no pool exceeds kPoolCap / 2 = 2048 — the scan's tiles are ordered by quantisation step with steps raised to their
      lane group's, which loosens the device's bound a little against this model's; half a pool is the headroom;
  (c) the final answer is the oracle's first k in (distance, id) order.

Only shapes that pass here may assert "none handed on" on the GPU.  The test prints the worst pool fill per pass."""
import pytest

import largek_cases as lc

CASES = lc.model_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_cascade_is_sound_exact_and_within_half_a_pool(name):
    X, Q, metric, ks = CASES[name]
    res = lc.cascade(X, Q, metric, ks)     # asserts (a) and (c)
    for k in ks:
        answer, fills = res[k]
        print("%s %s k=%d: worst pool fill per pass %s" % (name, metric, k, fills))
        assert len(answer) == len(Q) and len(fills) == len(lc.passes(len(X)))
        assert max(fills) <= lc.POOL_CAP // 2, "(b) %s k=%d: %s" % (name, k, fills)


def test_the_seed_serves_every_k_of_the_route():
    assert lc.SAMPLE >= 4 * lc.K_MAX                      # S >= 4 k
    for n in (16384, 17000, 20000, 10 ** 6, 2 ** 32 - 1):
        ids = lc.sample_ids(n)
        assert lc.K_MAX <= len(ids) <= lc.SAMPLE and ids[-1] < n and ids[0] == 0
    assert lc.K_MAX * lc.GROWTH <= lc.POOL_CAP // 4       # k g hits of a pass: a quarter of a pool at the largest k
