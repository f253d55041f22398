"""CPU model of the masked kNN's scan route (host logic, no GPU): the cascade of ehx_masked.cpp / k_radius.hip restated in
numpy on top of range_thr (tests/range_cases.py) and the int8 bound of tests/test_i8_model.py, as tests/test_range_model.py
does it.  Data: range_cases.i8_data(d), 20 000 rows, all 257 queries; bitmaps: tests/masked_cases.py; k in {1, 10, 48}.

  (a) soundness: at every pass no allowed row with D <= radius has S_lower > thr (D: the oracle's distance; the oracle's
      6 000 nearest per query are enough — every radius met lies below the 6 000th distance, asserted), and the cascade's
      answer is the oracle's top k of the allowed rows;
  (b) the GPU cases of tests/test_knn_masked.py stay within half a pool: carried keys + allowed rows through the threshold
      <= 2048 of kPoolCap = 4096 per pass and query;
  (c) without the bitmap in the scan's flush the pools would not do: for the 10 % bitmap at k = 48 the rows of ANY kind
      through the threshold exceed kPoolCap;
  (d) the same (a) and (b) for masked_cases.merge_cases(), the GPU cases of the merge of a pass's hits into the carried
      keys (k_radius.hip carries the keys beside the pool: (b), which still counts them, is the stricter statement).

Figures of one run, the worst query of the worst pass, as ranges over d in {128, 192, 384, 768} x {cosine, L2} (the test
prints every one of them before it asserts):
  bitmap              k = 10     k = 48
  50 % random         351-463    1059-1336
  50 % tail           367-461    1174-1363
  all ones            328-501    1089-1235
  10 % random         154-214     528-626     rows of ANY kind through the threshold at k = 48: 5347-6115"""
import functools

import numpy as np
import pytest

import masked_cases as mc
import range_cases as rc
import test_range_model as trm
from oracle import pyoracle

f32 = np.float32


@functools.lru_cache(maxsize=None)
def _case(d, metric):
    """S_lower [rows, queries], the queries' (u, v), max |x|^2, and the oracle's distances as a dense matrix: D[row, query],
    +Inf where the row is not among the query's 6 000 nearest (floor[query] = the 6 000th distance)"""
    X, Q = rc.i8_data(d)
    S, u, v = trm._s_lower(X, Q, metric, d)
    oids, odist = rc.i8_oracle(d, metric)
    D = np.full((X.shape[0], Q.shape[0]), np.inf, dtype=f32)
    for q in range(Q.shape[0]):
        D[oids[q].astype(np.int64), q] = odist[q]
    max_sumsq = f32((X ** 2).sum(axis=1, dtype=f32).max())
    return S, u, v, max_sumsq, D, odist[:, -1].copy()


@functools.lru_cache(maxsize=None)
def _merge_case(name):
    """_case for the rows and queries of masked_cases.merge_cases()[name]: every distance of the oracle, no floor"""
    X, Q, metric = mc.merge_cases()[name][:3]
    n, d = X.shape
    S, u, v = trm._s_lower(X, Q, metric, d)
    oids, odist, ocnt = pyoracle.exhaustive(X, Q, n, rc.OM[metric])
    assert (ocnt == n).all()
    D = np.empty((n, Q.shape[0]), dtype=f32)
    for q in range(Q.shape[0]):
        D[oids[q].astype(np.int64), q] = odist[q]
    return S, u, v, f32((X ** 2).sum(axis=1, dtype=f32).max()), D, np.full(Q.shape[0], np.inf, dtype=f32)


def _cascade(case, metric, d, allowed, k):
    """case: _case's tuple.  -> (answer ids [nq, k], worst pool fill per pass [passes], rows of any kind through the threshold
    per pass)"""
    S, u, v, max_sumsq, D, floor = case
    n, nq = D.shape
    smp = mc.sample_ids(allowed)
    assert k <= len(smp) <= mc.SAMPLE
    radius = np.sort(D[smp], axis=0)[k - 1].astype(f32)          # stage 0: the sample's exact k-th distance
    assert (radius < floor).all(), "a radius beyond the oracle's 6 000th distance: deepen range_cases.i8_oracle"
    carried = [np.zeros(0, dtype=np.int64) for _ in range(nq)]
    fills, anys = [], []
    for t0, nt in mc.passes(allowed):
        lo, hi = t0 * mc.TILE, min((t0 + nt) * mc.TILE, n)
        thr, marked = rc.range_thr(radius, u, v, metric, d, max_sumsq)
        assert not marked.any()
        through_any = S[lo:hi] <= thr[None, :]
        through = through_any & allowed[lo:hi, None]
        member = allowed[lo:hi, None] & (D[lo:hi] <= radius[None, :])
        assert not (member & ~through_any).any(), "(a) the threshold hides an allowed row within the radius"
        fills.append(int(max(len(carried[q]) + int(through[:, q].sum()) for q in range(nq))))
        anys.append(int(through_any.sum(axis=0).max()))
        for q in range(nq):                                       # radius_rerank_kernel
            pool = np.concatenate([carried[q], lo + np.nonzero(through[:, q])[0]])
            pool = pool[D[pool, q] <= radius[q]]
            pool = pool[np.lexsort((pool, D[pool, q]))][:k]
            if len(pool) == k:
                radius[q] = min(radius[q], D[pool[-1], q])
            carried[q] = pool
    return carried, fills, anys


@pytest.mark.parametrize("d", rc.I8_DIMS)
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_cascade_is_sound_and_the_gpu_cases_stay_within_half_a_pool(d, metric):
    S, u, v, max_sumsq, D, floor = _case(d, metric)
    n, nq = D.shape
    for name, allowed in mc.masks(n).items():
        assert allowed.sum() > mc.exact_cut(n), "the case must take the scan route"
        assert len(mc.passes(allowed)) == mc.PASSES[name]
        L = np.nonzero(allowed)[0]
        for k in mc.KS:
            answer, fills, anys = _cascade(_case(d, metric), metric, d, allowed, k)
            print("%s d=%d %s k=%d: worst pool fill per pass %s, rows of any kind %s" % (metric, d, name, k, fills, anys))
            for q in range(nq):   # the oracle's top k of the allowed rows, ties by id
                want = L[np.lexsort((L, D[L, q]))][:k]
                assert np.array_equal(answer[q], want), (name, k, q)
            assert max(fills) <= mc.POOL_CAP // 2, "(b) %s k=%d: %s" % (name, k, fills)
            if name == "tenth" and k == 48:
                assert max(anys) > mc.POOL_CAP, "(c) an unmasked pool would do: %s" % anys


@pytest.mark.parametrize("name", ["ties", "short", "f16"])
def test_the_merge_cases_are_sound_and_stay_within_half_a_pool(name):
    X, Q, metric, bitmaps, ks = mc.merge_cases()[name]
    D = _merge_case(name)[4]
    for bname, allowed in bitmaps.items():
        assert allowed.sum() > mc.exact_cut(len(X)), "the case must take the scan route"
        assert len(mc.passes(allowed)) == 2
        L = np.nonzero(allowed)[0]
        for k in ks:
            answer, fills, _ = _cascade(_merge_case(name), metric, X.shape[1], allowed, k)
            print("%s %s k=%d: worst pool fill per pass %s" % (name, bname, k, fills))
            for q in range(len(Q)):
                want = L[np.lexsort((L, D[L, q]))][:k]
                assert np.array_equal(answer[q], want), (name, bname, k, q)
            assert max(fills) <= mc.POOL_CAP // 2, "(d) %s %s k=%d: %s" % (name, bname, k, fills)


def test_pass_plan():
    n = 20000
    m = mc.masks(n)
    assert [nt for _, nt in mc.passes(m["ones"])] == [16, 63]            # 4096 rows = 16 tiles, then the rest of 79
    assert mc.passes(m["tenth"]) == [(0, 79)]
    t = mc.passes(m["tail"])
    # (tile 39 holds 240 allowed rows, with 15 more tiles 4080: the 16th passes 4096)
    assert t[0][0] == 0 and t[0][1] == 39 + 1 + 16 and sum(nt for _, nt in t) == 79
    assert mc.passes(np.ones(256 * 16, dtype=bool)) == [(0, 16)]          # exactly 4096: nothing is left for a second pass
    assert mc.passes(np.ones(70000, dtype=bool)) == [(0, 16), (16, 240), (256, 18)]
    sparse = np.zeros(70000, dtype=bool)
    sparse[60000:] = True                                                 # a bitmap clustered at the end of the id space
    assert [t0 for t0, _ in mc.passes(sparse)] == [0, 60000 // 256 + 16 + 1]
    assert len(mc.sample_ids(m["half"])) <= 256 and len(mc.sample_ids(np.ones(257, dtype=bool))) == 129
