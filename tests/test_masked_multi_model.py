"""CPU model of the scan route of the kNN under a table of bitmaps, one per query (host logic, no GPU): the pass plan and the
cascade of ehx_masked.cpp / k_radius.hip for several masks in one batch, restated in numpy on range_thr
(tests/range_cases.py) over the int8 bound of tests/i8_model.py (through test_range_model._s_lower), as
tests/test_masked_model.py does it for one bitmap.  Every query draws its first radius from the sample of its OWN mask and
collects the rows its OWN mask allows; the passes are the batch's (masked_multi_cases.passes).

For every GPU case of tests/test_knn_masked_multi.py that pins the route counters — the table of six at dims 128 .. 768, three
metrics, F32 and binary16 rows, k in {1, 10, 48}; the same table under n_bits below the row count (N_BITS, and APPEND_ROWS:
masks built before an append); the parity case — at every pass:
  (a) no row the query's mask allows with D <= radius has S_lower > thr, nothing is marked, and the cascade's answer is the
      oracle's top k of the allowed rows;
  (b) every pool (carried keys + allowed rows through the threshold) stays within half of kPoolCap = 4096.
The test prints the worst fill of every pass before it asserts."""
import functools

import numpy as np
import pytest

import masked_cases as mc
import masked_multi_cases as mmc
import range_cases as rc
import test_range_model as trm
from oracle import pyoracle

f32 = np.float32
N_BITS = 15003          # not a multiple of 32, below the row count: "tenth" stays on the scan route, "last_tenth" is empty
APPEND_ROWS = 19300     # rows when the masks of the append case are built


@functools.lru_cache(maxsize=4)
def _case(X_key, metric):
    """S_lower [rows, queries], the queries' (u, v), max |x|^2 and the oracle's distance of every (row, query) pair"""
    kind, d = X_key
    if kind == "parity":
        X, Q = mmc.parity()[:2]
    else:
        X, Q = rc.i8_data(d)
        Q = Q[:mmc.NQ]
        if kind == "f16":
            X = X.astype(np.float16).astype(f32)
    n = X.shape[0]
    S, u, v = trm._s_lower(X, Q, metric, d)
    oids, odist, ocnt = pyoracle.exhaustive(np.ascontiguousarray(X), Q, n, rc.OM[metric])
    assert (ocnt == n).all()
    D = np.empty((n, Q.shape[0]), dtype=f32)
    for q in range(Q.shape[0]):
        D[oids[q].astype(np.int64), q] = odist[q]
    return S, u, v, f32((X ** 2).sum(axis=1, dtype=f32).max()), D


def _cascade(case, metric, d, tab, mask_of, k):
    """tab: bool [masks, rows the bitmaps cover] (rows beyond are not scanned).  -> (answers of the scan-route queries
    {query: ids}, worst pool fill per pass)"""
    S, u, v, max_sumsq, D = case
    n = tab.shape[1]
    S, D = S[:n], D[:n]
    qs = np.nonzero(mmc.scans(tab)[mask_of])[0]
    A = tab[mask_of[qs]].T                                         # [rows, scan queries]: the query's OWN mask
    radius = np.empty(len(qs), dtype=f32)
    for j, q in enumerate(qs):                                     # stage 0: the exact k-th distance of its mask's sample
        smp = mc.sample_ids(tab[mask_of[q]])
        assert k <= len(smp) <= mc.SAMPLE
        radius[j] = np.sort(D[smp, q])[k - 1]
    carried = [np.zeros(0, dtype=np.int64) for _ in qs]
    fills = []
    for t0, nt in mmc.passes(tab, mask_of):
        lo, hi = t0 * mc.TILE, min((t0 + nt) * mc.TILE, n)
        thr, marked = rc.range_thr(radius, u[qs], v[qs], metric, d, max_sumsq)
        assert not marked.any()
        through_any = S[lo:hi][:, qs] <= thr[None, :]
        through = through_any & A[lo:hi]
        member = A[lo:hi] & (D[lo:hi][:, qs] <= radius[None, :])
        assert not (member & ~through_any).any(), "(a) the threshold hides an allowed row within the radius"
        fills.append(int(max(len(carried[j]) + int(through[:, j].sum()) for j in range(len(qs)))))
        for j, q in enumerate(qs):                                 # radius_rerank_kernel
            pool = np.concatenate([carried[j], lo + np.nonzero(through[:, j])[0]])
            pool = pool[D[pool, q] <= radius[j]]
            pool = pool[np.lexsort((pool, D[pool, q]))][:k]
            if len(pool) == k:
                radius[j] = min(radius[j], D[pool[-1], q])
            carried[j] = pool
    return dict(zip(qs.tolist(), carried)), fills


def _check(case, metric, d, tab, mask_of, what):
    D = case[4]
    for k in mmc.KS:
        answer, fills = _cascade(case, metric, d, tab, mask_of, k)
        print("%s k=%d: passes %s, worst pool fill per pass %s" % (what, k, mmc.passes(tab, mask_of), fills))
        for q, got in answer.items():   # the oracle's top k of the rows the query's own mask allows, ties by id
            L = np.nonzero(tab[mask_of[q]])[0]
            assert np.array_equal(got, L[np.lexsort((L, D[L, q]))][:k]), (what, k, q)
        assert max(fills) <= mc.POOL_CAP // 2, "(b) %s k=%d: %s" % (what, k, fills)


@pytest.mark.parametrize("rows", ["f32", "f16"])
@pytest.mark.parametrize("d", rc.I8_DIMS)
@pytest.mark.parametrize("metric", mmc.METRICS)
def test_the_table_of_six_is_sound_and_stays_within_half_a_pool(metric, d, rows):
    tab, mask_of = mmc.table(), mmc.interleaved(mmc.NQ, len(mmc.NAMES))
    assert mmc.scans(tab).tolist() == [True, True, True, False, False, True]
    assert len(mmc.passes(tab, mask_of)) == 2
    case = _case((rows, d), metric)
    _check(case, metric, d, tab, mask_of, "%s d=%d %s" % (metric, d, rows))
    if rows == "f32" and d == 128:   # masks that end below the row count: n_bits, and an append behind them
        for n_bits in (N_BITS, APPEND_ROWS):
            _check(case, metric, d, tab[:, :n_bits], mask_of, "%s d=%d n_bits=%d" % (metric, d, n_bits))


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_the_parity_case_is_sound_and_stays_within_half_a_pool(metric):
    X, Q, tab, mask_of = mmc.parity()
    assert mmc.scans(tab).all() and len(mmc.passes(tab, mask_of)) == 2
    _check(_case(("parity", X.shape[1]), metric), metric, X.shape[1], tab, mask_of, "parity " + metric)


def test_pass_plan_and_order():
    tab = mmc.table()
    of = mmc.interleaved(mmc.NQ, 6)
    # "ones" sees 4096 rows first: the plan is its plan; without it "half" leads, except where "last_tenth" overtakes it
    assert mmc.passes(tab, of) == mc.passes(tab[5]) == [(0, 16), (16, 63)]
    assert mmc.passes(tab[:1], np.zeros(4, dtype=np.uint32)) == mc.passes(tab[0])
    both = mmc.passes(tab[[0, 2]], mmc.interleaved(8, 2))
    assert both == mc.passes(tab[0]) and sum(nt for _, nt in both) == 79
    sparse = np.zeros((2, 70000), dtype=bool)
    sparse[0, ::16] = True           # 4375 rows, spread: alone one pass would end at tile 256
    sparse[1, 60000:] = True         # 10 000 rows clustered at the end: it reaches 4096 first only behind row 60 000
    p = mmc.passes(sparse, mmc.interleaved(8, 2))
    assert p[0] == (0, 60000 // 256 + 16 + 1) and len(p) == 2
    o = mmc.order(tab, of)
    assert sorted(o.tolist()) == list(range(mmc.NQ))
    assert of[o].tolist() == [0] * 16 + [1] * 16 + [2] * 16 + [5] * 16 + [3] * 16 + [4] * 16
    assert (np.diff(o[:16]) > 0).all()
    assert mmc.order(tab[:1], np.zeros(5, dtype=np.uint32)).tolist() == [0, 1, 2, 3, 4]   # one mask: the batch as it is
