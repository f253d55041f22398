"""Helper of the tests of the range search under row bitmaps (no test here): the oracle's answers under the table of six of
tests/masked_multi_cases.py, the radii of the cases, and a numpy restatement of how many rows the int8 scan's bound lets
through for a query under its mask (tests/test_range_model.py's bound and tests/range_cases.py's threshold), shared by the
CPU model (tests/test_range_masked_model.py) and the GPU tests (tests/test_range_masked.py)."""
import functools

import numpy as np

import masked_multi_cases as mmc
import range_cases as rc
from oracle import pyoracle

f32 = np.float32
DIMS = (128, 768)
RANKS = rc.I8_RANKS                   # radii at the oracle's j-th ALLOWED distance
MAX_RESULTS = rc.I8_MAX_RESULTS       # 256: rank 300 truncates
POOL = 4096                           # kPoolCap
SCAN_MASKS = (0, 1, 2, 5)             # half, tenth, last_tenth, ones: more than the cut of 1024 rows allowed
LIST_MASKS = (3, 4)                   # few, empty


def rows_as_stored(X, rows):
    return X.astype(np.float16).astype(f32) if rows == "f16" else X


def lists_under(X, Q, om, tab, mask_of):
    """{mask: (queries under it, ids [nq_m, allowed_m] mapped back to rows, dist, cnt)}: the oracle's sorted list of EVERY
    allowed row for every query of the mask; tab: bool [masks, <= rows]"""
    out = {}
    for m in np.unique(mask_of):
        at = np.nonzero(mask_of == m)[0]
        L = np.nonzero(np.asarray(tab[m])[:X.shape[0]])[0]
        if L.size == 0:
            out[int(m)] = (at, np.zeros((len(at), 0), dtype=np.uint64), np.zeros((len(at), 0), dtype=f32),
                           np.zeros(len(at), dtype=np.uint32))
            continue
        oi, od, oc = pyoracle.exhaustive(np.ascontiguousarray(X[L]), np.ascontiguousarray(Q[at]), len(L), om)
        out[int(m)] = (at, L[oi.astype(np.int64)].astype(np.uint64), od, oc)
    return out


def radii_at(lists, nq, rank, none=f32(1.0)):
    """radius per query: its rank-th allowed distance, the last one where its mask allows fewer, `none` under an empty mask"""
    r = np.full(nq, none, dtype=f32)
    for at, ids, dist, cnt in lists.values():
        for j, i in enumerate(at):
            if cnt[j]:
                r[i] = dist[j, min(rank, int(cnt[j])) - 1]
    return r


def want(lists, nq, radius, max_results):
    """[(ids, dist, total)] per query: every mask's lists cut at the queries' radii (range_cases.cut)"""
    out = [None] * nq
    for at, ids, dist, cnt in lists.values():
        for i, w in zip(at, rc.cut(ids, dist, cnt, radius[at], max_results)):
            out[i] = w
    return out


@functools.lru_cache(maxsize=None)
def six(d, metric, rows="f32"):
    """the table of six over range_cases.i8_data(d): (stored rows, queries, table, mask_of, lists_under)"""
    X, Q = rc.i8_data(d)
    Q = Q[:mmc.NQ]
    tab, of = mmc.table(), mmc.interleaved(mmc.NQ, len(mmc.NAMES))
    Xs = rows_as_stored(X, rows)
    return Xs, Q, tab, of, lists_under(Xs, Q, rc.OM[metric], tab, of)


@functools.lru_cache(maxsize=None)
def through(d, metric):
    """{rank: per scan-route query of six(d, metric) the ALLOWED rows the int8 bound lets through at the rank's radius, or
    -1 where the threshold marks the query as one the bound does not serve} — fp32 rows"""
    from test_range_model import _s_lower
    X, Q, tab, of, lists = six(d, metric)
    S, u, v = _s_lower(X, Q, metric, d)
    max_sumsq = f32((X ** 2).sum(axis=1, dtype=f32).max())
    at = np.nonzero(np.isin(of, SCAN_MASKS))[0]
    out = {}
    for rank in RANKS:
        thr, marked = rc.range_thr(radii_at(lists, len(Q), rank), u, v, metric, d, max_sumsq)
        n = ((S[:, at] <= thr[None, at]) & tab[of[at]].T).sum(axis=0)
        out[rank] = np.where(marked[at], -1, n)
    return out


def pinned(d, metric, rank):
    """the route counters of this case are pinned: no scan-route query is marked and none collects more than half a pool"""
    n = through(d, metric)[rank]
    return bool((n >= 0).all() and n.max() <= POOL // 2)
