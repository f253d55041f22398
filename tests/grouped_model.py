"""Helper of the grouped-kNN tests (no test here): the contract of ehx_knn_grouped as a plain-Python capped greedy, a
plain-Python model of the pass-by-pass algorithm of k_grouped.hip / ehx_grouped.cpp (sample, passes, cap, merge, cap,
falling radius), the data and labelings of the GPU cases of tests/test_knn_grouped.py, and the scan route's cascade on top
of the int8 lower bound and range_thr that tests/largek_cases.py models the large-k route with."""
import functools

import numpy as np

import largek_cases as lc
import range_cases as rc
from oracle import pyoracle

f32 = np.float32
NONE = 0xFFFFFFFF        # EHX_GROUP_NONE
POOL_CAP = lc.POOL_CAP   # kPoolCap: rows of one slab of the exact route, and the scan route's pool
K_MAX = 256              # EHX_MAX_K_GROUPED
SCAN_KS = (1, 10, 48, 100, 256)
SCAN_MS = (1, 4)


# ---- the contract ----

def ordered_rows(dist):
    """row ids of one query in (distance, id) order; NaN is never a neighbour"""
    d = np.asarray(dist)
    ids = np.nonzero(~np.isnan(d))[0]
    return [int(i) for i in ids[np.lexsort((ids, d[ids]))]]


def capped_greedy(order, labels, k, m):
    """The first k ELIGIBLE rows of `order` (row ids in (distance, id) order): a row is eligible iff its label is NONE or
    fewer than m rows of its label precede it.  Plain Python, one row at a time."""
    seen, out = {}, []
    for r in order:
        g = int(labels[r])
        if g != NONE:
            if seen.get(g, 0) >= m:
                continue
            seen[g] = seen.get(g, 0) + 1
        out.append(r)
        if len(out) == k:
            break
    return out


# ---- the algorithm, pass by pass ----

def _cap(rows, labels, m):
    """cap_sorted: `rows` in key order, every row dropped that is not among the first m of its label in `rows`"""
    seen, out = {}, []
    for r in rows:
        g = int(labels[r])
        if g != NONE:
            if seen.get(g, 0) >= m:
                continue
            seen[g] = seen.get(g, 0) + 1
        out.append(r)
    return out


def _key(dist):
    return lambda r: (dist[r], r)


def passes_model(dist, labels, k, m, ranges, sample=None, through=None, carried_at=None):
    """grouped_rerank_kernel over the row ranges [(lo, hi)] for one query.  dist: [rows] canonical distances (NaN: never a
    neighbour).  sample: row ids re-ranked in seed mode (their capped k-th distance is the first radius, +Inf below k
    capped rows; nothing is carried), or None: the exact route, radius +Inf first.  through(j, lo, hi, radius) -> bool
    [hi - lo]: the rows the scan of pass j lets through (None: all).  carried_at: a list that receives the number of keys
    carried into every pass, before `through` is asked about it.  -> (answer, radius in front of every pass, rows within the
    radius at every pass)."""
    key = _key(dist)
    ok = ~np.isnan(dist)
    radius = np.inf
    if sample is not None:
        s = _cap(sorted((int(r) for r in sample if ok[r]), key=key), labels, m)[:k]
        if len(s) == k:
            radius = dist[s[-1]]
    carried, radii, within = [], [], []
    for j, (lo, hi) in enumerate(ranges):
        radii.append(radius)
        if carried_at is not None:
            carried_at.append(len(carried))
        sel = ok[lo:hi] & (dist[lo:hi] <= radius)
        within.append(int(sel.sum()))
        if through is not None:
            t = through(j, lo, hi, radius)
            assert not (sel & ~t).any(), "the threshold hides a row within the radius"
        hits = sorted((lo + int(i) for i in np.nonzero(sel)[0]), key=key)
        a = _cap(hits, labels, m)[:k]                       # A: the hits capped, cut at k
        merged = sorted(a + carried, key=key)               # B: merged with the carried keys, capped again, cut at k
        carried = _cap(merged, labels, m)[:k]
        if len(carried) == k:
            assert dist[carried[-1]] <= radius              # the radius only falls
            radius = dist[carried[-1]]
    return carried, radii, within


def slabs(n):
    """the exact route's row ranges: consecutive slabs of kPoolCap rows (one empty slab when there is no row)"""
    return [(lo, min(lo + POOL_CAP, n)) for lo in range(0, max(n, 1), POOL_CAP)]


def scan_ranges(n):
    return [(t0 * lc.TILE, min((t0 + nt) * lc.TILE, n)) for t0, nt in lc.passes(n)]


# ---- labelings ----

def labels_mod37(n):
    """row % 37, every 11th row a group of its own"""
    g = (np.arange(n, dtype=np.int64) % 37).astype(np.uint32)
    g[::11] = NONE
    return g


def labels_scattered(n):
    return ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(2000)).astype(np.uint32)


def labels_clustered(n):
    return (np.arange(n, dtype=np.int64) // 10).astype(np.uint32)


LABELINGS = {"scattered": labels_scattered, "clustered": labels_clustered}


# ---- the expected answer of a GPU case: the oracle's distances of every prefix row, capped by the greedy ----

def oracle_all(X, Q, metric):
    """the oracle's full lists: ids [nq, n], dist [nq, n], counts (rows whose distance is NaN are not listed)"""
    return pyoracle.exhaustive(np.ascontiguousarray(X), np.ascontiguousarray(Q), len(X), rc.OM[metric])


def expected(full, labels, k, m):
    """-> [(ids, distances)] per query from oracle_all's lists: the greedy over the listed rows, in the oracle's order"""
    oids, odist, ocnt = full
    out = []
    for i in range(len(ocnt)):
        c = int(ocnt[i])
        got = capped_greedy(range(c), np.asarray(labels)[oids[i, :c].astype(np.int64)], k, m)   # positions in the oracle's list
        out.append((oids[i, got].astype(np.uint64), odist[i, got].astype(f32)))
    return out


@functools.lru_cache(maxsize=None)
def scan_oracle(metric):
    """the oracle's full lists for the scan cases' data, lc.gauss(20000, 64, 64, 1)"""
    X, Q = lc.gauss(20000, 64, 64, 1)
    full = oracle_all(X, Q, metric)
    assert (full[2] == len(X)).all()
    return full


# ---- the scan route's cascade (largek_cases.cascade with the cap) ----

@functools.lru_cache(maxsize=None)
def _scan_inputs(metric):
    X, Q = lc.gauss(20000, 64, 64, 1)
    full = scan_oracle(metric)
    D = np.empty((len(Q), len(X)), dtype=f32)
    for q in range(len(Q)):
        D[q, full[0][q].astype(np.int64)] = full[1][q]
    S, u, v = lc._s_lower(X, Q, metric, X.shape[1])
    return X, Q, full, D, S, u, v, f32((X ** 2).sum(axis=1, dtype=f32).max())


def scan_cascade(metric, labels, k, m):
    """The scan route on lc.gauss(20000, 64, 64, 1) under `labels` -> (answers per query, worst pool fill per pass, queries
    the bound does not serve: their sample holds fewer than k capped rows).  The pool fill is what the int8 threshold lets
    through under the model's radii, as in largek_cases.cascade; asserts that the threshold hides no row within a radius."""
    X, Q, full, D, S, u, v, max_sumsq = _scan_inputs(metric)
    n, d = X.shape
    ranges = scan_ranges(n)
    smp = lc.sample_ids(n)
    answers, fills, unserved = [], [0] * len(ranges), 0
    for q in range(len(Q)):
        def through(j, lo, hi, radius, q=q):
            thr, marked = rc.range_thr(np.array([radius], dtype=f32), u[q:q + 1], v[q:q + 1], metric, d, max_sumsq)
            if marked[0]:
                raise _Unserved()
            t = S[lo:hi, q] <= thr[0]
            fills[j] = max(fills[j], int(t.sum()))
            return t
        try:
            ans, _, _ = passes_model(D[q], labels, k, m, ranges, sample=smp, through=through)
        except _Unserved:
            unserved += 1
            ans = capped_greedy(ordered_rows(D[q]), labels, k, m)   # (the exact route's answer)
        answers.append(ans)
    return answers, fills, unserved


class _Unserved(Exception):
    pass


# The scan cases of tests/test_knn_grouped.py that assert "all 64 on the route, none handed on, 3 passes": the ones the
# cascade above clears — no unserved query and at most half a pool at every pass (tests/test_grouped_model.py checks this
# table against the model, case by case).  Scattered labels: the sample's rows 0, 20, 40, ... carry 100 distinct labels
# only (20 i * 2654435761 mod 2000 is a multiple of 20), so at per_group 1 it holds exactly 100 capped rows — a radius at
# k = 100 that lets more than half a pool through — and never 256.
def scan_cases():
    return [(lab, k, m) for lab in sorted(LABELINGS) for k in SCAN_KS for m in SCAN_MS]


NOT_CLEARED = {
    "scattered": {(100, 1), (256, 1)},
    "clustered": set(),
}


def cleared(lab, k, m):
    return (k, m) not in NOT_CLEARED[lab]
