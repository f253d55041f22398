"""Helper of the tests of the grouped kNN under row bitmaps (no test here): the contract of ehx_knn_grouped_masked — FILTER
FIRST, THEN CAP — as the oracle's full ordered list with the rows that are not allowed dropped and tests/grouped_model.py's
plain-Python greedy over what is left; the bitmaps of the scan cases; and the scan route's cascade (sample of the allowed
rows by rank, the unfiltered passes, the bitmap in the scan's flush) on top of grouped_model.passes_model."""
import functools

import numpy as np

import grouped_model as gm
import largek_cases as lc
import range_cases as rc

f32 = np.float32
SAMPLE = lc.SAMPLE       # kLargeKSample
SCAN_KS = (10, 100, 256)
SCAN_MS = (1, 4)
SCAN_DENSITIES = (0.5, 0.1)
N_SCAN_MASKS = 4


# ---- the contract ----

def allowed_rows(allow, n_eff):
    """bool [n_eff]: the rows of the prefix a bitmap (bool, any length) allows"""
    a = np.zeros(n_eff, dtype=bool)
    m = min(n_eff, len(allow))
    a[:m] = np.asarray(allow, dtype=bool)[:m]
    return a


def expected(full, labels, allows, mask_of, k, m, n_eff=None):
    """-> [(ids, distances)] per query from grouped_model.oracle_all's lists: the rows that query's bitmap does not allow
    (and the rows at or above n_eff = min(rows, labels, bits)) dropped from the oracle's order, the greedy over the rest."""
    oids, odist, ocnt = full
    labels = np.asarray(labels)
    allows = np.atleast_2d(np.asarray(allows, dtype=bool))
    if n_eff is None:
        n_eff = min(oids.shape[1], len(labels), allows.shape[1])
    ok = [allowed_rows(a, n_eff) for a in allows]
    out = []
    for i in range(len(ocnt)):
        c = int(ocnt[i])
        ids = oids[i, :c].astype(np.int64)
        a = ok[0 if mask_of is None else int(mask_of[i])]
        pos = np.nonzero((ids < n_eff) & a[np.minimum(ids, n_eff - 1)])[0] if n_eff else np.zeros(0, dtype=np.int64)
        by_pos = labels[np.minimum(ids, len(labels) - 1)] if len(labels) else ids
        got = gm.capped_greedy([int(p) for p in pos], by_pos, k, m)   # positions in the oracle's list
        out.append((oids[i, got].astype(np.uint64), odist[i, got].astype(f32)))
    return out


# ---- the scan cases: lc.gauss(20000, 64, 64, 1) under four random bitmaps of one density, query q under bitmap q % 4 ----

@functools.lru_cache(maxsize=None)
def scan_bitmaps(density, n=20000):
    rng = np.random.default_rng(7)
    a = np.stack([rng.random(n) < density for _ in range(N_SCAN_MASKS)])
    a.setflags(write=False)
    return a


def scan_mask_of(nq=64):
    return (np.arange(nq) % N_SCAN_MASKS).astype(np.uint32)


def sample_of(allow):
    """grouped_range_seed_kernel over the mask's list: every stride-th allowed id by rank, stride = ceil(allowed / kLargeKSample)"""
    ids = np.nonzero(allow)[0]
    if len(ids) == 0:
        return ids
    return ids[::-(-len(ids) // SAMPLE)]


def scan_cascade(metric, labels, allows, mask_of, k, m):
    """The scan route on lc.gauss(20000, 64, 64, 1) -> (answers per query, worst pool fill per pass, unserved queries).  The
    rows a query's bitmap does not allow get a NaN distance (the model never makes a NaN row a neighbour); the sample is the
    bitmap's, the passes are the unfiltered search's, and only ALLOWED rows under the int8 threshold take a pool slot."""
    X, Q, full, D, S, u, v, max_sumsq = gm._scan_inputs(metric)
    n, d = X.shape
    ranges = gm.scan_ranges(n)
    answers, fills, unserved = [], [0] * len(ranges), 0
    for q in range(len(Q)):
        a = allowed_rows(allows[int(mask_of[q])], n)
        dist = np.where(a, D[q], f32(np.nan)).astype(f32)

        def through(j, lo, hi, radius, q=q, a=a):
            thr, marked = rc.range_thr(np.array([radius], dtype=f32), u[q:q + 1], v[q:q + 1], metric, d, max_sumsq)
            if marked[0]:
                raise gm._Unserved()
            t = (S[lo:hi, q] <= thr[0]) & a[lo:hi]
            fills[j] = max(fills[j], int(t.sum()))
            return t
        try:
            ans, _, _ = gm.passes_model(dist, labels, k, m, ranges, sample=sample_of(a), through=through)
        except gm._Unserved:
            unserved += 1
            ans = gm.capped_greedy(gm.ordered_rows(dist), labels, k, m)   # (the list route's answer)
        answers.append(ans)
    return answers, fills, unserved


def scan_cases():
    return [(density, lab, k, m) for density in SCAN_DENSITIES for lab in sorted(gm.LABELINGS) for k in SCAN_KS for m in SCAN_MS]


# The scan cases tests/test_knn_grouped_masked.py asserts "all 64 on the scan route, none handed on, 3 passes" for: the ones
# the cascade above clears — no unserved query and at most half a pool at every pass (tests/test_grouped_masked_model.py
# checks this table against the model, case by case, for every metric).  None is left out: a bitmap's sample is strided by
# RANK, so its rows do not share the residues of 20 that starve the unfiltered sample of labels (grouped_model.NOT_CLEARED).
NOT_CLEARED = set()


def cleared(density, lab, k, m):
    return (density, lab, k, m) not in NOT_CLEARED
