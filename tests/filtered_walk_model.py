"""TEST INFRASTRUCTURE ONLY.  CPU model of the engine's graph walk under a row bitmap (ehx_graph_knn_masked*,
embeddinghub_amd/csrc/k_graphm.hip), in plain Python, for small cases — in the style of oracle/wide_walk_model.py.

Parity unpinned against the reference: the reference has no filtered search, and the oracle restates hnswlib 0.5.x, which
has none either.  This model states the ONE deviation the filtered walk makes from the strict walk (k_graph.hip, the
oracle's searchBaseLayerST in one-list form) and nothing else, so that the kernel can be checked bit for bit against
something that is not itself.  The deviation is the rule hnswlib >= 0.7 applies to a filter (isIdAllowed), plus one bound
a GPU needs:

  * upper levels: the greedy descent, unchanged; the filter is ignored above level 0; a NaN distance counts as +Inf;
  * level 0: ONE list R of (distance, id) entries sorted by (distance, id), each expanded or not; whether an entry is
    allowed is a fact about its id.  R starts as the descent's end node, allowed or not (with the NaN-seed key, above
    +Inf, if the strict walk would seed so).  A step takes the closest unexpanded entry of R — entries that are not allowed
    included: they are walked through and never returned — marks it expanded, takes its level-0 neighbours in stored
    order that were not visited (fresh; marks them visited; n_dist += len(fresh), n_hops0 += 1), drops the fresh rows
    whose distance is NaN, and R <- sort(R u fresh).  TRIM: if R holds at least ef allowed entries everything behind the
    ef-th allowed one is deleted; then everything behind position cap.  The walk ends when R has no unexpanded entry;
  * the answer: the first k allowed entries of R (the NaN seed is never returned); there may be fewer than k.

ef = max(space ef, k) as in searchKnn; cap = walk_cap(ef) in the engine.  With every row allowed and cap >= ef the trim
is "R <- the ef smallest": the strict walk.  With cap = infinity and distinct distances the answer is hnswlib's filtered
searchBaseLayerST (tests/test_filtered_walk_model.py holds both arguments as tests).

(The list is kept sorted by insertion and the trim counts from the back: the same list as sorting and counting from the
front at every step, in a fraction of the time.)
"""
import bisect
import math

import numpy as np

WALK_LIST_FACTOR = 12     # EHX_WALK_LIST_FACTOR
WALK_LIST_MAX = 4096      # EHX_WALK_LIST_MAX


def walk_cap(ef):
    """length of the engine's walk list: max(ef, min(WALK_LIST_FACTOR ef, WALK_LIST_MAX))"""
    return max(int(ef), min(WALK_LIST_FACTOR * int(ef), WALK_LIST_MAX))


def allowed_rows(allow, n_bits, n_rows):
    """the engine's definition of an allowed row as a bool array [n_rows]: r < n_bits, r < n_rows, bit r of the mask set.
    allow: bool array (entry r) or packed uint32 words (bit r & 31 of word r >> 5)"""
    a = np.asarray(allow)
    if a.dtype != np.bool_:
        a = np.unpackbits(np.ascontiguousarray(a, dtype="<u4").view(np.uint8), bitorder="little").astype(bool)
    out = np.zeros(n_rows, dtype=bool)
    m = min(int(n_bits), n_rows, a.shape[0])
    out[:m] = a[:m]
    return out


def filtered_search(level0, upper, entry_point, max_level, dist_row, allowed, ef, cap, k):
    """level0: [n, 1 + 2M] u32 rows (count, ids...) as Hnsw.export_graph() returns them; upper: {(node, level): ids};
    dist_row[i]: the oracle's canonical distance of the query to row i (float32); allowed: bool [n]; cap: an int or
    math.inf.  -> (ids u64, dists f32, counters) with counters n_dist, n_hops0, n_hops_up, hit_cap (R held cap entries
    behind some step's trim) and max_len (the longest R behind a trim)."""
    n_dist = n_hops0 = n_hops_up = 0
    cur = int(entry_point)
    curdist = np.float32(dist_row[cur])
    n_dist += 1
    nan_seed = bool(curdist != curdist)
    if nan_seed:
        curdist = np.float32(np.inf)
    for level in range(int(max_level), 0, -1):
        changed = True
        while changed:
            changed = False
            lst = upper.get((cur, level), ())
            n_hops_up += 1
            n_dist += len(lst)
            best, best_d = None, curdist
            for nb in lst:                       # first strictly-smaller minimum in stored order (NaN: never smaller)
                d = np.float32(dist_row[int(nb)])
                if d < best_d:
                    best, best_d = int(nb), d
            if best is not None:
                cur, curdist, changed, nan_seed = best, best_d, True, False
    ef = max(int(ef), int(k))
    assert cap >= ef

    def entry(d, i, seed=False):
        # sorted as a tuple: (NaN seed above everything, distance, id); ids are distinct, the flag is never compared
        return (1 if seed else 0, float(d), int(i), bool(allowed[i]))

    R = [entry(curdist, cur, nan_seed)]
    n_allowed = 1 if allowed[cur] else 0         # allowed entries of R
    expanded = set()
    visited = {cur}
    first = 0                                    # every entry of R before this index is expanded
    hit_cap, max_len = False, 1
    while True:
        while first < len(R) and R[first][2] in expanded:
            first += 1
        if first == len(R):
            break
        c = R[first][2]
        expanded.add(c)
        n_hops0 += 1
        row = level0[c]
        fresh = []
        for nb in row[1:1 + int(row[0])]:
            nb = int(nb)
            if nb not in visited:
                visited.add(nb)
                fresh.append(nb)
        n_dist += len(fresh)
        for i in fresh:
            d = np.float32(dist_row[i])
            if d != d:
                continue
            e = entry(d, i)
            at = bisect.bisect_left(R, e)
            R.insert(at, e)
            n_allowed += 1 if e[3] else 0
            first = min(first, at)
        # trim: behind the ef-th allowed entry, then behind cap
        if n_allowed >= ef:
            while n_allowed > ef or not R[-1][3]:
                n_allowed -= 1 if R.pop()[3] else 0
        while len(R) > cap:
            n_allowed -= 1 if R.pop()[3] else 0
        max_len = max(max_len, len(R))
        hit_cap = hit_cap or len(R) == cap
    top = [e for e in R if e[3] and not e[0]][:k]
    ids = np.array([e[2] for e in top], dtype=np.uint64)
    dists = np.array([e[1] for e in top], dtype=np.float32)
    return ids, dists, {"n_dist": n_dist, "n_hops0": n_hops0, "n_hops_up": n_hops_up, "hit_cap": hit_cap,
                        "max_len": max_len}
