"""TEST INFRASTRUCTURE ONLY.  CPU model of the engine's GROUPED graph walk (ehx_graph_knn_grouped*, k_graphg.hip) in plain
Python: filtered_walk_model.filtered_search with "allowed" replaced by ELIGIBLE, a fact about the list R.  A row r is labelled
iff r < len(labels); an entry is eligible iff it is labelled and its label is GROUP_NONE or fewer than per_group labelled
entries of R with the same label lie in front of it.  TRIM, eligibility evaluated anew after every merge: behind the ef-th
eligible entry if there is one, then behind position cap.  The answer: the first k eligible entries, never the NaN seed."""
import bisect

import numpy as np

GROUP_NONE = 0xFFFFFFFF


def eligible_flags(R, labels, per_group):
    """[len(R)] bools: entry (seed, dist, id) of the sorted list R is eligible"""
    seen, out = {}, []
    for _, _, i in R:
        if i >= len(labels):
            out.append(False)
            continue
        g = int(labels[i])
        out.append(g == GROUP_NONE or seen.get(g, 0) < per_group)
        if g != GROUP_NONE:
            seen[g] = seen.get(g, 0) + 1
    return out


def grouped_search(level0, upper, entry_point, max_level, dist_row, labels, per_group, ef, cap, k):
    """filtered_search's arguments, labels [n_eff] u32 in place of the bitmap -> (ids u64, dists f32, {hit_cap})"""
    cur, curdist = int(entry_point), np.float32(dist_row[int(entry_point)])
    nan_seed = bool(curdist != curdist)
    if nan_seed:
        curdist = np.float32(np.inf)
    for level in range(int(max_level), 0, -1):
        changed = True
        while changed:
            changed, best, best_d = False, None, curdist
            for nb in upper.get((cur, level), ()):   # first strictly-smaller minimum in stored order (NaN: never smaller)
                d = np.float32(dist_row[int(nb)])
                if d < best_d:
                    best, best_d = int(nb), d
            if best is not None:
                cur, curdist, changed, nan_seed = best, best_d, True, False
    ef = max(int(ef), int(k))
    assert cap >= ef
    R = [(1 if nan_seed else 0, float(curdist), cur)]   # sorted as a tuple: the NaN seed above everything
    expanded, visited = set(), {cur}
    hit_cap = False
    while True:
        todo = [e for e in R if e[2] not in expanded]
        if not todo:
            break
        c = todo[0][2]
        expanded.add(c)
        row = level0[c]
        fresh = [int(nb) for nb in row[1:1 + int(row[0])] if int(nb) not in visited]
        visited.update(fresh)
        for i in fresh:
            d = np.float32(dist_row[i])
            if d == d:
                bisect.insort(R, (0, float(d), i))
        at = [j for j, e in enumerate(eligible_flags(R, labels, per_group)) if e]
        if len(at) >= ef:
            del R[at[ef - 1] + 1:]
        del R[cap:]
        hit_cap = hit_cap or len(R) == cap
    top = [e for e, ok in zip(R, eligible_flags(R, labels, per_group)) if ok and not e[0]][:k]
    return (np.array([e[2] for e in top], dtype=np.uint64), np.array([e[1] for e in top], dtype=np.float32),
            {"hit_cap": hit_cap})
