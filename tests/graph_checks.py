"""Structural invariants of an HNSW graph export — the same ones the oracle's import (orc_hnsw_import) enforces, stated
once in numpy so that any export can be checked: the oracle's own (Hnsw.export_graph()) and every graph the GPU built
(Space.graph_export()).

level0 [n, 1+2M] u32 rows (count, ids..., zero padding); levels [n] i32; upper {(node, level >= 1): ids}.
"""
import numpy as np


def check_graph(level0, levels, upper, entry_point, max_level, M):
    """Assert the invariants hnswlib's addPoint keeps, and return a small summary dict (rows, upper lists, levels)."""
    l0 = np.asarray(level0)
    lv = np.asarray(levels)
    n = lv.shape[0]
    M0 = 2 * M
    assert l0.shape == (n, 1 + M0), l0.shape
    assert n > 0
    assert (lv >= 0).all(), "negative level"
    assert int(max_level) == int(lv.max()), ("max_level is not the highest level", max_level, int(lv.max()))
    assert 0 <= int(entry_point) < n and int(lv[int(entry_point)]) == int(max_level), ("entry point", entry_point)
    # level 0: counts within 2M, ids < n, no self-link, no duplicate in a list, zero padding
    cnt = l0[:, 0].astype(np.int64)
    assert (cnt <= M0).all(), ("level-0 count above 2M at nodes", np.nonzero(cnt > M0)[0][:10])
    ids = l0[:, 1:].astype(np.int64)
    live = np.arange(M0)[None, :] < cnt[:, None]
    assert (ids[~live] == 0).all(), "level-0 padding is not zero"
    bad = np.nonzero((live & (ids >= n)).any(axis=1))[0]
    assert len(bad) == 0, ("level-0 id >= n at nodes", bad[:10])
    bad = np.nonzero((live & (ids == np.arange(n)[:, None])).any(axis=1))[0]
    assert len(bad) == 0, ("level-0 self-link at nodes", bad[:10])
    srt = np.sort(np.where(live, ids, -1 - np.arange(M0)[None, :]), axis=1)  # (padding: distinct negatives)
    bad = np.nonzero((srt[:, 1:] == srt[:, :-1]).any(axis=1))[0]
    assert len(bad) == 0, ("duplicate id in a level-0 list at nodes", bad[:10])
    # upper levels: exactly the lists (node, 1..levels[node]), at most M ids, neighbours that have the level
    want = {(int(i), l) for i in np.nonzero(lv > 0)[0] for l in range(1, int(lv[i]) + 1)}
    have = set(upper)
    assert have == want, ("upper lists missing", sorted(want - have)[:10], "or extra", sorted(have - want)[:10])
    n_upper_ids = 0
    for (node, level), lst in upper.items():
        a = np.asarray(lst, dtype=np.int64)
        n_upper_ids += a.size
        assert a.size <= M, ("upper list above M", node, level, a.size)
        assert ((a >= 0) & (a < n)).all(), ("upper id >= n", node, level)
        assert not (a == node).any(), ("upper self-link", node, level)
        assert len(np.unique(a)) == a.size, ("duplicate id in an upper list", node, level)
        assert (lv[a] >= level).all(), ("upper neighbour below the list's level", node, level)
    return {"rows": int(n), "upper_lists": len(upper), "upper_ids": int(n_upper_ids), "max_level": int(max_level),
            "mean_degree0": float(cnt.mean())}
