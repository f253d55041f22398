"""CPU tests of tests/version_oracle.py: the window of versions a search may answer for, the rejection of answers mixed
from two versions, and — with the oracle alone — the input conditions that keep test_rewrite_under_search.py from
passing on a wrong engine, for every case's generator."""
import numpy as np
import pytest

from oracle import pyoracle
import version_oracle as vo


def _small(metric="cos", T=5):
    cen = vo.centres(3, 4, 24)
    probe = cen if metric == "cos" else cen * np.float32(2.0)
    X0 = vo._synthetic(4000 + 200, 24) if metric == "cos" else vo._l2_base(4000 + 200, 24)
    queries = {"a": (vo.queries_near(probe, 3, 8), 10), "b": (vo.queries_near(probe, 2, 9), 70)}
    batches = vo.make_rewrite_batches(X0, cen, [10, 70], metric, T, 3, probe, vo._flat_top(vo.OM[metric]),
                                      far_norm=None if metric == "cos" else (1.7, 2.6))
    oracles, X = vo.flat_versions(X0, batches, queries, vo.OM[metric])
    return X0, batches, queries, oracles, X


@pytest.mark.parametrize("metric", ["cos", "l2"])
def test_versions_are_the_full_scan_of_each_state(metric):
    X0, batches, queries, oracles, X = _small(metric)
    Y = X0.copy()
    for v in range(len(batches) + 1):
        if v:
            ids, rows = batches[v - 1]
            for i, row in zip(ids, rows):       # call order: the last write of a key wins
                Y[i] = row
        for t, (Q, k) in queries.items():
            oids, odist, ocnt = pyoracle.exhaustive(Y, Q, k, vo.OM[metric])
            ids_v, dist_v, cnt_v = oracles[t].answer(v)
            np.testing.assert_array_equal(ids_v, oids)
            assert dist_v.tobytes() == odist.tobytes() and np.array_equal(cnt_v, ocnt)
    assert X.tobytes() == Y.tobytes()


def test_the_window_at_both_edges():
    _, batches, _, oracles, _ = _small()
    o, T = oracles["a"], len(batches)
    assert T == 5
    for v in range(T + 1):
        assert o.assert_is_some_version(*o.answer(v), v, v) == v            # v = a
    assert o.assert_is_some_version(*o.answer(3), 1, 2) == 3                # v = b + 1: committed, the counter not moved yet
    with pytest.raises(AssertionError, match="no version"):
        o.assert_is_some_version(*o.answer(4), 1, 2)                        # v = b + 2
    with pytest.raises(AssertionError, match="no version"):
        o.assert_is_some_version(*o.answer(1), 2, 4)                        # v = a - 1: stale
    assert list(o.window(4, 5)) == [4, 5] and list(o.window(5, 5)) == [5]   # b + 1 > T
    assert o.assert_is_some_version(*o.answer(T), T, T) == T
    with pytest.raises(AssertionError, match="bad window"):
        o.assert_is_some_version(*o.answer(T), T, T + 1)
    with pytest.raises(AssertionError, match="closest is version 1"):       # the report names the version a stale answer is
        o.assert_is_some_version(*o.answer(1), 3, 4)


def test_mixed_answers_are_rejected():
    _, batches, _, oracles, _ = _small()
    for t in ("a", "b"):
        o = oracles[t]
        assert o.min_id_difference() >= 2
        i2, d2, c2 = o.answer(2)
        i3, d3, c3 = o.answer(3)
        nq, k = i2.shape
        ids, dist = i2.copy(), d2.copy()        # half the queries from version 2, half from version 3
        ids[nq // 2:], dist[nq // 2:] = i3[nq // 2:], d3[nq // 2:]
        with pytest.raises(AssertionError, match="no version"):
            o.assert_is_some_version(ids, dist, c2, 0, 5)
        ids, dist = i2.copy(), d2.copy()        # a top-k spliced from two versions (page 2 of another state)
        ids[:, k // 2:], dist[:, k // 2:] = i3[:, k // 2:], d3[:, k // 2:]
        with pytest.raises(AssertionError, match="no version"):
            o.assert_is_some_version(ids, dist, c2, 0, 5)
        ids = i2.copy()                         # one id, one distance bit, one count
        ids[0, 3] = ids[0, 4]
        with pytest.raises(AssertionError):
            o.assert_is_some_version(ids, d2, c2, 2, 2)
        dist = d2.copy()
        dist[1, 2] = np.nextafter(dist[1, 2], np.float32(np.inf))
        with pytest.raises(AssertionError):
            o.assert_is_some_version(i2, dist, c2, 2, 2)
        cnt = c2.copy()
        cnt[0] -= 1
        with pytest.raises(AssertionError):
            o.assert_is_some_version(i2, d2, cnt, 2, 2)


def test_tile_is_the_kernels_tile():
    """version_oracle.TILE is the row count of the int8 / fp16 scan tiles (ehx_kernels.h: kTileRows16, which flat_pass8 and
    make_scan8 use)"""
    import os
    import re
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "embeddinghub_amd", "csrc",
                          "ehx_kernels.h")).read()
    assert int(re.search(r"constexpr uint32_t kTileRows16 = (\d+);", h).group(1)) == vo.TILE


def _tiles(ids, G):
    ids = np.asarray(ids)
    return (ids // G) // vo.TILE, (ids // G) % vo.TILE


@pytest.mark.parametrize("name", sorted(vo.CASE_INPUTS))
def test_case_inputs_change_every_answer_in_every_batch(name):
    """with the oracle alone: any two versions differ in >= 2 ids for every query; every rewriting batch evicts >= 2 rows of
    every query's top-k and lands >= 2 rewritten far rows inside it; the rewritten ids are scattered as the tiles need"""
    ci = vo.CASE_INPUTS[name]()
    oracles, X, h = ci.versions()
    T = len(ci.batches)
    for t, o in oracles.items():
        assert o.T == T and o.min_id_difference() >= 2, (t, o.min_id_difference())
    n = ci.n
    for j, (ids, rows) in enumerate(ci.batches, start=1):
        written = set(int(i) for i in ids)
        if j in ci.appends:
            assert sorted(written) == list(range(n, n + len(ids))), "an append batch holds fresh keys only"
            n += len(ids)
        else:
            assert max(written) < n, "a rewriting batch holds known keys only"
            assert len(written) == len(ids) - 2, "two keys are written twice"
            assert list(ids) != sorted(ids), "ids are listed out of order"
            for t, o in oracles.items():
                before, after = o.answer(j - 1)[0], o.answer(j)[0]
                for q in range(before.shape[0]):
                    out = [i for i in before[q] if int(i) in written and i not in after[q]]
                    came = [i for i in after[q] if int(i) in written and i not in before[q]]
                    assert len(out) >= 2 and len(came) >= 2, (j, t, q, len(out), len(came))
            if not ci.graph:
                assert set(i % ci.G for i in written) == set(range(ci.G)), "every shard takes rows of every batch"
                tile, pos = _tiles(sorted(written), ci.G)
                per_tile = np.bincount(tile)
                assert (per_tile >= 3).any(), "several in one tile"
                if len(per_tile) >= 64:
                    assert (per_tile == 1).any(), "one in others"
                else:   # r_f16flt, r_f32, r_paged, r_one, r_shards: fewer tiles than a batch has rows — no tile gets just one;
                    # what holds there: the tiles are hit unevenly, the fullest at least twice as often as the emptiest
                    assert per_tile.max() >= 2 * max(1, per_tile.min()), "tiles hit unevenly"
                assert (pos == 0).any() and (pos == vo.TILE - 1).any(), "the first and the last row of a tile"
                assert tile.max() == (ci.n // ci.G) // vo.TILE and (ci.n // ci.G) % vo.TILE, "the tile that straddles the count"
    assert n == len(X)
    if ci.graph:
        assert len(ci.appends) >= 2 and len(h) == ci.total
        # the entry point is among the keys of every update batch made while it was the entry point: replay and look
        g = pyoracle.Hnsw(ci.d, vo.OM[ci.metric], ci.total)
        g.add_rows(np.ascontiguousarray(ci.held(ci.X0)))
        for j, (ids, rows) in enumerate(ci.batches, start=1):
            if j not in ci.appends:
                assert int(g.enterpoint) in set(int(i) for i in ids), "batch %d does not update the entry point" % j
            for i, row in zip(ids, ci.held(rows)):
                g.add(row, int(i))
    if ci.round16:
        assert any((vo.f16(rows) != rows).any() for _, rows in ci.batches), "rounding must change the rows"
