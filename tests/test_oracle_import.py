"""CPU tests of the oracle's graph import (orc_hnsw_import / pyoracle.Hnsw.import_graph): a graph exported from one
oracle and imported into a fresh one is the same index — the same export, and searchKnn returns the same ids, distance
bytes, counts and work counters — for graphs of the sequential build and of the bulk-build model (rounds whose rows do
not see each other: the shape of a GPU-built graph).  Every structural violation the import rejects has a case built by
corrupting a valid export, and the shared checker (tests/graph_checks.py) agrees with the import on each of them."""
import numpy as np
import pytest

from graph_checks import check_graph
from oracle import pyoracle

METRICS = [pyoracle.METRIC_L2, pyoracle.METRIC_IP, pyoracle.METRIC_COSINE]


def _round_trip(h, X, Q, om, M, efs, k):
    l0, lv, upper = h.export_graph()
    check_graph(l0, lv, upper, h.enterpoint, h.maxlevel, M)
    g = pyoracle.Hnsw(X.shape[1], om, 16, M=M)      # (smaller capacity than n: the import grows it)
    g.import_graph(X, l0, lv, upper, h.enterpoint, h.maxlevel, threads=4)
    assert len(g) == len(h) and (g.enterpoint, g.maxlevel) == (h.enterpoint, h.maxlevel)
    gl0, glv, gupper = g.export_graph()
    np.testing.assert_array_equal(gl0, l0)
    np.testing.assert_array_equal(glv, lv)
    assert sorted(gupper) == sorted(upper)
    for key in upper:
        np.testing.assert_array_equal(gupper[key], upper[key])
    assert g.export_vectors().tobytes() == h.export_vectors().tobytes()
    for ef in efs:
        h.set_ef(ef)
        g.set_ef(ef)
        a = h.search_batch(Q, k, threads=4)
        b = g.search_batch(Q, k, threads=4)
        np.testing.assert_array_equal(b[2], a[2])
        np.testing.assert_array_equal(b[0], a[0])
        assert b[1].tobytes() == a[1].tobytes()
        assert b[4] == a[4], (ef, a[4], b[4])
    # single-query search and the label lookup (an existing label re-added = updatePoint, not a new element)
    for i in range(3):
        assert np.array_equal(g.search(Q[i], k)[0], h.search(Q[i], k)[0])
    return g


@pytest.mark.parametrize("om", METRICS)
@pytest.mark.parametrize("M,n,d", [(8, 1200, 24), (16, 2000, 32), (32, 1500, 20)])
def test_round_trip_of_the_sequential_build(om, M, n, d):
    rng = np.random.default_rng(M * 10 + om)
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((24, d)).astype(np.float32)
    h = pyoracle.Hnsw(d, om, n, M=M)
    h.add_rows(X)
    g = _round_trip(h, X, Q, om, M, efs=(10, 50, 300), k=10)
    _round_trip(h, X, Q, om, M, efs=(10,), k=64)      # k > ef: searchKnn keeps max(ef, k)
    # the imported index is a live one: an update of an existing label and a fresh label behave as in the original
    v = rng.standard_normal(d).astype(np.float32)
    for idx in (h, g):
        idx.resize(n + 1)
        idx.add(v, 5)
        idx.add(-v, n)
    l0a, lva, upa = h.export_graph()
    l0b, lvb, upb = g.export_graph()
    np.testing.assert_array_equal(l0b, l0a)
    np.testing.assert_array_equal(lvb, lva)
    assert {key: val.tolist() for key, val in upa.items()} == {key: val.tolist() for key, val in upb.items()}


@pytest.mark.parametrize("om", METRICS)
def test_round_trip_of_the_bulk_build_model(om):
    n, d = 6000, 32
    rng = np.random.default_rng(40 + om)
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((32, d)).astype(np.float32)
    h = pyoracle.Hnsw(d, om, n)
    h.add_rows_rounds(X, div=16, cap=256, threads=4)
    _round_trip(h, X, Q, om, 16, efs=(10, 50, 300), k=10)


def test_empty_and_single_row_graphs():
    g = pyoracle.Hnsw(4, pyoracle.METRIC_L2, 8)
    g.import_graph(np.zeros((0, 4), np.float32), np.zeros((0, 33), np.uint32), np.zeros(0, np.int32), {}, 0, -1)
    assert len(g) == 0
    X = np.ones((1, 4), np.float32)
    h = pyoracle.Hnsw(4, pyoracle.METRIC_L2, 8)
    h.add_rows(X)
    l0, lv, upper = h.export_graph()
    g.import_graph(X, l0, lv, upper, h.enterpoint, h.maxlevel)
    assert g.search(X[0], 3)[0].tolist() == [0]
    with pytest.raises(RuntimeError, match="not empty"):
        g.import_graph(X, l0, lv, upper, h.enterpoint, h.maxlevel)


@pytest.fixture(scope="module")
def valid():
    n, d, M = 800, 16, 8
    X = np.random.default_rng(3).standard_normal((n, d)).astype(np.float32)
    h = pyoracle.Hnsw(d, pyoracle.METRIC_L2, n, M=M)
    h.add_rows(X)
    l0, lv, upper = h.export_graph()
    assert h.maxlevel >= 2
    return X, l0, lv, upper, h.enterpoint, h.maxlevel, M


def _node_at(lv, level, but=()):
    return int([i for i in np.nonzero(lv >= level)[0] if i not in but][0])


def _full_upper(upper, lv, level, M):
    """an upper list at `level` that has room for one more id, and its node"""
    for (node, l), ids in sorted(upper.items()):
        if l == level and len(ids) < M:
            return node
    raise AssertionError("no upper list with room")


def _corrupt(case, X, l0, lv, upper, ep, ml, M):
    l0, lv = l0.copy(), lv.copy()
    upper = {key: val.copy() for key, val in upper.items()}
    n = l0.shape[0]
    if case == "id_ge_n":
        l0[7, 1] = n
    elif case == "self_link":
        l0[7, 1] = 7
    elif case == "duplicate":
        l0[7, 2] = l0[7, 1]
    elif case == "count_above_2M":
        l0[7, 0] = 2 * M + 1          # (the row holds 2M ids: the count is checked before any id is read)
    elif case == "count_above_M_upper":
        node = _node_at(lv, 1)
        others = [int(i) for i in np.nonzero(lv >= 1)[0] if i != node and int(i) not in upper[(node, 1)]]
        upper[(node, 1)] = np.concatenate([upper[(node, 1)], others])[:M + 1].astype(np.uint32)
        assert len(upper[(node, 1)]) == M + 1
    elif case == "upper_duplicate":
        node = _node_at(lv, 1)
        upper[(node, 1)] = np.concatenate([upper[(node, 1)], upper[(node, 1)][:1]]).astype(np.uint32)
    elif case == "upper_list_missing":
        node = _node_at(lv, 1)
        del upper[(node, int(lv[node]))]
    elif case == "upper_list_above_level":
        node = int(np.nonzero(lv == 0)[0][0])
        upper[(node, 1)] = np.zeros(0, np.uint32)
    elif case == "neighbour_below_level":
        node = _full_upper(upper, lv, 1, M)
        low = int([i for i in np.nonzero(lv == 0)[0] if i != node][0])
        upper[(node, 1)] = np.concatenate([upper[(node, 1)], [low]]).astype(np.uint32)
    elif case == "max_level_wrong":
        ml = ml + 1
    elif case == "entry_point_level":
        ep = int(np.nonzero(lv < ml)[0][0])
    elif case == "entry_point_ge_n":
        ep = n
    else:
        raise AssertionError(case)
    return X, l0, lv, upper, ep, ml


REJECTIONS = [("id_ge_n", ">= n"), ("self_link", "self-link"), ("duplicate", "twice in one list"),
              ("count_above_2M", "list of 17 > 16"), ("count_above_M_upper", "list of 9 > 8"),
              ("upper_duplicate", "twice in one list"), ("upper_list_missing", "upper list missing"),
              ("upper_list_above_level", "level the node does not have"),
              ("neighbour_below_level", "of level 0 linked"), ("max_level_wrong", "not the highest level"),
              ("entry_point_level", "not max_level"), ("entry_point_ge_n", "entry point")]


@pytest.mark.parametrize("case,msg", REJECTIONS)
def test_import_rejects_a_corrupted_export(valid, case, msg):
    X, l0, lv, upper, ep, ml, M = valid
    check_graph(l0, lv, upper, ep, ml, M)                 # the export itself is valid ...
    args = _corrupt(case, X, l0, lv, upper, ep, ml, M)
    g = pyoracle.Hnsw(X.shape[1], pyoracle.METRIC_L2, 16, M=M)
    with pytest.raises(RuntimeError, match=msg):
        g.import_graph(*args)
    assert len(g) == 0                                    # ... nothing of the bad graph was kept
    with pytest.raises(AssertionError):                   # and the shared checker refuses it too
        check_graph(*args[1:], M)
    g.import_graph(X, l0, lv, upper, ep, ml)              # the same index still takes the valid graph
    assert len(g) == X.shape[0]


def test_import_rejects_wrong_shapes(valid):
    X, l0, lv, upper, ep, ml, M = valid
    g = pyoracle.Hnsw(X.shape[1], pyoracle.METRIC_L2, 16, M=M + 1)
    with pytest.raises(ValueError):
        g.import_graph(X, l0, lv, upper, ep, ml)
