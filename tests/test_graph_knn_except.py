"""The graph walk under per-query exclusion lists (ehx_graph_knn_except*, k_graphx.hip) on the GPU, compared for equality of
ids, distance bytes and counts: with tests/filtered_walk_model.py, with the bitmap walk, with the oracle's exhaustive list."""
import ctypes as C

import numpy as np
import pytest

from filtered_walk_model import filtered_search, walk_cap
from oracle import pyoracle

pytestmark = pytest.mark.gpu
ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402
from embeddinghub_amd.space import marshal_mask_table  # noqa: E402

METRICS = {"l2": (ehx.METRIC_L2SQ, pyoracle.METRIC_L2), "ip": (ehx.METRIC_IP, pyoracle.METRIC_IP),
           "cosine": (ehx.METRIC_COSINE, pyoracle.METRIC_COSINE)}
NO_ID = np.uint64(2**64 - 1)
_small = {}


def _same(a, b):
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[0], b[0])
    assert np.ascontiguousarray(a[1]).tobytes() == np.ascontiguousarray(b[1]).tobytes()


def _hook(s):
    out = (C.c_uint64 * 4)()
    fn = C.CDLL(_lib.LIB_PATH).ehx_test_graph_masked_counters
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    assert fn(s._h, out) == 0
    return np.array([int(v) for v in out], dtype=np.int64)   # walked, exact, calls, walked queries at cap


@pytest.fixture(scope="module", autouse=True)
def _drop_spaces():
    yield
    for v in _small.values():
        v[0].drop()
    _small.clear()


def _oracle_case(metric):
    """an oracle graph imported into a graph space, the oracle's distances, the four kinds of list (query i: kind i % 4)"""
    if metric not in _small:
        em, om = METRICS[metric]
        n, d, nq = 1200, 24, 14
        rng = np.random.default_rng(n + d)
        X = rng.standard_normal((n, d)).astype(np.float32)
        h = pyoracle.Hnsw(d, om, n, M=16)
        h.add_rows(X)
        s = ehx.Space.unique("gx", d, metric=em, mode=ehx.MODE_GRAPH, M=16, initial_capacity=n, build_batch=0xFFFFFFFF)
        s.set_batch(["k%d" % i for i in range(n)], X)
        l0, lv, upper = h.export_graph()
        s.graph_import(l0, lv, upper, h.enterpoint, h.maxlevel)
        Q = rng.standard_normal((nq, d)).astype(np.float32)
        order, dist, _ = pyoracle.exhaustive(X, Q, n, om)
        D = np.empty((nq, n), dtype=np.float32)
        np.put_along_axis(D, order.astype(np.int64), dist, axis=1)
        lists = [[np.zeros(0, dtype=np.uint64), order[i, :1], order[i, :300],
                  rng.integers(0, 2 * n, 4096).astype(np.uint64)][i % 4] for i in range(nq)]
        _small[metric] = (s, (l0, upper, int(h.enterpoint), int(h.maxlevel)), Q, D, lists)
    return _small[metric]


@pytest.mark.parametrize("ef", [10, 64])
@pytest.mark.parametrize("metric", list(METRICS))
def test_walk_is_the_models_walk_under_the_complement_of_each_list(metric, ef):
    s, graph, Q, D, lists = _oracle_case(metric)
    n, k = D.shape[1], 10
    s.set_ef(ef)
    before = _hook(s)
    ids, dist, cnt = s.graph_knn_except(Q, k, lists, route=ehx.WALK_GRAPH)
    hit_cap = 0
    for i, lst in enumerate(lists):
        allowed = np.ones(n, dtype=bool)
        allowed[lst[lst < n].astype(np.int64)] = False
        m_ids, m_dist, c = filtered_search(*graph, D[i], allowed, ef, walk_cap(ef), k)
        hit_cap += int(c["hit_cap"])
        assert cnt[i] == len(m_ids), (i, cnt[i], len(m_ids))
        np.testing.assert_array_equal(ids[i, :cnt[i]], m_ids, err_msg="query %d" % i)
        assert dist[i, :cnt[i]].tobytes() == m_dist.tobytes(), i
        assert (ids[i, cnt[i]:] == NO_ID).all() and np.isposinf(dist[i, cnt[i]:]).all(), i
    assert (_hook(s) - before).tolist() == [len(lists), 0, 1, hit_cap]
    if ef == 10:    # the 300 nearest rows exceed cap - ef: the walk went through excluded nodes to its cap
        assert hit_cap >= 1


@pytest.mark.parametrize("dtype", [ehx.DTYPE_F32, ehx.DTYPE_F16])
def test_one_launch_of_mixed_list_lengths_is_the_bitmap_walk(dtype):
    torch = pytest.importorskip("torch")
    n, d, nq, k = 5000, 67, 64, 10
    rng = np.random.default_rng(67)
    s = ehx.Space.unique("gx-built", d, metric=ehx.METRIC_L2SQ, mode=ehx.MODE_GRAPH, M=16, initial_capacity=n, dtype=dtype)
    s.set_batch(["k%d" % i for i in range(n)], rng.standard_normal((n, d)).astype(np.float32))
    s.set_ef(40)
    entry = int(s.graph_export()[3])
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    lens = [(0, 1, 63, 64, 65, 255, 4095, 4096)[i % 8] for i in range(nq)]
    head = np.array([0, n - 1, entry], dtype=np.uint64)
    perms = [rng.permutation(n).astype(np.uint64) for _ in lens]
    lists = [np.concatenate([head, p[~np.isin(p, head)]])[:m] for p, m in zip(perms, lens)]
    tab = np.ones((nq, n), dtype=bool)
    for i, lst in enumerate(lists):
        tab[i, lst.astype(np.int64)] = False
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    outs = lambda: (torch.zeros((nq, k), dtype=torch.int64, device="cuda"),  # noqa: E731
                    torch.zeros((nq, k), dtype=torch.float32, device="cuda"), torch.zeros(nq, dtype=torch.int32, device="cuda"))
    host = lambda o: (o[0].cpu().numpy().view(np.uint64), o[1].cpu().numpy(), o[2].cpu().numpy().view(np.uint32))  # noqa: E731
    want = outs()
    s.graph_knn_masked_multi_device(dev(Q), k, dev(marshal_mask_table(tab)[0].view(np.int32)), nq, n,
                                    dev(np.arange(nq, dtype=np.int32)), *want, route=ehx.WALK_GRAPH)
    # every list shuffled, every id twice (where two copies fit the limit): the same lists
    for these in (lists, [rng.permutation(np.concatenate([lst, lst]) if len(lst) <= 2048 else lst) for lst in lists]):
        off = np.concatenate([[0], np.cumsum([len(lst) for lst in these])]).astype(np.int64)
        got = outs()
        s.graph_knn_except_device(dev(Q), k, dev(np.concatenate(these).view(np.int64)), dev(off), *got, route=ehx.WALK_GRAPH)
        torch.cuda.synchronize()
        _same(host(got), host(want))
    s.drop()


def test_routes_and_forms():
    torch = pytest.importorskip("torch")
    n, d, nq, k = 600, 24, 6, 10
    rng = np.random.default_rng(600)
    X = rng.standard_normal((n, d)).astype(np.float32)
    s = ehx.Space.unique("gx-routes", d, metric=ehx.METRIC_L2SQ, mode=ehx.MODE_GRAPH, M=16, initial_capacity=n)
    s.set_batch(["k%d" % i for i in range(n)], X)
    s.set_ef(32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    # 551 of 600 rows listed: 12 * 49 < 600, EHX_WALK_AUTO answers exactly; 550: walked; 595: five rows are left
    lists = [rng.permutation(n)[:m].astype(np.uint64) for m in (551, 550, 595, 0, 551, 40)]
    order, dist, _ = pyoracle.exhaustive(X, Q, n, pyoracle.METRIC_L2)
    exact_rows = [0, 2, 4]
    before = _hook(s)
    auto = s.graph_knn_except(Q, k, lists)
    assert (_hook(s) - before)[:3].tolist() == [3, 3, 1]
    _same(tuple(a[[1, 3, 5]] for a in auto), tuple(a[[1, 3, 5]] for a in s.graph_knn_except(Q, k, lists, route=ehx.WALK_GRAPH)))
    everywhere = s.graph_knn_except(Q, k, lists, route=ehx.WALK_EXACT)
    for i in range(nq):
        keep = ~np.isin(order[i], lists[i])
        w_ids, w_dist = order[i][keep][:k], dist[i][keep][:k]
        for got in ([everywhere, auto] if i in exact_rows else [everywhere]):
            assert got[2][i] == len(w_ids) == (5 if i == 2 else k)
            np.testing.assert_array_equal(got[0][i, :len(w_ids)], w_ids)
            assert got[1][i, :len(w_ids)].tobytes() == w_dist.tobytes()
    # the forms: stored keys (one of them unknown: it excludes nothing) and device tensors
    _same(s.graph_knn_except_keys(Q, k, [["k%d" % r for r in lst] + ["nobody"] for lst in lists]), auto)
    off = np.concatenate([[0], np.cumsum([len(lst) for lst in lists])]).astype(np.int64)
    d_ids = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    d_dist, d_cnt = torch.zeros((nq, k), dtype=torch.float32, device="cuda"), torch.zeros(nq, dtype=torch.int32, device="cuda")
    s.graph_knn_except_device(torch.from_numpy(Q).cuda(), k, torch.from_numpy(np.concatenate(lists).view(np.int64)).cuda(),
                              torch.from_numpy(off).cuda(), d_ids, d_dist, d_cnt)
    torch.cuda.synchronize()
    _same((d_ids.cpu().numpy().view(np.uint64), d_dist.cpu().numpy(), d_cnt.cpu().numpy().view(np.uint32)), auto)
    s.drop()
