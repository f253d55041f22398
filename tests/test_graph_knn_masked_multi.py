"""The graph walk under a table of bitmaps, one per query (ehx_graph_knn_masked_multi*, k_graphm.hip's
graph_search_tabled_kernel) on the GPU.

Every walked row is held, bit for bit, to tests/filtered_walk_model.py run for that query under ITS OWN bitmap, fed the
ORACLE's graph and the ORACLE's canonical distances: ids, distance bytes, counts, padding, and over the batch the rows
fetched, nodes expanded and queries whose list reached its cap.  Every row, on every route, is the one-bitmap call's for that
query alone; a batch EHX_WALK_AUTO splits has its walked rows from the model and its exact rows from ehx_knn_masked_multi.
Then: the visited bitmaps come back clean, the limits and refusals, host and device forms.  The graphs are the oracle's,
imported as tests/test_graph_knn_masked.py imports them; shapes are the smallest at which that kernel can go wrong."""
import ctypes as C

import numpy as np
import pytest

import graph_masked_multi_cases as gc
from oracle import pyoracle

pytestmark = pytest.mark.gpu
ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402
from embeddinghub_amd.space import marshal_mask_table  # noqa: E402

METRICS = [(ehx.METRIC_L2SQ, pyoracle.METRIC_L2), (ehx.METRIC_IP, pyoracle.METRIC_IP),
           (ehx.METRIC_COSINE, pyoracle.METRIC_COSINE)]
L2 = METRICS[0]
# (metric, rows, dims, queries, k, efs)
FIRST = (3000, 64, 24, 10, (10, 50, 200))       # several levels; the reference's default ef first
SHAPES = [m + FIRST for m in METRICS] + [
    L2 + (500, 19, 7, 3, (16,)),                # residual distance path; fewer queries than masks
    L2 + (4000, 64, 8, 100, (10, 300))]         # k > ef: the list holds max(ef, k) (ef 300: cap = 3600)
ROUTES = (ehx.WALK_GRAPH, ehx.WALK_EXACT, ehx.WALK_AUTO)
NO_ID = np.uint64(2**64 - 1)
_built = {}


def _case(em, om, n, d, nq, dtype=None):
    """an oracle graph imported into a graph space, queries and the oracle's distances of every query to every row — built
    once per (metric, shape), shared by the tests"""
    key = (em, n, d, nq, dtype)
    if key not in _built:
        rng = np.random.default_rng(n + d)
        X = rng.standard_normal((n, d)).astype(np.float32)
        Xs = X.astype(np.float16).astype(np.float32) if dtype == ehx.DTYPE_F16 else X   # (rows as an F16 space stores them)
        h = pyoracle.Hnsw(d, om, n, M=16)
        h.add_rows(Xs)
        kw = {} if dtype is None else {"dtype": dtype}
        s = ehx.Space.unique("gmm", d, metric=em, mode=ehx.MODE_GRAPH, M=16, initial_capacity=n, build_batch=0xFFFFFFFF, **kw)
        s.set_batch(["k%d" % i for i in range(n)], X)
        l0, lv, upper = h.export_graph()
        s.graph_import(l0, lv, upper, h.enterpoint, h.maxlevel)
        Q = rng.standard_normal((nq, d)).astype(np.float32)
        ids, dist, _ = pyoracle.exhaustive(Xs, Q, n, om)
        D = np.empty((nq, n), dtype=np.float32)
        np.put_along_axis(D, ids.astype(np.int64), dist, axis=1)
        _built[key] = {"key": key, "Xs": Xs, "h": h, "s": s, "Q": Q, "D": D, "n": n,
                       "graph": (l0, upper, int(h.enterpoint), int(h.maxlevel))}
    return _built[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_spaces():
    yield
    for v in _built.values():
        v["s"].drop()
    _built.clear()


def _hook(s):
    out = (C.c_uint64 * 4)()
    fn = C.CDLL(_lib.LIB_PATH).ehx_test_graph_masked_counters
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    assert fn(s._h, out) == 0
    return np.array([int(v) for v in out], dtype=np.int64)   # walked, exact, calls, walked queries at cap


def _assert_rows_are_models(got, rows, want, what):
    ids, dist, cnt = got
    for i, (m_ids, m_dist) in zip(rows, want):
        c = len(m_ids)
        assert cnt[i] == c, (what, i, cnt[i], c)
        np.testing.assert_array_equal(ids[i, :c], m_ids, err_msg="%s query %d" % (what, i))
        assert dist[i, :c].tobytes() == m_dist.tobytes(), (what, i)
        assert (ids[i, c:] == NO_ID).all() and np.isposinf(dist[i, c:]).all(), (what, i)


def _same(a, b, rows_a=slice(None), rows_b=slice(None)):
    np.testing.assert_array_equal(a[2][rows_a], b[2][rows_b])
    np.testing.assert_array_equal(a[0][rows_a], b[0][rows_b])
    assert np.ascontiguousarray(a[1][rows_a]).tobytes() == np.ascontiguousarray(b[1][rows_b]).tobytes()


def _walk_and_check(case, words, tab, n_bits, mask_of, ef, k, what):
    """one batch, every query walked, against the model: answers, work counters, queries at cap; -> the model's totals.
    words: what the call is given; tab: the bool table it means (cut at the rows covered here)"""
    s, Q, n = case["s"], case["Q"], case["n"]
    cut = tab.copy()
    cut[:, gc.covered(n_bits, n):] = False
    s.set_ef(ef)
    s.stats_reset()
    before = _hook(s)
    got = s.graph_knn_masked_multi(Q, k, words, mask_of, n_bits, route=ehx.WALK_GRAPH)
    want, tot = gc.model_rows(case["key"], case["graph"], case["D"], cut, mask_of, ef, k)
    _assert_rows_are_models(got, range(Q.shape[0]), want, what)
    g = s.graph_counters()
    assert (g[0], g[1], g[2]) == (tot["n_dist"], tot["n_hops0"], tot["n_hops_up"]), (what, g[:3], tot)
    assert s.stats()["n_queries"] == Q.shape[0]
    assert (_hook(s) - before).tolist() == [Q.shape[0], 0, 1, tot["hit_cap"]], what
    return tot


def _assert_plain_knn_is_the_oracles(case, ef, k, Q=None):
    """the visited bitmaps came back clean: an ordinary search on the same space is the oracle's, bit for bit"""
    h, s = case["h"], case["s"]
    Q = case["Q"] if Q is None else Q
    h.set_ef(ef)
    s.set_ef(ef)
    labels, dists, counts, _, _ = h.search_batch(Q, k, threads=1)
    ids, dist, cnt = s.knn(Q, k)
    np.testing.assert_array_equal(cnt, counts)
    np.testing.assert_array_equal(ids, labels)
    assert dist.tobytes() == dists.tobytes()


# ---- 1. the walk is the model's, per query ----
@pytest.mark.parametrize("assign", ["interleaved", "shuffled", "short_bits"])
@pytest.mark.parametrize("em,om,n,d,nq,k,efs", SHAPES)
def test_walk_is_the_models_walk_per_query(em, om, n, d, nq, k, efs, assign):
    case = _case(em, om, n, d, nq)
    tab = gc.table(gc.KINDS, n, case["graph"][2])
    mask_of = gc.shuffled(nq, len(gc.KINDS)) if assign == "shuffled" else gc.interleaved(nq, len(gc.KINDS))
    if assign == "short_bits":    # n_bits = n - 37: the last word's spare bits, and the words behind it, set
        n_bits = n - 37
        words = gc.short_bits(tab, n_bits)
    else:
        n_bits, words = n, tab
    for ef in efs:
        _walk_and_check(case, words, tab, n_bits, mask_of, ef, k, "%s ef %d" % (assign, ef))
    _assert_plain_knn_is_the_oracles(case, efs[-1], k)


def test_f16_graph_space():
    n, d, nq, k = 1800, 72, 12, 10
    case = _case(ehx.METRIC_COSINE, pyoracle.METRIC_COSINE, n, d, nq, dtype=ehx.DTYPE_F16)
    tab = gc.table(("ones", "tenth", "half", "none", "first_half"), n, case["graph"][2])
    _walk_and_check(case, tab, tab, n, gc.interleaved(nq, 5), 40, k, "f16")
    _assert_plain_knn_is_the_oracles(case, 40, k)


# ---- 2. the cap binds inside a table ----
@pytest.mark.parametrize("em,om", METRICS)
def test_sparse_bitmap_where_the_cap_binds_beside_dense_masks(em, om):
    n, d, nq, k, _ = FIRST
    case = _case(em, om, n, d, nq)
    tab = gc.table(("half", ("fiftieth", gc.SPARSE_SEED), "ones"), n, 0)
    mask_of = np.ones(nq, dtype=np.uint32)      # the sparse bitmap, but for two queries under each dense one
    mask_of[[0, 12]] = 0
    mask_of[[5, 17]] = 2
    tot = _walk_and_check(case, tab, tab, n, mask_of, 50, k, "fiftieth ef 50")
    assert tot["hit_cap"] >= 1, "the cap must bind in this case: choose another SPARSE_SEED"
    _assert_plain_knn_is_the_oracles(case, 50, k)


# ---- 3. row i is the one-bitmap call's ----
@pytest.mark.parametrize("route", ROUTES)
def test_row_i_is_the_one_bitmap_calls(route):
    n, d, nq, k, _ = FIRST
    case = _case(*METRICS[2], n, d, nq)
    s, Q = case["s"], case["Q"]
    s.set_ef(50)
    # (200 allowed rows: 12 * 200 < 3000, EHX_WALK_AUTO answers that mask exactly)
    tab = np.concatenate([gc.table(("ones", "half", "tenth", "none"), n, 0), gc.counted_table(n, n, (200,))])
    for mask_of in (gc.interleaved(nq, 5), gc.shuffled(nq, 5)):
        got = s.graph_knn_masked_multi(Q, k, tab, mask_of, route=route)
        for i in range(nq):
            _same(got, s.graph_knn_masked(Q[i:i + 1], k, tab[mask_of[i]], route=route), slice(i, i + 1))
    for m in (1, 4):   # a table of one is the one-bitmap call on the whole batch
        before = _hook(s)
        one = s.graph_knn_masked(Q, k, tab[m], route=route)
        mid = _hook(s)
        _same(s.graph_knn_masked_multi(Q, k, tab[m:m + 1], np.zeros(nq, dtype=np.uint32), route=route), one)
        assert (_hook(s) - mid)[:3].tolist() == (mid - before)[:3].tolist()
    _assert_plain_knn_is_the_oracles(case, 50, k)


# ---- 4. a batch EHX_WALK_AUTO splits ----
@pytest.mark.parametrize("em,om", METRICS)
def test_mixed_auto_batch(em, om):
    n, d, nq, k, _ = FIRST
    case = _case(em, om, n, d, nq)
    s, Q = case["s"], case["Q"]
    ef = 50
    s.set_ef(ef)
    # exactly 250 allowed rows (12 * 250 >= 3000: walked), exactly 249 (exact), half (walked), none (exact)
    tab = np.concatenate([gc.counted_table(n, n, (250, 249)), gc.table(("half", "none"), n, 0)])
    walks = gc.auto_walks(tab, n, n)
    assert walks.tolist() == [True, False, True, False]
    for mask_of in (gc.interleaved(nq, 4), gc.shuffled(nq, 4, seed=23)):
        iw, ix = gc.split(mask_of, walks)
        assert len(iw) and len(ix)
        s.stats_reset()
        before = _hook(s)
        got = s.graph_knn_masked_multi(Q, k, tab, mask_of)      # route = WALK_AUTO
        delta = _hook(s) - before
        want, tot = gc.model_rows(case["key"], case["graph"], case["D"], tab, mask_of, ef, k, rows=iw)
        _assert_rows_are_models(got, iw, want, "mixed, walked")
        assert delta.tolist() == [len(iw), len(ix), 1, tot["hit_cap"]]
        g = s.graph_counters()                                  # the walked queries' work only
        assert (g[0], g[1], g[2]) == (tot["n_dist"], tot["n_hops0"], tot["n_hops_up"])
        assert s.stats()["n_queries"] == nq                     # every query once
        _same(got, s.knn_masked_multi(Q, k, tab, mask_of), ix, ix)
    # all walk, all exact: answered in place
    mask_of = gc.interleaved(nq, 2)
    before = _hook(s)
    got = s.graph_knn_masked_multi(Q, k, tab[[0, 2]], mask_of)
    want, tot = gc.model_rows(case["key"], case["graph"], case["D"], tab[[0, 2]], mask_of, ef, k)
    _assert_rows_are_models(got, range(nq), want, "all walked")
    assert (_hook(s) - before).tolist() == [nq, 0, 1, tot["hit_cap"]]
    before = _hook(s)
    _same(s.graph_knn_masked_multi(Q, k, tab[[1, 3]], mask_of), s.knn_masked_multi(Q, k, tab[[1, 3]], mask_of))
    assert (_hook(s) - before).tolist() == [0, nq, 1, 0]
    _assert_plain_knn_is_the_oracles(case, ef, k)


# ---- 5. visited bitmaps come back clean ----
def test_bitmaps_come_back_clean_between_batches_of_different_size():
    n, d, nq, k, _ = FIRST
    case = _case(*L2, n, d, nq)
    s, Q = case["s"], case["Q"]
    tab = gc.table(("tenth", "half", "entry_cleared"), n, case["graph"][2])
    mask_of = gc.interleaved(nq, 3)
    want, _ = gc.model_rows(case["key"], case["graph"], case["D"], tab, mask_of, 50, k)
    s.set_ef(50)
    for rows in (slice(0, nq), slice(0, 3), slice(5, 6), slice(0, nq)):    # large, then small, back to back
        got = s.graph_knn_masked_multi(Q[rows], k, tab, mask_of[rows], route=ehx.WALK_GRAPH)
        _assert_rows_are_models(got, range(len(want[rows])), want[rows], rows)
        _assert_plain_knn_is_the_oracles(case, 50, k, Q[rows])
        _assert_plain_knn_is_the_oracles(case, 50, k, Q[:2])


# ---- 6. limits and errors ----
def test_sixty_four_masks_and_a_mask_no_query_uses():
    n, d, nq, k, _ = FIRST
    case = _case(*L2, n, d, nq)
    s, Q = case["s"], case["Q"]
    s.set_ef(50)
    tab = gc.table([("half", 100 + m) for m in range(gc.MAX_MASKS + 1)], n, 0)
    mask_of = ((np.arange(nq) * 11 + 63) % gc.MAX_MASKS).astype(np.uint32)      # the last bitmap first
    got = s.graph_knn_masked_multi(Q, k, tab[:64], mask_of, route=ehx.WALK_GRAPH)
    want, _ = gc.model_rows(case["key"], case["graph"], case["D"], tab[:64], mask_of, 50, k)
    _assert_rows_are_models(got, range(nq), want, "64 masks")
    for route in ROUTES:
        with pytest.raises(ehx.EhxError) as e:
            s.graph_knn_masked_multi(Q, k, tab, mask_of, route=route)
        assert e.value.code == _lib.EUNSUPPORTED
    # bitmap 1 is used by nobody — on AUTO it would be answered exactly, had it a query
    tab = np.concatenate([gc.table(("half",), n, 0), gc.counted_table(n, n, (7,)), gc.table(("tenth",), n, 0)])
    mask_of = (gc.interleaved(nq, 2) * 2).astype(np.uint32)
    for route in ROUTES:
        before = _hook(s)
        got = s.graph_knn_masked_multi(Q, k, tab, mask_of, route=route)
        assert (_hook(s) - before)[:3].tolist() == ([0, nq, 1] if route == ehx.WALK_EXACT else [nq, 0, 1])
        _same(got, s.graph_knn_masked_multi(Q, k, tab[[0, 2]], mask_of // 2, route=route))
    _assert_plain_knn_is_the_oracles(case, 50, k)


def _raw_args(Q, nq, k):
    q = np.ascontiguousarray(Q[:nq])
    o_ids, o_dist, o_cnt = np.zeros((nq, k), dtype=np.uint64), np.zeros((nq, k), dtype=np.float32), np.zeros(nq, dtype=np.uint32)
    return q, o_ids, o_dist, o_cnt


P = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731


def test_error_returns():
    n, d, nq, k = 500, 19, 7, 3
    case = _case(*L2, n, d, nq)
    s, Q, Xs = case["s"], case["Q"], case["Xs"]
    tab = np.ones((2, n), dtype=bool)
    mask_of = gc.interleaved(nq, 2)
    for kk, route, code in ((0, ehx.WALK_GRAPH, _lib.EINVAL), (1025, ehx.WALK_GRAPH, _lib.EUNSUPPORTED),
                            (3, 3, _lib.EINVAL), (3, 0xFFFFFFFF, _lib.EINVAL)):
        with pytest.raises(ehx.EhxError) as e:
            s.graph_knn_masked_multi(Q, kk, tab, mask_of, route=route)
        assert e.value.code == code
    s.set_ef(5000)          # effective ef above 4096: the walk refuses, as ehx_knn_device does in graph mode
    with pytest.raises(ehx.EhxError) as e:
        s.graph_knn_masked_multi(Q, 3, tab, mask_of, route=ehx.WALK_GRAPH)
    assert e.value.code == _lib.EUNSUPPORTED
    s.set_ef(16)
    ids, dist, cnt = s.graph_knn_masked_multi(np.zeros((0, d), dtype=np.float32), 4, tab, np.zeros(0, dtype=np.uint32))
    assert ids.shape == (0, 4) and cnt.shape == (0,)          # no queries: EHX_OK
    L = _lib.load()
    q, o_ids, o_dist, o_cnt = _raw_args(Q, 3, 4)
    words = marshal_mask_table(tab)[0]
    of = np.array([0, 1, 1], dtype=np.uint32)
    W, OF = P(words, C.c_uint32), P(of, C.c_uint32)
    args = [P(o_ids, C.c_uint64), P(o_dist, C.c_float), P(o_cnt, C.c_uint32)]
    G = ehx.WALK_GRAPH
    fn = L.ehx_graph_knn_masked_multi
    for hole in range(3):
        a = list(args)
        a[hole] = None
        assert fn(s._h, 3, P(q, C.c_float), 4, W, 2, n, OF, G, *a) == _lib.EINVAL
    assert fn(s._h, 3, None, 4, W, 2, n, OF, G, *args) == _lib.EINVAL
    assert fn(s._h, 3, P(q, C.c_float), 4, None, 2, n, OF, G, *args) == _lib.EINVAL     # NULL masks with n_bits > 0
    assert fn(s._h, 3, P(q, C.c_float), 4, W, 2, n, None, G, *args) == _lib.EINVAL      # a NULL mask_of
    assert fn(s._h, 3, P(q, C.c_float), 4, W, 0, n, OF, G, *args) == _lib.EINVAL        # no bitmap, with queries
    assert fn(s._h, 0, P(q, C.c_float), 4, W, 0, n, OF, G, *args) == _lib.OK            # ... and without
    assert fn(s._h, 3, P(q, C.c_float), 4, W, 65, n, OF, G, *args) == _lib.EUNSUPPORTED
    for route in ROUTES:                                                                # n_bits == 0: count 0
        o_cnt[:] = 7
        assert fn(s._h, 3, P(q, C.c_float), 4, None, 2, 0, OF, route, *args) == _lib.OK
        assert (o_cnt == 0).all() and (o_ids == NO_ID).all() and np.isposinf(o_dist).all()
    assert fn(s._h, 3, P(q, C.c_float), 4, W, 2, n, OF, G, *args) == _lib.OK and (o_cnt == 4).all()
    assert L.ehx_graph_knn_masked_multi_device(s._h, None, 3, None, 4, None, 2, n, None, G, None, None, None) == _lib.EINVAL
    assert fn(None, 3, P(q, C.c_float), 4, W, 2, n, OF, G, *args) == _lib.EINVAL
    # a graph that does not cover the rows: the walk refuses, the exact route answers
    t = ehx.Space.unique("gmm-bare", d, metric=ehx.METRIC_L2SQ, mode=ehx.MODE_GRAPH, initial_capacity=n, build_batch=0xFFFFFFFF)
    t.set_batch(["k%d" % i for i in range(n)], Xs)
    with pytest.raises(ehx.EhxError) as e:
        t.graph_knn_masked_multi(Q, 3, tab, mask_of, route=ehx.WALK_GRAPH)
    assert e.value.code == _lib.EUNSUPPORTED and "graph covers" in str(e.value)
    assert (t.graph_knn_masked_multi(Q, 3, tab, mask_of, route=ehx.WALK_EXACT)[2] == 3).all()
    hnd = t._h
    t.drop()   # the tombstone answers for the dropped handle
    assert fn(hnd, 3, P(q, C.c_float), 4, W, 2, n, OF, G, *args) == _lib.ENOTFOUND
    sh = ehx.Space.unique("gmm-sh", d, metric=ehx.METRIC_L2SQ, shards=2)
    sh.set_batch(["k%d" % i for i in range(n)], Xs)
    with pytest.raises(ehx.EhxError) as e:
        sh.graph_knn_masked_multi(Q, 4, tab, mask_of)
    assert e.value.code == _lib.EUNSUPPORTED and "sharded" in str(e.value)
    sh.drop()


def test_a_bad_mask_of_leaves_the_outputs_unwritten_in_both_forms():
    torch = pytest.importorskip("torch")
    n, d, nq, k = 500, 19, 7, 3
    case = _case(*L2, n, d, nq)
    s, Q = case["s"], case["Q"]
    s.set_ef(16)
    L = _lib.load()
    tab = gc.table(("half", "ones"), n, 0)
    words = marshal_mask_table(tab)[0]
    of = gc.interleaved(nq, 2)
    of[4] = 2                                   # n_masks = 2
    q, o_ids, o_dist, o_cnt = _raw_args(Q, nq, k)
    dq, dm = torch.from_numpy(q).cuda(), torch.from_numpy(words.view(np.int32)).cuda()
    dof = torch.from_numpy(of.view(np.int32)).cuda()
    for route in ROUTES:
        o_ids[:], o_dist[:], o_cnt[:] = 77, -5.0, 9
        assert L.ehx_graph_knn_masked_multi(s._h, nq, P(q, C.c_float), k, P(words, C.c_uint32), 2, n, P(of, C.c_uint32), route,
                                            P(o_ids, C.c_uint64), P(o_dist, C.c_float), P(o_cnt, C.c_uint32)) == _lib.EINVAL
        assert b"mask_of[4] = 2" in L.ehx_last_error()
        assert (o_ids == 77).all() and (o_dist == -5.0).all() and (o_cnt == 9).all()
        d_ids = torch.full((nq, k), 77, dtype=torch.int64, device="cuda")
        d_dist = torch.full((nq, k), -5.0, dtype=torch.float32, device="cuda")
        d_cnt = torch.full((nq,), 9, dtype=torch.int32, device="cuda")
        with pytest.raises(ehx.EhxError) as e:
            s.graph_knn_masked_multi_device(dq, k, dm, 2, n, dof, d_ids, d_dist, d_cnt, route=route)
        assert e.value.code == _lib.EINVAL and "mask_of[4] = 2" in str(e.value)
        torch.cuda.synchronize()
        assert (d_ids == 77).all() and (d_dist == -5.0).all() and (d_cnt == 9).all()
    _assert_plain_knn_is_the_oracles(case, 16, k)


def test_a_flat_space_is_answered_exactly_on_every_route():
    n, d, nq, k, _ = FIRST
    case = _case(*L2, n, d, nq)
    Q = case["Q"]
    f = ehx.Space.unique("gmm-flat", d, metric=ehx.METRIC_L2SQ, initial_capacity=n)
    f.set_batch(["k%d" % i for i in range(n)], case["Xs"])
    tab = gc.table(("half", "tenth", "none", "ones"), n, 0)
    mask_of = gc.shuffled(nq, 4)
    want = f.knn_masked_multi(Q, k, tab, mask_of)
    for route in ROUTES:
        _same(f.graph_knn_masked_multi(Q, k, tab, mask_of, route=route), want)
    assert _hook(f)[:3].tolist() == [0, 3 * nq, 3]
    with pytest.raises(ehx.EhxError) as e:
        f.graph_knn_masked_multi(Q, k, tab, mask_of, route=3)
    assert e.value.code == _lib.EINVAL
    f.drop()


# ---- 7. host and device forms agree ----
def test_host_and_device_forms_agree():
    torch = pytest.importorskip("torch")
    n, d, nq, k, _ = FIRST
    case = _case(*METRICS[1], n, d, nq)
    s, Q = case["s"], case["Q"]
    s.set_ef(50)
    # (AUTO splits this table: 100 allowed rows are answered exactly)
    tab = np.concatenate([gc.table(("tenth", "half"), n, 0), gc.counted_table(n, n, (100,))])
    n_bits = n - 37
    words = gc.short_bits(tab, n_bits)
    mask_of = gc.shuffled(nq, 3)
    dq = torch.from_numpy(Q).cuda()
    # (the device table is dense at ceil(n_bits / 32) words per bitmap)
    dm = torch.from_numpy(np.ascontiguousarray(words[:, :(n_bits + 31) // 32]).view(np.int32)).cuda()
    dof = torch.from_numpy(mask_of.view(np.int32)).cuda()
    for route in ROUTES:
        d_ids = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
        d_dist = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
        d_cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
        before = _hook(s)
        s.graph_knn_masked_multi_device(dq, k, dm, 3, n_bits, dof, d_ids, d_dist, d_cnt, route=route)
        torch.cuda.synchronize()
        mid = _hook(s)
        host = s.graph_knn_masked_multi(Q, k, words, mask_of, n_bits, route=route)
        assert (_hook(s) - mid).tolist() == (mid - before).tolist()
        _same((d_ids.cpu().numpy().view(np.uint64), d_dist.cpu().numpy(), d_cnt.cpu().numpy().view(np.uint32)), host)
    with pytest.raises(ValueError):
        s.graph_knn_masked_multi_device(dq, k, dm[:2], 3, n_bits, dof, d_ids, d_dist, d_cnt)
    with pytest.raises(ValueError):
        s.graph_knn_masked_multi_device(dq, k, dm, 3, n_bits, dof[:5], d_ids, d_dist, d_cnt)
    _assert_plain_knn_is_the_oracles(case, 50, k)
