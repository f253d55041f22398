"""The graph walk under a row bitmap (ehx_graph_knn_masked*, k_graphm.hip) on the GPU.

The kernel is held, bit for bit, to tests/filtered_walk_model.py — a plain-Python statement of the walk, itself checked on
the CPU against the oracle's strict walk and against hnswlib's filtered search (tests/test_filtered_walk_model.py) — fed
the ORACLE's graph and the ORACLE's canonical distances: ids, distance bytes, counts, rows fetched, nodes expanded, and the
number of queries whose list reached its cap.  Then: the visited bitmap comes back clean, the routes, F16 rows, host and
device forms, errors, one query per call.  (Concurrency is not tested here: the call takes the locks ehx_knn_device takes
in graph mode.)"""
import ctypes as C

import numpy as np
import pytest

from filtered_walk_model import allowed_rows, filtered_search, walk_cap
from oracle import pyoracle

pytestmark = pytest.mark.gpu
ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402
from embeddinghub_amd.space import marshal_mask  # noqa: E402

METRICS = [(ehx.METRIC_L2SQ, pyoracle.METRIC_L2), (ehx.METRIC_IP, pyoracle.METRIC_IP),
           (ehx.METRIC_COSINE, pyoracle.METRIC_COSINE)]
# (rows, dims, queries, k, efs)
SHAPES = [(3000, 64, 24, 10, (10, 50, 200)),     # several levels; the reference's default ef first
          (1500, 768, 12, 10, (64,)),            # BASELINE dims
          (500, 19, 7, 3, (16,)),                # residual distance path
          (4000, 64, 8, 100, (10, 300))]         # k > ef: the list holds max(ef, k) (ef 300: cap = 3600)
BITMAPS = ["ones", "half", "tenth", "first_half", "entry_cleared", "one_row", "none", "short_bits"]
NO_ID = np.uint64(2**64 - 1)
SPARSE_SEED = 5     # chosen on the CPU: at 3000 x 64, share 1 / 50, ef 50 the model's list reaches cap (asserted below)
_built = {}


def _all_distances(X, Q, om):
    n = X.shape[0]
    ids, dist, _ = pyoracle.exhaustive(X, Q, n, om)
    D = np.empty((Q.shape[0], n), dtype=np.float32)
    np.put_along_axis(D, ids.astype(np.int64), dist, axis=1)
    return D


def _case(em, om, n, d, nq, dtype=None):
    """an oracle graph imported into a graph space (as tests/test_graph_wide.py builds it), queries and the oracle's
    distances of every query to every row — built once per (metric, shape), shared by the tests"""
    key = (em, n, d, nq, dtype)
    if key not in _built:
        rng = np.random.default_rng(n + d)
        X = rng.standard_normal((n, d)).astype(np.float32)
        Xs = X.astype(np.float16).astype(np.float32) if dtype == ehx.DTYPE_F16 else X   # (rows as an F16 space stores them)
        h = pyoracle.Hnsw(d, om, n, M=16)
        h.add_rows(Xs)
        kw = {} if dtype is None else {"dtype": dtype}
        s = ehx.Space.unique("gm", d, metric=em, mode=ehx.MODE_GRAPH, M=16, initial_capacity=n, build_batch=0xFFFFFFFF, **kw)
        s.set_batch(["k%d" % i for i in range(n)], X)
        l0, lv, upper = h.export_graph()
        s.graph_import(l0, lv, upper, h.enterpoint, h.maxlevel)
        Q = rng.standard_normal((nq, d)).astype(np.float32)
        _built[key] = (Xs, h, s, l0, upper, Q, _all_distances(Xs, Q, om))
    return _built[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_spaces():
    yield
    for v in _built.values():
        v[2].drop()
    _built.clear()


def _bitmap(name, n, entry, seed=1):
    """-> (packed words, n_bits)"""
    rng = np.random.default_rng(seed)
    a = np.zeros(n, dtype=bool)
    if name == "ones":
        a[:] = True
    elif name == "half":
        a = rng.random(n) < 0.5
    elif name == "tenth":
        a = rng.random(n) < 0.1
    elif name == "fiftieth":
        a = rng.random(n) < 0.02
    elif name == "first_half":
        a[:n // 2] = True
    elif name == "entry_cleared":
        a = rng.random(n) < 0.5
        a[entry] = False
    elif name == "one_row":
        a[(entry + n // 3) % n] = True
    elif name == "short_bits":          # n_bits = n - 37, the last word's spare bits (and the words behind it) set
        a = rng.random(n) < 0.5
        words, _ = marshal_mask(a)
        n_bits = n - 37
        words = words.copy()
        words[n_bits >> 5] |= np.uint32((0xFFFFFFFF << (n_bits & 31)) & 0xFFFFFFFF)
        words[(n_bits >> 5) + 1:] = 0xFFFFFFFF
        return words, n_bits
    return marshal_mask(a)


def _hook(s):
    out = (C.c_uint64 * 4)()
    fn = C.CDLL(_lib.LIB_PATH).ehx_test_graph_masked_counters
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    assert fn(s._h, out) == 0
    return np.array([int(v) for v in out], dtype=np.int64)   # walked, exact, calls, walked queries at cap


def _model(case, allowed, ef, k):
    Xs, h, s, l0, upper, Q, D = case
    e = max(ef, k)
    out, tot = [], {"n_dist": 0, "n_hops0": 0, "n_hops_up": 0, "hit_cap": 0}
    for i in range(Q.shape[0]):
        ids, dist, c = filtered_search(l0, upper, h.enterpoint, h.maxlevel, D[i], allowed, ef, walk_cap(e), k)
        out.append((ids, dist))
        for f in tot:
            tot[f] += int(c[f])
    return out, tot


def _assert_is_model(got, want, k, what):
    ids, dist, cnt = got
    for i, (m_ids, m_dist) in enumerate(want):
        c = len(m_ids)
        assert cnt[i] == c, (what, i, cnt[i], c)
        np.testing.assert_array_equal(ids[i, :c], m_ids, err_msg="%s query %d" % (what, i))
        assert dist[i, :c].tobytes() == m_dist.tobytes(), (what, i)
        assert (ids[i, c:] == NO_ID).all() and np.isposinf(dist[i, c:]).all(), (what, i)


def _walk_and_check(case, words, n_bits, ef, k, what):
    """one walked batch against the model: answers, work counters, queries at cap; -> the model's totals"""
    Xs, h, s, l0, upper, Q, D = case
    allowed = allowed_rows(words, n_bits, Xs.shape[0])
    s.set_ef(ef)
    s.stats_reset()
    before = _hook(s)
    got = s.graph_knn_masked(Q, k, words, n_bits, route=ehx.WALK_GRAPH)
    want, tot = _model(case, allowed, ef, k)
    _assert_is_model(got, want, k, what)
    g = s.graph_counters()
    assert (g[0], g[1], g[2]) == (tot["n_dist"], tot["n_hops0"], tot["n_hops_up"]), (what, g[:3], tot)
    st = s.stats()
    assert st["n_queries"] == Q.shape[0]
    d = Xs.shape[1]
    assert st["bytes_algorithmic"] == tot["n_dist"] * d * 4 + tot["n_hops0"] * (4 + 4 * 32) + tot["n_hops_up"] * (4 + 4 * 16)
    assert (_hook(s) - before).tolist() == [Q.shape[0], 0, 1, tot["hit_cap"]], what
    return tot


def _assert_plain_knn_is_the_oracles(case, ef, k, Q=None):
    """the visited bitmaps came back clean: an ordinary search on the same space is the oracle's, bit for bit"""
    Xs, h, s, l0, upper, Q0, D = case
    Q = Q0 if Q is None else Q
    h.set_ef(ef)
    s.set_ef(ef)
    labels, dists, counts, _, _ = h.search_batch(Q, k, threads=1)
    ids, dist, cnt = s.knn(Q, k)
    np.testing.assert_array_equal(cnt, counts)
    np.testing.assert_array_equal(ids, labels)
    assert dist.tobytes() == dists.tobytes()


@pytest.mark.parametrize("bitmap", BITMAPS)
@pytest.mark.parametrize("n,d,nq,k,efs", SHAPES)
@pytest.mark.parametrize("em,om", METRICS)
def test_walk_is_the_models_walk(em, om, n, d, nq, k, efs, bitmap):
    case = _case(em, om, n, d, nq)
    Xs, h, s, l0, upper, Q, D = case
    words, n_bits = _bitmap(bitmap, n, int(h.enterpoint))
    for ef in efs:
        _walk_and_check(case, words, n_bits, ef, k, "%s ef %d" % (bitmap, ef))
        if bitmap == "ones":   # ... which is then the oracle's own search
            h.set_ef(ef)
            labels, dists, counts, _, _ = h.search_batch(Q, k, threads=1)
            ids, dist, cnt = s.graph_knn_masked(Q, k, words, n_bits, route=ehx.WALK_GRAPH)
            np.testing.assert_array_equal(cnt, counts)
            np.testing.assert_array_equal(ids, labels)
            assert dist.tobytes() == dists.tobytes()
    _assert_plain_knn_is_the_oracles(case, efs[-1], k)


@pytest.mark.parametrize("em,om", METRICS)
def test_sparse_bitmap_where_the_cap_binds(em, om):
    n, d, nq, k, _ = SHAPES[0]
    case = _case(em, om, n, d, nq)
    words, n_bits = _bitmap("fiftieth", n, 0, seed=SPARSE_SEED)
    tot = _walk_and_check(case, words, n_bits, 50, k, "fiftieth ef 50")
    assert tot["hit_cap"] >= 1, "the cap must bind in this case: choose another SPARSE_SEED"
    _assert_plain_knn_is_the_oracles(case, 50, k)


def test_bitmaps_come_back_clean_between_batches_of_different_size():
    n, d, nq, k, _ = SHAPES[0]
    case = _case(ehx.METRIC_L2SQ, pyoracle.METRIC_L2, n, d, nq)
    Xs, h, s, l0, upper, Q, D = case
    words, n_bits = _bitmap("tenth", n, 0)
    allowed = allowed_rows(words, n_bits, n)
    want, _ = _model(case, allowed, 50, k)
    s.set_ef(50)
    for rows in (slice(0, nq), slice(0, 3), slice(5, 6), slice(0, nq)):    # large, then small, back to back
        got = s.graph_knn_masked(Q[rows], k, words, n_bits, route=ehx.WALK_GRAPH)
        _assert_is_model(got, want[rows], k, rows)
        _assert_plain_knn_is_the_oracles(case, 50, k, Q[rows])
        _assert_plain_knn_is_the_oracles(case, 50, k, Q[:2])


def test_one_query_per_call_is_its_row_of_the_batch():
    n, d, nq, k, _ = SHAPES[0]
    case = _case(ehx.METRIC_COSINE, pyoracle.METRIC_COSINE, n, d, nq)
    s, Q = case[2], case[5]
    words, n_bits = _bitmap("half", n, 0)
    s.set_ef(50)
    ids, dist, cnt = s.graph_knn_masked(Q, k, words, n_bits, route=ehx.WALK_GRAPH)
    for i in range(6):
        i1, d1, c1 = s.graph_knn_masked(Q[i:i + 1], k, words, n_bits, route=ehx.WALK_GRAPH)
        np.testing.assert_array_equal(i1[0], ids[i])
        assert d1.tobytes() == dist[i].tobytes() and c1[0] == cnt[i]


def _same(a, b):
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[0], b[0])
    assert a[1].tobytes() == b[1].tobytes()


def test_routes():
    n, d, nq, k, _ = SHAPES[0]
    case = _case(ehx.METRIC_L2SQ, pyoracle.METRIC_L2, n, d, nq)
    Xs, h, s, l0, upper, Q, D = case
    s.set_ef(50)
    # the exact route, and AUTO below the cut: ehx_knn_masked's answer byte for byte
    for name in ("half", "tenth", "one_row", "none"):
        words, n_bits = _bitmap(name, n, int(h.enterpoint))
        before = _hook(s)
        _same(s.graph_knn_masked(Q, k, words, n_bits, route=ehx.WALK_EXACT), s.knn_masked(Q, k, words, n_bits))
        assert (_hook(s) - before)[:3].tolist() == [0, nq, 1]
    # AUTO walks iff allowed * EHX_WALK_LIST_FACTOR >= rows covered: at the cut, one row below it, far above it
    n_bits = _lib.WALK_LIST_FACTOR * 187                 # rows covered: the cut is at exactly 187 allowed rows
    rng = np.random.default_rng(3)
    for n_allowed, walks in ((187, True), (186, False), (1500, True)):
        a = np.zeros(n, dtype=bool)
        a[rng.choice(n_bits, n_allowed, replace=False)] = True
        a[n_bits:] = True                                # (beyond n_bits: not allowed, not counted)
        words, _ = marshal_mask(a)
        before = _hook(s)
        got = s.graph_knn_masked(Q, k, words, n_bits)    # route = WALK_AUTO
        assert _lib.WALK_LIST_FACTOR * n_allowed >= n_bits if walks else _lib.WALK_LIST_FACTOR * n_allowed < n_bits
        if walks:
            want, tot = _model(case, allowed_rows(words, n_bits, n), 50, k)
            _assert_is_model(got, want, k, ("auto", n_allowed))
            assert (_hook(s) - before).tolist() == [nq, 0, 1, tot["hit_cap"]]
        else:
            _same(got, s.knn_masked(Q, k, words, n_bits))
            assert (_hook(s) - before)[:3].tolist() == [0, nq, 1]
    _assert_plain_knn_is_the_oracles(case, 50, k)
    # a flat space: the exact route whatever the route says
    f = ehx.Space.unique("gm-flat", d, metric=ehx.METRIC_L2SQ, initial_capacity=n)
    f.set_batch(["k%d" % i for i in range(n)], Xs)
    words, n_bits = _bitmap("half", n, 0)
    want = f.knn_masked(Q, k, words, n_bits)
    for route in (ehx.WALK_AUTO, ehx.WALK_GRAPH, ehx.WALK_EXACT):
        _same(f.graph_knn_masked(Q, k, words, n_bits, route=route), want)
    assert _hook(f)[:3].tolist() == [0, 3 * nq, 3]
    with pytest.raises(ehx.EhxError) as e:
        f.graph_knn_masked(Q, k, words, n_bits, route=3)
    assert e.value.code == _lib.EINVAL
    f.drop()


def test_f16_graph_space():
    n, d, nq, k = 1800, 72, 12, 10
    case = _case(ehx.METRIC_COSINE, pyoracle.METRIC_COSINE, n, d, nq, dtype=ehx.DTYPE_F16)
    for name in ("ones", "tenth"):
        words, n_bits = _bitmap(name, n, 0)
        _walk_and_check(case, words, n_bits, 40, k, "f16 " + name)
    _assert_plain_knn_is_the_oracles(case, 40, k)


def test_host_and_device_forms_agree():
    torch = pytest.importorskip("torch")
    n, d, nq, k, _ = SHAPES[0]
    case = _case(ehx.METRIC_IP, pyoracle.METRIC_IP, n, d, nq)
    s, Q = case[2], case[5]
    s.set_ef(50)
    words, n_bits = _bitmap("tenth", n, 0)
    dq = torch.from_numpy(Q).cuda()
    dm = torch.from_numpy(words.view(np.int32)).cuda()
    for route in (ehx.WALK_GRAPH, ehx.WALK_EXACT, ehx.WALK_AUTO):
        d_ids = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
        d_dist = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
        d_cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
        s.graph_knn_masked_device(dq, k, dm, n_bits, d_ids, d_dist, d_cnt, route=route)
        torch.cuda.synchronize()
        host = s.graph_knn_masked(Q, k, words, n_bits, route=route)
        _same((d_ids.cpu().numpy().view(np.uint64), d_dist.cpu().numpy(), d_cnt.cpu().numpy().view(np.uint32)), host)
    with pytest.raises(ValueError):
        s.graph_knn_masked_device(dq, k, dm[:3], n_bits, d_ids, d_dist, d_cnt)


def test_error_returns():
    n, d, nq, k, _ = SHAPES[2]
    Xs, h, s, l0, upper, Q, D = _case(ehx.METRIC_L2SQ, pyoracle.METRIC_L2, n, d, nq)
    allowed = np.ones(n, dtype=bool)
    for kk, route, code in ((0, ehx.WALK_GRAPH, _lib.EINVAL), (1025, ehx.WALK_GRAPH, _lib.EUNSUPPORTED),
                            (3, 3, _lib.EINVAL), (3, 0xFFFFFFFF, _lib.EINVAL)):
        with pytest.raises(ehx.EhxError) as e:
            s.graph_knn_masked(Q, kk, allowed, route=route)
        assert e.value.code == code
    s.set_ef(5000)          # effective ef above 4096: the walk refuses, as ehx_knn_device does in graph mode
    with pytest.raises(ehx.EhxError) as e:
        s.graph_knn_masked(Q, 3, allowed, route=ehx.WALK_GRAPH)
    assert e.value.code == _lib.EUNSUPPORTED
    s.set_ef(16)
    ids, dist, cnt = s.graph_knn_masked(np.zeros((0, d), dtype=np.float32), 4, allowed)   # no queries: EHX_OK
    assert ids.shape == (0, 4) and cnt.shape == (0,)
    L = _lib.load()
    q = np.ascontiguousarray(Q[:3])
    words = marshal_mask(allowed)[0]
    o_ids, o_dist, o_cnt = np.zeros((3, 4), dtype=np.uint64), np.zeros((3, 4), dtype=np.float32), np.zeros(3, dtype=np.uint32)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    args = [P(o_ids, C.c_uint64), P(o_dist, C.c_float), P(o_cnt, C.c_uint32)]
    G = ehx.WALK_GRAPH
    for hole in range(3):
        a = list(args)
        a[hole] = None
        assert L.ehx_graph_knn_masked(s._h, 3, P(q, C.c_float), 4, P(words, C.c_uint32), n, G, a[0], a[1], a[2]) == _lib.EINVAL
    assert L.ehx_graph_knn_masked(s._h, 3, None, 4, P(words, C.c_uint32), n, G, *args) == _lib.EINVAL
    assert L.ehx_graph_knn_masked(s._h, 3, P(q, C.c_float), 4, None, n, G, *args) == _lib.EINVAL    # a NULL mask with n_bits > 0
    for route in (ehx.WALK_AUTO, ehx.WALK_GRAPH, ehx.WALK_EXACT):                                  # n_bits == 0: count 0
        o_cnt[:] = 7
        assert L.ehx_graph_knn_masked(s._h, 3, P(q, C.c_float), 4, None, 0, route, *args) == _lib.OK
        assert (o_cnt == 0).all() and (o_ids == NO_ID).all() and np.isposinf(o_dist).all()
    assert L.ehx_graph_knn_masked(s._h, 3, P(q, C.c_float), 4, P(words, C.c_uint32), n, G, *args) == _lib.OK and (o_cnt == 4).all()
    assert L.ehx_graph_knn_masked_device(s._h, None, 3, None, 4, None, n, G, None, None, None) == _lib.EINVAL
    assert L.ehx_graph_knn_masked(None, 3, P(q, C.c_float), 4, P(words, C.c_uint32), n, G, *args) == _lib.EINVAL
    t = ehx.Space.unique("gm-drop", d, metric=ehx.METRIC_L2SQ, mode=ehx.MODE_GRAPH, initial_capacity=n)
    t.set_batch(["k%d" % i for i in range(n)], Xs)
    hnd = t._h
    t.drop()   # the tombstone answers for the dropped handle
    assert L.ehx_graph_knn_masked(hnd, 3, P(q, C.c_float), 4, P(words, C.c_uint32), n, G, *args) == _lib.ENOTFOUND
    sh = ehx.Space.unique("gm-sh", d, metric=ehx.METRIC_L2SQ, shards=2)
    sh.set_batch(["k%d" % i for i in range(n)], Xs)
    with pytest.raises(ehx.EhxError) as e:
        sh.graph_knn_masked(Q, 4, allowed)
    assert e.value.code == _lib.EUNSUPPORTED and "sharded" in str(e.value)
    sh.drop()
