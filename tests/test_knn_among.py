"""GPU tests of the exact kNN restricted to lists of row ids (ehx_knn_among, ehx_knn_among_device, ehx_knn_among_keys).

Expected answers come from the oracle only: a list L is sorted and made unique on the host (ids at or above the row count
dropped), pyoracle.exhaustive(X[L], q, k, metric) answers, and its local ids are mapped back through L — tie order by
local id is then tie order by global id.  Ids must be equal and distance BYTES must be equal.  F16 spaces use the oracle
on X.astype(float16).astype(float32)."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402
from embeddinghub_amd.space import marshal_keys  # noqa: E402

METRICS = [(ehx.METRIC_L2SQ, pyoracle.METRIC_L2), (ehx.METRIC_IP, pyoracle.METRIC_IP),
           (ehx.METRIC_COSINE, pyoracle.METRIC_COSINE)]
NO_ID = np.uint64(2**64 - 1)


def _keys(n):
    return ["k%d" % i for i in range(n)]


def _expected(X, Q, k, om, lists):
    """[(ids, dist)] per query; `lists`: one id sequence per query"""
    out = []
    for i, L in enumerate(lists):
        Lu = np.unique(np.asarray(L, dtype=np.uint64))
        Lu = Lu[Lu < np.uint64(X.shape[0])].astype(np.int64)
        if Lu.size == 0:
            out.append(([], np.zeros(0, dtype=np.float32)))
            continue
        oi, od, oc = pyoracle.exhaustive(X[Lu], Q[i:i + 1], k, om, threads=1)
        c = int(oc[0])
        out.append(([int(v) for v in Lu[oi[0, :c].astype(np.int64)]], od[0, :c].copy()))
    return out


def _expected_shared(X, Q, k, om, L):
    Lu = np.unique(np.asarray(L, dtype=np.uint64))
    Lu = Lu[Lu < np.uint64(X.shape[0])].astype(np.int64)
    oi, od, oc = pyoracle.exhaustive(X[Lu], Q, k, om)
    return [([int(v) for v in Lu[oi[i, :int(oc[i])].astype(np.int64)]], od[i, :int(oc[i])].copy()) for i in range(len(Q))]


def _assert_rows(ids, dist, cnt, want, what):
    assert len(cnt) == len(want)
    k = ids.shape[1]
    for i, (wids, wdist) in enumerate(want):
        c = int(cnt[i])
        assert c == len(wids), "%s: query %d has %d results, the oracle %d" % (what, i, c, len(wids))
        assert [int(v) for v in ids[i, :c]] == wids, "%s: query %d ids differ" % (what, i)
        assert dist[i, :c].tobytes() == wdist.tobytes(), "%s: query %d distance bytes differ" % (what, i)
        assert (ids[i, c:k] == NO_ID).all() and np.isposinf(dist[i, c:k]).all(), "%s: query %d tail sentinels" % (what, i)


def _device_form(space, Q, k, ids, off, hint):
    import torch
    dq = torch.tensor(np.ascontiguousarray(Q, dtype=np.float32), device="cuda")
    d_ids = torch.tensor(np.asarray(ids, dtype=np.uint64).view(np.int64), device="cuda")
    d_off = None if off is None else torch.tensor(np.asarray(off, dtype=np.uint64).view(np.int64), device="cuda")
    o_ids = torch.full((len(Q), k), -7, dtype=torch.int64, device="cuda")
    o_dist = torch.full((len(Q), k), -7.0, dtype=torch.float32, device="cuda")
    o_cnt = torch.full((len(Q),), 77, dtype=torch.int32, device="cuda")
    space.knn_among_device(dq, k, d_ids, d_off, o_ids, o_dist, o_cnt, max_list_hint=hint)
    torch.cuda.synchronize()
    return (o_ids.cpu().numpy().view(np.uint64), o_dist.cpu().numpy(), o_cnt.cpu().numpy().view(np.uint32))


def _ragged_lists(rng, n, nq, k):
    """per-query lists of lengths {0, 1, k-1, 63, 64, 65, 257, 1500}, unsorted, some holding ids >= n"""
    lens = [0, 1, k - 1, 63, 64, 65, 257, 1500]
    lists = []
    for i in range(nq):
        L = rng.choice(n, size=lens[i % len(lens)], replace=False).astype(np.uint64)
        if i % 3 == 1:
            L = np.concatenate([L, np.array([n, n + 5, 2**40], dtype=np.uint64)])
            rng.shuffle(L)
        lists.append(L)
    return lists


def _flat(ids_lists):
    off = np.zeros(len(ids_lists) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(L) for L in ids_lists])
    return np.concatenate(ids_lists).astype(np.uint64), off


@pytest.mark.parametrize("d", [3, 7, 24, 30, 96, 129])
@pytest.mark.parametrize("em,om", METRICS)
def test_per_query_lists_flat_f32(em, om, d):
    rng = np.random.default_rng(100 + d)
    n, nq, k = 3000, 64, 10
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    s = ehx.Space.unique("among", d, metric=em, initial_capacity=n)
    s.set_batch(_keys(n), X)
    lists = _ragged_lists(rng, n, nq, k)
    want = _expected(X, Q, k, om, lists)
    _assert_rows(*s.knn_among(Q, k, [list(map(int, L)) for L in lists]), want, "host form, list of lists")
    ids, off = _flat(lists)
    _assert_rows(*s.knn_among(Q, k, ids, off), want, "host form, offsets")
    # the grid-stride loop: the hint sizes the launch only
    for hint in (0, 1503, 64):
        _assert_rows(*_device_form(s, Q, k, ids, off, hint), want, "device form, hint %d" % hint)
    s.drop()


@pytest.mark.parametrize("em,om", METRICS)
def test_shared_list(em, om):
    rng = np.random.default_rng(7)
    n, d, nq = 3000, 40, 203   # 26 query tiles, the last one ragged
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    s = ehx.Space.unique("among-sh", d, metric=em, initial_capacity=n)
    s.set_batch(_keys(n), X)
    L = rng.choice(n, size=1000, replace=False).astype(np.uint64)
    for k in (1, 10, 48, 64):
        want = _expected_shared(X, Q, k, om, L)
        _assert_rows(*s.knn_among(Q, k, L), want, "shared list k=%d" % k)
    want = _expected_shared(X, Q, 10, om, L)
    _assert_rows(*_device_form(s, Q, 10, L, None, 0), want, "shared list, device form")
    # a hint of 64: ONE workgroup per query tile walks all 16 chunks of the list (grid-stride loop, keys reset per chunk,
    # every chunk merged into the lists kept in registers)
    _assert_rows(*_device_form(s, Q, 10, L, None, 64), want, "shared list, device form, hint 64")
    s.drop()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("em,om", [METRICS[0], METRICS[2]])
def test_shared_list_longer_than_the_grid(em, om, dtype):
    """1030 queries are 129 query tiles, which leaves 4096 / 129 = 31 workgroups per tile: the 40 chunks of a 2500-id list
    make some workgroups walk two chunks, others one; k = 100 does it once more with a floor"""
    rng = np.random.default_rng(21)
    n, d, nq = 3000, 20, 1030
    X = rng.standard_normal((n, d)).astype(np.float32)
    Xs = X.astype(np.float16).astype(np.float32) if dtype == "f16" else X
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    s = ehx.Space.unique("among-grid", d, metric=em, initial_capacity=n,
                         dtype=ehx.DTYPE_F16 if dtype == "f16" else ehx.DTYPE_F32)
    s.set_batch(_keys(n), X)
    L = np.concatenate([rng.choice(n, size=2500, replace=False), [n + 3]]).astype(np.uint64)
    _assert_rows(*s.knn_among(Q, 10, L), _expected_shared(Xs, Q, 10, om, L), "long shared list")
    _assert_rows(*s.knn_among(Q, 100, L), _expected_shared(Xs, Q, 100, om, L), "long shared list, paged")
    s.drop()


@pytest.mark.parametrize("d", [1030, 2500])
def test_shared_list_long_rows(d):
    """d = 1030: the staged tiles need more than the default 64 KiB of LDS per workgroup; d = 2500: they do not fit the
    CU's LDS at all and the shared list goes through the per-query kernel"""
    rng = np.random.default_rng(d)
    n, nq, k = 600, 17, 10
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    s = ehx.Space.unique("among-long", d, metric=ehx.METRIC_COSINE, initial_capacity=n)
    s.set_batch(_keys(n), X)
    L = rng.choice(n, size=300, replace=False)
    _assert_rows(*s.knn_among(Q, k, L), _expected_shared(X, Q, k, pyoracle.METRIC_COSINE, L), "long rows")
    s.drop()


@pytest.mark.parametrize("shared", [True, False])
def test_paging(shared):
    rng = np.random.default_rng(11)
    n, d, nq = 3000, 24, 9
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    s = ehx.Space.unique("among-pg", d, metric=ehx.METRIC_L2SQ, initial_capacity=n)
    s.set_batch(_keys(n), X)
    L = rng.choice(n, size=400, replace=False).astype(np.uint64)
    for k in (100, 300, 700):   # 700 > the list: count = list length, tail sentinels
        if shared:
            want = _expected_shared(X, Q, k, pyoracle.METRIC_L2, L)
            got = s.knn_among(Q, k, L)
        else:
            want = _expected(X, Q, k, pyoracle.METRIC_L2, [L] * nq)
            got = s.knn_among(Q, k, [L] * nq)
        assert all(len(w[0]) == min(k, 400) for w in want)
        _assert_rows(*got, want, "k=%d" % k)
    s.drop()


@pytest.mark.parametrize("d", [24, 72])
@pytest.mark.parametrize("em,om", [METRICS[0], METRICS[2]])
def test_f16_flat_space(em, om, d):
    rng = np.random.default_rng(d)
    n, nq, k = 3000, 64, 10
    X = rng.standard_normal((n, d)).astype(np.float32)
    Xs = X.astype(np.float16).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    s = ehx.Space.unique("among-f16", d, metric=em, initial_capacity=n, dtype=ehx.DTYPE_F16)
    s.set_batch(_keys(n), X)
    lists = _ragged_lists(rng, n, nq, k)
    _assert_rows(*s.knn_among(Q, k, lists), _expected(Xs, Q, k, om, lists), "f16 per-query lists")
    L = rng.choice(n, size=1000, replace=False)
    _assert_rows(*s.knn_among(Q, k, L), _expected_shared(Xs, Q, k, om, L), "f16 shared list")
    s.drop()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("d", [32, 100])
@pytest.mark.parametrize("em,om", [METRICS[0], METRICS[2]])
def test_graph_spaces(em, om, d, dtype):
    """the listed rows are scanned exactly, whatever the graph: F32 graph spaces store their rows once, block-permuted"""
    rng = np.random.default_rng(1000 + d)
    n, nq, k = 2000, 64, 10
    X = rng.standard_normal((n, d)).astype(np.float32)
    Xs = X.astype(np.float16).astype(np.float32) if dtype == "f16" else X
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    s = ehx.Space.unique("among-graph", d, metric=em, mode=ehx.MODE_GRAPH, M=16, initial_capacity=n,
                         dtype=ehx.DTYPE_F16 if dtype == "f16" else ehx.DTYPE_F32)
    s.set_batch(_keys(n), X)
    lists = _ragged_lists(rng, n, nq, k)
    _assert_rows(*s.knn_among(Q, k, lists), _expected(Xs, Q, k, om, lists), "graph per-query lists")
    L = rng.choice(n, size=700, replace=False)
    _assert_rows(*s.knn_among(Q, k, L), _expected_shared(Xs, Q, k, om, L), "graph shared list")
    _assert_rows(*s.knn_among(Q[:5], 100, L), _expected_shared(Xs, Q[:5], 100, om, L), "graph shared list, paged")
    _assert_rows(*_device_form(s, Q, k, L, None, 64), _expected_shared(Xs, Q, k, om, L), "graph shared list, one block")
    s.drop()


def test_ties_come_back_in_id_order():
    rng = np.random.default_rng(3)
    n, d = 500, 24
    X = rng.standard_normal((n, d)).astype(np.float32)
    X[[17, 230, 401]] = X[5]
    Q = np.stack([X[5], X[5] + 0.25]).astype(np.float32)
    s = ehx.Space.unique("among-ties", d, metric=ehx.METRIC_L2SQ, initial_capacity=n)
    s.set_batch(_keys(n), X)
    L = np.array([401, 8, 230, 17, 300, 44], dtype=np.uint64)
    for form in (L, [L, L]):
        ids, dist, cnt = s.knn_among(Q, 3, form)
        for i in range(2):
            assert [int(v) for v in ids[i]] == [17, 230, 401] and dist[i, 0] == dist[i, 1] == dist[i, 2]
        _assert_rows(ids, dist, cnt, _expected_shared(X, Q, 3, pyoracle.METRIC_L2, L), "ties")
    s.drop()


def test_non_finite_values():
    rng = np.random.default_rng(4)
    n, d = 300, 24
    X = rng.standard_normal((n, d)).astype(np.float32)
    X[10, 3] = np.nan          # a NaN distance is no neighbour
    X[20] = 3.0e38             # (q - x)^2 overflows: +Inf is a distance
    Q = rng.standard_normal((4, d)).astype(np.float32)
    s = ehx.Space.unique("among-nf", d, metric=ehx.METRIC_L2SQ, initial_capacity=n)
    s.set_batch(_keys(n), X)
    L = np.array([10, 20, 1, 2, 3], dtype=np.uint64)
    for form in (L, [L] * 4):
        ids, dist, cnt = s.knn_among(Q, 5, form)
        assert (cnt == 4).all()
        for i in range(4):
            got = [int(v) for v in ids[i, :4]]
            assert 10 not in got and got[3] == 20 and np.isposinf(dist[i, 3])
        _assert_rows(ids, dist, cnt, _expected_shared(X, Q, 5, pyoracle.METRIC_L2, L), "non-finite")
    s.drop()


@pytest.mark.parametrize("shared", [True, False])
def test_repeated_ids_do_no_harm(shared):
    rng = np.random.default_rng(5)
    n, d, nq, k = 1000, 30, 16, 70   # two pages
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    s = ehx.Space.unique("among-dup", d, metric=ehx.METRIC_L2SQ, initial_capacity=n)
    s.set_batch(_keys(n), X)
    base = rng.choice(n, size=90, replace=False)
    L = np.concatenate([base, base[:40], base[:7], base[:7]]).astype(np.uint64)
    rng.shuffle(L)
    ids, dist, cnt = s.knn_among(Q, k, L if shared else [L] * nq)   # (EHX_OK: no exception)
    allowed = set(int(v) for v in base)
    for i in range(nq):
        c = int(cnt[i])
        assert 0 < c <= k
        assert all(int(v) in allowed for v in ids[i, :c])
        assert (np.diff(dist[i, :c]) >= 0).all()
        for j in range(c):
            want = np.float32(pyoracle.dist(pyoracle.METRIC_L2, Q[i], X[int(ids[i, j])]))
            assert dist[i, j].tobytes() == want.tobytes()
    s.drop()


def test_keys_form():
    rng = np.random.default_rng(6)
    n, d, nq, k = 1500, 24, 20, 10
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    keys = _keys(n)
    s = ehx.Space.unique("among-keys", d, metric=ehx.METRIC_COSINE, initial_capacity=n)
    s.set_batch(keys, X)
    L = rng.choice(n, size=333, replace=False)
    got = s.knn_among_keys(Q, k, [keys[i] for i in L])
    _assert_rows(*got, _expected_shared(X, Q, k, pyoracle.METRIC_COSINE, L), "keys form")
    ref = s.knn_among(Q, k, L)
    assert np.array_equal(got[0], ref[0]) and got[1].tobytes() == ref[1].tobytes() and np.array_equal(got[2], ref[2])
    # an unknown key: ENOTFOUND, its index, outputs untouched
    bad = [keys[1], keys[2], "nope", keys[3]]
    with pytest.raises(ehx.EhxError) as e:
        s.knn_among_keys(Q, k, bad)
    assert e.value.code == _lib.ENOTFOUND and e.value.bad_index == 2
    na, arr, lens, keep = marshal_keys(bad)
    ids = np.full((nq, k), 12345, dtype=np.uint64)
    dist = np.full((nq, k), -3.0, dtype=np.float32)
    cnt = np.full(nq, 99, dtype=np.uint32)
    bi = C.c_size_t(77)
    q = np.ascontiguousarray(Q)
    rc = _lib.load().ehx_knn_among_keys(s._h, nq, q.ctypes.data_as(C.POINTER(C.c_float)), k, na, arr, lens,
                                        ids.ctypes.data_as(C.POINTER(C.c_uint64)), dist.ctypes.data_as(C.POINTER(C.c_float)),
                                        cnt.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(bi))
    del keep
    assert rc == _lib.ENOTFOUND and bi.value == 2
    assert (ids == 12345).all() and (dist == -3.0).all() and (cnt == 99).all()
    s.drop()


def test_error_returns():
    rng = np.random.default_rng(8)
    n, d = 200, 8
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((3, d)).astype(np.float32)
    s = ehx.Space.unique("among-err", d, metric=ehx.METRIC_L2SQ, initial_capacity=n)
    s.set_batch(_keys(n), X)
    ids = np.arange(10, dtype=np.uint64)
    for off in ([0, 5, 3, 10], [0, 3, 5, 9], [2, 1, 5, 10]):   # decreasing; not ending at n_cand
        with pytest.raises(ehx.EhxError) as e:
            s.knn_among(Q, 2, ids, np.array(off, dtype=np.uint64))
        assert e.value.code == _lib.EINVAL
    with pytest.raises(ehx.EhxError) as e:
        s.knn_among(Q, 1025, ids)
    assert e.value.code == _lib.EUNSUPPORTED
    with pytest.raises(ehx.EhxError) as e:
        s.knn_among(Q, 0, ids)
    assert e.value.code == _lib.EINVAL
    # an empty shared list, and a space that is still empty: count 0
    ids0, dist0, cnt0 = s.knn_among(Q, 4, np.zeros(0, dtype=np.uint64))
    assert (cnt0 == 0).all() and (ids0 == NO_ID).all() and np.isposinf(dist0).all()
    s.drop()
    e0 = ehx.Space.unique("among-empty", d, metric=ehx.METRIC_L2SQ)
    assert (e0.knn_among(Q, 4, ids)[2] == 0).all()
    e0.drop()
    sh = ehx.Space.unique("among-sh2", d, metric=ehx.METRIC_L2SQ, shards=2)
    sh.set_batch(_keys(n), X)
    with pytest.raises(ehx.EhxError) as e:
        sh.knn_among(Q, 2, ids)
    assert e.value.code == _lib.EUNSUPPORTED and "sharded" in str(e.value)
    sh.drop()


def test_stats_deltas():
    rng = np.random.default_rng(9)
    n, d, nq = 1000, 16, 12
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    s = ehx.Space.unique("among-stats", d, metric=ehx.METRIC_L2SQ, initial_capacity=n)
    s.set_batch(_keys(n), X)
    L = rng.choice(n, size=250, replace=False).astype(np.uint64)
    st0 = s.stats()
    s.knn_among(Q, 5, L)
    st1 = s.stats()
    assert st1["n_queries"] - st0["n_queries"] == nq
    assert st1["n_dist"] - st0["n_dist"] == nq * 250
    lists = [L[:i * 3] for i in range(nq)]
    s.knn_among(Q, 5, lists)
    st2 = s.stats()
    assert st2["n_queries"] - st1["n_queries"] == nq
    assert st2["n_dist"] - st1["n_dist"] == sum(len(x) for x in lists)
    assert st2["n_rerank"] == st0["n_rerank"] and st2["n_uncertified"] == 0
    s.drop()


def test_search_rewrite_search():
    rng = np.random.default_rng(10)
    n, d, nq, k = 2000, 48, 32, 10
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    keys = _keys(n)
    s = ehx.Space.unique("among-rw", d, metric=ehx.METRIC_COSINE, initial_capacity=n)
    s.set_batch(keys, X)
    L = rng.choice(n, size=600, replace=False)
    _assert_rows(*s.knn_among(Q, k, L), _expected_shared(X, Q, k, pyoracle.METRIC_COSINE, L), "before the rewrite")
    rew = L[:200]
    X[rew] = (Q[rng.integers(0, nq, size=200)] + 0.1 * rng.standard_normal((200, d))).astype(np.float32)
    s.set_batch([keys[i] for i in rew], X[rew])
    _assert_rows(*s.knn_among(Q, k, L), _expected_shared(X, Q, k, pyoracle.METRIC_COSINE, L), "after the rewrite")
    lists = [L[i::4] for i in range(nq)]
    _assert_rows(*s.knn_among(Q, k, lists), _expected(X, Q, k, pyoracle.METRIC_COSINE, lists), "after, per-query lists")
    s.drop()
