"""GPU tests of the batched nearest-neighbour lookup by stored key (ehx_knn_by_keys, ehx_knn_by_keys_keys,
ehx_knn_by_ids_device): the query batch is gathered from the stored rows on the device, searched with k + 1, and every
row is dropped from its own list on the device.

Expected answers come from the oracle, never from the engine: pyoracle.exhaustive(X, X[idx], k + 1) (flat spaces) or
pyoracle.Hnsw.search_batch(X[idx], k + 1) over the identical graph (graph spaces), then the rule of server.cc:205-207 in
Python — remove the first occurrence of the query's own id if present, else the last entry, truncate to k.  Ids must be
equal and distance BYTES must be equal.  Beside the oracle, every batch row must equal ehx_knn_by_key of that key."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib, offlinehub  # noqa: E402
from embeddinghub_amd.space import marshal_keys  # noqa: E402

METRICS = [(ehx.METRIC_L2SQ, pyoracle.METRIC_L2), (ehx.METRIC_IP, pyoracle.METRIC_IP),
           (ehx.METRIC_COSINE, pyoracle.METRIC_COSINE)]


def _keys(n):
    return ["k%d" % i for i in range(n)]


def _drop_rule(oids, odist, ocnt, idx, k):
    """server.cc:205-207 over the oracle's (k + 1)-long lists -> [(ids, dist)] per query"""
    out = []
    for i, own in enumerate(idx):
        c = int(ocnt[i])
        ids, dist = list(oids[i, :c]), list(odist[i, :c])
        if ids:
            p = ids.index(own) if own in ids else len(ids) - 1
            del ids[p], dist[p]
        out.append((ids[:k], np.asarray(dist[:k], dtype=np.float32)))
    return out


def _expected_flat(X, idx, k, ometric):
    oids, odist, ocnt = pyoracle.exhaustive(X, X[idx], k + 1, ometric)
    return _drop_rule(oids, odist, ocnt, idx, k)


def _assert_rows(ids, dist, cnt, want, what):
    assert len(cnt) == len(want)
    for i, (wids, wdist) in enumerate(want):
        c = int(cnt[i])
        assert c == len(wids), "%s: query %d has %d results, the oracle %d" % (what, i, c, len(wids))
        assert list(ids[i, :c]) == wids, "%s: query %d ids differ" % (what, i)
        assert dist[i, :c].tobytes() == wdist.tobytes(), "%s: query %d distance bytes differ" % (what, i)


def _check(space, keys, idx, k, want, what="batch"):
    """the host form against `want`, and every row against ehx_knn_by_key of its key (a cross-check, not the reference)"""
    ids, dist, cnt = space.knn_by_keys([keys[i] for i in idx], k)
    assert ids.shape == (len(idx), k) and dist.shape == (len(idx), k)
    _assert_rows(ids, dist, cnt, want, what)
    single = {}
    for row, i in enumerate(idx):
        if i not in single:
            single[i] = space.knn_by_key(keys[i], k)
        sids, sdist = single[i]
        c = int(cnt[row])
        assert list(ids[row, :c]) == list(sids) and dist[row, :c].tobytes() == sdist.tobytes(), \
            "%s: row %d differs from knn_by_key(%r)" % (what, row, keys[i])
    return ids, dist, cnt


def _device_form(space, idx, k):
    import torch
    d_ids = torch.tensor(np.asarray(idx, dtype=np.int64), device="cuda")
    o_ids = torch.full((len(idx), k), -7, dtype=torch.int64, device="cuda")
    o_dist = torch.full((len(idx), k), -7.0, dtype=torch.float32, device="cuda")
    o_cnt = torch.full((len(idx),), 77, dtype=torch.int32, device="cuda")
    space.knn_by_ids_device(d_ids, k, o_ids, o_dist, o_cnt)
    torch.cuda.synchronize()
    return (o_ids.cpu().numpy().view(np.uint64), o_dist.cpu().numpy(), o_cnt.cpu().numpy().view(np.uint32))


# ---- flat spaces -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("em,om", METRICS)
def test_flat_int8_chain(em, om):
    """20 000 x 96 rows: the int8 filter answers first; 1024 keys with repeats, k = 10"""
    rng = np.random.default_rng(100 + em)
    n, d, k = 20_000, 96, 10
    X = rng.standard_normal((n, d)).astype(np.float32)
    keys = _keys(n)
    s = ehx.Space.unique("byk-i8", d, metric=em)
    s.set_batch(keys, X)
    assert s.scan_engine() == "i8"
    idx = [int(i) for i in rng.integers(0, n, size=900)]
    idx += idx[:100] + [0, n - 1] * 12                      # repeats
    assert len(idx) == 1024
    want = _expected_flat(X, idx, k, om)
    before = s.stats()["n_queries"]
    ids, dist, cnt = s.knn_by_keys([keys[i] for i in idx], k)
    st = s.stats()
    assert st["n_queries"] - before == 1024, "the batch must count its 1024 queries"
    assert st["n_uncertified"] == 0
    _assert_rows(ids, dist, cnt, want, "int8 chain")
    _check(s, keys, idx, k, want)
    dids, ddist, dcnt = _device_form(s, idx, k)
    _assert_rows(dids, ddist, dcnt, want, "device form")
    s.drop()


def test_flat_small_space_fp16_filter():
    rng = np.random.default_rng(7)
    n, d, k = 3000, 24, 20
    X = rng.standard_normal((n, d)).astype(np.float32)
    keys = _keys(n)
    for em, om in METRICS:
        s = ehx.Space.unique("byk-small", d, metric=em)
        s.set_batch(keys, X)
        assert s.scan_engine() == "f16"
        idx = [int(i) for i in rng.integers(0, n, size=200)] + [5, 5, 5]
        want = _expected_flat(X, idx, k, om)
        _check(s, keys, idx, k, want)
        _assert_rows(*_device_form(s, idx, k), want, "device form")
        s.drop()


@pytest.mark.parametrize("n,d", [(3000, 24), (20_000, 72), (700, 30)])
def test_f16_spaces(n, d):
    """EHX_DTYPE_F16: rows are stored rounded to binary16 and searched as stored (the gather widens them exactly)"""
    rng = np.random.default_rng(n)
    k = 10
    X = rng.standard_normal((n, d)).astype(np.float32)
    Xr = X.astype(np.float16).astype(np.float32)
    keys = _keys(n)
    for em, om in (METRICS[0], METRICS[2]):
        s = ehx.Space.unique("byk-f16", d, metric=em, dtype=ehx.DTYPE_F16)
        s.set_batch(keys, X)
        idx = [int(i) for i in rng.integers(0, n, size=150)]
        want = _expected_flat(Xr, idx, k, om)
        _check(s, keys, idx, k, want)
        _assert_rows(*_device_form(s, idx, k), want, "device form")
        s.drop()


@pytest.mark.parametrize("k", [48, 100])
def test_k_plus_one_crosses_into_the_paged_exhaustive_pass(k):
    rng = np.random.default_rng(k)
    n, d = 400, 20
    X = rng.standard_normal((n, d)).astype(np.float32)
    keys = _keys(n)
    for em, om in METRICS:
        s = ehx.Space.unique("byk-paged", d, metric=em)
        s.set_batch(keys, X)
        idx = [int(i) for i in rng.integers(0, n, size=40)] + [0, n - 1]
        want = _expected_flat(X, idx, k, om)
        _check(s, keys, idx, k, want)
        _assert_rows(*_device_form(s, idx, k), want, "device form")
        s.drop()


def test_duplicate_vectors_drop_the_last():
    """40 identical rows, queried by the key of the highest id: the row is not among the k + 1 = 6 results, so the last
    is dropped and the answer is the five lowest ids"""
    d, k = 12, 5
    X = np.tile(np.arange(1, d + 1, dtype=np.float32), (40, 1))
    keys = _keys(40)
    for em, om in METRICS:
        s = ehx.Space.unique("byk-dup", d, metric=em)
        s.set_batch(keys, X)
        want = _expected_flat(X, [39, 39, 0], k, om)
        assert want[0][0] == [0, 1, 2, 3, 4] and want[2][0] == [1, 2, 3, 4, 5]
        _check(s, keys, [39, 39, 0], k, want)
        _assert_rows(*_device_form(s, [39, 39, 0], k), want, "device form")
        assert s.knn_by_keys_keys([keys[39]], k) == [keys[:5]]
        s.drop()


def test_short_list():
    """3 rows, k = 20: the answer is the two other keys"""
    rng = np.random.default_rng(3)
    X = rng.standard_normal((3, 9)).astype(np.float32)
    keys = _keys(3)
    s = ehx.Space.unique("byk-short", 9)
    s.set_batch(keys, X)
    want = _expected_flat(X, [1, 0, 2, 1], 20, pyoracle.METRIC_L2)
    assert [len(w[0]) for w in want] == [2, 2, 2, 2]
    ids, dist, cnt = _check(s, keys, [1, 0, 2, 1], 20, want)
    assert sorted(ids[0, :2]) == [0, 2] and list(cnt) == [2, 2, 2, 2]
    assert (ids[:, 2:] == np.uint64(2**64 - 1)).all() and np.isinf(dist[:, 2:]).all()
    assert [sorted(r) for r in s.knn_by_keys_keys([keys[1], keys[0]], 20)] == [[keys[0], keys[2]], [keys[1], keys[2]]]
    _assert_rows(*_device_form(s, [1, 0, 2, 1], 20), want, "device form")
    s.drop()


# ---- graph spaces ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("em,om,d,dtype", [(ehx.METRIC_L2SQ, pyoracle.METRIC_L2, 32, "f32"),
                                           (ehx.METRIC_L2SQ, pyoracle.METRIC_L2, 21, "f32"),   # x_perm rows, dims % 16 != 0
                                           (ehx.METRIC_COSINE, pyoracle.METRIC_COSINE, 32, "f32"),
                                           (ehx.METRIC_COSINE, pyoracle.METRIC_COSINE, 27, "f32"),
                                           (ehx.METRIC_L2SQ, pyoracle.METRIC_L2, 24, "f16")])
def test_graph_mode(em, om, d, dtype):
    """build_batch = 1: the graph is the oracle's, so the strict walk's answers are its searchKnn's, at ef 10 and 64; the
    wide walk is held to the per-key path"""
    rng = np.random.default_rng(d)
    n, k = 2000, 10
    X = rng.standard_normal((n, d)).astype(np.float32)
    Xs = X.astype(np.float16).astype(np.float32) if dtype == "f16" else X
    keys = _keys(n)
    s = ehx.Space.unique("byk-graph", d, metric=em, mode=ehx.MODE_GRAPH, build_batch=1, initial_capacity=n,
                         dtype=ehx.DTYPE_F16 if dtype == "f16" else ehx.DTYPE_F32)
    s.set_batch(keys, X)
    h = pyoracle.Hnsw(d, om, n)
    for i in range(n):
        h.add(Xs[i], i)
    idx = [int(i) for i in rng.integers(0, n, size=300)] + [0, 0, n - 1]
    for i in (0, 1, n - 1):   # the gather returns Get's bytes
        assert s.get(keys[i]).tobytes() == Xs[i].tobytes()
    s.set_search_width(1)
    for ef in (10, 64):
        h.set_ef(ef)
        s.set_ef(ef)
        oids, odist, ocnt, _, _ = h.search_batch(Xs[idx], k + 1, threads=1)
        want = _drop_rule(oids, odist, ocnt, idx, k)
        before = s.stats()["n_queries"]
        _check(s, keys, idx, k, want, "graph ef=%d" % ef)
        _assert_rows(*_device_form(s, idx, k), want, "graph device form ef=%d" % ef)
        assert s.stats()["n_queries"] - before >= 2 * len(idx)
    s.set_ef(64)
    s.set_search_width(4)     # the wide walk: no oracle walks this order; every row must be the per-key path's
    ids, dist, cnt = s.knn_by_keys([keys[i] for i in idx], k)
    for row, i in enumerate(idx[:80]):
        sids, sdist = s.knn_by_key(keys[i], k)
        c = int(cnt[row])
        assert list(ids[row, :c]) == list(sids) and dist[row, :c].tobytes() == sdist.tobytes()
        assert i not in ids[row, :c]
    s.drop()


# ---- row-sharded spaces ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("em,om", METRICS)
def test_shards(em, om):
    import torch
    rng = np.random.default_rng(33)
    n, d, k = 9001, 40, 10
    X = rng.standard_normal((n, d)).astype(np.float32)
    keys = _keys(n)
    s = ehx.Space.unique("byk-shards", d, metric=em, shards=3)
    for i0 in range(0, n, 2500):
        s.set_batch(keys[i0:i0 + 2500], X[i0:i0 + 2500])
    idx = [int(i) for i in rng.integers(0, n, size=200)] + [0, 1, 2, n - 1, n - 2, n - 3, 1]
    want = _expected_flat(X, idx, k, om)          # the GLOBAL oracle
    before = s.stats()["n_queries"]
    _check(s, keys, idx, k, want, "3 shards")
    assert s.stats()["n_queries"] > before
    assert s.knn_by_keys_keys([keys[7]], 3) == [[keys[i] for i in _expected_flat(X, [7], 3, om)[0][0]]]
    with pytest.raises(ehx.EhxError) as e:        # the device form has no sharded variant
        t = torch.zeros(4, dtype=torch.int64, device="cuda")
        s.knn_by_ids_device(t, 2, torch.zeros((4, 2), dtype=torch.int64, device="cuda"),
                            torch.zeros((4, 2), dtype=torch.float32, device="cuda"),
                            torch.zeros(4, dtype=torch.int32, device="cuda"))
    assert e.value.code == _lib.EUNSUPPORTED
    s.drop()


# ---- the device form's own rules ---------------------------------------------------------------------------------------
def test_device_form_out_of_range_ids_give_count_zero():
    rng = np.random.default_rng(12)
    n, d, k = 5000, 48, 10
    X = rng.standard_normal((n, d)).astype(np.float32)
    s = ehx.Space.unique("byk-dev", d, metric=ehx.METRIC_COSINE)
    s.set_batch(_keys(n), X)
    idx = [3, n, 4, 2**40, n - 1, n + 1, 3]
    good = [r for r, i in enumerate(idx) if i < n]
    ids, dist, cnt = _device_form(s, idx, k)
    assert [int(c) for c in cnt] == [k if i < n else 0 for i in idx]
    want = _expected_flat(X, [idx[r] for r in good], k, pyoracle.METRIC_COSINE)
    _assert_rows(ids[good], dist[good], cnt[good], want, "neighbours of an out-of-range id")
    s.drop()


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_errors():
    rng = np.random.default_rng(2)
    n, d = 500, 16
    X = rng.standard_normal((n, d)).astype(np.float32)
    keys = _keys(n)
    s = ehx.Space.unique("byk-err", d)
    s.set_batch(keys, X)
    L = _lib.load()
    for p in (0, 3, 6):
        batch = [keys[i] for i in range(7)]
        batch[p] = "no such key"
        with pytest.raises(ehx.EhxError) as e:
            s.knn_by_keys(batch, 5)
        assert e.value.code == _lib.ENOTFOUND and e.value.bad_index == p
        with pytest.raises(ehx.EhxError) as e:
            s.knn_by_keys_keys(batch, 5)
        assert e.value.code == _lib.ENOTFOUND and e.value.bad_index == p
    # ... and the outputs stay unwritten
    m, arr, lens, keep = marshal_keys([keys[0], "nope"])
    ids = np.full((2, 5), 123, dtype=np.uint64)
    dist = np.full((2, 5), 4.5, dtype=np.float32)
    cnt = np.full(2, 9, dtype=np.uint32)
    bad = C.c_size_t(99)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    assert L.ehx_knn_by_keys(s._h, m, arr, lens, 5, P(ids, C.c_uint64), P(dist, C.c_float), P(cnt, C.c_uint32),
                             C.byref(bad)) == _lib.ENOTFOUND
    assert bad.value == 1 and (ids == 123).all() and (dist == 4.5).all() and (cnt == 9).all()
    assert L.ehx_knn_by_keys(s._h, m, arr, lens, 5, P(ids, C.c_uint64), P(dist, C.c_float), P(cnt, C.c_uint32),
                             None) == _lib.ENOTFOUND                      # bad_index may be NULL
    with pytest.raises(ehx.EhxError) as e:
        s.knn_by_keys(keys[:4], 1025)
    assert e.value.code == _lib.EUNSUPPORTED
    with pytest.raises(ehx.EhxError) as e:
        s.knn_by_keys_keys(keys[:4], 1025)
    assert e.value.code == _lib.EUNSUPPORTED
    # n == 0 and k == 0 as in ehx_knn
    ids0, dist0, cnt0 = s.knn_by_keys([], 5)
    assert ids0.shape == (0, 5) and cnt0.shape == (0,)
    ids0, dist0, cnt0 = s.knn_by_keys(keys[:3], 0)
    assert list(cnt0) == [0, 0, 0]
    assert s.knn_by_keys_keys(keys[:3], 0) == [[], [], []]
    # the _keys form: EHX_ERANGE on a 1-byte arena, then it succeeds once the arena has grown
    m, arr, lens, keep = marshal_keys(keys[:6])
    ids = np.zeros((6, 4), dtype=np.uint64)
    dist = np.zeros((6, 4), dtype=np.float32)
    cnt = np.zeros(6, dtype=np.uint32)
    off = np.zeros(6 * 4 + 1, dtype=np.uint64)
    arena = C.create_string_buffer(1)
    assert L.ehx_knn_by_keys_keys(s._h, m, arr, lens, 4, P(ids, C.c_uint64), P(dist, C.c_float), P(cnt, C.c_uint32), None,
                                  arena, 1, P(off, C.c_uint64)) == _lib.ERANGE
    arena = C.create_string_buffer(4096)
    assert L.ehx_knn_by_keys_keys(s._h, m, arr, lens, 4, P(ids, C.c_uint64), P(dist, C.c_float), P(cnt, C.c_uint32), None,
                                  arena, 4096, P(off, C.c_uint64)) == _lib.OK
    want = _expected_flat(X, list(range(6)), 4, pyoracle.METRIC_L2)
    got = [[arena.raw[int(off[i * 4 + j]):int(off[i * 4 + j + 1])].decode() for j in range(4)] for i in range(6)]
    assert got == [[keys[j] for j in w[0]] for w in want]
    assert s.knn_by_keys_keys(keys[:6], 4) == got
    # a frozen space is searched like any other; a dropped one answers "Not found"
    s.freeze()
    _check(s, keys, [1, 2, 3], 4, _expected_flat(X, [1, 2, 3], 4, pyoracle.METRIC_L2), "frozen")
    h = s._h
    s.drop()
    m, arr, lens, keep = marshal_keys(keys[:2])
    assert L.ehx_knn_by_keys(h, m, arr, lens, 4, P(ids, C.c_uint64), P(dist, C.c_float), P(cnt, C.c_uint32),
                             None) == _lib.ENOTFOUND
    assert L.ehx_knn_by_ids_device(h, None, 2, 8, 4, 8, 8, 8) == _lib.ENOTFOUND


# ---- the layers above the ABI --------------------------------------------------------------------------------------------
def test_offlinehub_nearest_neighbors():
    rng = np.random.default_rng(9)
    n, d = 300, 10
    X = rng.standard_normal((n, d)).astype(np.float32)
    ix = offlinehub.Index(((i, X[i]) for i in range(n)), d)          # integer keys, as the reference's own tests use
    idx = [5, 17, 5, 299]
    want = _expected_flat(X, idx, 7, pyoracle.METRIC_L2)
    got = ix.nearest_neighbors(7, idx)
    assert got == [[int(j) for j in w[0]] for w in want]
    assert got == [ix.nearest_neighbor(7, key=i) for i in idx]
    ix.close()
