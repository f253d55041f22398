"""Rows in and out without staging: Space.set_batch_device (ehx_set_batch_device: the rows of a Set read from device memory
by scatter_rows_kernel), Space.get_batch and Space.get_by_ids_device.

The yardstick of a write is a TWIN: a space of the same parameters given the same keys and values through the unchanged
ehx_set_batch.  The two must agree on get_by_id of every row (as uint32; where both hold a NaN, "both NaN" is all that is
asked — the inputs hold exactly the NaNs of CASE_VALUES), and on knn ids, distance bytes and counts of 16 queries at k = 10;
the twin of a flat space is itself compared with the oracle, as the parity tests do.  Every first row of a chunk carries
CASE_VALUES: ties of the binary16 rounding in both directions, the last finite binary16 value and the overflow to +-Inf, the
binary16 subnormal range and its rounding to zero, -0.0, an fp32 subnormal, one NaN and one Inf."""
import ctypes as C
import os
import sys
import threading
import uuid

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import pyoracle  # noqa: E402
from prefix_oracle import PrefixOracle  # noqa: E402
import range_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
torch = pytest.importorskip("torch")
_lib = ehx._lib

f32 = np.float32
CASE_VALUES = np.array([1 + 2.0**-11, 1 + 3 * 2.0**-11, 65519.996, 65520.0, -65520.0, 6.0e-8, 2.9e-8, 3.0e-8, -0.0, 1e-40,
                        np.nan, np.inf], dtype=f32)
KINDS = {   # space kind -> (Space keywords, the oracle's metric)
    "f32-l2": (dict(metric=ehx.METRIC_L2SQ), pyoracle.METRIC_L2),
    "f16-cos": (dict(metric=ehx.METRIC_COSINE, dtype=ehx.DTYPE_F16), pyoracle.METRIC_COSINE),
    "f32-ip": (dict(metric=ehx.METRIC_IP), pyoracle.METRIC_IP),
}
SRC = {"f32": torch.float32, "f16": torch.float16}


def _keys(n, prefix="k"):
    return ["%s%d" % (prefix, i) for i in range(n)]


def _values(n, dims, seed, chunk_starts):
    X = np.random.default_rng(seed).standard_normal((n, dims)).astype(f32)
    m = min(dims, len(CASE_VALUES))
    for r0 in chunk_starts:
        X[r0, :m] = CASE_VALUES[:m]
    return X


def _source(X, src):
    """the values as the device source holds them (a torch CUDA tensor of dtype `src`) and as fp32 for the twin"""
    with np.errstate(over="ignore"):
        t = torch.from_numpy(X).cuda().to(SRC[src])
    return t, t.float().cpu().numpy()


def _stored(Xw, kw):
    """what a space of these keywords holds for the fp32 values Xw (F16 spaces: rounded to nearest-even binary16)"""
    if kw.get("dtype") == ehx.DTYPE_F16:
        with np.errstate(over="ignore"):
            return Xw.astype(np.float16).astype(f32)
    return Xw


def _rows(s):
    return np.stack([s.get_by_id(i) for i in range(len(s))])


def _assert_same_rows(s, t, expect=None):
    a, b = _rows(s), _rows(t)
    assert a.shape == b.shape
    nan = np.isnan(a) & np.isnan(b)
    assert np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]), "stored rows differ from the twin's"
    if expect is not None:   # exactly the NaNs of the input, and the input's bytes elsewhere
        assert np.array_equal(nan, np.isnan(expect))
        assert np.array_equal(a.view(np.uint32)[~nan], expect.view(np.uint32)[~nan]), "stored rows differ from the input"


def _assert_same_knn(s, t, Q, k=10):
    ids, dist, cnt = s.knn(Q, k)
    tids, tdist, tcnt = t.knn(Q, k)
    assert cnt.tolist() == tcnt.tolist()
    keep = np.arange(k)[None, :] < cnt[:, None]
    assert np.array_equal(ids[keep], tids[keep])
    assert dist[keep].tobytes() == tdist[keep].tobytes()
    return tids, tdist, tcnt


def _assert_oracle(ans, X, Q, k, om):
    ids, dist, cnt = ans
    oids, odist, ocnt = pyoracle.exhaustive(X, Q, k, om)
    assert cnt.tolist() == ocnt.tolist()
    for i in range(Q.shape[0]):
        c = int(cnt[i])
        assert ids[i, :c].tolist() == oids[i, :c].tolist(), "query %d ids differ from the oracle's" % i
        assert dist[i, :c].tobytes() == odist[i, :c].tobytes(), "query %d distances differ from the oracle's" % i


def _queries(dims, seed=77):
    return np.random.default_rng(seed).standard_normal((16, dims)).astype(f32)


# ---- shapes x space kinds x source dtypes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("src", sorted(SRC))
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("dims", [1, 3, 8, 20, 100, 136])
def test_device_set_equals_the_host_set(dims, kind, src):
    """700 rows as chunks of 300 and 400 (the second append straddles a 256-row tile)"""
    kw, om = KINDS[kind]
    n, chunks = 700, [(0, 300), (300, 700)]
    t_src, Xw = _source(_values(n, dims, 1000 + dims, [a for a, _ in chunks]), src)
    keys = _keys(n)
    s, t = ehx.Space.unique("rio", dims, **kw), ehx.Space.unique("rio-twin", dims, **kw)
    for a, b in chunks:
        s.set_batch_device(keys[a:b], t_src[a:b])
        t.set_batch(keys[a:b], Xw[a:b])
    assert len(s) == len(t) == n
    X = _stored(Xw, kw)
    _assert_same_rows(s, t, X)
    Q = _queries(dims)
    _assert_oracle(_assert_same_knn(s, t, Q), X, Q, 10, om)
    s.drop()
    t.drop()


@pytest.mark.parametrize("src", sorted(SRC))
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("dims", [8, 136])
def test_a_source_that_is_only_element_aligned(dims, kind, src):
    """the rows start one element into an allocation: a view of a larger tensor"""
    kw, om = KINDS[kind]
    n = 300
    t_src, Xw = _source(_values(n, dims, 2000 + dims, [0]), src)
    flat = torch.zeros(n * dims + 9, dtype=SRC[src], device="cuda")
    flat[1:1 + n * dims] = t_src.reshape(-1)
    view = flat[1:1 + n * dims].view(n, dims)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    s, t = ehx.Space.unique("rio-un", dims, **kw), ehx.Space.unique("rio-un-twin", dims, **kw)
    s.set_batch_device(_keys(n), view)
    t.set_batch(_keys(n), Xw)
    X = _stored(Xw, kw)
    _assert_same_rows(s, t, X)
    Q = _queries(dims)
    _assert_oracle(_assert_same_knn(s, t, Q), X, Q, 10, om)
    s.drop()
    t.drop()


# ---- rewrites -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", sorted(SRC))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_batch_that_rewrites_keys_keeps_the_last_row_of_a_repeated_key(kind, src):
    """64 known keys, 64 fresh keys and one key given three times with three different rows, in one batch (the exclusive path)"""
    kw, om = KINDS[kind]
    dims, n0 = 20, 200
    rng = np.random.default_rng(5)
    t0, X0 = _source(_values(n0, dims, 31, [0]), src)
    keys0 = _keys(n0)
    known = [keys0[i] for i in rng.choice(n0, 64, replace=False)]
    batch = known + _keys(64, "fresh") + ["thrice"] * 3
    order = rng.permutation(len(batch))
    batch = [batch[i] for i in order]
    t1, X1 = _source(_values(len(batch), dims, 32, [0]), src)
    s, t = ehx.Space.unique("rio-rw", dims, **kw), ehx.Space.unique("rio-rw-twin", dims, **kw)
    s.set_batch_device(keys0, t0)
    t.set_batch(keys0, X0)
    s.set_batch_device(batch, t1)
    t.set_batch(batch, X1)
    assert len(s) == len(t) == n0 + 65
    _assert_same_rows(s, t)
    last = max(i for i, k in enumerate(batch) if k == "thrice")
    want = _stored(X1[last:last + 1], kw)[0]
    got = s.get("thrice")
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "the third row is the one stored"
    Q = _queries(dims)
    _assert_oracle(_assert_same_knn(s, t, Q), _rows(t), Q, 10, om)
    s.drop()
    t.drop()


# ---- the int8 engine: scan copies and tile ordering made from scattered rows -------------------------------------------------
def test_int8_engine_on_rows_written_from_the_device():
    X, Q = rc.i8_data(128)
    n = X.shape[0]
    keys = _keys(n)
    kw = dict(metric=ehx.METRIC_COSINE)
    s, t = ehx.Space.unique("rio-i8", 128, **kw), ehx.Space.unique("rio-i8-twin", 128, **kw)
    d = torch.from_numpy(X.copy()).cuda()
    cuts = [0, 7000, 13001, n]
    for a, b in zip(cuts, cuts[1:]):
        s.set_batch_device(keys[a:b], d[a:b])
        t.set_batch(keys[a:b], X[a:b])
    assert s.scan_engine() == "i8" and t.scan_engine() == "i8"
    i8_0 = s.stats()["n_i8_queries"]
    tids, tdist, tcnt = _assert_same_knn(s, t, Q)
    assert s.stats()["n_i8_queries"] > i8_0, "the int8 engine did not run"
    oids, odist = rc.i8_oracle(128, "cosine")
    assert (tcnt == 10).all() and np.array_equal(tids, oids[:, :10]) and tdist.tobytes() == odist[:, :10].tobytes()
    probe = np.random.default_rng(1).choice(n, 64, replace=False)
    for i in probe:
        assert np.array_equal(s.get_by_id(i).view(np.uint32), X[i].view(np.uint32))
    s.drop()
    t.drop()


# ---- graph spaces -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [ehx.DTYPE_F32, ehx.DTYPE_F16])   # the single-copy layout, and the two-copy one
def test_graph_built_from_device_rows_equals_the_twins(dtype):
    n, dims = 2000, 16
    kw = dict(metric=ehx.METRIC_L2SQ, mode=ehx.MODE_GRAPH, M=8, ef_construction=40, seed=7, dtype=dtype)
    X = np.random.default_rng(9).standard_normal((n, dims)).astype(f32)
    d = torch.from_numpy(X).cuda()
    keys = _keys(n)
    s, t = ehx.Space.unique("rio-g", dims, **kw), ehx.Space.unique("rio-g-twin", dims, **kw)
    for a in range(0, n, 256):
        s.set_batch_device(keys[a:a + 256], d[a:a + 256])
        t.set_batch(keys[a:a + 256], X[a:a + 256])
    again = np.random.default_rng(10).choice(n, 50, replace=False)
    X2 = np.random.default_rng(11).standard_normal((50, dims)).astype(f32)
    s.set_batch_device([keys[i] for i in again], torch.from_numpy(X2).cuda())
    t.set_batch([keys[i] for i in again], X2)
    _assert_same_rows(s, t)
    gs, gt = s.graph_export(), t.graph_export()
    assert np.array_equal(gs[0], gt[0]) and np.array_equal(gs[1], gt[1]) and gs[3:] == gt[3:]
    assert sorted(gs[2]) == sorted(gt[2]) and all(np.array_equal(gs[2][k], gt[2][k]) for k in gs[2])
    _assert_same_knn(s, t, _queries(dims))
    s.drop()
    t.drop()


# ---- row-sharded spaces -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", sorted(SRC))
def test_sharded_parent_written_from_the_device(src):
    dims, n = 20, 900
    kw = dict(metric=ehx.METRIC_L2SQ, shards=3)
    t_src, Xw = _source(_values(n, dims, 41, [0, 500]), src)
    keys = _keys(n)
    s, t = ehx.Space.unique("rio-sh", dims, **kw), ehx.Space.unique("rio-sh-twin", dims, **kw)
    for a, b in ((0, 500), (500, 900)):
        s.set_batch_device(keys[a:b], t_src[a:b])
        t.set_batch(keys[a:b], Xw[a:b])
    rng = np.random.default_rng(42)
    batch = [keys[i] for i in rng.choice(n, 70, replace=False)] + _keys(50, "new") + ["twice", keys[3], "twice", keys[3]]
    batch = [batch[i] for i in rng.permutation(len(batch))]
    t1, X1 = _source(_values(len(batch), dims, 43, [0]), src)
    s.set_batch_device(batch, t1)
    t.set_batch(batch, X1)
    assert len(s) == len(t) == n + 51
    _assert_same_rows(s, t)
    last = max(i for i, k in enumerate(batch) if k == "twice")
    assert np.array_equal(s.get("twice").view(np.uint32), X1[last].view(np.uint32))
    Q = _queries(dims)
    _assert_oracle(_assert_same_knn(s, t, Q), _rows(t), Q, 10, pyoracle.METRIC_L2)
    s.drop()
    t.drop()


# ---- the producer's stream --------------------------------------------------------------------------------------------------
def test_rows_produced_on_a_side_stream_are_complete_when_they_are_read():
    n, dims = 4096, 136
    s = ehx.Space.unique("rio-st", dims, metric=ehx.METRIC_COSINE)
    side = torch.cuda.Stream()
    a = torch.randn((2048, 2048), device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        t = torch.zeros((n, dims), device="cuda")
        for _ in range(12):               # (work in front of the fill: the Set is enqueued while the producer still runs)
            a = torch.tanh(a @ a)
        t += a[:, :dims].repeat(2, 1) + torch.arange(n, device="cuda", dtype=torch.float32)[:, None]
    s.set_batch_device(_keys(n), t, stream=side.cuda_stream)
    side.synchronize()
    want = t.cpu().numpy()
    assert not (want == 0).all(axis=1).any()
    assert np.array_equal(s.get_batch(_keys(n)).view(np.uint32), want.view(np.uint32))
    s.drop()


# ---- errors -----------------------------------------------------------------------------------------------------------------
def _raw_set(h, keys, ptr, dtype=0, stream=None):
    n, arr, lens, keep = ehx.space.marshal_keys(keys)
    rc_ = _lib.load().ehx_set_batch_device(h, stream, n, arr, lens, C.c_void_p(ptr), dtype)
    del keep
    return rc_


def test_errors_leave_the_space_as_it_was():
    lib = _lib.load()
    dims, n = 8, 40
    X = np.random.default_rng(3).standard_normal((n, dims)).astype(f32)
    d = torch.from_numpy(X).cuda()
    s = ehx.Space.unique("rio-err", dims)
    s.set_batch_device(_keys(n), d)
    before = _rows(s)

    def unchanged():
        assert len(s) == n and np.array_equal(_rows(s).view(np.uint32), before.view(np.uint32))
    other = np.ones((2, dims), dtype=f32)
    d_other = torch.from_numpy(other).cuda()
    assert _raw_set(s._h, ["k0", "zz"], other.ctypes.data) == _lib.EINVAL     # a host pointer
    assert b"device memory" in lib.ehx_last_error()
    unchanged()
    assert _raw_set(s._h, ["k0", "zz"], d_other.data_ptr(), dtype=7) == _lib.EINVAL   # a bad src_dtype
    unchanged()
    assert _raw_set(s._h, ["k0", "zz"], 0) == _lib.EINVAL                       # NULL rows
    unchanged()
    s.freeze()
    with pytest.raises(ehx.EhxError) as e:
        s.set_batch_device(["k0", "zz"], d_other)
    assert e.value.code == _lib.EIMMUTABLE and "Cannot write to immutable space" in str(e.value)
    unchanged()
    h = s._h
    s.drop()
    assert _raw_set(h, ["k0", "zz"], d_other.data_ptr()) == _lib.ENOTFOUND      # a dropped handle
    # a shard's handle: written through its parent
    p = ehx.Space.unique("rio-err-sh", dims, shards=3)
    p.set_batch_device(_keys(n), d)
    rows = _rows(p)
    shard = lib.ehx_test_shard
    shard.restype, shard.argtypes = C.c_void_p, [C.c_void_p, C.c_uint32]
    hs = shard(p._h, 1)
    assert hs
    assert _raw_set(C.c_void_p(hs), ["k0", "zz"], d_other.data_ptr()) == _lib.EINVAL
    assert lib.ehx_last_error() == b"a shard is written through its parent space"
    assert len(p) == n and np.array_equal(_rows(p).view(np.uint32), rows.view(np.uint32))
    p.drop()


# ---- appends beside a search -------------------------------------------------------------------------------------------------
def test_device_appends_beside_a_search_answer_for_a_published_prefix():
    dims, m, n_chunks = 32, 512, 16
    X = np.random.default_rng(21).standard_normal(((n_chunks + 1) * m, dims)).astype(f32)
    Q = _queries(dims, 22)
    d = torch.from_numpy(X).cuda()
    keys = _keys(len(X))
    s = ehx.Space.unique("rio-app", dims, metric=ehx.METRIC_L2SQ)
    s.set_batch_device(keys[:m], d[:m])
    errs, records = [], []

    def writer():
        try:
            for j in range(1, n_chunks + 1):
                s.set_batch_device(keys[j * m:(j + 1) * m], d[j * m:(j + 1) * m])
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))
    w = threading.Thread(target=writer)
    w.start()
    while True:
        alive = w.is_alive()
        lo = len(s)
        ans = s.knn(Q, 10)
        hi = len(s)
        records.append((lo, ans, hi))
        if not alive:
            break
    w.join()
    assert not errs, errs
    assert len(s) == len(X)
    oracle = PrefixOracle(X, Q, 10, pyoracle.METRIC_L2, [m * (j + 1) for j in range(n_chunks + 1)])
    for lo, ans, hi in records:
        oracle.assert_is_some_prefix(*ans, lo, hi)
    assert records[-1][0] == len(X)
    s.drop()


# ---- Gets -------------------------------------------------------------------------------------------------------------------
GET_KINDS = {
    "f32": dict(metric=ehx.METRIC_L2SQ),
    "f16": dict(metric=ehx.METRIC_COSINE, dtype=ehx.DTYPE_F16),
    "graph-single-copy": dict(metric=ehx.METRIC_L2SQ, mode=ehx.MODE_GRAPH, M=8, ef_construction=40),
    "shards": dict(metric=ehx.METRIC_L2SQ, shards=3),
}


@pytest.mark.parametrize("kind", sorted(GET_KINDS))
def test_gets(kind):
    lib = _lib.load()
    dims, n = 20, 400
    kw = GET_KINDS[kind]
    X = _values(n, dims, 51, [] if "graph" in kind else [0, 256])   # (no NaN in a graph: its build walks distances)
    keys = _keys(n)
    s = ehx.Space.unique("rio-get", dims, **kw)
    s.set_batch(keys, X)
    rng = np.random.default_rng(52)
    pick = rng.integers(0, n, 1000)
    assert len(set(pick.tolist())) < 1000
    loop = np.stack([s.get(keys[i]) for i in range(n)])
    got = s.get_batch([keys[i] for i in pick])
    assert got.dtype == np.float32 and got.shape == (1000, dims)
    assert np.array_equal(got.view(np.uint32), loop[pick].view(np.uint32)), "get_batch differs from the loop of get"
    # an unknown key in position 7: ENOTFOUND, its index, the output untouched
    ask = [keys[i] for i in pick[:20]]
    ask[7] = "no-such-key"
    with pytest.raises(ehx.EhxError) as e:
        s.get_batch(ask)
    assert e.value.code == _lib.ENOTFOUND and e.value.bad_index == 7
    nk, arr, lens, keep = ehx.space.marshal_keys(ask)
    out = np.full((20, dims), 123.25, dtype=f32)
    bad = C.c_size_t(99)
    assert lib.ehx_get_batch(s._h, nk, arr, lens, out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(bad)) == _lib.ENOTFOUND
    assert bad.value == 7 and (out == f32(123.25)).all()
    # by row ids on the device: one id at the row count, one far beyond it
    ids = pick[:300].astype(np.int64)
    ids[11], ids[200] = n, 2**40
    d_ids = torch.from_numpy(ids).cuda()
    d_out = torch.full((300, dims), 7.0, device="cuda")
    d_valid = torch.full((300,), 5, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    s.get_by_ids_device(d_ids, d_out, d_valid, stream=st.cuda_stream)
    st.synchronize()
    o, v = d_out.cpu().numpy(), d_valid.cpu().numpy()
    want_valid = np.ones(300, dtype=np.int32)
    want_valid[[11, 200]] = 0
    assert v.tolist() == want_valid.tolist()
    assert (o[[11, 200]].view(np.uint32) == 0).all()
    ok = want_valid == 1
    by_id = np.stack([s.get_by_id(int(i)) for i in ids[ok]])
    assert np.array_equal(o[ok].view(np.uint32), by_id.view(np.uint32))
    # n == 0: nothing is asked of any pointer
    assert lib.ehx_set_batch_device(s._h, None, 0, None, None, None, 0) == _lib.OK
    assert lib.ehx_get_batch(s._h, 0, None, None, None, None) == _lib.OK
    assert lib.ehx_get_by_ids_device(s._h, None, 0, None, None, None) == _lib.OK
    assert s.get_batch([]).shape == (0, dims)
    s.drop()


# ---- Download through the gRPC shim --------------------------------------------------------------------------------------------
def test_download_streams_what_the_per_key_loop_yields():
    from embeddinghub_amd.rpc import server as srv
    from embeddinghub_amd.rpc.client import EmbeddingHubClient
    store = srv.EngineStore()
    server, port = srv.make_server(store, "127.0.0.1:0", max_workers=8)
    server.start()
    client = EmbeddingHubClient(host="127.0.0.1", port=port)
    try:
        name, dims, n = "rio-dl-%s" % uuid.uuid4(), 16, 3000
        client.create_space(name, dims)
        sp = store.get_space(name)
        X = np.random.default_rng(61).standard_normal((n, dims)).astype(f32)
        sp.set_batch(["key-%d" % i for i in np.random.default_rng(62).permutation(n)], X)
        assert callable(getattr(sp, "get_many", None))
        want = [(k, sp.get(k).tolist()) for k in sp.keys_sorted()]
        got = [(k, list(v)) for k, v in client.download(name)]
        assert len(got) == n and got == want
        store.delete_space(name)
    finally:
        client.close()
        server.stop(0)
