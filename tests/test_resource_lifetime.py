"""GPU tests of what a space leaves behind: the owners of csrc/ehx_own.h count the device allocations, pinned allocations,
events and streams alive in the process (test hook ehx_test_live_resources, not part of the ABI).  Every case creates a
space, runs the paths that create its lazy resources — checking answers against the oracle, so that the paths really
ran — drops it, and expects the four counts back at what they were after ehx_init."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402


def _live():
    raw = C.CDLL(_lib.LIB_PATH)
    out = (C.c_uint64 * 4)()
    raw.ehx_test_live_resources(out)
    return list(out)


@pytest.fixture(scope="module")
def baseline():
    L = _lib.load()
    _lib.check(L.ehx_init(None, 0))
    return _live()   # [device allocations, pinned allocations, events, streams]


def _keys(n):
    return ["k%d" % i for i in range(n)]


def _exact(got, X, Q, k, om):
    ids, dist, cnt = got
    oids, odist, ocnt = pyoracle.exhaustive(X, Q, k, om)
    np.testing.assert_array_equal(cnt, ocnt)
    np.testing.assert_array_equal(ids, oids)
    assert dist.tobytes() == odist.tobytes()


def _by_keys_expected(X, rows, k, om):
    """server.cc:198-207 per key: search k + 1, erase the own row if it is there, else drop the last"""
    oids, odist, ocnt = pyoracle.exhaustive(X, X[rows], k + 1, om)
    out = []
    for i, r in enumerate(rows):
        l = [(int(a), b.tobytes()) for a, b in zip(oids[i, :ocnt[i]], odist[i, :ocnt[i]])]
        own = [j for j, (a, _) in enumerate(l) if a == r]
        if own:
            del l[own[0]]
        out.append(l[:k])
    return out


def _by_keys_check(s, X, rows, k, om):
    ids, dist, cnt = s.knn_by_keys(["k%d" % r for r in rows], k)
    for i, exp in enumerate(_by_keys_expected(X, rows, k, om)):
        assert int(cnt[i]) == len(exp)
        assert [(int(a), b.tobytes()) for a, b in zip(ids[i, :cnt[i]], dist[i, :cnt[i]])] == exp, "key %d" % i


def _drop_checked(s, baseline):
    L, h = _lib.load(), s._h
    s.drop()
    assert _live() == baseline, "device allocations, pinned allocations, events, streams alive after the drop"
    n = C.c_uint64()
    assert L.ehx_space_size(h, C.byref(n)) == _lib.ENOTFOUND   # (the tombstone answers for the dropped handle)


def test_flat_cosine_space_frees_everything(baseline):
    import torch
    rng = np.random.default_rng(11)
    n, d, k, om = 20_000, 128, 10, pyoracle.METRIC_COSINE
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((300, d)).astype(np.float32)
    s = ehx.Space.unique("life_flat", d, metric=ehx.METRIC_COSINE, initial_capacity=4096)
    s.set_batch(_keys(n)[:9000], X[:9000])         # 4096 -> 16384 ...
    s.set_batch(_keys(n)[9000:], X[9000:])         # ... -> 32768: fp32 rows, fp16 and int8 scan copies grow twice
    assert s.stats()["capacity"] >= n and s.scan_engine() == "i8"
    _exact(s.knn(Q[:1], k), X, Q[:1], k, om)       # one launch
    assert s.stats()["n_exhaustive"] == 1          # (ehx_stats counts the one-launch pass as an exhaustive one)
    _exact(s.knn(Q[:8], k), X, Q[:8], k, om)       # the small-call block
    _exact(s.knn(Q, k), X, Q, k, om)               # a host slot, the int8 scratch set
    assert s.stats()["n_i8_queries"] > 0
    dq = torch.from_numpy(Q[:64]).cuda()
    ids = torch.empty((64, k), dtype=torch.int64, device="cuda")
    dst = torch.empty((64, k), dtype=torch.float32, device="cuda")
    cnt = torch.empty((64,), dtype=torch.int32, device="cuda")
    s.knn_device(dq, k, ids, dst, cnt, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _exact((ids.cpu().numpy().astype(np.uint64), dst.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32)), X, Q[:64], k, om)
    _exact(s.knn(Q[:4], 100), X, Q[:4], 100, om)   # paged exhaustive
    _by_keys_check(s, X, [0, 77, 9000, n - 1], k, om)
    for scan in (ehx.SCAN_F16, ehx.SCAN_F32):
        s.set_scan(scan)
        _exact(s.knn(Q[:40], k), X, Q[:40], k, om)
    del dq, ids, dst, cnt
    _drop_checked(s, baseline)


def test_flat_l2_fp16_rows_space_frees_everything(baseline):
    rng = np.random.default_rng(12)
    n, d, k, om = 3000, 64, 10, pyoracle.METRIC_L2
    X = rng.standard_normal((n, d)).astype(np.float32)
    Xh = X.astype(np.float16).astype(np.float32)   # (rows are rounded to binary16 once, on Set)
    Q = rng.standard_normal((70, d)).astype(np.float32)
    s = ehx.Space.unique("life_f16", d, metric=ehx.METRIC_L2SQ, dtype=ehx.DTYPE_F16)
    s.set_batch(_keys(n), X)
    _exact(s.knn(Q[:3], k), Xh, Q[:3], k, om)      # a small call
    _exact(s.knn(Q, k), Xh, Q, k, om)              # a batch
    _drop_checked(s, baseline)


def test_graph_spaces_built_and_imported_free_everything(baseline):
    rng = np.random.default_rng(13)
    n, d, k, M, om = 2000, 32, 10, 8, pyoracle.METRIC_COSINE
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((64, d)).astype(np.float32)
    s = ehx.Space.unique("life_g", d, metric=ehx.METRIC_COSINE, mode=ehx.MODE_GRAPH, M=M)   # built on the GPU
    s.set_batch(_keys(n), X)
    exp = s.graph_export()
    h = pyoracle.Hnsw(d, om, n, M=M)
    h.import_graph(X, *exp)
    labels, dists, counts, _, _ = h.search_batch(Q, k, threads=1)   # the oracle's searchKnn on the engine's graph

    def same(got, sl):
        np.testing.assert_array_equal(got[2], counts[sl])
        np.testing.assert_array_equal(got[0], labels[sl])
        assert got[1].tobytes() == dists[sl].tobytes()
    same(s.knn(Q[:1], k), slice(0, 1))             # one launch
    same(s.knn(Q, k), slice(None))
    t = ehx.Space.unique("life_gi", d, metric=ehx.METRIC_COSINE, mode=ehx.MODE_GRAPH, M=M, initial_capacity=n,
                         build_batch=0xFFFFFFFF)   # no build: the graph is imported
    t.set_batch(_keys(n), X)
    t.graph_import(*exp)
    same(t.knn(Q, k), slice(None))
    L, hs = _lib.load(), s._h
    s.drop()
    _drop_checked(t, baseline)
    n_out = C.c_uint64()
    assert L.ehx_space_size(hs, C.byref(n_out)) == _lib.ENOTFOUND


def test_sharded_space_frees_everything(baseline):
    rng = np.random.default_rng(14)
    n, d, k, om = 6000, 64, 10, pyoracle.METRIC_L2
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((70, d)).astype(np.float32)
    s = ehx.Space.unique("life_sh", d, metric=ehx.METRIC_L2SQ, shards=2)   # (both on one device when one is visible)
    s.set_batch(_keys(n), X)
    _exact(s.knn(Q, k), X, Q, k, om)
    _by_keys_check(s, X, [5, 6, 3001, n - 1], k, om)
    _drop_checked(s, baseline)                     # the parent's drop takes its shards along
