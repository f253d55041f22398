"""GPU tests of the four routes of ehx_knn from host pointers (ehx_search.cpp: knn_host_direct) and of the sharded search's
packed results, at shapes on both sides of every boundary their layout arithmetic has.  Every answer must equal the
oracle's in ids and in distance BYTES.

The routes, by the constants of ehx_search.cpp (kSmallCall = 32 768 bytes, for the queries and for the packed results each;
a result block is nq * k * (8 + 4) + nq * 4 bytes, ResultBlock::bytes):
  d = 64, k = 10:  nq = 128 -> queries 128 * 64 * 4 = 32 768 B, results 15 872 B: the small call
                   nq = 129 -> queries 33 024 B:                                   a slot (on the large space: pipelined int8 stage)
  d = 64, k = 48:  nq = 56  -> results 56 * 48 * 12 + 56 * 4 = 32 480 B:           the small call
                   nq = 57  -> results 57 * 48 * 12 = 32 832 B of lists alone (33 060 B with the counts): a slot
  nq = 5, k = 3:   15 distances = 60 B: the counts start off an 8-byte boundary
  sharded, nq = 1, k = 3: one shard's pack is 3 * 12 + 4 = 40 B, rounded up to 48
test_route_arithmetic checks these figures on the CPU."""
import ctypes as C
import threading

import numpy as np
import pytest

from oracle import pyoracle

K_SMALL_CALL = 32 << 10     # ehx_search.cpp: kSmallCall
D = 64
KMAX = 48                   # the references are computed once at k = 48: a shorter list is its prefix ((distance, id) order)


def _qbytes(nq):
    return nq * D * 4


def _out_bytes(nq, k):      # ResultBlock::bytes(nq, k, false)
    return nq * k * (8 + 4) + nq * 4


def _is_small(nq, k):       # knn_host_direct's condition
    return _qbytes(nq) <= K_SMALL_CALL and _out_bytes(nq, k) <= K_SMALL_CALL


def test_route_arithmetic():
    assert _qbytes(128) == 32768 and _out_bytes(128, 10) == 15872 and _is_small(128, 10)
    assert _qbytes(129) == 33024 and not _is_small(129, 10)
    assert _out_bytes(56, 48) == 32480 and _qbytes(56) < K_SMALL_CALL and _is_small(56, 48)
    assert 57 * 48 * 12 == 32832 and _out_bytes(57, 48) == 33060 and _qbytes(57) < K_SMALL_CALL and not _is_small(57, 48)
    assert (5 * 3 * 8 + 5 * 3 * 4) % 8 == 4 and _is_small(5, 3)
    assert _out_bytes(1, 3) == 40 and -(-40 // 16) * 16 == 48
    assert _is_small(1, 64) and _is_small(1, 65)


gpu = pytest.mark.gpu
ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402


def _one_launch_count(s):
    f = C.CDLL(_lib.LIB_PATH).ehx_test_one_launch_count
    f.restype = C.c_uint64
    return int(f(s._h))


def _same(got, ref, nq, k, what):
    ids, dist, cnt = got
    oids, odist = ref
    assert (np.asarray(cnt) == k).all(), "%s: counts %s" % (what, cnt)
    assert np.array_equal(ids, oids[:nq, :k]), "%s: ids differ from the oracle" % what
    assert np.ascontiguousarray(dist).tobytes() == np.ascontiguousarray(odist[:nq, :k]).tobytes(), \
        "%s: distance bytes differ from the oracle" % what


@pytest.fixture(scope="module")
def large():
    """20 000 x 64 fp32, L2: the int8 filter scan answers first; queries [129], the oracle's 48 nearest of each"""
    rng = np.random.default_rng(2024)
    X = rng.standard_normal((20000, D)).astype(np.float32)
    Q = rng.standard_normal((129, D)).astype(np.float32)
    s = ehx.Space.unique("routes-l2", D, metric=ehx.METRIC_L2SQ, initial_capacity=X.shape[0])
    s.set_batch(["k%d" % i for i in range(X.shape[0])], X)
    assert s.scan_engine() == "i8"
    oids, odist, ocnt = pyoracle.exhaustive(X, Q, KMAX, pyoracle.METRIC_L2)
    assert (ocnt == KMAX).all()
    yield s, Q, (oids, odist)
    s.drop()


@pytest.fixture(scope="module")
def small():
    """2 000 x 64 cosine, below i8_min_rows: the fp16 filter answers first"""
    rng = np.random.default_rng(2025)
    X = rng.standard_normal((2000, D)).astype(np.float32)
    Q = rng.standard_normal((129, D)).astype(np.float32)
    s = ehx.Space.unique("routes-cos", D, metric=ehx.METRIC_COSINE, initial_capacity=X.shape[0])
    s.set_batch(["k%d" % i for i in range(X.shape[0])], X)
    assert s.scan_engine() == "f16"
    oids, odist, ocnt = pyoracle.exhaustive(X, Q, KMAX, pyoracle.METRIC_COSINE)
    assert (ocnt == KMAX).all()
    yield s, Q, (oids, odist)
    s.drop()


# (nq, k): on either side of the boundary by query bytes, of the boundary by result bytes, and an odd nq * k
SHAPES = [(128, 10), (129, 10), (56, 48), (57, 48), (5, 3)]


@gpu
@pytest.mark.parametrize("nq,k", SHAPES)
def test_small_call_and_slot_on_the_int8_space(large, nq, k):
    s, Q, ref = large
    before = s.stats()["n_i8_queries"]
    _same(s.knn(Q[:nq], k), ref, nq, k, "nq %d k %d" % (nq, k))
    assert s.stats()["n_i8_queries"] == before + nq      # (small call or slot: the int8 stage answered first)


@gpu
@pytest.mark.parametrize("nq,k", SHAPES)
def test_small_call_and_slot_on_the_fp16_space(small, nq, k):
    s, Q, ref = small
    _same(s.knn(Q[:nq], k), ref, nq, k, "nq %d k %d" % (nq, k))
    assert s.stats()["n_i8_queries"] == 0                # (a slot batch here runs the whole chain under the pipeline lock)


@gpu
def test_two_callers_on_the_slot_route(large):
    s, Q, ref = large
    got, errs = {}, []

    def caller(t):
        try:
            for b in range(4):
                got[t, b] = s.knn(Q, 10)
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=caller, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
        assert not t.is_alive()
    assert not errs, errs
    assert len(got) == 8
    for key, g in got.items():
        _same(g, ref, 129, 10, "caller %d batch %d" % key)


@gpu
def test_one_launch_flat_and_its_k_limit():
    rng = np.random.default_rng(7)
    X = rng.standard_normal((300, D)).astype(np.float32)
    q = rng.standard_normal((1, D)).astype(np.float32)
    s = ehx.Space.unique("routes-one", D, metric=ehx.METRIC_L2SQ, initial_capacity=300)
    s.set_batch(["k%d" % i for i in range(300)], X)
    oids, odist, _ = pyoracle.exhaustive(X, q, 65, pyoracle.METRIC_L2)
    for k in (1, 10, 64):
        before = _one_launch_count(s)
        _same(s.knn(q, k), (oids, odist), 1, k, "one launch, k %d" % k)
        assert _one_launch_count(s) == before + 1, k
    before = _one_launch_count(s)
    _same(s.knn(q, 65), (oids, odist), 1, 65, "k 65: the small call into the paged pass")
    assert _one_launch_count(s) == before
    s.drop()


@gpu
def test_one_launch_graph():
    """one query on a graph space against the oracle's searchKnn on the graph the GPU built, as
    tests/test_graph_gpu_built_parity.py"""
    M, ef, k = 16, 40, 10
    rng = np.random.default_rng(8)
    X = rng.standard_normal((2000, D)).astype(np.float32)
    q = rng.standard_normal((1, D)).astype(np.float32)
    s = ehx.Space.unique("routes-graph", D, metric=ehx.METRIC_L2SQ, mode=ehx.MODE_GRAPH, M=M, ef=ef, initial_capacity=2000)
    s.set_batch(["k%d" % i for i in range(2000)], X)
    l0, lv, upper, ep, ml = s.graph_export()
    h = pyoracle.Hnsw(D, pyoracle.METRIC_L2, 2000, M=M)
    h.import_graph(X, l0, lv, upper, ep, ml, threads=4)
    h.set_ef(ef)
    labels, dists, counts = h.search_batch(q, k, threads=1)[:3]
    before = _one_launch_count(s)
    ids, dist, cnt = s.knn(q, k)
    assert _one_launch_count(s) == before + 1
    assert int(cnt[0]) == int(counts[0]) == k
    assert np.array_equal(ids, labels.astype(np.uint64).reshape(1, k))
    assert np.ascontiguousarray(dist).tobytes() == np.ascontiguousarray(dists).tobytes()
    del h
    s.drop()


@gpu
def test_sharded_packs(large):
    """shards = 3 in one process: the shards' packed results, the gather buffer's slots and the parent's merged block"""
    import torch
    _, Q, _ = large
    rng = np.random.default_rng(9)
    n = 3000
    X = rng.standard_normal((n, D)).astype(np.float32)
    s = ehx.Space.unique("routes-sh", D, metric=ehx.METRIC_L2SQ, shards=3)
    s.set_batch(["k%d" % i for i in range(n)], X)
    oids, odist, _ = pyoracle.exhaustive(X, Q[:7], 5, pyoracle.METRIC_L2)
    _same(s.knn(Q[:1], 3), (oids, odist), 1, 3, "sharded, nq 1 k 3")
    _same(s.knn(Q[:7], 5), (oids, odist), 7, 5, "sharded, nq 7 k 5, host pointers")
    dq = torch.from_numpy(Q[:7]).cuda()
    ids = torch.empty((7, 5), dtype=torch.int64, device="cuda")
    dst = torch.empty((7, 5), dtype=torch.float32, device="cuda")
    cnt = torch.empty((7,), dtype=torch.int32, device="cuda")
    s.knn_device(dq, 5, ids, dst, cnt, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _same((ids.cpu().numpy().astype(np.uint64), dst.cpu().numpy(), cnt.cpu().numpy()), (oids, odist), 7, 5,
          "sharded, nq 7 k 5, ehx_knn_device")
    # the neighbours of three stored rows: the oracle's k + 1 nearest of each row without the row itself
    rows = [5, 1234, 2999]
    bids, bdist, _ = pyoracle.exhaustive(X, X[rows], 5, pyoracle.METRIC_L2)
    want_ids = np.stack([bids[i][bids[i] != r][:4] for i, r in enumerate(rows)])
    want_dist = np.stack([bdist[i][bids[i] != r][:4] for i, r in enumerate(rows)])
    assert all((bids[i] == r).sum() == 1 for i, r in enumerate(rows))
    _same(s.knn_by_keys(["k%d" % r for r in rows], 4), (want_ids, want_dist), 3, 4, "sharded, knn_by_keys n 3 k 4")
    s.drop()
