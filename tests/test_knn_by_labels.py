"""GPU tests of the multi-probe label search (Space.knn_by_labels*, k_probe.hip): kNN under a per-query SET of stored labels.

Truth: for query i, pyoracle.exhaustive over the rows whose stored label is in the query's set (a repeat counts once, an
absent label adds nothing), ids mapped back — ids equal, distance BYTES equal, counts equal, the sentinels behind the count.
F16 spaces: the oracle on the rounded rows, as tests/test_exact_one_walk.py.  The label sizes sit on the kernel's edges:
no row, 1, 8 and 9 rows (one staging step, then one more), 63 / 64 / 65 (one batch of 64 keys), about 700."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402

METRICS = {"l2": (ehx.METRIC_L2SQ, pyoracle.METRIC_L2), "ip": (ehx.METRIC_IP, pyoracle.METRIC_IP),
           "cosine": (ehx.METRIC_COSINE, pyoracle.METRIC_COSINE)}
SIZES = {7: 1, 0: 8, 11: 9, 5: 63, 0xFFFFFFFF: 64, 1000: 65, 42: 700, 3: 590}   # label -> rows; 999 is carried by no row
ABSENT, COL = 999, 2
NAMES = np.array(list(SIZES) + [ABSENT], dtype=np.uint32)


def _column(sizes, seed=1):
    col = np.concatenate([np.full(n, lab, dtype=np.uint32) for lab, n in sizes.items()])
    return np.random.default_rng(seed).permutation(col)


def _space(d, metric, kind, col, seed=0):
    rng = np.random.default_rng(100 * d + seed)
    X = rng.standard_normal((len(col), d)).astype(np.float32)
    kw = {"mode": ehx.MODE_GRAPH, "M": 16} if kind == "graph_f32" else {}
    s = ehx.Space.unique("by-labels", d, metric=METRICS[metric][0], initial_capacity=len(col),
                         dtype=ehx.DTYPE_F16 if kind == "flat_f16" else ehx.DTYPE_F32, **kw)
    s.set_batch_cols(["k%d" % i for i in range(len(col))], X, {COL: col})
    return s, (X.astype(np.float16).astype(np.float32) if kind == "flat_f16" else X)


def _sets(nq, n_want, d, seed=5):
    rng = np.random.default_rng(seed + nq)
    return rng.standard_normal((nq, d)).astype(np.float32), NAMES[rng.integers(0, len(NAMES), size=(nq, n_want))]


def _check(got, Xs, col, Q, k, om, want, want_count=None, what=""):
    ids, dist, cnt = got
    for i in range(len(Q)):
        allowed = np.flatnonzero(np.isin(col, want[i, :want.shape[1] if want_count is None else want_count[i]]))
        n = min(k, len(allowed))
        assert cnt[i] == n, (what, i, cnt[i], n)
        if n:
            oids, odist, _ = pyoracle.exhaustive(Xs[allowed], Q[i:i + 1], n, om, threads=1)
            assert np.array_equal(ids[i, :n], allowed[oids[0]].astype(np.uint64)), (what, i)
            assert dist[i, :n].tobytes() == odist[0].tobytes(), (what, i)
        assert (ids[i, n:] == np.uint64(2**64 - 1)).all() and np.isposinf(dist[i, n:]).all(), (what, i)


def _counters(s):
    out = (C.c_uint64 * 4)()
    C.CDLL(_lib.LIB_PATH).ehx_test_probe_counters(s._h, out)
    return [int(v) for v in out]


def _device(s, Q, k, want, want_count=None):
    import torch
    dq = torch.tensor(Q, device="cuda")
    dw = torch.tensor(np.ascontiguousarray(want).view(np.int32), device="cuda")
    dc = None if want_count is None else torch.tensor(np.asarray(want_count, dtype=np.uint32).view(np.int32), device="cuda")
    o_ids = torch.full((len(Q), k), -7, dtype=torch.int64, device="cuda")
    o_dist = torch.full((len(Q), k), -7.0, dtype=torch.float32, device="cuda")
    o_cnt = torch.full((len(Q),), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s.knn_by_labels_device(dq, k, COL, dw, o_ids, o_dist, o_cnt, d_want_count=dc)
    torch.cuda.synchronize()
    return o_ids.cpu().numpy().view(np.uint64), o_dist.cpu().numpy(), o_cnt.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def flat():
    col = _column(SIZES)
    s, Xs = _space(100, "l2", "flat_f32", col)
    yield s, Xs, col
    s.drop()


@pytest.mark.parametrize("kind", ["flat_f32", "flat_f16", "graph_f32"])
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_every_metric_and_kind(metric, kind):
    col = _column(SIZES)
    s, Xs = _space(100, metric, kind, col)
    Q, want = _sets(9, 3, 100)
    _check(s.knn_by_labels(Q, 10, COL, want), Xs, col, Q, 10, METRICS[metric][1], want, what=(metric, kind))
    s.drop()


@pytest.mark.parametrize("d", [7, 129, 650])   # tail only, the ring, the residual join behind a full ring
def test_row_lengths(d):
    col = _column(SIZES)
    s, Xs = _space(d, "cosine", "flat_f32", col)
    Q, want = _sets(9, 3, d)
    _check(s.knn_by_labels(Q, 10, COL, want), Xs, col, Q, 10, pyoracle.METRIC_COSINE, want, what=d)
    s.drop()


# a label is named by 1, by 8 or 9 and by more than 16 queries (the tile cut at 8 pairs); 17 slots over 9 names repeat labels
@pytest.mark.parametrize("k", [10, 64, 65, 100])   # the page boundary
@pytest.mark.parametrize("n_want,nq", [(1, 1), (3, 9), (17, 70)])
def test_set_sizes_batches_and_pages(flat, n_want, nq, k):
    s, Xs, col = flat
    Q, want = _sets(nq, n_want, 100)
    _check(s.knn_by_labels(Q, k, COL, want), Xs, col, Q, k, pyoracle.METRIC_L2, want, what=(n_want, nq, k))


def test_repeats_absent_labels_counts_and_short_answers(flat):
    s, Xs, col = flat
    Q = np.random.default_rng(3).standard_normal((5, 100)).astype(np.float32)
    want = np.array([[5, 5, ABSENT, 5], [42, 7, 0, 11], [ABSENT, ABSENT, ABSENT, ABSENT], [7, 0, 7, 42], [3, 42, 5, 1000]],
                    dtype=np.uint32)
    count = np.array([4, 0, 4, 3, 2], dtype=np.uint32)   # query 3: labels 7 and 0 alone — 9 rows, fewer than k
    _check(s.knn_by_labels(Q, 10, COL, want, count), Xs, col, Q, 10, pyoracle.METRIC_L2, want, count, "host")
    _check(_device(s, Q, 10, want, count), Xs, col, Q, 10, pyoracle.METRIC_L2, want, count, "device")


def test_one_label_equals_knn_by_label_and_device_equals_host(flat):
    s, _, _ = flat
    Q, want = _sets(70, 1, 100)
    a, b = s.knn_by_labels(Q, 65, COL, want), s.knn_by_label(Q, 65, COL, want[:, 0])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    Q, want = _sets(70, 17, 100)
    a, b = s.knn_by_labels(Q, 65, COL, want), _device(s, Q, 65, want)
    assert all(np.ascontiguousarray(x).tobytes() == y.tobytes() for x, y in zip(a, b))


def test_a_staged_row_serves_eight_queries(flat):
    s, _, _ = flat
    Q, _ = _sets(64, 3, 100)
    rows = SIZES[42] + SIZES[11] + SIZES[1000]
    before = _counters(s)
    s.knn_by_labels(Q, 10, COL, np.tile(np.array([42, 11, 1000], dtype=np.uint32), (64, 1)))
    calls, items, staged, pairs = (a - b for a, b in zip(_counters(s), before))
    assert (calls, items, staged, pairs) == (1, 3 * 8, 8 * rows, 64 * rows)


def test_a_long_list_is_split_into_chunks():
    """one list of 5000 rows: more than kProbeChunk = 4096, so every pair that names it leaves two key lists"""
    sizes = {1: 5000, 2: 3000, 3: 1000}
    col = _column(sizes)
    s, Xs = _space(7, "l2", "flat_f32", col)
    Q = np.random.default_rng(8).standard_normal((9, 7)).astype(np.float32)
    want = np.array([[1, 3]] * 8 + [[2, 1]], dtype=np.uint32)
    before = _counters(s)
    _check(s.knn_by_labels(Q, 100, COL, want), Xs, col, Q, 100, pyoracle.METRIC_L2, want, what="chunks")
    # per page: label 1 — 9 pairs: 2 tiles x 2 chunks; labels 2 and 3: one item each
    assert _counters(s)[1] - before[1] == 2 * (2 * 2 + 1 + 1)
    s.drop()
