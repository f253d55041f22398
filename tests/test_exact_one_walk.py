"""GPU test of what the exact paths share (k_exact_common.h): one row walk, one key rule, one page writer.

The 100 nearest of 700 rows are asked for in every way the library has of computing exact canonical distances — the paged
exhaustive pass (exhaustive_kernel, two pages), the exact kNN among a shared id list (among_tile_kernel) and among the same
list given per query (among_list_kernel), the range search under an infinite radius (range_exact_kernel) and, for its first
10, the one-launch single query (single_query_kernel) — over fp32, binary16 and block-permuted (single-copy graph) rows.
Every answer must equal every other and the oracle's in ids and in distance BYTES.  F16 spaces: the oracle on the rounded
rows, as tests/test_knn_among.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402

METRICS = {"l2": (ehx.METRIC_L2SQ, pyoracle.METRIC_L2), "ip": (ehx.METRIC_IP, pyoracle.METRIC_IP),
           "cosine": (ehx.METRIC_COSINE, pyoracle.METRIC_COSINE)}
N, NQ, K, K1 = 700, 5, 100, 10


def _one_launch_count(s):
    f = C.CDLL(_lib.LIB_PATH).ehx_test_one_launch_count
    f.restype = C.c_uint64
    return int(f(s._h))


def _same(got, oids, odist, k, what):
    ids, dist, cnt = got[0], got[1], got[2]
    assert (np.asarray(cnt) == k).all(), "%s: counts %s" % (what, cnt)
    assert np.array_equal(ids[:, :k], oids[:, :k]), "%s: ids differ from the oracle" % what
    assert np.ascontiguousarray(dist[:, :k]).tobytes() == np.ascontiguousarray(odist[:, :k]).tobytes(), \
        "%s: distance bytes differ from the oracle" % what


@pytest.mark.parametrize("kind", ["flat_f32", "flat_f16", "graph_f32"])
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
# 160 .. 896: the register ring of the lane walk (blocks of 32 floats) and of the group walk (blocks of 128) — the steady
# state left with 2, 3 and 4 blocks, the four-at-a-time and single leftovers, and at 650 the residual join behind a full ring
@pytest.mark.parametrize("d", [3, 7, 30, 100, 129, 160, 192, 231, 640, 650, 896])
def test_every_exact_path_is_one_walk(d, metric, kind):
    em, om = METRICS[metric]
    rng = np.random.default_rng(9000 + d)
    X = rng.standard_normal((N, d)).astype(np.float32)
    Q = rng.standard_normal((NQ, d)).astype(np.float32)
    kw = {"mode": ehx.MODE_GRAPH, "M": 16} if kind == "graph_f32" else {}
    s = ehx.Space.unique("onewalk", d, metric=em, initial_capacity=N,
                         dtype=ehx.DTYPE_F16 if kind == "flat_f16" else ehx.DTYPE_F32, **kw)
    s.set_batch(["k%d" % i for i in range(N)], X)
    Xs = X.astype(np.float16).astype(np.float32) if kind == "flat_f16" else X
    oids, odist, ocnt = pyoracle.exhaustive(Xs, Q, K, om)
    assert (ocnt == K).all()
    every = np.arange(N, dtype=np.uint64)
    if kind != "graph_f32":
        _same(s.knn(Q, K), oids, odist, K, "(a) knn, paged exhaustive pass")
    _same(s.knn_among(Q, K, every), oids, odist, K, "(b) knn_among, shared list")
    off = np.arange(NQ + 1, dtype=np.uint64) * np.uint64(N)
    _same(s.knn_among(Q, K, np.tile(every, NQ), off), oids, odist, K, "(c) knn_among, per-query lists")
    ids, dist, cnt, total = s.range_search(Q, np.inf, K)
    _same((ids, dist, cnt), oids, odist, K, "(d) range, infinite radius")
    assert [int(t) for t in total] == [N] * NQ
    if kind != "graph_f32":
        before = _one_launch_count(s)
        _same(s.knn(Q[:1], K1), oids[:1], odist[:1], K1, "single query, one launch")
        assert _one_launch_count(s) == before + 1
    s.drop()
