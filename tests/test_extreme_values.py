"""The kNN engines against the oracle at extreme and non-finite values.

Reference rule (tests/test_oracle_nonfinite.py): the first k (query, row) pairs in (canonical distance, id) order, pairs
whose distance is NaN excluded; +-Inf distances are neighbours.  Bar everywhere: ids, distance bytes and counts equal to
that reference, and no query left uncertified.  The filters bound rows whose sumsq is 0 or lies in (1e-24, 1e30); a row
outside that band sends the space to the fp32 scan, a query outside it must go uncertified by the filters.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import pyoracle  # noqa: E402
from extreme_cases import (F16_EDGE, KINDS, N_I8, NEG_NAN, ODD_AT, POS_NAN, SAFE, _kind_rows, _ladder, _odd_queries,  # noqa: E402
                           _scaled)

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")

METRICS = [(ehx.METRIC_L2SQ, pyoracle.METRIC_L2), (ehx.METRIC_IP, pyoracle.METRIC_IP),
           (ehx.METRIC_COSINE, pyoracle.METRIC_COSINE)]
N_SMALL = 4000


def _keys(n):
    return ["k%d" % i for i in range(n)]


def _check(space, X, Q, k, om, what=""):
    ids, dist, cnt = space.knn(Q, k)
    oids, odist, ocnt = pyoracle.exhaustive(X, Q, k, om)
    assert cnt.tolist() == ocnt.tolist(), "%s counts differ" % what
    for i in range(Q.shape[0]):
        c = int(cnt[i])
        assert ids[i, :c].tolist() == oids[i, :c].tolist(), "%s query %d ids differ" % (what, i)
        assert dist[i, :c].tobytes() == odist[i, :c].tobytes(), "%s query %d distances differ" % (what, i)
    assert space.stats()["n_uncertified"] == 0, what
    return ids, dist, cnt


def _assert_engine(space, kind, fast):
    assert space.scan_engine() == (fast if kind in SAFE else "f32"), (kind, space.scan_engine())


@pytest.mark.parametrize("em,om", METRICS)
@pytest.mark.parametrize("kind", KINDS)
def test_row_magnitude_ladder_d128(kind, em, om):
    """Ordinary rows plus a block of one kind: int8 batch (k 10, paged k 100, single queries), fp16 filter, fp32 scan and
    in-process shards at k 10 and 100"""
    d = 128
    X, Q = _ladder(kind, d, seed=KINDS.index(kind) * 3 + em)
    s = ehx.Space.unique("xv-i8", d, metric=em, initial_capacity=N_I8)
    s.set_batch(_keys(N_I8), X)
    _assert_engine(s, kind, "i8")
    _check(s, X, Q, 10, om, "i8 k10")
    ids, dist, cnt = _check(s, X, Q, 100, om, "paged k100")
    if kind == "d" and em == ehx.METRIC_L2SQ:   # a huge row's query: itself at 0, then +Inf entries in id order
        r = 20
        assert cnt[r] == 100 and dist[r, 0] == 0 and np.isposinf(dist[r, 1:]).all()
        assert (np.diff(ids[r, 1:].astype(np.int64)) > 0).all()
    if kind == "g":   # the NaN rule shows: NaN-row queries have no neighbour
        assert cnt[20] == 0 and cnt[21] == 0
    for i in (0, 20, 24, 25):
        _check(s, X, Q[i:i + 1], 10, om, "single %d" % i)
    s.drop()
    Xs = X[:N_SMALL]
    for name, kw, fast in (("f16", {}, "f16"), ("f32", dict(scan=ehx.SCAN_F32), "f32")):
        t = ehx.Space.unique("xv-" + name, d, metric=em, **kw)
        t.set_batch(_keys(N_SMALL), Xs)
        _assert_engine(t, kind, fast)
        _check(t, Xs, Q, 10, om, name)
        t.drop()
    sh = ehx.Space.unique("xv-sh", d, metric=em, shards=3)
    sh.set_batch(_keys(N_SMALL), Xs)
    _check(sh, Xs, Q, 10, om, "shards k10")
    _check(sh, Xs, Q, 100, om, "shards k100")
    sh.drop()


@pytest.mark.parametrize("em,om", METRICS)
@pytest.mark.parametrize("kind", KINDS)
def test_row_magnitude_ladder_d768_int8(kind, em, om):
    d = 768
    X, Q = _ladder(kind, d, seed=100 + KINDS.index(kind) * 3 + em)
    s = ehx.Space.unique("xv-768", d, metric=em, initial_capacity=N_I8)
    s.set_batch(_keys(N_I8), X)
    _assert_engine(s, kind, "i8")
    _check(s, X, Q, 10, om, "i8 d768")
    s.drop()


@pytest.mark.parametrize("em,om", METRICS)
@pytest.mark.parametrize("kind", ["a_lo", "a_hi", "b_lo", "b_hi", "f"])
def test_spaces_made_entirely_of_one_kind(kind, em, om):
    d = 128
    rng = np.random.default_rng(7 + KINDS.index(kind))
    X = _kind_rows(kind, rng, N_I8, d)
    Q = np.concatenate([rng.standard_normal((6, d)).astype(np.float32), X[[3, 17, 4000]],
                        np.zeros((1, d), np.float32)])
    s = ehx.Space.unique("xv-all", d, metric=em, initial_capacity=N_I8)
    s.set_batch(_keys(N_I8), X)
    _assert_engine(s, kind, "i8")
    _check(s, X, Q, 10, om, "all-%s i8" % kind)
    s.drop()
    t = ehx.Space.unique("xv-all16", d, metric=em)
    t.set_batch(_keys(N_SMALL), X[:N_SMALL])
    _assert_engine(t, kind, "f16")
    _check(t, X[:N_SMALL], Q, 10, om, "all-%s f16" % kind)
    t.drop()


@pytest.mark.parametrize("em,om", METRICS)
def test_non_finite_rows_when_k_exceeds_the_finite_rows(em, om):
    """300 rows, 240 of them holding a NaN or Inf: counts below k show the NaN rule, on every flat path"""
    rng = np.random.default_rng(em)
    d = 24
    X = rng.standard_normal((300, d)).astype(np.float32)
    X[:240] = _kind_rows("g", rng, 240, d)
    X[250] = 0.0
    Q = np.concatenate([rng.standard_normal((5, d)).astype(np.float32), X[[0, 2, 250]]])
    for kw in ({}, dict(scan=ehx.SCAN_F32), dict(shards=3)):
        s = ehx.Space.unique("xv-k", d, metric=em, **kw)
        s.set_batch(_keys(300), X)
        for k in (10, 48, 100, 300):
            ids, dist, cnt = _check(s, X, Q, k, om, "%s k%d" % (kw, k))
            if k == 300:   # the 120 NaN rows are never neighbours
                assert (cnt[:5] <= 180).all() and (cnt[:5] >= 60).all()
        _check(s, X, Q[:1], 100, om, "single")
        s.drop()


# ---- B. odd queries inside ordinary batches -----------------------------------------------------------------------
@pytest.mark.parametrize("em,om", METRICS)
@pytest.mark.parametrize("engine", ["i8", "f16", "f32"])
def test_odd_queries_inside_ordinary_batches(engine, em, om):
    d = 128
    rng = np.random.default_rng(50 + em)
    n = N_I8 if engine == "i8" else N_SMALL
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((257, d)).astype(np.float32)
    odd = _odd_queries(rng, d)
    assert len(odd) == len(ODD_AT)
    for at, q in zip(ODD_AT, odd):
        Q[at] = q
    s = ehx.Space.unique("xv-odd", d, metric=em, scan=ehx.SCAN_F32 if engine == "f32" else ehx.SCAN_AUTO)
    s.set_batch(_keys(n), X)
    assert s.scan_engine() == engine
    ids, dist, cnt = _check(s, X, Q, 10, om, "batch with odd queries")
    assert cnt[1] == 0 and cnt[2] == 0   # NaN queries
    keep = np.array([i for i in range(257) if i not in ODD_AT])
    ids2, dist2, cnt2 = s.knn(Q[keep], 10)
    assert np.array_equal(ids2, ids[keep]) and dist2.tobytes() == dist[keep].tobytes()
    assert np.array_equal(cnt2, cnt[keep])
    assert s.stats()["n_uncertified"] == 0
    s.drop()


# ---- C. cross-band: the B * gamma_q term of the int8 bound overflows ----------------------------------------------
@pytest.mark.parametrize("em,om", METRICS[:2])
@pytest.mark.parametrize("engine", ["i8", "f16"])
@pytest.mark.parametrize("rows_huge", [True, False])
def test_cross_band_rows_and_queries(rows_huge, engine, em, om):
    d = 128
    rng = np.random.default_rng(70 + em + 2 * rows_huge)
    n = N_I8 if engine == "i8" else N_SMALL
    big, small = (1.25e29, 5e29), (2e-24, 8e-24)
    X = _scaled(rng, n, d, *(big if rows_huge else small))
    Q = _scaled(rng, 64, d, *(small if rows_huge else big))
    Q[:4] = _scaled(rng, 4, d, *(big if rows_huge else small))   # and a few queries of the rows' own scale
    s = ehx.Space.unique("xv-cross", d, metric=em)
    s.set_batch(_keys(n), X)
    assert s.scan_engine() == engine
    _check(s, X, Q, 10, om, "cross-band")
    s.drop()


# ---- D. garbage queries do not widen the int8 candidate list ------------------------------------------------------
def _child_trace():
    d, n = 128, N_I8
    rng = np.random.default_rng(90)
    X = rng.standard_normal((n, d)).astype(np.float32)
    s = ehx.Space.unique("xv-trace", d, metric=ehx.METRIC_COSINE)
    s.set_batch(_keys(n), X)
    assert s.scan_engine() == "i8"
    odd = _odd_queries(rng, d)
    garbage = [odd[1], odd[2], odd[6], odd[8], odd[10]]   # NaN and out-of-band queries
    for b in range(8):
        Q = rng.standard_normal((64, d)).astype(np.float32)
        for j in range(4):
            Q[7 + 13 * j] = garbage[(b + j) % len(garbage)]
        _check(s, X, Q, 10, pyoracle.METRIC_COSINE, "batch %d" % b)
    s.drop()


def test_garbage_queries_do_not_widen_the_int8_candidate_list():
    env = dict(os.environ, EHX_I8_TRACE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, timeout=300,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, "child failed (rc %d):\n%s" % (r.returncode, r.stderr[-6000:])
    assert "candidate list now" not in r.stderr, r.stderr[-3000:]


# ---- E. fp16 storage at the binary16 boundaries; fp32 Get is bit-exact ---------------------------------------------
@pytest.mark.parametrize("em,om", METRICS)
@pytest.mark.parametrize("n,engine", [(N_I8 + 64, "i8"), (N_SMALL, "f16")])
def test_fp16_storage_boundaries(n, engine, em, om):
    d = 64
    rng = np.random.default_rng(110 + em)
    X = rng.standard_normal((n, d)).astype(np.float32)
    for i, v in enumerate(F16_EDGE):
        X[500 + i, i] = v                     # one edge value in an ordinary row
        X[600 + i, :] = v                     # a row made of it
    Xh = X.astype(np.float16).astype(np.float32)
    s = ehx.Space.unique("xv-f16", d, metric=em, dtype=ehx.DTYPE_F16)
    s.set_batch(_keys(n), X)
    for i in range(len(F16_EDGE)):
        for r in (500 + i, 600 + i):
            assert s.get("k%d" % r).tobytes() == Xh[r].tobytes(), (r, F16_EDGE[i])
    # the 65520 rows hold Inf now: the filters cannot bound them
    assert s.scan_engine() == "f32"
    Q = np.concatenate([rng.standard_normal((12, d)).astype(np.float32), X[[505, 600, 604, 606, 608]]])
    _check(s, Xh, Q, 10, om, "f16 rows")
    # the same space without the rows that rounded to Inf: the filter engine itself answers
    fin = np.isfinite(Xh).all(axis=1)
    t = ehx.Space.unique("xv-f16b", d, metric=em, dtype=ehx.DTYPE_F16)
    t.set_batch(_keys(int(fin.sum())), X[fin])
    assert t.scan_engine() == engine
    _check(t, Xh[fin], Q, 10, om, "f16 finite rows")
    s.drop()
    t.drop()


def test_f32_get_returns_exactly_what_was_set():
    bits = np.array([0x80000000, 0x00000001, 0x007FFFFF, 0x00400000, 0x7F800000, 0xFF800000, 0x7FC12345, 0xFFC00001,
                     0x7FA00001, 0xFF800001, 0x7F7FFFFF, 0xFF7FFFFF, 0x00800000, 0x3F800000, 0x80000001, 0x0000FFFF],
                    dtype=np.uint32)
    X = np.random.default_rng(1).standard_normal((40, 16)).astype(np.float32)
    X[3] = bits.view(np.float32)
    X[9, 5] = bits.view(np.float32)[6]
    for em, _ in METRICS:
        s = ehx.Space.unique("xv-get", 16, metric=em)
        s.set_batch(_keys(40), X)
        s.set("single", X[3])
        assert s.get("k3").view(np.uint32).tolist() == bits.tolist()
        assert s.get("single").view(np.uint32).tolist() == bits.tolist()
        assert s.get("k9").tobytes() == X[9].tobytes()
        s.drop()


# ---- F. the shard-merge ABI ---------------------------------------------------------------------------------------
def _merge(L, fn, G, nq, k, g_ids, g_dist, g_cnt, stride=False):
    import ctypes as C
    import torch
    from embeddinghub_amd import _lib
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d_ids, d_dist, d_cnt = t(g_ids), t(g_dist), t(g_cnt)
    o_ids = torch.full((nq, k), -1, dtype=torch.int64, device="cuda")
    o_dist = torch.full((nq, k), np.nan, dtype=torch.float32, device="cuda")
    o_cnt = torch.full((nq,), -1, dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    if stride:
        rc = L.ehx_merge_topk_strided_device(st, nq, k, G, P(d_ids), nq * k * 8, P(d_dist), nq * k * 4, P(d_cnt),
                                             nq * 4, P(o_ids), P(o_dist), P(o_cnt))
    else:
        rc = L.ehx_merge_topk_device(st, nq, k, G, P(d_ids), P(d_dist), P(d_cnt), P(o_ids), P(o_dist), P(o_cnt))
    torch.cuda.synchronize()
    if rc != _lib.OK:
        return rc, None
    return rc, (o_ids.cpu().numpy(), o_dist.cpu().numpy(), o_cnt.cpu().numpy())


def _merge_lists(rng, G, nq, k):
    vals = np.array([-np.inf, -1.0, 0.0, 0.5, 1.0, np.inf], np.float32)
    g_dist = np.where(rng.random((G, nq, k)) < 0.3, rng.choice(vals, (G, nq, k)),
                      rng.standard_normal((G, nq, k))).astype(np.float32)
    g_dist[:, :, k - 3:] = np.inf                       # valid +Inf entries at every tail
    g_ids = rng.permutation(G * nq * k).reshape(G, nq, k).astype(np.int64)
    for g in range(G):
        for q in range(nq):
            o = np.lexsort((g_ids[g, q], g_dist[g, q]))
            g_dist[g, q], g_ids[g, q] = g_dist[g, q][o], g_ids[g, q][o]
    g_cnt = rng.integers(0, k + 1, size=(G, nq)).astype(np.int32)
    g_cnt[:, ::7] = k
    g_cnt[:, 0] = 0                                     # a query no list has results for
    g_cnt[0, 1:] = k
    return g_ids, g_dist, g_cnt


@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("G", [1, 64])
@pytest.mark.parametrize("stride", [False, True])
def test_merge_abi_with_inf_entries_empty_lists_and_ties(k, G, stride):
    from embeddinghub_amd import _lib
    from test_sharded import _np_merge
    L = _lib.load()
    rng = np.random.default_rng(k + G)
    nq = 33
    g_ids, g_dist, g_cnt = _merge_lists(rng, G, nq, k)
    e_ids, e_dist, e_cnt = np.full((nq, k), -1, np.int64), np.full((nq, k), np.inf, np.float32), np.zeros(nq, np.int32)
    _np_merge(g_ids, g_dist, g_cnt, k, e_ids, e_dist, e_cnt)
    rc, out = _merge(L, None, G, nq, k, g_ids, g_dist, g_cnt, stride)
    assert rc == _lib.OK
    o_ids, o_dist, o_cnt = out
    assert o_cnt.tolist() == e_cnt.tolist()
    for q in range(nq):
        c = e_cnt[q]
        assert o_ids[q, :c].tolist() == e_ids[q, :c].tolist(), q
        assert o_dist[q, :c].tobytes() == e_dist[q, :c].tobytes(), q
    assert e_cnt[0] == 0 and (e_cnt[1:] == k).all() and np.isposinf(e_dist).any()


def test_merge_abi_refuses_65_lists_beyond_k_64():
    from embeddinghub_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(65)
    g_ids, g_dist, g_cnt = _merge_lists(rng, 65, 4, 100)
    rc, out = _merge(L, None, 65, 4, 100, g_ids, g_dist, g_cnt)
    assert rc != _lib.OK and out is None


# ---- G. graph mode ------------------------------------------------------------------------------------------------
def _graph_rows(rng, n, d):
    X = rng.standard_normal((n, d)).astype(np.float32)
    return (X * np.exp(rng.uniform(np.log(1e-10), np.log(1e13), n))[:, None].astype(np.float32)).astype(np.float32)


def _graph_space(X, em, om, graph_X=None, ep=None):
    n, d = X.shape
    h = pyoracle.Hnsw(d, om, n, M=16)
    h.add_rows(X if graph_X is None else graph_X)
    s = ehx.Space.unique("xv-graph", d, metric=em, mode=ehx.MODE_GRAPH, M=16, initial_capacity=n,
                         build_batch=0xFFFFFFFF)
    s.set_batch(_keys(n), X)
    l0, lv, upper = h.export_graph()
    s.graph_import(l0, lv, upper, h.enterpoint if ep is None else ep, h.maxlevel)
    return h, s


def _nan_queries(rng, d):
    Q = rng.standard_normal((4, d)).astype(np.float32)
    Q[0, 1] = POS_NAN
    Q[1, 7] = NEG_NAN
    Q[2, :] = POS_NAN
    Q[3, :] = NEG_NAN
    return Q


@pytest.mark.parametrize("em,om", METRICS)
def test_graph_walk_on_rows_scaled_across_the_band(em, om):
    n, d, k, ef = 3000, 32, 10, 40
    rng = np.random.default_rng(130 + em)
    X = _graph_rows(rng, n, d)
    h, s = _graph_space(X, em, om)
    h.set_ef(ef)
    s.set_ef(ef)
    Q = np.concatenate([rng.standard_normal((24, d)).astype(np.float32), X[[5, 77, 1234]],
                        _scaled(rng, 2, d, 2e-24, 4e-24), _scaled(rng, 2, d, 2.5e29, 5e29)])
    if em == ehx.METRIC_L2SQ:   # (IP / cosine: a zero query ties every row at 1; see the property check below)
        Q = np.concatenate([Q, np.zeros((1, d), np.float32)])
    nq = Q.shape[0]
    s.stats_reset()
    labels, dists, counts, _, st = h.search_batch(Q, k, threads=1)
    ids, dist, cnt = s.knn(Q, k)
    assert cnt.tolist() == counts.tolist()
    assert np.array_equal(ids, labels) and dist.tobytes() == dists.tobytes()
    g = s.stats()
    assert g["n_dist"] == st["n_dist"] - nq and g["n_hops"] == st["n_hops0"] + st["n_hops_up"]
    # NaN queries (both signs) inside the batch: count 0, every other answer unchanged; strict and wide walk
    QN = np.concatenate([Q[:3], _nan_queries(rng, d), Q[3:]])
    for width in (1, 2):
        s.set_search_width(width)
        base = s.knn(Q, k)
        i2, d2, c2 = s.knn(QN, k)
        assert c2[3:7].tolist() == [0, 0, 0, 0], width
        keep = np.r_[0:3, 7:QN.shape[0]]
        assert np.array_equal(i2[keep], base[0]) and d2[keep].tobytes() == base[1].tobytes()
        assert np.array_equal(c2[keep], base[2])
    s.set_search_width(1)
    if em != ehx.METRIC_L2SQ:   # zero queries under IP / cosine: every distance is 1, answered in full
        z = s.knn(np.zeros((2, d), np.float32), k)
        assert (z[2] == k).all() and (z[1] == np.float32(1.0)).all()
    s.drop()


def _sorted_by_dist_id(ids, dist, c):
    pairs = list(zip(dist[:c].tolist(), ids[:c].tolist()))
    return pairs == sorted(pairs)


@pytest.mark.parametrize("em,om", METRICS)
def test_graph_walk_over_non_finite_rows(em, om):
    """+-NaN / +-Inf rows in the graph, one of them the entry point (and the first row): hnswlib is undefined there, so
    this is checked by properties, and by recall against the same walk over a space without those rows.  (Under IP an
    Inf component gives a +-Inf distance, a valid neighbour that a greedy walk need not find: there only NaN rows are
    barred from the answer and recall is not compared.)"""
    n, d, k, ef = 3000, 32, 10, 64
    rng = np.random.default_rng(150 + em)
    Xf = rng.standard_normal((n, d)).astype(np.float32)
    h0 = pyoracle.Hnsw(d, om, n, M=16)
    h0.add_rows(Xf)
    ep = h0.enterpoint
    bad = sorted({0, ep} | set(rng.choice(n, 60, replace=False).tolist()))
    X = Xf.copy()
    for j, r in enumerate(bad):
        X[r, (r * 5) % d] = (POS_NAN, NEG_NAN, np.inf, -np.inf)[j % 4]
    X[ep, :] = NEG_NAN
    X[0, :] = POS_NAN
    _, s = _graph_space(X, em, om, graph_X=Xf, ep=ep)     # the finite rows' graph, the non-finite rows Set
    _, s0 = _graph_space(Xf, em, om)
    Q = np.concatenate([rng.standard_normal((60, d)).astype(np.float32), _nan_queries(rng, d)])
    good = np.setdiff1d(np.arange(n), bad)
    truth, _, _ = pyoracle.exhaustive(X[good], Q[:60], k, om)
    truth = good[truth]
    truth0, _, _ = pyoracle.exhaustive(Xf, Q[:60], k, om)
    badset = set(bad) if em != ehx.METRIC_IP else {r for r in bad if np.isnan(X[r]).any()}
    for width in (1, 2):
        for sp in (s, s0):
            sp.set_ef(ef)
            sp.set_search_width(width)
        ids, dist, cnt = s.knn(Q, k)
        assert cnt[60:].tolist() == [0, 0, 0, 0]
        for i in range(60):
            c = int(cnt[i])
            assert c == k, (width, i, c)
            assert not (set(ids[i, :c].tolist()) & badset), (width, i)
            assert not np.isnan(dist[i, :c]).any()
            assert _sorted_by_dist_id(ids[i], dist[i], c)
            for j in range(c):
                assert dist[i, j] == np.float32(pyoracle.dist(om, Q[i], X[ids[i, j]])), (width, i, j)
        rec = np.mean([len(set(ids[i].tolist()) & set(truth[i].tolist())) / k for i in range(60)])
        ids0, _, _ = s0.knn(Q[:60], k)
        rec0 = np.mean([len(set(ids0[i].tolist()) & set(truth0[i].tolist())) / k for i in range(60)])
        assert em == ehx.METRIC_IP or rec >= rec0 - 0.02, (width, rec, rec0)
    s.drop()
    s0.drop()


if __name__ == "__main__":
    _child_trace()
