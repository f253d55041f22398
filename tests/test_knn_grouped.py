"""GPU tests of the grouped kNN (ehx_knn_grouped*, ehx_grouped.cpp, k_grouped.hip): exact top-k with at most per_group rows
per group label, on the scan route (the falling-radius int8 scan with a cap per label in its re-rank) and on the exact route
(every prefix row in slabs of 4096).

Expected answers come from the oracle's distances of every prefix row (pyoracle.exhaustive at k = rows), capped by the
plain-Python greedy of tests/grouped_model.py: ids equal, distance BYTES equal, sentinels behind the count.  The scan cases
that assert "none handed on" are the ones tests/test_grouped_model.py clears (grouped_model.cleared)."""
import ctypes as C

import numpy as np
import pytest

import grouped_model as gm
import largek_cases as lc

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402
from embeddinghub_amd.space import marshal_groups  # noqa: E402

EM = {"l2": ehx.METRIC_L2SQ, "ip": ehx.METRIC_IP, "cosine": ehx.METRIC_COSINE}
NO_ID = np.uint64(2**64 - 1)
NONE = gm.NONE
f32 = np.float32
PASSES = 3   # of a prefix of 16 385 .. 65 536 rows at the default growth


def _keys(n, first=0):
    return ["k%d" % i for i in range(first, first + n)]


def _counters(s):
    out = (C.c_uint64 * 5)()
    C.CDLL(_lib.LIB_PATH).ehx_test_grouped_counters(s._h, out)
    return np.array(list(out), dtype=np.int64)   # on the scan route, handed to the exact route, of those overflowed, passes, calls


def _space(name, X, metric, cap=None, **kw):
    s = ehx.Space.unique(name, X.shape[1], metric=EM[metric], initial_capacity=cap or len(X), **kw)
    s.set_batch(_keys(len(X)), X)
    return s


def _i8_space(name, X, metric, **kw):
    s = _space(name, X, metric, **kw)
    assert s.scan_engine() == "i8"
    return s


def _assert_rows(got, want, k, what):
    ids, dist, cnt = got
    assert ids.shape == (len(want), k) and dist.shape == (len(want), k) and cnt.shape == (len(want),)
    for i, (wi, wd) in enumerate(want):
        c = len(wi)
        assert int(cnt[i]) == c, "%s: query %d count %d, expected %d" % (what, i, cnt[i], c)
        assert np.array_equal(ids[i, :c], wi), "%s: query %d ids differ" % (what, i)
        assert dist[i, :c].tobytes() == wd.tobytes(), "%s: query %d distance bytes differ" % (what, i)
        assert (ids[i, c:] == NO_ID).all() and np.isposinf(dist[i, c:]).all(), "%s: query %d tail sentinels" % (what, i)


def _same_bytes(a, b):
    return all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes() for x, y in zip(a, b))


def _device_form(space, Q, k, labels, per_group, n_labels=None):
    import torch
    g, n = marshal_groups(labels)
    n = n if n_labels is None else n_labels
    dq = torch.tensor(np.ascontiguousarray(Q, dtype=f32), device="cuda")
    dg = torch.tensor(g.view(np.int32), device="cuda") if len(g) else None
    o_ids = torch.full((len(Q), k), -7, dtype=torch.int64, device="cuda")
    o_dist = torch.full((len(Q), k), -7.0, dtype=torch.float32, device="cuda")
    o_cnt = torch.full((len(Q),), 77, dtype=torch.int32, device="cuda")
    space.knn_grouped_device(dq, k, dg, n, o_ids, o_dist, o_cnt, per_group=per_group)
    torch.cuda.synchronize()
    return (o_ids.cpu().numpy().view(np.uint64), o_dist.cpu().numpy(), o_cnt.cpu().numpy().view(np.uint32))


# ---- 1. the exact route, every layout ----

@pytest.mark.parametrize("kind", ["flat_f32", "flat_f16", "graph_f32"])
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
@pytest.mark.parametrize("d", [7, 129, 650])
def test_exact_route_every_layout(d, metric, kind):
    n, nq = 700, 5
    rng = np.random.default_rng(1000 + d)
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    kw = {"mode": ehx.MODE_GRAPH, "M": 16} if kind == "graph_f32" else {}
    s = _space("grouped-small", X, metric, dtype=ehx.DTYPE_F16 if kind == "flat_f16" else ehx.DTYPE_F32, **kw)
    Xs = X.astype(np.float16).astype(f32) if kind == "flat_f16" else X   # the oracle reads the rows as stored
    full = gm.oracle_all(Xs, Q, metric)
    labels = gm.labels_mod37(n)
    for k in (10, 100):
        for m in (1, 3):
            c0 = _counters(s)
            got = s.knn_grouped(Q, k, labels, per_group=m)
            _assert_rows(got, gm.expected(full, labels, k, m), k, "%s %s d=%d k=%d m=%d" % (kind, metric, d, k, m))
            assert (_counters(s) - c0).tolist() == [0, nq, 0, 0, 1]
    assert _same_bytes(got, _device_form(s, Q, 100, labels, 3))
    s.drop()


# ---- 2. slab boundaries of the exact route ----

@pytest.mark.parametrize("n", [4095, 4097, 8193])
def test_slab_boundary(n):
    d, nq = 16, 5
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    # group 7 around query 0: row n - 1 (the LAST slab) nearest, then rows 5, 6, 4090 (the first slab), then row 4094 or 4096
    near = [n - 1, 5, 6, 4090, min(4096, n - 2)]
    for j, r in enumerate(near):
        X[r] = Q[0]
        X[r, 0] += f32(0.01 * (j + 1))
    labels = (100 + np.arange(n) % 37).astype(np.uint32)
    labels[::11] = NONE
    labels[near] = 7
    s = _space("grouped-slab", X, "l2")
    full = gm.oracle_all(X, Q, "l2")
    assert [int(v) for v in full[0][0, :5]] == near
    for k in (4, 10, 256):
        for m in (1, 2, 3):
            got = s.knn_grouped(Q, k, labels, per_group=m)
            _assert_rows(got, gm.expected(full, labels, k, m), k, "n=%d k=%d m=%d" % (n, k, m))
            # the first m of group 7 straddle the slab edge; rows 5 and 6, carried from the first slab, are displaced by the last
            assert [int(v) for v in got[0][0, :m]] == near[:m] and near[m] not in got[0][0]
    s.drop()


# ---- 3. the scan route ----

@pytest.mark.parametrize("lab", sorted(gm.LABELINGS))
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_scan_route(metric, lab):
    X, Q = lc.gauss(20000, 64, 64, 1)
    full = gm.scan_oracle(metric)
    labels = gm.LABELINGS[lab](len(X))
    s = _i8_space("grouped-scan", X, metric)
    for k in gm.SCAN_KS:
        for m in gm.SCAN_MS:
            c0, st0 = _counters(s), s.stats()
            got = s.knn_grouped(Q, k, labels, per_group=m)
            dc, st1 = _counters(s) - c0, s.stats()
            what = "%s %s k=%d m=%d" % (metric, lab, k, m)
            print(what, dc.tolist())
            _assert_rows(got, gm.expected(full, labels, k, m), k, what)
            assert dc[0] + dc[1] == 64 and dc[3] == PASSES and dc[4] == 1, (what, dc)
            if gm.cleared(lab, k, m):
                assert dc.tolist() == [64, 0, 0, PASSES, 1], (what, dc)
            assert st1["n_queries"] - st0["n_queries"] == 64, what
            assert st1["n_i8_queries"] - st0["n_i8_queries"] == 64 and st1["n_i8_fallback"] - st0["n_i8_fallback"] == dc[1], what
            assert st1["n_dist"] > st0["n_dist"]
    # the sample's rows carry 100 labels: at per_group 1 it never holds 256 capped rows, the radius stays +Inf, all are handed on
    if lab == "scattered":
        c0 = _counters(s)
        s.knn_grouped(Q, 256, labels, per_group=1)
        assert (_counters(s) - c0).tolist() == [0, 64, 0, PASSES, 1]
    s.drop()


# ---- 4. equivalences ----

def test_equivalences_on_both_routes():
    X, Q = lc.gauss(20000, 64, 64, 1)
    labels = gm.labels_scattered(len(X))
    none = np.full(len(X), NONE, dtype=np.uint32)
    s = _i8_space("grouped-eq", X, "cosine")
    for q, route in ((Q, [64, 0]), (Q[:5], [0, 5])):
        for k in (10, 100):
            plain = s.knn(q, k)
            for lb, m in ((labels, k), (labels, 2 ** 32 - 1), (none, 1)):
                c0 = _counters(s)
                got = s.knn_grouped(q, k, lb, per_group=m)
                assert (_counters(s) - c0)[:2].tolist() == route, (k, m)
                assert _same_bytes(got, plain), (len(q), k, m)
            for m in (1, 4):
                assert _same_bytes(s.knn_grouped(q, k, labels, per_group=m), _device_form(s, q, k, labels, m)), (len(q), k, m)
    s.drop()


# ---- 5. a giant group ----

def test_giant_group_is_handed_on_and_fewer_than_k_groups_exist():
    rng = np.random.default_rng(55)
    n, d = 20000, 64
    X = (f32(0.1) * rng.standard_normal((n, d))).astype(f32)       # 19 900 rows of ONE label around the origin, nearest
    Q = (f32(0.1) * rng.standard_normal((64, d))).astype(f32)
    far = np.arange(100) * 200 + 7                                  # 100 rows far away, none of them in the sample (stride 20)
    X[far] = (f32(3.0) * rng.standard_normal((100, d))).astype(f32)
    labels = np.full(n, 1, dtype=np.uint32)
    labels[far] = 2 + np.arange(100) % 5                            # 6 groups in all
    s = _i8_space("grouped-giant", X, "l2")
    full = gm.oracle_all(X, Q, "l2")
    c0 = _counters(s)
    got = s.knn_grouped(Q, 10, labels, per_group=1)
    dc = _counters(s) - c0
    # the sample holds ONE label: no radius, every query is one the bound does not serve
    assert dc.tolist() == [0, 64, 0, PASSES, 1], dc
    want = gm.expected(full, labels, 10, 1)
    assert all(len(w[0]) == 6 for w in want)
    _assert_rows(got, want, 10, "giant group")
    # at per_group 4 the sample holds four capped rows: still below k = 10
    c0 = _counters(s)
    got = s.knn_grouped(Q, 10, labels, per_group=4)
    assert (_counters(s) - c0)[:2].tolist() == [0, 64]
    _assert_rows(got, gm.expected(full, labels, 10, 4), 10, "giant group, per_group 4")
    s.drop()


# ---- 6. ties ----

def test_ties_are_cut_by_id_within_and_across_groups():
    X, Q, at = lc.ties()            # 300 copies of row 5 spread over the ids of all three passes; query 0 is that row
    labels = gm.labels_scattered(len(X)) + np.uint32(20000)
    for j, r in enumerate(at):      # every third copy in ONE group, the others in groups of two neighbours
        labels[r] = 9999 if j % 3 == 0 else 10000 + j // 2
    s = _i8_space("grouped-ties", X, "l2")
    full = gm.oracle_all(X, Q, "l2")
    for q in (Q, Q[:5]):            # the scan route, and the exact route over five slabs
        sub = tuple(a[:len(q)] for a in full)
        for k, m in ((100, 1), (100, 2), (256, 4), (10, 1)):
            got = s.knn_grouped(q, k, labels, per_group=m)
            want = gm.expected(sub, labels, k, m)
            _assert_rows(got, want, k, "ties nq=%d k=%d m=%d" % (len(q), k, m))
            tied = [int(v) for v in got[0][0] if int(v) in set(int(a) for a in at)]
            assert len(tied) >= min(k, 10) and tied == sorted(tied)
    s.drop()


# ---- 7. gates and edges ----

def test_gates_and_the_prefix():
    X, Q = lc.gauss(20000, 64, 64, 1)
    labels = gm.labels_clustered(len(X))
    s = _i8_space("grouped-gates", X, "l2", cap=len(X) + 64)
    full = gm.scan_oracle("l2")
    want = gm.expected(full, labels, 10, 1)
    c0 = _counters(s)
    _assert_rows(s.knn_grouped(Q[:63], 10, labels), want[:63], 10, "63 queries")
    assert (_counters(s) - c0).tolist() == [0, 63, 0, 0, 1]
    c0 = _counters(s)
    _assert_rows(s.knn_grouped(Q, 10, labels), want, 10, "64 queries")
    assert (_counters(s) - c0).tolist() == [64, 0, 0, PASSES, 1]
    # n_labels below the row count: only the prefix is searched — 18 000 rows on the scan route, 15 000 on the exact route
    for n_labels, route in ((18000, [64, 0]), (15000, [0, 64])):
        c0 = _counters(s)
        got = s.knn_grouped(Q, 10, labels[:n_labels])
        assert (_counters(s) - c0)[:2].tolist() == route
        _assert_rows(got, gm.expected(gm.oracle_all(X[:n_labels], Q, "l2"), labels, 10, 1), 10, "n_labels=%d" % n_labels)
        assert (got[0] < n_labels).all()
        assert _same_bytes(got, _device_form(s, Q, 10, labels, 1, n_labels=n_labels))
    # n_labels above the row count is fine
    longer = np.concatenate([labels, np.arange(5000, dtype=np.uint32)])
    assert _same_bytes(s.knn_grouped(Q, 10, longer), s.knn_grouped(Q, 10, labels))
    # n_labels = 0: nothing is searched
    for q in (Q, Q[:3]):
        got = s.knn_grouped(q, 10, [])
        assert (got[2] == 0).all() and (got[0] == NO_ID).all() and np.isposinf(got[1]).all()
    # rows appended after the labels were built are not returned
    s.set_batch(_keys(64, first=len(X)), Q)                    # every query is now a stored row, at distance 0
    assert len(s) == len(X) + 64
    for q in (Q, Q[:5]):
        _assert_rows(s.knn_grouped(q, 10, labels), want[:len(q)], 10, "appended rows, nq=%d" % len(q))
    got = s.knn_grouped(Q[:5], 1, np.concatenate([labels, np.full(64, NONE, dtype=np.uint32)]))
    assert got[0][:, 0].tolist() == [len(X) + i for i in range(5)]      # ... until the labels cover them
    s.drop()


def test_error_returns():
    rng = np.random.default_rng(8)
    n, d = 200, 8
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((3, d)).astype(f32)
    labels = (np.arange(n) % 5).astype(np.uint32)
    s = _space("grouped-err", X, "l2")
    for k, m, code in ((0, 1, _lib.EINVAL), (4, 0, _lib.EINVAL), (257, 1, _lib.EUNSUPPORTED)):
        with pytest.raises(ehx.EhxError) as e:
            s.knn_grouped(Q, k, labels, per_group=m)
        assert e.value.code == code
    ids, dist, cnt = s.knn_grouped(np.zeros((0, d), dtype=f32), 4, labels)   # no queries: EHX_OK, nothing written
    assert ids.shape == (0, 4) and cnt.shape == (0,)
    got = s.knn_grouped(Q, 256, labels, per_group=1)                         # k = 256 is served; five groups exist
    assert (got[2] == 5).all()
    L = _lib.load()
    q = np.ascontiguousarray(Q)
    o_ids, o_dist, o_cnt = np.zeros((3, 4), dtype=np.uint64), np.zeros((3, 4), dtype=f32), np.zeros(3, dtype=np.uint32)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    args = [P(o_ids, C.c_uint64), P(o_dist, C.c_float), P(o_cnt, C.c_uint32)]
    for hole in range(3):
        a = list(args)
        a[hole] = None
        assert L.ehx_knn_grouped(s._h, 3, P(q, C.c_float), 4, 1, P(labels, C.c_uint32), n, a[0], a[1], a[2]) == _lib.EINVAL
    assert L.ehx_knn_grouped(s._h, 3, None, 4, 1, P(labels, C.c_uint32), n, *args) == _lib.EINVAL
    assert L.ehx_knn_grouped(s._h, 3, P(q, C.c_float), 4, 1, None, n, *args) == _lib.EINVAL   # NULL labels with n_labels > 0
    assert L.ehx_knn_grouped(s._h, 3, P(q, C.c_float), 4, 1, None, 0, *args) == _lib.OK and (o_cnt == 0).all()
    assert L.ehx_knn_grouped(s._h, 3, P(q, C.c_float), 4, 1, P(labels, C.c_uint32), n, *args) == _lib.OK and (o_cnt == 4).all()
    assert L.ehx_knn_grouped_device(s._h, None, 3, None, 4, 1, None, n, None, None, None) == _lib.EINVAL
    assert L.ehx_knn_grouped(None, 3, P(q, C.c_float), 4, 1, P(labels, C.c_uint32), n, *args) == _lib.EINVAL
    h = s._h
    s.drop()   # the tombstone answers for the dropped handle
    assert L.ehx_knn_grouped(h, 3, P(q, C.c_float), 4, 1, P(labels, C.c_uint32), n, *args) == _lib.ENOTFOUND
    e0 = ehx.Space.unique("grouped-empty", d, metric=ehx.METRIC_L2SQ)
    got = e0.knn_grouped(Q, 4, labels)
    assert (got[2] == 0).all() and (got[0] == NO_ID).all() and np.isposinf(got[1]).all()
    e0.drop()
    sh = ehx.Space.unique("grouped-sh", d, metric=ehx.METRIC_L2SQ, shards=2)
    sh.set_batch(_keys(n), X)
    with pytest.raises(ehx.EhxError) as e:
        sh.knn_grouped(Q, 4, labels)
    assert e.value.code == _lib.EUNSUPPORTED and "sharded" in str(e.value)
    sh.drop()


def test_rows_up_to_the_lds_budget_are_served_and_longer_ones_refused():
    max_ld = 21728   # grouped_rerank_max_ld(): 160 KiB less the pool, the cap's images and the key lists, in floats, % 32
    rng = np.random.default_rng(31)
    n, nq = 300, 3
    labels = (np.arange(n) % 7).astype(np.uint32)
    for d, served in ((max_ld, True), (max_ld + 1, False)):
        X = rng.standard_normal((n, d)).astype(f32)
        Q = rng.standard_normal((nq, d)).astype(f32)
        s = _space("grouped-long", X, "l2")
        if served:
            got = s.knn_grouped(Q, 10, labels, per_group=2)
            _assert_rows(got, gm.expected(gm.oracle_all(X, Q, "l2"), labels, 10, 2), 10, "d=%d" % d)
        else:
            with pytest.raises(ehx.EhxError) as e:
                s.knn_grouped(Q, 10, labels, per_group=2)
            assert e.value.code == _lib.EUNSUPPORTED and "LDS" in str(e.value)
        s.drop()


@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_nan_rows_and_nan_queries(metric):
    rng = np.random.default_rng(21)
    n, d = 600, 12
    X = rng.standard_normal((n, d)).astype(f32)
    X[10, 3] = np.nan                        # a NaN distance is never a neighbour: the row neither enters nor uses up its group
    X[20:23] = X[5]                          # ties
    X[30] = f32(3e38)                        # +-Inf distances are ordered
    Q = np.stack([X[5] + f32(0.25), rng.standard_normal(d).astype(f32), np.full(d, np.nan, dtype=f32)]).astype(f32)
    labels = (np.arange(n) % 3).astype(np.uint32)      # three groups: 10, 20..22 and 30 each share one with many rows
    labels[::7] = NONE
    s = _space("grouped-nan", X, metric)
    full = gm.oracle_all(X, Q, metric)
    for k, m in ((8, 1), (8, 3), (256, 250)):
        got = s.knn_grouped(Q, k, labels, per_group=m)
        _assert_rows(got, gm.expected(full, labels, k, m), k, "NaN %s k=%d m=%d" % (metric, k, m))
        assert got[2][2] == 0 and 10 not in got[0]
    s.drop()
