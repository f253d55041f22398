"""GPU tests of the grouped kNN under row bitmaps (ehx_knn_grouped_masked*, ehx_groupedm.cpp, k_grouped.hip): FILTER FIRST,
THEN CAP — the first k eligible rows among the rows a query's bitmap allows — on the scan route (the falling-radius int8
scan, the bitmaps in its flush, a cap per label in its re-rank, the first radius from a sample of the allowed rows) and on
the list route (every allowed row in slabs of 4096 drawn from the bitmap's compacted list).

Expected answers come from the oracle's distances of every prefix row (grouped_model.oracle_all), the rows that are not
allowed dropped, capped by the plain-Python greedy (tests/grouped_masked_model.py): ids equal, distance BYTES equal, sentinels
behind the count.  The scan cases that assert "none handed on" are the ones tests/test_grouped_masked_model.py clears."""
import ctypes as C

import numpy as np
import pytest

import grouped_masked_model as gmm
import grouped_model as gm
import largek_cases as lc

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402
from embeddinghub_amd.space import marshal_groups, marshal_mask_table  # noqa: E402

EM = {"l2": ehx.METRIC_L2SQ, "ip": ehx.METRIC_IP, "cosine": ehx.METRIC_COSINE}
NO_ID = np.uint64(2**64 - 1)
NONE = gm.NONE
f32 = np.float32
PASSES = 3   # of a prefix of 16 385 .. 65 536 rows at the default growth


def _keys(n, first=0):
    return ["k%d" % i for i in range(first, first + n)]


def _hook(s, name):
    out = (C.c_uint64 * 5)()
    getattr(C.CDLL(_lib.LIB_PATH), name)(s._h, out)
    return np.array(list(out), dtype=np.int64)


def _counters(s):
    return _hook(s, "ehx_test_grouped_masked_counters")   # on the scan route, on the list route, of those overflowed, passes, calls


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


def _device_form(space, Q, k, labels, allows, mask_of, per_group, n_labels=None, n_bits=None, own_stream=False):
    import torch
    g, n = marshal_groups(labels)
    n = n if n_labels is None else n_labels
    words, n_masks, nb = marshal_mask_table(np.atleast_2d(np.asarray(allows)), n_bits)
    dq = torch.tensor(np.ascontiguousarray(Q, dtype=f32), device="cuda")
    dg = torch.tensor(g.view(np.int32), device="cuda") if len(g) else None
    dm = torch.tensor(words.view(np.int32), device="cuda") if words.size else None
    dof = None if mask_of is None else torch.tensor(np.asarray(mask_of, dtype=np.uint32).view(np.int32), device="cuda")
    o_ids = torch.full((len(Q), k), -7, dtype=torch.int64, device="cuda")
    o_dist = torch.full((len(Q), k), -7.0, dtype=torch.float32, device="cuda")
    o_cnt = torch.full((len(Q),), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream() if own_stream else None
    space.knn_grouped_masked_device(dq, k, dg, n, dm, n_masks, nb, dof, o_ids, o_dist, o_cnt, per_group=per_group,
                                    stream=st.cuda_stream if st else None)
    torch.cuda.synchronize()
    return (o_ids.cpu().numpy().view(np.uint64), o_dist.cpu().numpy(), o_cnt.cpu().numpy().view(np.uint32))


# ---- 1. the list route, every layout ----

@pytest.mark.parametrize("kind", ["flat_f32", "flat_f16", "graph_f32"])
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
@pytest.mark.parametrize("d", [7, 129, 650])
def test_list_route_every_layout(d, metric, kind):
    n, nq = 700, 5
    rng = np.random.default_rng(2000 + d)
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    allows = np.stack([rng.random(n) < 0.5, rng.random(n) < 0.05, np.zeros(n, dtype=bool)])
    mask_of = (np.arange(nq) % 3).astype(np.uint32)
    kw = {"mode": ehx.MODE_GRAPH, "M": 16} if kind == "graph_f32" else {}
    s = _space("groupedm-small", X, metric, dtype=ehx.DTYPE_F16 if kind == "flat_f16" else ehx.DTYPE_F32, **kw)
    Xs = X.astype(np.float16).astype(f32) if kind == "flat_f16" else X   # the oracle reads the rows as stored
    full = gm.oracle_all(Xs, Q, metric)
    labels = gm.labels_mod37(n)
    for k in (10, 100):
        for m in (1, 3):
            c0 = _counters(s)
            got = s.knn_grouped_masked(Q, k, labels, allows, mask_of, per_group=m)
            what = "%s %s d=%d k=%d m=%d" % (kind, metric, d, k, m)
            _assert_rows(got, gmm.expected(full, labels, allows, mask_of, k, m), k, what)
            assert (_counters(s) - c0).tolist() == [0, nq, 0, 0, 1], what
            assert got[2][2] == 0 and (got[0][2] == NO_ID).all() and np.isposinf(got[1][2]).all()   # the empty bitmap's query
            assert got[2][0] > 0 and got[2][3] > 0                                               # ... and only its
    assert _same_bytes(got, _device_form(s, Q, 100, labels, allows, mask_of, 3, own_stream=True))
    s.drop()


# ---- 2. slab edges of a LIST ----

@pytest.mark.parametrize("n_long", [8193, 4097])
def test_slab_edges_of_a_list(n_long):
    n, d, nq, n_short = 9000, 16, 5, 4095
    rng = np.random.default_rng(n_long)
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    Q[1] = Q[0]                                                       # the same point under the shorter list
    long_ids = np.sort(rng.choice(n, size=n_long, replace=False))
    # group 7 around query 0, at LIST positions: the last (the LAST slab) nearest, then 5, 6, 4090 (the first slab), then 4096
    # (or 4095 where 4096 is the last)
    near = [int(long_ids[p]) for p in (n_long - 1, 5, 6, 4090, min(4096, n_long - 2))]
    for j, r in enumerate(near):
        X[r] = Q[0]
        X[r, 0] += f32(0.01 * (j + 1))
    rest = np.setdiff1d(np.arange(n), near)
    short_ids = np.sort(np.concatenate([near, rng.choice(rest, size=n_short - len(near), replace=False)]))
    allows = np.zeros((2, n), dtype=bool)
    allows[0, long_ids] = True
    allows[1, short_ids] = True
    assert allows.sum(axis=1).tolist() == [n_long, n_short]           # lists that end in different slabs of one batch
    mask_of = np.array([0, 1, 0, 1, 0], dtype=np.uint32)
    labels = (100 + np.arange(n) % 37).astype(np.uint32)
    labels[::11] = NONE
    labels[near] = 7
    s = _space("groupedm-slab", X, "l2")
    full = gm.oracle_all(X, Q, "l2")
    assert [int(v) for v in full[0][0, :5]] == near
    for k in (4, 10, 256):
        for m in (1, 2, 3):
            c0 = _counters(s)
            got = s.knn_grouped_masked(Q, k, labels, allows, mask_of, per_group=m)
            assert (_counters(s) - c0).tolist() == [0, nq, 0, 0, 1]
            _assert_rows(got, gmm.expected(full, labels, allows, mask_of, k, m), k, "long=%d k=%d m=%d" % (n_long, k, m))
            # the first m of group 7 straddle the slab edges of the LIST; the keys carried from the first slab are displaced
            for q in (0, 1):   # (query 1 runs its later passes with an empty pool)
                assert [int(v) for v in got[0][q, :m]] == near[:m] and near[m] not in got[0][q]
    s.drop()


# ---- 3. filter before cap ----

def test_filter_before_cap():
    n, d, k = 700, 24, 37   # k = the number of groups: every group is represented, whatever is forbidden
    rng = np.random.default_rng(33)
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((3, d)).astype(f32)
    labels = (np.arange(n) % 37).astype(np.uint32)
    s = _space("groupedm-filter", X, "l2")
    full = gm.oracle_all(X, Q, "l2")
    plain = s.knn_grouped(Q, k, labels, per_group=1)
    allow = np.ones(n, dtype=bool)
    hit = [int(r) for r in plain[0][0, [0, 2, 5]]]                    # the rows that represent three groups for query 0
    allow[hit] = False
    got = s.knn_grouped_masked(Q, k, labels, allow, per_group=1)
    _assert_rows(got, gmm.expected(full, labels, allow, None, k, 1), k, "filter before cap")
    order = [int(v) for v in full[0][0]]
    for r in hit:                                                     # each group by its nearest ALLOWED row
        second = next(x for x in order if labels[x] == labels[r] and allow[x])
        assert second in got[0][0] and r not in got[0][0]
    assert (got[2] == k).all()
    # grouped search first, forbidden rows dropped on the host: the three groups are lost
    host = [int(v) for v in plain[0][0] if allow[int(v)]]
    assert len(host) == k - 3 and host != [int(v) for v in got[0][0]]
    assert not np.array_equal(got[0][0], plain[0][0])
    s.drop()


# ---- 4. the scan route ----

@pytest.mark.parametrize("lab", sorted(gm.LABELINGS))
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_scan_route(metric, lab):
    X, Q = lc.gauss(20000, 64, 64, 1)
    full = gm.scan_oracle(metric)
    labels = gm.LABELINGS[lab](len(X))
    mask_of = gmm.scan_mask_of(len(Q))
    s = _i8_space("groupedm-scan", X, metric)
    for density, _, k, m in (c for c in gmm.scan_cases() if c[1] == lab):
        allows = gmm.scan_bitmaps(density)
        c0, st0 = _counters(s), s.stats()
        got = s.knn_grouped_masked(Q, k, labels, allows, mask_of, per_group=m)
        dc, st1 = _counters(s) - c0, s.stats()
        what = "%s %s density %g k=%d m=%d" % (metric, lab, density, k, m)
        print(what, dc.tolist())
        _assert_rows(got, gmm.expected(full, labels, allows, mask_of, k, m), k, what)
        assert gmm.cleared(density, lab, k, m)   # (the model leaves no case out)
        assert dc.tolist() == [64, 0, 0, PASSES, 1], (what, dc)
        assert st1["n_queries"] - st0["n_queries"] == 64, what
        assert st1["n_i8_queries"] - st0["n_i8_queries"] == 64 and st1["n_i8_fallback"] == st0["n_i8_fallback"], what
        assert st1["n_dist"] > st0["n_dist"]
    assert _same_bytes(got, _device_form(s, Q, k, labels, allows, mask_of, m, own_stream=True))
    s.drop()


# ---- 5. equivalences ----

def test_equivalences():
    X, Q = lc.gauss(20000, 64, 64, 1)
    n = len(X)
    full = gm.scan_oracle("cosine")
    labels = gm.labels_scattered(n)
    none = np.full(n, NONE, dtype=np.uint32)
    allows, mask_of = gmm.scan_bitmaps(0.5), gmm.scan_mask_of(len(Q))
    ones = np.ones((2, n), dtype=bool)
    s = _i8_space("groupedm-eq", X, "cosine")
    # every bit set: the grouped kNN
    for k, m in ((10, 1), (100, 4)):
        c0 = _counters(s)
        got = s.knn_grouped_masked(Q, k, labels, ones, mask_of % 2, per_group=m)
        assert (_counters(s) - c0)[:2].sum() == 64
        assert _same_bytes(got, s.knn_grouped(Q, k, labels, per_group=m)), (k, m)
        assert _same_bytes(s.knn_grouped_masked(Q[:5], k, labels, ones[0], per_group=m), s.knn_grouped(Q[:5], k, labels, per_group=m))
    # every label NONE, or per_group at least the largest group (clustered: ten rows): the kNN under the table
    for k in (10, 100):
        table = s.knn_masked_multi(Q, k, allows, mask_of)
        for lb, m in ((none, 1), (gm.labels_clustered(n), 10), (labels, 2 ** 32 - 1)):
            c0 = _counters(s)
            got = s.knn_grouped_masked(Q, k, lb, allows, mask_of, per_group=m)
            assert (_counters(s) - c0)[:2].sum() == 64
            assert _same_bytes(got, table), (k, m)
    # one bitmap with no mask_of: the table of one
    for q in (Q, Q[:5]):
        one = s.knn_grouped_masked(q, 10, labels, allows[1], per_group=2)
        assert _same_bytes(one, s.knn_grouped_masked(q, 10, labels, allows[1:2], np.zeros(len(q), dtype=np.uint32), per_group=2))
        assert _same_bytes(one, _device_form(s, q, 10, labels, allows[1], None, 2))
        _assert_rows(one, gmm.expected(full, labels, allows[1], None, 10, 2)[:len(q)], 10, "one bitmap, nq=%d" % len(q))
    # the prefix is min(rows, labels, bits): rows at or above the smaller limit never appear
    for n_labels, n_bits in ((15000, 18000), (18000, 15000)):
        got = s.knn_grouped_masked(Q, 10, labels[:n_labels], allows[:, :n_bits], mask_of, per_group=1)
        lim = min(n_labels, n_bits)
        _assert_rows(got, gmm.expected(full, labels[:n_labels], allows[:, :n_bits], mask_of, 10, 1), 10,
                     "n_labels=%d n_bits=%d" % (n_labels, n_bits))
        assert (got[0][got[0] != NO_ID] < lim).all() and (got[2] == 10).all()
        assert _same_bytes(got, _device_form(s, Q, 10, labels, allows, mask_of, 1, n_labels=n_labels, n_bits=n_bits))
    s.drop()


# ---- 6. handed on ----

def test_a_sample_without_k_groups_hands_every_query_on_under_its_own_bitmap():
    X, Q = lc.gauss(20000, 64, 64, 1)
    full = gm.scan_oracle("l2")
    labels = (np.arange(len(X)) % 5).astype(np.uint32)
    allows, mask_of = gmm.scan_bitmaps(0.5), gmm.scan_mask_of(len(Q))
    s = _i8_space("groupedm-handed", X, "l2")
    c0, st0 = _counters(s), s.stats()
    got = s.knn_grouped_masked(Q, 10, labels, allows, mask_of, per_group=1)
    dc, st1 = _counters(s) - c0, s.stats()
    # five groups exist: no sample reaches k = 10 capped rows, the radius stays +Inf, the bound serves no query
    assert dc.tolist() == [0, 64, 0, PASSES, 1], dc
    assert (got[2] == 5).all()
    _assert_rows(got, gmm.expected(full, labels, allows, mask_of, 10, 1), 10, "handed on")
    assert st1["n_queries"] - st0["n_queries"] == 64 and st1["n_i8_fallback"] - st0["n_i8_fallback"] == 64
    s.drop()


# ---- 7. errors ----

def test_error_returns():
    rng = np.random.default_rng(8)
    n, d = 200, 8
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((3, d)).astype(f32)
    labels = (np.arange(n) % 5).astype(np.uint32)
    allow = np.ones(n, dtype=bool)
    table = np.ones((2, n), dtype=bool)
    s = _space("groupedm-err", X, "l2")
    for k, m, code in ((0, 1, _lib.EINVAL), (4, 0, _lib.EINVAL), (257, 1, _lib.EUNSUPPORTED)):
        with pytest.raises(ehx.EhxError) as e:
            s.knn_grouped_masked(Q, k, labels, allow, per_group=m)
        assert e.value.code == code
    with pytest.raises(ehx.EhxError) as e:
        s.knn_grouped_masked(Q, 4, labels, np.ones((65, n), dtype=bool), [0, 1, 64])
    assert e.value.code == _lib.EUNSUPPORTED
    ids, dist, cnt = s.knn_grouped_masked(np.zeros((0, d), dtype=f32), 4, labels, allow)   # no queries: EHX_OK
    assert ids.shape == (0, 4) and cnt.shape == (0,)
    got = s.knn_grouped_masked(Q, 256, labels, allow, per_group=1)                          # k = 256 is served; five groups exist
    assert (got[2] == 5).all()
    L = _lib.load()
    q = np.ascontiguousarray(Q)
    words, n_masks, n_bits = marshal_mask_table(table)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731

    def fresh():
        return np.full((3, 4), 7, dtype=np.uint64), np.full((3, 4), 7, dtype=f32), np.full(3, 7, dtype=np.uint32)

    def untouched(o):
        return (o[0] == 7).all() and (o[1] == 7).all() and (o[2] == 7).all()

    def call(o, k=4, m=1, lb=labels, nl=n, mk=words, nm=n_masks, nb=n_bits, of=np.array([0, 1, 0], dtype=np.uint32), qq=q):
        return L.ehx_knn_grouped_masked(s._h, 3, P(qq, C.c_float) if qq is not None else None, k, m,
                                        P(lb, C.c_uint32) if lb is not None else None, nl,
                                        P(mk, C.c_uint32) if mk is not None else None, nm, nb,
                                        P(of, C.c_uint32) if of is not None else None,
                                        P(o[0], C.c_uint64), P(o[1], C.c_float), P(o[2], C.c_uint32))
    # EHX_EINVAL with the outputs unwritten: k or per_group 0, no bitmap with queries, a mask_of entry at or above n_masks
    for kw in ({"k": 0}, {"m": 0}, {"nm": 0}, {"of": np.array([0, 2, 0], dtype=np.uint32)}, {"of": None}, {"lb": None},
               {"mk": None}, {"qq": None}):
        o = fresh()
        assert call(o, **kw) == _lib.EINVAL and untouched(o), kw
    o = fresh()
    assert call(o, nm=65) == _lib.EUNSUPPORTED and untouched(o)
    assert call(o, k=257) == _lib.EUNSUPPORTED and untouched(o)
    for hole in range(3):
        o = fresh()
        a = [P(o[0], C.c_uint64), P(o[1], C.c_float), P(o[2], C.c_uint32)]
        a[hole] = None
        assert L.ehx_knn_grouped_masked(s._h, 3, P(q, C.c_float), 4, 1, P(labels, C.c_uint32), n, P(words, C.c_uint32), 2, n,
                                        P(np.zeros(3, dtype=np.uint32), C.c_uint32), *a) == _lib.EINVAL
    o = fresh()
    assert call(o, nm=1, of=None) == _lib.OK and (o[2] == 4).all()           # one bitmap: mask_of may be NULL
    assert call(o) == _lib.OK and (o[2] == 4).all()
    assert call(o, lb=None, nl=0) == _lib.OK and (o[2] == 0).all()           # no label, or no bit: nothing is searched
    assert call(o, mk=None, nb=0) == _lib.OK and (o[2] == 0).all()
    # the device form reads mask_of back and checks it before anything writes the outputs
    import torch
    dq = torch.tensor(q, device="cuda")
    dg = torch.tensor(labels.view(np.int32), device="cuda")
    dm = torch.tensor(words.view(np.int32), device="cuda")
    o_ids = torch.full((3, 4), -7, dtype=torch.int64, device="cuda")
    o_dist = torch.full((3, 4), -7.0, dtype=torch.float32, device="cuda")
    o_cnt = torch.full((3,), 77, dtype=torch.int32, device="cuda")
    bad = torch.tensor(np.array([0, 2, 1], dtype=np.int32), device="cuda")
    with pytest.raises(ehx.EhxError) as e:
        s.knn_grouped_masked_device(dq, 4, dg, n, dm, 2, n, bad, o_ids, o_dist, o_cnt)
    torch.cuda.synchronize()
    assert e.value.code == _lib.EINVAL
    assert (o_ids == -7).all() and (o_dist == -7.0).all() and (o_cnt == 77).all()
    with pytest.raises(ehx.EhxError) as e:
        s.knn_grouped_masked_device(dq, 4, dg, n, dm, 2, n, None, o_ids, o_dist, o_cnt)   # a table needs mask_of
    assert e.value.code == _lib.EINVAL
    assert L.ehx_knn_grouped_masked(None, 3, P(q, C.c_float), 4, 1, P(labels, C.c_uint32), n, P(words, C.c_uint32), 2, n,
                                    None, None, None, None) == _lib.EINVAL
    assert L.ehx_last_error() == b"space is NULL"
    h = s._h
    s.drop()   # the tombstone answers for the dropped handle
    o = fresh()
    assert L.ehx_knn_grouped_masked(h, 3, P(q, C.c_float), 4, 1, P(labels, C.c_uint32), n, P(words, C.c_uint32), 2, n,
                                    P(np.zeros(3, dtype=np.uint32), C.c_uint32), P(o[0], C.c_uint64), P(o[1], C.c_float),
                                    P(o[2], C.c_uint32)) == _lib.ENOTFOUND
    e0 = ehx.Space.unique("groupedm-empty", d, metric=ehx.METRIC_L2SQ)
    got = e0.knn_grouped_masked(Q, 4, labels, allow)
    assert (got[2] == 0).all() and (got[0] == NO_ID).all() and np.isposinf(got[1]).all()
    e0.drop()
    sh = ehx.Space.unique("groupedm-sh", d, metric=ehx.METRIC_L2SQ, shards=2)
    sh.set_batch(_keys(n), X)
    with pytest.raises(ehx.EhxError) as e:
        sh.knn_grouped_masked(Q, 4, labels, allow)
    assert e.value.code == _lib.EUNSUPPORTED and "sharded" in str(e.value)
    sh.drop()


def test_rows_too_long_are_refused():
    max_ld = 21728   # grouped_rerank_max_ld()
    rng = np.random.default_rng(31)
    n, nq = 40, 2
    X = rng.standard_normal((n, max_ld + 1)).astype(f32)
    Q = rng.standard_normal((nq, max_ld + 1)).astype(f32)
    s = _space("groupedm-long", X, "l2")
    with pytest.raises(ehx.EhxError) as e:
        s.knn_grouped_masked(Q, 10, np.arange(n) % 7, np.ones(n, dtype=bool), per_group=2)
    assert e.value.code == _lib.EUNSUPPORTED and "LDS" in str(e.value)
    s.drop()
