"""GPU tests of the exact kNN under a label column (ehx_knn_labeled, ehx_knn_labeled_device).

Truth comes from the oracle only: for every wanted label, with L the ascending list of the rows that carry it (below n_labels
and the row count) and Q_L the queries that want it, pyoracle.exhaustive(X[L], Q_L, k) answers and its local ids are mapped
back through L.  Ids must be equal and distance BYTES equal, tails the sentinels.  F16 spaces use the oracle on
X.astype(float16).astype(float32).  Column and batches: tests/labeled_cases.py."""
import ctypes as C

import numpy as np
import pytest

import extreme_cases as xc
import labeled_cases as lbc
import masked_multi_cases as mmc
import range_cases as rc
import side_extreme_cases as sx
from test_knn_masked import METRICS, NO_ID, _assert_rows, _expected, _i8_space, _keys, _raw, _same_bytes
from test_knn_masked import _counters as _masked_counters

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402

f32 = np.float32


def _counters(s):
    out = (C.c_uint64 * 5)()
    _raw().ehx_test_labeled_counters(s._h, out)
    return np.array(list(out), dtype=np.int64)   # scan route, list route, overflowed, scan passes, calls


def _want(X, Q, k, om, col, want):
    """per query (ids, dist) of the oracle over the rows that carry its wanted label; col: labels of (a prefix of) the rows"""
    out = [None] * len(Q)
    for lab in np.unique(want):
        at = np.nonzero(want == lab)[0]
        for i, w in zip(at, _expected(X, np.ascontiguousarray(Q[at]), k, om, col == lab)):
            out[i] = w
    return out


def _cut(want, k):
    return [(ids[:k], dist[:k]) for ids, dist in want]


def _device_form(space, Q, k, col, want, n_labels=None, fill=None):
    import torch
    col = np.ascontiguousarray(col, dtype=np.uint32)
    n_labels = len(col) if n_labels is None else n_labels
    dq = torch.tensor(np.ascontiguousarray(Q, dtype=f32), device="cuda")
    dc = torch.tensor(col.view(np.int32), device="cuda") if col.size else None
    dw = torch.tensor(np.ascontiguousarray(want, dtype=np.uint32).view(np.int32), device="cuda")
    o_ids = torch.full((len(Q), k), -7, dtype=torch.int64, device="cuda")
    o_dist = torch.full((len(Q), k), -7.0, dtype=torch.float32, device="cuda")
    o_cnt = torch.full((len(Q),), 77, dtype=torch.int32, device="cuda")
    try:
        space.knn_labeled_device(dq, k, dc, n_labels, dw, o_ids, o_dist, o_cnt)
    finally:
        torch.cuda.synchronize()
        out = (o_ids.cpu().numpy().view(np.uint64), o_dist.cpu().numpy(), o_cnt.cpu().numpy().view(np.uint32))
        if fill is not None:
            fill.extend(out)
    return out


def _both_forms(s, Q, k, col, want, expect, what, n_labels=None):
    """host form against the oracle, device form byte for byte the host form's; -> (answer, counter deltas of the host call)"""
    c0 = _counters(s)
    got = s.knn_labeled(Q, k, col, want, n_labels)
    dc = _counters(s) - c0
    _assert_rows(got, expect, what)
    assert _same_bytes(got, _device_form(s, Q, k, col, want, n_labels)), what + ": host and device forms differ"
    return got, dc


# ---- 1. a mixed batch on more labels than a table of bitmaps takes ----

@pytest.mark.parametrize("rows", ["f32", "f16"])
@pytest.mark.parametrize("d", rc.I8_DIMS)
@pytest.mark.parametrize("metric", mmc.METRICS)
def test_mixed_batch_on_more_than_64_labels(metric, d, rows):
    om = METRICS[metric][1]
    X, Q = rc.i8_data(d)
    Q = Q[:lbc.NQ]
    col, want = lbc.column(), lbc.mixed_batch()
    assert len(np.unique(want)) > 64
    s = _i8_space("labeled-mixed", d, metric, X, dtype=ehx.DTYPE_F16 if rows == "f16" else ehx.DTYPE_F32)
    Xs = X.astype(np.float16).astype(f32) if rows == "f16" else X
    expect_all = _want(Xs, Q, max(lbc.KS), om, col, want)
    for k in lbc.KS:
        what = "%s d=%d %s k=%d" % (metric, d, rows, k)
        got, dc = _both_forms(s, Q, k, col, want, _cut(expect_all, k), what)
        assert (got[2][want == lbc.ABSENT] == 0).all() and (got[2][want == lbc.FEW] == k).all(), what   # ITS queries only
        assert (got[2][want == lbc.ALL_ONES] == 1).all() and (got[0][want == lbc.ALL_ONES, 0] == lbc.ALL_ONES_ROW).all(), what
        assert dc[0] + dc[1] == lbc.NQ and dc[4] == 1, (what, dc)
        if k > 48:
            assert dc[0] == 0 and dc[3] == 0, (what, dc)
    assert s.stats()["n_uncertified"] == 0
    s.drop()


# ---- 2. the same answer and the same plan as the table of bitmaps that says the same ----

@pytest.mark.parametrize("d", [128, 768])
def test_equals_knn_masked_multi_byte_for_byte_and_counter_for_counter(d):
    X, Q = rc.i8_data(d)
    Q = Q[:lbc.NQ]
    col, want = lbc.column(), lbc.table_batch()
    tab, of = lbc.as_table(col, want)
    assert len(tab) <= 64 and all((want == lab).any() for lab in lbc.DENSE)
    s = _i8_space("labeled-table", d, "cosine", X)
    for k in (10, 48):
        m0 = _masked_counters(s)
        masked = s.knn_masked_multi(Q, k, tab, of)
        dm = _masked_counters(s) - m0
        l0 = _counters(s)
        labeled = s.knn_labeled(Q, k, col, want)
        dl = _counters(s) - l0
        assert _same_bytes(masked, labeled), (d, k)
        assert dm[3] > 0 and dl.tolist() == dm.tolist(), (d, k, dl, dm)   # scanned; same routes, passes and overflows
        assert _same_bytes(masked, _device_form(s, Q, k, col, want)), (d, k)
        assert (_counters(s) - l0 - dl).tolist() == dm.tolist(), (d, k)
    s.drop()


# ---- 2b. the same wanted labels asked four ways: from the call and from a stored column, ungrouped and grouped ----

def _hook(s, name):
    out = (C.c_uint64 * 5)()
    getattr(_raw(), name)(s._h, out)
    return np.array(list(out), dtype=np.int64)


def test_one_batch_asked_four_ways_scans_and_lists_alike():
    """knn_labeled_device, knn_by_label_device on a stored copy of the column, and their grouped counterparts with every
    group EHX_GROUP_NONE and per_group 1 (a cap that caps nothing): one body (labeled_call), two views' users.  66 queries
    name scanning labels and 68 listed ones, so the grouped forms' 64-query gate opens."""
    import torch
    d, k, label_col, group_col = 64, 10, 1, 2   # (column 2 is never written: EHX_GROUP_NONE for every row)
    X, Q = rc.i8_data(d)
    col = lbc.column()
    want, scans = lbc.both_routes_batch()
    nq, n = len(want), len(X)
    Q = np.ascontiguousarray(Q[:nq])
    s = ehx.Space.unique("labeled-four-ways", d, metric=METRICS["cosine"][0], initial_capacity=n)
    s.set_batch_cols(_keys(n), X, {label_col: col})
    assert s.scan_engine() == "i8"
    dq = torch.tensor(Q, device="cuda")
    dc = torch.tensor(np.ascontiguousarray(col).view(np.int32), device="cuda")
    dg = torch.full((n,), -1, dtype=torch.int32, device="cuda")   # EHX_GROUP_NONE
    dw = torch.tensor(want.view(np.int32), device="cuda")
    assert ehx.GROUP_NONE == 0xFFFFFFFF
    forms = (("ehx_test_labeled_counters", lambda o: s.knn_labeled_device(dq, k, dc, n, dw, *o)),
             ("ehx_test_labeled_counters", lambda o: s.knn_by_label_device(dq, k, label_col, dw, *o)),
             ("ehx_test_grouped_labeled_counters", lambda o: s.knn_grouped_labeled_device(dq, k, dg, dc, n, dw, *o, per_group=1)),
             ("ehx_test_grouped_labeled_counters",
              lambda o: s.knn_grouped_by_label_device(dq, k, group_col, label_col, dw, *o, per_group=1)))
    answers, splits = [], []
    for hook, call in forms:
        o = (torch.full((nq, k), -7, dtype=torch.int64, device="cuda"), torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda"),
             torch.full((nq,), 77, dtype=torch.int32, device="cuda"))
        c0 = _hook(s, hook)
        call(o)
        torch.cuda.synchronize()
        dcnt = (_hook(s, hook) - c0).tolist()
        print(hook, dcnt)
        answers.append((o[0].cpu().numpy().view(np.uint64), o[1].cpu().numpy(), o[2].cpu().numpy().view(np.uint32)))
        splits.append(dcnt[:2])
        assert dcnt[4] == 1, (hook, dcnt)
    _assert_rows(answers[0], _want(X, Q, k, METRICS["cosine"][1], col, want), "four ways")
    assert _same_bytes(answers[0], answers[1]), "knn_labeled_device and knn_by_label_device differ"
    assert _same_bytes(answers[2], answers[3]), "the grouped forms differ"
    assert _same_bytes(answers[0], answers[2]), "the grouped answer differs from the kNN's"
    assert splits == [[int(scans.sum()), int((~scans).sum())]] * 4, splits   # 66 on the scan route, 68 on the lists
    s.drop()


# ---- 3. no query is judged by another query's label ----

@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_no_query_is_judged_by_another_query_s_label(metric):
    """masked_multi_cases.parity: every vector stored at rows 2 j and 2 j + 1, the label the row's parity, queries alternating —
    the wrong label shows as an id of the wrong parity at the right distance"""
    om = METRICS[metric][1]
    X, Q, _, of = mmc.parity()
    col = (np.arange(len(X)) % 2).astype(np.uint32)
    s = _i8_space("labeled-parity", X.shape[1], metric, X)
    for k in mmc.KS:
        what = "parity %s k=%d" % (metric, k)
        got, dc = _both_forms(s, Q, k, col, of, _want(X, Q, k, om, col, of), what)
        assert (got[2] == k).all() and ((got[0] % np.uint64(2)) == of[:, None].astype(np.uint64)).all(), what
        assert dc[0] + dc[1] == len(Q) and dc[4] == 1, (what, dc)
    s.drop()


# ---- 4. more queries than one device batch ----

def test_two_device_batches():
    metric, d, k = "cosine", 128, 10
    om = METRICS[metric][1]
    X, Q0 = rc.i8_data(d)
    col, want = lbc.column(), lbc.two_batches()
    Q = np.ascontiguousarray(Q0[np.arange(len(want)) % len(Q0)])
    assert len(Q) == lbc.SIDE_CHUNK + 64
    s = _i8_space("labeled-two", d, metric, X)
    got, dc = _both_forms(s, Q, k, col, want, _want(X, Q, k, om, col, want), "two batches")
    assert dc[0] + dc[1] == len(Q) and dc[4] == 1, dc
    assert s.stats()["n_uncertified"] == 0
    s.drop()


# ---- 5. rows the column does not cover ----

def test_n_labels_below_the_row_count_and_not_a_multiple_of_256():
    metric, d, nl = "cosine", 128, 15003
    om = METRICS[metric][1]
    X, Q = rc.i8_data(d)
    Q = Q[:lbc.NQ]
    col, want = lbc.column(), lbc.mixed_batch()
    assert nl % 256 and nl < len(X)
    s = _i8_space("labeled-prefix", d, metric, X)
    for k in (10, 48):
        what = "n_labels=%d k=%d" % (nl, k)
        got, dc = _both_forms(s, Q, k, col, want, _want(X, Q, k, om, col[:nl], want), what, n_labels=nl)
        assert (got[0][got[0] != NO_ID] < nl).all() and (got[2][want == lbc.LAST] == 0).all(), what
        assert _same_bytes(got, s.knn_labeled(Q, k, col[:nl], want)), what + ": a shorter column"
    s.drop()


def test_rows_appended_after_the_column_was_built_never_appear():
    metric, d, k = "l2", 128, 10
    om = METRICS[metric][1]
    X, Q = rc.i8_data(d)
    Q = Q[:lbc.NQ]
    n0, n1 = 19300, rc.I8_ROWS
    want = lbc.mixed_batch()
    built = lbc.column()[:n0]                                     # the column as it was while the space held n0 rows
    s = _i8_space("labeled-append", d, metric, X[:n0], cap=n1)
    expect = _want(X[:n0], Q, k, om, built, want)
    before, _ = _both_forms(s, Q, k, built, want, expect, "before the append")
    s.set_batch(_keys(n1 - n0, n0), Q[np.arange(n1 - n0) % lbc.NQ])   # the queries themselves: nearer than any old row
    after, _ = _both_forms(s, Q, k, built, want, expect, "after the append")
    assert _same_bytes(before, after) and (after[0][after[0] != NO_ID] < n0).all()
    grown = np.concatenate([built, np.full(n1 - n0, 99, dtype=np.uint32)])   # ... a longer column finds them
    ids = s.knn_labeled(Q, 1, grown, np.full(lbc.NQ, 99, dtype=np.uint32))[0]
    assert (ids[:, 0] >= n0).all()
    s.drop()


# ---- 6. spaces off the int8 engine ----

@pytest.mark.parametrize("kind", ["flat_f32", "flat_f16", "graph_f32"])
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_small_and_graph_spaces_answer_from_their_stored_rows(metric, kind):
    em, om = METRICS[metric]
    n, d, nq = 3000, 24, 21
    rng = np.random.default_rng(410)
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    kw = {"mode": ehx.MODE_GRAPH, "M": 16} if kind == "graph_f32" else {}
    s = ehx.Space.unique("labeled-small", d, metric=em, initial_capacity=n,
                         dtype=ehx.DTYPE_F16 if kind == "flat_f16" else ehx.DTYPE_F32, **kw)
    s.set_batch(_keys(n), X)
    Xs = X.astype(np.float16).astype(f32) if kind == "flat_f16" else X
    col = np.where(rng.random(n) < 0.5, 1, 2 + rng.integers(0, 30, size=n)).astype(np.uint32)
    col[77] = lbc.ALL_ONES
    want = np.array([1] * 9 + [lbc.ALL_ONES, 999] + [2 + i for i in range(10)], dtype=np.uint32)[::-1].copy()
    for k in (1, 10, 100):
        got, dc = _both_forms(s, Q, k, col, want, _want(Xs, Q, k, om, col, want), "%s %s k=%d" % (kind, metric, k))
        assert dc.tolist() == [0, nq, 0, 0, 1], dc
    s.drop()


# ---- 7. values ----

@pytest.mark.parametrize("kind", ["g", "f"])
@pytest.mark.parametrize("metric", sx.METRICS)
def test_non_finite_rows_and_zero_rows(kind, metric):
    """side_extreme_cases.ladder: ordinary rows and a block of rows with one NaN / -NaN / +Inf / -Inf component (g: the space
    stays on the exact kernels) or of zero rows (f: an int8 space, the scan route); the rows — the block's too — split
    between two labels by parity, 300 rows outside the block on a third, and a label nobody carries"""
    em, om = METRICS[metric]
    X, Q = sx.ladder(kind, metric)
    n = len(X)
    rng = np.random.default_rng(77)
    col = (20 + np.arange(n) % 2).astype(np.uint32)
    outside = np.r_[0:xc.BLOCK0, xc.BLOCK0 + xc.NBLOCK:n]
    col[rng.choice(outside, size=300, replace=False)] = 30
    block = col[xc.BLOCK0:xc.BLOCK0 + xc.NBLOCK]
    assert (block == 20).sum() == (block == 21).sum() == xc.NBLOCK // 2
    want = np.array([20, 21, 30, 40], dtype=np.uint32)[np.arange(len(Q)) % 4]
    s = ehx.Space.unique("labeled-%s" % kind, X.shape[1], metric=em, initial_capacity=n)
    s.set_batch(_keys(n), X)
    assert s.scan_engine() == ("i8" if kind == "f" else "f32")
    for k in sx.MASKED_KS:
        what = "ladder %s %s k=%d" % (kind, metric, k)
        got, dc = _both_forms(s, Q, k, col, want, _want(X, Q, k, om, col, want), what)
        assert dc[0] + dc[1] == len(Q) and dc[4] == 1, (what, dc)
        if kind == "g":
            assert dc.tolist() == [0, len(Q), 0, 0, 1], (what, dc)
    assert s.stats()["n_uncertified"] == 0
    s.drop()


# ---- 8. no answer depends on the order of the queries or of a short list's rows ----

def test_the_answer_does_not_depend_on_the_order_of_the_queries():
    d = 128
    X, Q = rc.i8_data(d)
    Q = Q[:lbc.NQ]
    col, want = lbc.column(), lbc.mixed_batch()
    perm = np.random.default_rng(12).permutation(lbc.NQ)
    s = _i8_space("labeled-order", d, "cosine", X)
    for k in (10, 60):
        once = s.knn_labeled(Q, k, col, want)
        assert _same_bytes(once, s.knn_labeled(Q, k, col, want)), k
        moved = s.knn_labeled(np.ascontiguousarray(Q[perm]), k, col, want[perm])
        back = [np.empty_like(a) for a in moved]
        for a, b in zip(moved, back):
            b[perm] = a
        assert _same_bytes(once, back), k
    s.drop()


# ---- 9. errors and accounting ----

def test_error_returns():
    rng = np.random.default_rng(8)
    n, d, nq = 200, 8, 3
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    col = (np.arange(n) % 3).astype(np.uint32)
    want = np.array([0, 1, 5], dtype=np.uint32)
    s = ehx.Space.unique("labeled-err", d, metric=ehx.METRIC_L2SQ, initial_capacity=n)
    s.set_batch(_keys(n), X)
    for k, code in ((0, _lib.EINVAL), (1025, _lib.EUNSUPPORTED)):
        with pytest.raises(ehx.EhxError) as e:
            s.knn_labeled(Q, k, col, want)
        assert e.value.code == code
        with pytest.raises(ehx.EhxError) as e:
            _device_form(s, Q, k, col, want)
        assert e.value.code == code
    ids, dist, cnt = s.knn_labeled(np.zeros((0, d), dtype=f32), 4, col, np.zeros(0, dtype=np.uint32))   # no queries
    assert ids.shape == (0, 4) and cnt.shape == (0,)
    assert (s.knn_labeled(Q, 4, col[:0], want)[2] == 0).all()                                            # no labels
    assert (_device_form(s, Q, 4, col[:0], want)[2] == 0).all()
    assert s.knn_labeled(Q, 4, col, want)[2].tolist() == [4, 4, 0]                                       # ITS queries only
    with pytest.raises(ValueError):
        s.knn_labeled(Q, 4, col, want[:2])
    L = _lib.load()
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    q = np.ascontiguousarray(Q)
    o_ids, o_dist, o_cnt = np.full((nq, 4), 7, dtype=np.uint64), np.full((nq, 4), 7, dtype=f32), np.full(nq, 7, dtype=np.uint32)
    args = [P(o_ids, C.c_uint64), P(o_dist, C.c_float), P(o_cnt, C.c_uint32)]
    call = lambda a_q, a_c, a_w, a: L.ehx_knn_labeled(s._h, nq, a_q, 4, a_c, n, a_w, a[0], a[1], a[2])  # noqa: E731
    for hole in range(3):
        a = list(args)
        a[hole] = None
        assert call(P(q, C.c_float), P(col, C.c_uint32), P(want, C.c_uint32), a) == _lib.EINVAL
    assert call(None, P(col, C.c_uint32), P(want, C.c_uint32), args) == _lib.EINVAL
    assert call(P(q, C.c_float), None, P(want, C.c_uint32), args) == _lib.EINVAL        # NULL label_of with n_labels > 0
    assert call(P(q, C.c_float), P(col, C.c_uint32), None, args) == _lib.EINVAL         # NULL want
    assert (o_ids == 7).all() and (o_dist == 7).all() and (o_cnt == 7).all()
    assert L.ehx_knn_labeled(None, nq, P(q, C.c_float), 4, P(col, C.c_uint32), n, P(want, C.c_uint32), *args) == _lib.EINVAL
    assert L.ehx_last_error() == b"space is NULL"
    assert L.ehx_knn_labeled_device(None, None, nq, None, 4, None, n, None, None, None, None) == _lib.EINVAL
    assert L.ehx_last_error() == b"space is NULL"
    assert L.ehx_knn_labeled_device(s._h, None, nq, None, 4, None, n, None, None, None, None) == _lib.EINVAL
    assert call(P(q, C.c_float), P(col, C.c_uint32), P(want, C.c_uint32), args) == _lib.OK and o_cnt.tolist() == [4, 4, 0]
    h = s._h
    s.drop()   # the tombstone answers for the dropped handle
    assert L.ehx_knn_labeled(h, nq, P(q, C.c_float), 4, P(col, C.c_uint32), n, P(want, C.c_uint32), *args) == _lib.ENOTFOUND
    assert L.ehx_knn_labeled_device(h, None, nq, P(q, C.c_float), 4, P(col, C.c_uint32), n, P(want, C.c_uint32),
                                    *args) == _lib.ENOTFOUND
    sh = ehx.Space.unique("labeled-sh", d, metric=ehx.METRIC_L2SQ, shards=2)
    sh.set_batch(_keys(n), X)
    with pytest.raises(ehx.EhxError) as e:
        sh.knn_labeled(Q, 4, col, want)
    assert e.value.code == _lib.EUNSUPPORTED and "sharded" in str(e.value)
    with pytest.raises(ehx.EhxError) as e:
        _device_form(sh, Q, 4, col, want)
    assert e.value.code == _lib.EUNSUPPORTED and "sharded" in str(e.value)
    sh.drop()


def test_stats_deltas_on_the_list_route():
    rng = np.random.default_rng(9)
    n, d, nq = 1000, 16, 24
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    col = rng.integers(0, 7, size=n).astype(np.uint32)
    want = np.array([0] * 10 + [1, 2, 3, 4, 5, 6, 99] * 2, dtype=np.uint32)   # a shared list, per-query lists, an absent label
    s = ehx.Space.unique("labeled-stats", d, metric=ehx.METRIC_L2SQ, initial_capacity=n)
    s.set_batch(_keys(n), X)
    st0, c0 = s.stats(), _counters(s)
    s.knn_labeled(Q, 5, col, want)
    st1, dc = s.stats(), _counters(s) - c0   # every query against every row that carries its label
    assert dc.tolist() == [0, nq, 0, 0, 1], dc
    assert st1["n_queries"] - st0["n_queries"] == nq
    assert st1["n_dist"] - st0["n_dist"] == sum(int((col == w).sum()) for w in want)
    assert st1["n_rerank"] == st0["n_rerank"] and st1["n_uncertified"] == 0
    s.drop()
