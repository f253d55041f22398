"""GPU tests of the Boolean filters on stored columns (ehx_knn_filter*, ehx_knn_grouped_filter*, ehx_range_filter*,
ehx_graph_knn_filter*) and of the kernel that builds their bitmaps (k_filter.hip, through the hook ehx_test_filter_bitmaps).

The bitmaps are checked against numpy (filter_cases: OR of clauses, unsigned compares and membership, a column never written
reading as 0xFFFFFFFF).  The kNN answers against the oracle as tests/test_where.py takes its truth — pyoracle.exhaustive over the
rows numpy allows, ids equal and distance BYTES equal, tails the sentinels — and, byte for byte and counter for counter, against
the bitmap forms given the numpy bitmaps; the grouped answers against the model tests/test_knn_grouped_masked.py uses; the graph
walk against ehx_graph_knn_masked_multi on the same space.  Filters and their counts: tests/filter_cases.py.  The sets are
handed to the library UNPACKED (pack=False) wherever the kernel's result is judged, so the sorting is the library's own."""
import ctypes as C
import threading

import numpy as np
import pytest

import column_cases as cc
import filter_cases as fc
import grouped_masked_model as gmm
import grouped_model as gm
import masked_multi_cases as mmc
import range_cases as rc
import where_cases as wc
from oracle import pyoracle
from test_knn_grouped_masked import _assert_rows as _assert_grouped_rows
from test_knn_masked import METRICS, NO_ID, _assert_rows, _i8_space, _keys, _same_bytes
from test_knn_masked_multi import _cut, _want
from test_where import _built as _where_built, _device_args, _hook5, _host, _masked_counters, _stored, _torch_outputs

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402
from embeddinghub_amd.space import FilterTable, marshal_filter_table, marshal_filters  # noqa: E402

f32 = np.float32
NONE = fc.NONE
A, B, CC, NEVER = fc.A, fc.B, fc.CC, fc.NEVER
ROUTES = (ehx.WALK_GRAPH, ehx.WALK_EXACT, ehx.WALK_AUTO)


def _raw():
    return C.CDLL(_lib.LIB_PATH)


def _unpacked(filters):
    return filters if isinstance(filters, FilterTable) else marshal_filters(filters, pack=False)


def _built(s, filters):
    """the builder alone -> (words u32 [n_filters, ceil(n / 32)], the snapshot n)"""
    ft = _unpacked(filters)
    rows = len(s)
    words = np.full((ft.n_filters, max((rows + 31) // 32, 1)), 0xA5A5A5A5, dtype=np.uint32)
    got_n = C.c_uint64(12345)
    L = _raw()
    L.ehx_test_filter_bitmaps.restype = C.c_int
    rc_ = L.ehx_test_filter_bitmaps(s._h, C.byref(ft.struct), words.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(got_n))
    assert rc_ == 0, "ehx_test_filter_bitmaps: %d %s" % (rc_, _lib.load().ehx_last_error())
    return words[:, :(rows + 31) // 32], int(got_n.value)


def _assert_built(s, filters, truth, what):
    n = len(s)
    words, got_n = _built(s, filters)
    assert got_n == n, what
    want = wc.packed(truth)
    assert words.shape == want.shape, what
    bad = np.nonzero((words != want).any(axis=1))[0]
    assert bad.size == 0, "%s: filters %s differ from numpy" % (what, bad.tolist())
    if n % 32:
        assert (words[:, -1] >> np.uint32(n % 32) == 0).all(), what + ": the last word's tail"


def _device(s, method, Q, of, k, *args, total=False, fill=None, **kw):
    """a _device form on a stream of its own -> the host copies of its outputs; args go between the queries and filter_of"""
    import torch
    dq, dof = _device_args(Q, of)
    o = _torch_outputs(len(Q), k, total=total)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    try:
        method(dq, *args, dof, *o, stream=st.cuda_stream, **kw)
    finally:
        torch.cuda.synchronize()
        if fill is not None:
            fill.extend(_host(o))
    return _host(o)


# ---- 1. the bitmaps against numpy ----

@pytest.mark.parametrize("n", fc.BITMAP_ROWS)
def test_bitmaps_against_numpy(n):
    rng = np.random.default_rng(n)
    extra = 37
    X = rng.standard_normal((n + extra, 4)).astype(f32)
    cols = {c: v[:n] for c, v in wc.columns().items()}
    s = _stored("filter-bits", X[:n], "l2", cols, cap=n + extra)
    truth = fc.bitmaps(fc.TABLE, cols, n)
    for i, name in enumerate(fc.NAMES):                                       # every filter alone ...
        _assert_built(s, [fc.TABLE[i]], truth[i:i + 1], "n=%d %s" % (n, name))
    _assert_built(s, fc.TABLE, truth, "n=%d the table" % n)                   # ... and together
    cl, runs = fc.limits()                                                    # every limit at once
    _assert_built(s, marshal_filter_table(cl, runs, pack=False), fc.run_bitmaps(cl, runs, cols, n), "n=%d the limits" % n)
    cl, runs = fc.overlapping()                                               # shared clauses
    _assert_built(s, marshal_filter_table(cl, runs, pack=False), fc.run_bitmaps(cl, runs, cols, n), "n=%d overlapping runs" % n)
    sets = [f for length in fc.SET_LENGTHS for f in fc.set_filters(length)]   # set lengths 0 .. 1024, IN and NOT IN
    _assert_built(s, sets, fc.bitmaps(sets, cols, n), "n=%d set lengths" % n)
    # one-clause filters without IN terms: word for word what the predicates' builder writes
    plain = [[p] for p in wc.sixty_four()]
    words, _ = _built(s, plain)
    assert np.array_equal(words, _where_built(s, wc.sixty_four())[0]), "n=%d against ehx_test_where_bitmaps" % n
    _assert_built(s, plain, wc.bitmaps(wc.sixty_four(), cols, n), "n=%d 64 plain predicates" % n)
    # rows appended by a plain Set after the columns exist hold the default
    s.set_batch(_keys(extra, n), X[n:])
    grown = {c: np.concatenate([v, np.full(extra, NONE, dtype=np.uint32)]) for c, v in cols.items()}
    _assert_built(s, fc.TABLE, fc.bitmaps(fc.TABLE, grown, n + extra), "n=%d + %d plain rows" % (n, extra))
    default = [[[(A, "in", [NONE])]], [[(B, "in", [0, NONE], True)], [(A, 1, 0)]]]
    _assert_built(s, default, fc.bitmaps(default, grown, n + extra), "n=%d the plain rows' default" % n)
    s.drop()
    # 0, 2^31 - 1, 2^31 and 2^32 - 1 and their neighbours as members
    e = {0: wc.edge_column(n)}
    s = _stored("filter-edges", X[:n], "l2", e)
    _assert_built(s, fc.edge_filters(), fc.bitmaps(fc.edge_filters(), e, n), "n=%d edge values" % n)
    s.drop()


def test_bitmaps_of_an_empty_space():
    s = ehx.Space.unique("filter-empty", 4, metric=ehx.METRIC_L2SQ)
    words, n = _built(s, fc.TABLE)
    assert n == 0 and words.shape == (len(fc.TABLE), 0)
    got = s.knn_filter(np.zeros((3, 4), dtype=f32), 5, fc.TABLE, [0, 6, 11])
    assert (got[2] == 0).all() and (got[0] == NO_ID).all() and np.isposinf(got[1]).all()
    s.drop()


# ---- 2. kNN ----

@pytest.mark.parametrize("metric", mmc.METRICS)
def test_knn_filter_is_the_oracle_s_and_the_bitmap_form_s_answer(metric):
    om = METRICS[metric][1]
    X, Q = rc.i8_data(128)
    Q = Q[:fc.NQ]
    tab, of = fc.table_truth(), fc.filter_of()
    ft = _unpacked(fc.TABLE)
    s = _stored("filter-knn", X, metric, wc.columns())
    twin = _i8_space("filter-twin", 128, metric, X)                          # no column: the bitmap form under numpy's bitmaps
    assert s.scan_engine() == "i8"
    want_all = _want(X, Q, 60, om, tab, of)                                  # every query, under its own filter's rows
    assert all(w is not None for w in want_all)
    for k in (1, 10, 48, 60):
        what = "%s k=%d" % (metric, k)
        c0 = _masked_counters(s)
        got = s.knn_filter(Q, k, ft, of)
        dc = _masked_counters(s) - c0
        _assert_rows(got, _cut(want_all, k), what)
        t0 = _masked_counters(twin)
        ref = twin.knn_masked_multi(Q, k, tab, of)
        dt = _masked_counters(twin) - t0
        assert _same_bytes(got, ref), what + ": differs from knn_masked_multi under numpy's bitmaps"
        assert dc.tolist() == dt.tolist(), (what, dc, dt)                     # the routes, the passes, the calls
        if k <= 48:                                                           # one batch holds both routes
            n_scan = int(mmc.scans(tab)[of].sum())
            assert 0 < n_scan < fc.NQ and dc[0] > 0 and dc[1] >= fc.NQ - n_scan, (what, dc)
        for name in ("no_clause", "in_empty"):                                # empty: for ITS queries only
            assert (got[2][of == fc.NAMES.index(name)] == 0).all(), (what, name)
        assert (got[2][of == fc.NAMES.index("small_in")] == min(k, 3)).all(), what
        for name in ("not_in_empty", "never_in", "b_1024"):
            assert (got[2][of == fc.NAMES.index(name)] == k).all(), (what, name)
        assert _same_bytes(got, _device(s, s.knn_filter_device, Q, of, k, k, ft)), what + ": host and device forms differ"
        assert _same_bytes(got, s.knn_filter(Q, k, fc.TABLE, of)), what + ": packed in Python and packed by the library differ"
    # one filter, filter_of=None: every query under it
    one = s.knn_filter(Q, 10, [fc.TABLE[0]])
    assert _same_bytes(one, twin.knn_masked_multi(Q, 10, tab[:1], np.zeros(fc.NQ, dtype=np.uint32)))
    assert np.isin(wc.columns()[A][one[0].astype(np.int64)], [3, 7, 11]).all()
    assert s.stats()["n_uncertified"] == 0
    s.drop()
    twin.drop()


def test_a_row_two_clauses_allow_comes_back_once_and_the_merge_of_two_predicate_calls_does_not_do_that():
    """(A = 3) OR (B >= 18000): 125 rows satisfy both.  The queries are those whose k nearest allowed rows, by the oracle,
    hold one of the 125: ehx_knn_filter returns k DISTINCT ids for them — the oracle's — while two ehx_knn_where calls merged
    by ehx_merge_topk_device, the workaround the header used to advise, return such a row twice and so fewer distinct rows."""
    import torch
    metric, k = "cosine", 10
    om = METRICS[metric][1]
    X, Q = rc.i8_data(128)
    Q = Q[:fc.NQ]
    cols = wc.columns()
    flt = fc.TABLE[fc.NAMES.index("a3_or_late")]
    allow = fc.table_truth()[fc.NAMES.index("a3_or_late")]
    both = (cols[A] == 3) & (cols[B] >= 18000)
    lists = _want(X, Q, k, om, allow[None], np.zeros(fc.NQ, dtype=np.uint32))
    pick = np.array([i for i, (ids, _) in enumerate(lists) if both[np.asarray(ids, dtype=np.int64)].any()])
    assert len(pick) >= 4, "choose other queries: %d of them have a common row among their %d nearest" % (len(pick), k)
    Qp, nq = np.ascontiguousarray(Q[pick]), len(pick)
    s = _stored("filter-or", X, metric, cols)
    got = s.knn_filter(Qp, k, [flt])
    _assert_rows(got, [lists[i] for i in pick], "a3_or_late")
    assert (got[2] == k).all() and all(len(set(row.tolist())) == k for row in got[0]), "k distinct rows"
    assert all(both[row.astype(np.int64)].any() for row in got[0])
    # the workaround: one predicate per clause, two calls, one merge
    dq, dof = _device_args(Qp, np.zeros(nq, dtype=np.uint32))
    parts = [_torch_outputs(nq, k) for _ in flt]
    for clause, o in zip(flt, parts):
        s.knn_where_device(dq, k, [clause], dof, *o)
    torch.cuda.synchronize()
    g = [torch.stack([p[j] for p in parts]).contiguous() for j in range(3)]
    o = _torch_outputs(nq, k)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    _lib.check(_lib.load().ehx_merge_topk_device(C.c_void_p(torch.cuda.current_stream().cuda_stream), nq, k, len(flt), P(g[0]), P(g[1]),
                                                 P(g[2]), P(o[0]), P(o[1]), P(o[2])))
    torch.cuda.synchronize()
    merged = _host(o)
    dup = [len(set(row[:c].tolist())) < c for row, c in zip(merged[0], merged[2])]
    assert any(dup), "the merged answer holds no duplicate: the case shows nothing"
    assert not _same_bytes(merged, got)
    s.drop()


@pytest.mark.parametrize("kind", ["flat_f16", "graph_f32"])
def test_f16_and_graph_spaces_answer_from_their_stored_rows(kind):
    n, d, nq, k = 1000, 16, 21, 10
    rng = np.random.default_rng(77)
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    kw = {"mode": ehx.MODE_GRAPH, "M": 16} if kind == "graph_f32" else {"dtype": ehx.DTYPE_F16}
    cols = {c: v[:n] for c, v in wc.columns().items()}
    s = _stored("filter-small", X, "l2", cols, **kw)
    Xs = X.astype(np.float16).astype(f32) if kind == "flat_f16" else X
    tab = fc.table_truth(n)
    of = fc.filter_of(nq)[::-1].copy()
    ft = _unpacked(fc.TABLE)
    c0 = _masked_counters(s)
    got = s.knn_filter(Q, k, ft, of)
    assert (_masked_counters(s) - c0).tolist() == [0, nq, 0, 0, 1]
    _assert_rows(got, _want(Xs, Q, k, METRICS["l2"][1], tab, of), kind)
    assert _same_bytes(got, s.knn_masked_multi(Q, k, tab, of))
    assert _same_bytes(got, _device(s, s.knn_filter_device, Q, of, k, k, ft))
    s.drop()


# ---- 3. the wrong filter ----

@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_no_query_is_judged_by_another_query_s_filter(metric):
    """masked_multi_cases.parity: every vector stored at rows 2 j and 2 j + 1, a column holding row & 1, one filter per parity,
    queries alternating — the wrong filter shows as an id of the wrong parity at the right distance"""
    om = METRICS[metric][1]
    X, Q, tab, of = mmc.parity()
    s = _stored("filter-parity", X, metric, {2: (np.arange(len(X)) & 1).astype(np.uint32)})
    filters = [[[(2, "in", [0])]], [[(2, "in", [7, 1, 9])], [(2, 5, 6)]]]
    for k in mmc.KS:
        what = "parity %s k=%d" % (metric, k)
        got = s.knn_filter(Q, k, filters, of)
        _assert_rows(got, _want(X, Q, k, om, tab, of), what)
        assert (got[2] == k).all() and ((got[0] % np.uint64(2)) == of[:, None].astype(np.uint64)).all(), what
        assert _same_bytes(got, _device(s, s.knn_filter_device, Q, of, k, k, filters)), what
    s.drop()


# ---- 4. grouped ----

GROUPED = ("a_in", "a3_or_late", "small_in", "not_in", "mixed_exact", "mixed_scan", "windows", "no_clause", "not_in_empty")


@pytest.mark.parametrize("groups", ["stored", "never_written"])
def test_grouped_filter(groups):
    metric, k = "cosine", 10
    X, Q = rc.i8_data(128)
    Q = Q[:fc.NQ]
    pick = [fc.NAMES.index(name) for name in GROUPED]                        # (none names column 3)
    filters, tab = [fc.TABLE[i] for i in pick], fc.table_truth()[pick]
    ft = _unpacked(filters)
    of = mmc.interleaved(fc.NQ, len(pick))
    cols = dict(wc.columns())
    labels = np.full(fc.N, NONE, dtype=np.uint32)                             # never written: every row a group of its own
    if groups == "stored":
        labels = (np.arange(fc.N) // 4).astype(np.uint32)
        cols[3] = labels
    s = _stored("filter-grouped", X, metric, cols)
    full = gm.oracle_all(X, Q, metric)
    for m in (1, 3):
        what = "%s per_group=%d" % (groups, m)
        c0 = _hook5(s, "ehx_test_grouped_masked_counters")
        got = s.knn_grouped_filter(Q, k, 3, ft, of, per_group=m)
        c1 = _hook5(s, "ehx_test_grouped_masked_counters")
        _assert_grouped_rows(got, gmm.expected(full, labels, tab, of, k, m), k, what)
        ref = s.knn_grouped_masked(Q, k, labels, tab, of, per_group=m)
        c2 = _hook5(s, "ehx_test_grouped_masked_counters")
        assert _same_bytes(got, ref), what + ": differs from knn_grouped_masked under numpy's bitmaps"
        assert (c1 - c0).tolist() == (c2 - c1).tolist() and (c1 - c0)[4] == 1, (what, c1 - c0, c2 - c1)
        dev = _device(s, s.knn_grouped_filter_device, Q, of, k, k, 3, ft, per_group=m)
        assert _same_bytes(got, dev), what + ": host and device forms differ"
        if groups == "stored":   # at most m rows of a group
            for i in range(fc.NQ):
                assert np.unique(got[0][i, :got[2][i]] // np.uint64(4), return_counts=True)[1].max(initial=0) <= m, (what, i)
    one = s.knn_grouped_filter(Q, k, 3, [filters[1]], per_group=1)            # one filter, filter_of=None
    assert _same_bytes(one, s.knn_grouped_masked(Q, k, labels, tab[1], per_group=1))
    s.drop()


# ---- 5. range ----

@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_range_filter(metric):
    om = METRICS[metric][1]
    mr = 256
    X, Q = rc.i8_data(128)
    Q = Q[:fc.NQ]
    tab, of = fc.table_truth(), fc.filter_of()
    ft = _unpacked(fc.TABLE)
    s = _stored("filter-range", X, metric, wc.columns())
    lists = _want(X, Q, 300, om, tab, of)
    for rank in (10, 300):
        what = "%s rank=%d" % (metric, rank)
        r = np.array([(d[min(rank, len(d)) - 1] if len(d) else 1.0) for _, d in lists], dtype=f32)
        c0 = _hook5(s, "ehx_test_range_masked_counters")
        got = s.range_filter(Q, r, mr, ft, of)
        c1 = _hook5(s, "ehx_test_range_masked_counters")
        ref = s.range_masked(Q, r, mr, tab, of)
        c2 = _hook5(s, "ehx_test_range_masked_counters")
        assert _same_bytes(got, ref), what + ": differs from range_masked under numpy's bitmaps"
        assert (c1 - c0).tolist() == (c2 - c1).tolist() and (c1 - c0)[4] == 1, (what, c1 - c0, c2 - c1)
        import torch
        dr = torch.tensor(np.ascontiguousarray(r, dtype=f32), device="cuda")
        dev = _device(s, s.range_filter_device, Q, of, mr, dr, mr, ft, total=True)
        assert _same_bytes(got, dev), what + ": host and device forms differ"
        for i, (wi, wd) in enumerate(lists):                                  # ... and the oracle's list up to the radius
            c = int(got[2][i])
            assert c == min(mr, int(got[3][i])) and int(got[3][i]) >= min(rank, len(wi)), (what, i)
            assert [int(v) for v in got[0][i, :c]] == [int(v) for v in wi[:c]] and got[1][i, :c].tobytes() == wd[:c].tobytes(), (what, i)
            assert (got[0][i, c:] == NO_ID).all() and np.isposinf(got[1][i, c:]).all(), (what, i)
    one = s.range_filter(Q, 0.5, mr, [fc.TABLE[1]])                           # one filter, filter_of=None
    assert _same_bytes(one, s.range_masked(Q, 0.5, mr, tab[1]))
    s.drop()


# ---- 6. the graph walk under filters ----

def _graph_counters(s):
    out = (C.c_uint64 * 4)()
    fn = _raw().ehx_test_graph_masked_counters
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    assert fn(s._h, out) == 0
    return np.array([int(v) for v in out], dtype=np.int64)   # walked, exact, calls, walked queries at cap


# at 3000 rows: 563 (walked by AUTO: 12 x 563 >= 3000) | 30 (exact) | 1000 (walked) | 0 (exact) | 3000 (walked) | 188 + 0 (exact)
GRAPH_FILTERS = (fc.TABLE[fc.NAMES.index("a_in")], [[(B, "in", [97 * j + 3 for j in range(30)])]], fc.TABLE[fc.NAMES.index("windows")],
                 [], fc.TABLE[fc.NAMES.index("not_in_empty")], fc.TABLE[fc.NAMES.index("a3_or_late")])


def test_graph_walk_under_filters_is_the_walk_under_their_bitmaps():
    n, d, nq, k = 3000, 64, 24, 10
    rng = np.random.default_rng(n + d)
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    cols = {c: v[:n] for c, v in wc.columns().items()}
    s = _stored("filter-graph", X, "l2", cols, mode=ehx.MODE_GRAPH, M=16)    # the graph built by the Sets themselves
    s.set_ef(50)
    filters = list(GRAPH_FILTERS)
    ft = _unpacked(filters)
    tab = fc.bitmaps(filters, cols, n)
    cnt = tab.sum(axis=1)
    assert cnt.tolist() == [563, 30, 1000, 0, 3000, 188]
    walks = cnt * _lib.WALK_LIST_FACTOR >= n
    assert walks.tolist() == [True, False, True, False, True, False]          # AUTO: a sparse filter beside dense ones
    of = mmc.interleaved(nq, len(filters))
    for route in ROUTES:
        what = "route %d" % route
        c0 = _graph_counters(s)
        got = s.graph_knn_filter(Q, k, ft, of, route=route)
        c1 = _graph_counters(s)
        ref = s.graph_knn_masked_multi(Q, k, tab, of, route=route)
        c2 = _graph_counters(s)
        assert _same_bytes(got, ref), what + ": differs from graph_knn_masked_multi under numpy's bitmaps"
        assert (c1 - c0).tolist() == (c2 - c1).tolist() and (c1 - c0)[2] == 1, (what, c1 - c0, c2 - c1)
        n_walk = {ehx.WALK_GRAPH: nq, ehx.WALK_EXACT: 0, ehx.WALK_AUTO: int(walks[of].sum())}[route]
        assert (c1 - c0)[:2].tolist() == [n_walk, nq - n_walk], (what, c1 - c0)
        dev = _device(s, s.graph_knn_filter_device, Q, of, k, k, ft, route=route)
        assert _same_bytes(got, dev), what + ": host and device forms differ"
        for i in range(nq):                                                   # whatever the route: allowed rows only
            assert tab[of[i]][got[0][i, :got[2][i]].astype(np.int64)].all(), (what, i)
        if route != ehx.WALK_GRAPH:                                           # the exact rows are the oracle's
            rows = np.nonzero(~walks[of])[0] if route == ehx.WALK_AUTO else np.arange(nq)
            want = _want(X, Q, k, METRICS["l2"][1], tab, of)
            _assert_rows(tuple(a[rows] for a in got), [want[i] for i in rows], what)
    # a table of ONE filter on the walk: the builder must have written the bitmap the walk reads
    for f in (0, 2):
        c0 = _graph_counters(s)
        got = s.graph_knn_filter(Q, k, [filters[f]], route=ehx.WALK_GRAPH)
        c1 = _graph_counters(s)
        ref = s.graph_knn_masked_multi(Q, k, tab[f:f + 1], np.zeros(nq, dtype=np.uint32), route=ehx.WALK_GRAPH)
        assert _same_bytes(got, ref) and (got[2] == k).all(), "one filter %d walked" % f
        assert (c1 - c0).tolist() == (_graph_counters(s) - c1).tolist() and (c1 - c0)[:3].tolist() == [nq, 0, 1]
        assert tab[f][got[0].astype(np.int64)].all()
        dev = _device(s, s.graph_knn_filter_device, Q, np.zeros(nq, dtype=np.uint32), k, k, [filters[f]], route=ehx.WALK_GRAPH)
        assert _same_bytes(got, dev)
    # an ordinary search afterwards: the visited bitmaps came back clean (the exact answer for most queries at this ef)
    ids, _, c = s.knn(Q, k)
    assert (c == k).all()
    s.drop()


# ---- 7. freshness ----

def test_relabelled_and_appended_rows_are_seen_by_the_next_call():
    n0, n1, d, nq, k = 2500, 3000, 16, 12, 10
    om = METRICS["l2"][1]
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n1, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    col = (np.arange(n1) % 4).astype(np.uint32)
    filters = [[[(0, "in", [1])]], [[(0, 2, 2)], [(0, "in", [3, 9])]], [[(0, "in", [9, 1], True)]]]
    of = mmc.interleaved(nq, 3)
    s = _stored("filter-fresh", X[:n0], "l2", {0: col[:n0]}, cap=n1)

    def check(n, what):
        tab = fc.bitmaps(filters, {0: col}, n)
        got = s.knn_filter(Q, k, filters, of)
        _assert_rows(got, _want(X[:n], Q, k, om, tab, of), what)
        assert _same_bytes(got, _device(s, s.knn_filter_device, Q, of, k, k, filters)), what
        return got

    before = check(n0, "as written")
    moved = np.unique(before[0][of == 0][:, :4].astype(np.int64))[:100]       # rows the first filter returned ...
    moved = np.concatenate([moved, np.setdiff1d(np.nonzero(col[:n0] == 1)[0], moved)[:100 - len(moved)]])
    assert len(moved) == 100 and (col[moved] == 1).all()
    col[moved] = 2                                                            # ... relabelled: they leave it, and join the second
    s.column_set(0, [_keys(1, int(r))[0] for r in moved], col[moved])
    after = check(n0, "after column_set")
    assert not np.isin(after[0][of == 0], moved.astype(np.uint64)).any() and not _same_bytes(before, after)
    X[n0:] = Q[np.arange(n1 - n0) % nq]                                       # the queries themselves: nearer than any old row
    s.set_batch_cols(_keys(n1 - n0, n0), X[n0:], {0: col[n0:]})
    grown = check(n1, "after an append with labels")
    assert (grown[0][:, 0] >= n0).any()
    s.drop()


def test_filter_searches_beside_appends_with_labels():
    """writers append chunks with set_batch_cols while searchers call knn_filter (host and device form) under filters that
    reduce to one tenant each — (tenant IN {v, 1000 + v}) OR (tenant = v AND a never-written column <= 5): every answer is the
    oracle's answer over the labelled rows of ONE published prefix between the search's start and its return
    (column_cases.LabelledPrefixOracle, as tests/test_where.py builds its run)"""
    import torch
    from test_append_under_search import _centres, _chunk_rows, _queries
    d, base, n_chunks, per, k = 128, 20000, 8, 60, 10
    cen = _centres(41, 16, d)
    rng = np.random.default_rng(3)
    Xb = (rng.standard_normal((base, d)).astype(f32) / np.sqrt(f32(d))).astype(f32)
    m = 16 * per - 37                                                   # no boundary on a 256-row tile, nor on a 1024-row span
    chunks = [_chunk_rows(cen, j, per, lambda j, m, r: 1.0, 9)[:m] for j in range(n_chunks)]
    X = np.concatenate([Xb] + chunks)
    col = rng.integers(1, 4, size=len(X)).astype(np.uint32)             # three tenants, above the scan route's cut
    col[rng.random(len(X)) < 0.1] = 50                                  # ... and a small one on the list route
    bounds = [base + j * m for j in range(n_chunks + 1)]
    Q = _queries(cen, 4, 2)
    labels = [1, 2, 3, 50]
    ft = marshal_filters([[[(0, "in", [1000 + v, v])], [(0, v, v), (1, 0, 5)]] for v in labels], pack=False)
    of = (np.arange(len(Q)) % 4).astype(np.uint32)
    want = np.array(labels, dtype=np.uint32)[of]
    s = ehx.Space.unique("filter-stream", d, metric=ehx.METRIC_COSINE, initial_capacity=len(X) + 256)
    s.set_batch_cols(_keys(base), Xb, {0: col[:base]})
    assert s.scan_engine() == "i8"
    errs, records, stop, tick = [], [], threading.Event(), threading.Condition()

    def record(r):
        with tick:
            records.append(r)
            tick.notify_all()

    def writer():
        try:
            for j in range(n_chunks):   # paced by the searchers: a chunk lands after another answer has come back
                with tick:
                    seen = len(records)
                    assert tick.wait_for(lambda: len(records) > seen or errs, timeout=120), "no search returned"
                s.set_batch_cols(_keys(m, bounds[j]), chunks[j], {0: col[bounds[j]:bounds[j + 1]]})
        except Exception as e:  # noqa: BLE001
            errs.append("writer: %r" % (e,))

    def host_searcher():
        try:
            while not stop.is_set():
                lo = len(s)
                ans = s.knn_filter(Q, k, ft, of)
                record((lo, ans, len(s)))
        except Exception as e:  # noqa: BLE001
            errs.append("searcher: %r" % (e,))
            record(None)

    def device_searcher():
        try:
            st = torch.cuda.Stream()
            dq, dof = _device_args(Q, of)
            o = _torch_outputs(len(Q), k)
            torch.cuda.synchronize()
            while not stop.is_set():
                lo = len(s)
                s.knn_filter_device(dq, k, ft, dof, *o, stream=st.cuda_stream)
                st.synchronize()
                record((lo, _host(o), len(s)))
        except Exception as e:  # noqa: BLE001
            errs.append("device searcher: %r" % (e,))
            record(None)

    th = [threading.Thread(target=f) for f in (host_searcher, device_searcher)]
    w = threading.Thread(target=writer)
    for t in th + [w]:
        t.start()
    w.join(timeout=300)
    assert not w.is_alive(), "the writer hung"
    stop.set()
    for t in th:
        t.join(timeout=300)
        assert not t.is_alive(), "a searcher hung"
    assert not errs, errs
    assert len(s) == len(X)
    oracle = cc.LabelledPrefixOracle(X, col, Q, want, k, pyoracle.METRIC_COSINE, bounds)
    for lo, ans, hi in records:
        oracle.assert_is_some_prefix(*ans, lo, hi)
    seen = {lo for lo, _, _ in records if lo < bounds[-1]}
    assert len(seen) >= 3, "the searches ran across %d publishes only" % len(seen)
    final = s.knn_filter(Q, k, ft, of)
    assert oracle.assert_is_some_prefix(*final, len(X), len(X)) == len(X)
    s.drop()


# ---- 8. errors ----

def _table(n_clauses=2, n_terms=1, n_filters=2, run=(0, 1), n_values=4, col=0, lo=0, hi=0, flags=0):
    """an ehx_filters of equal clauses, terms and runs -> (struct, what it points into)"""
    cl = (_lib.Pred * max(n_clauses, 1))()
    for p in cl:
        p.n_terms = n_terms
        for j in range(min(n_terms, _lib.PRED_MAX_TERMS)):
            p.terms[j] = _lib.Term(col, lo, hi, flags)
    vals = (C.c_uint32 * max(n_values, 1))()
    fl = (_lib.Filter * max(n_filters, 1))()
    for f in fl:
        f.first_clause, f.n_clauses = run
    return _lib.Filters(cl, n_clauses, vals, n_values, fl, n_filters), (cl, vals, fl)


def test_error_returns():
    rng = np.random.default_rng(8)
    n, d, nq, k = 200, 8, 3, 4
    X = rng.standard_normal((n, d)).astype(f32)
    Q = np.ascontiguousarray(rng.standard_normal((nq, d)).astype(f32))
    s = _stored("filter-err", X, "l2", {0: (np.arange(n) % 2).astype(np.uint32)})
    L = _lib.load()
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    IN, NOT = _lib.TERM_IN, _lib.TERM_NOT
    of = np.array([0, 1, 0], dtype=np.uint32)
    r = np.full(nq, 1e9, dtype=f32)
    o_ids, o_dist, o_cnt = np.full((nq, k), 7, dtype=np.uint64), np.full((nq, k), 7, dtype=f32), np.full(nq, 7, dtype=np.uint32)
    o_tot = np.full(nq, 7, dtype=np.uint64)
    out = [P(o_ids, C.c_uint64), P(o_dist, C.c_float), P(o_cnt, C.c_uint32)]
    forms = {
        "knn": lambda h, q_n, f, a_of, a=out: L.ehx_knn_filter(h, q_n, P(Q, C.c_float), k, f, a_of, *a),
        "grouped": lambda h, q_n, f, a_of, a=out: L.ehx_knn_grouped_filter(h, q_n, P(Q, C.c_float), k, 1, 1, f, a_of, *a),
        "range": lambda h, q_n, f, a_of, a=out: L.ehx_range_filter(h, q_n, P(Q, C.c_float), P(r, C.c_float), k, f, a_of, *a,
                                                                   P(o_tot, C.c_uint64)),
        "graph": lambda h, q_n, f, a_of, a=out: L.ehx_graph_knn_filter(h, q_n, P(Q, C.c_float), k, f, a_of, ehx.WALK_AUTO, *a),
    }
    sh = ehx.Space.unique("filter-sh", d, metric=ehx.METRIC_L2SQ, shards=2)
    sh.set_batch(_keys(n), X)
    good, keep_good = _table()
    bad = {   # name -> (table, code)
        "no filter": (_table(n_filters=0), _lib.EINVAL),
        "a run past the clauses": (_table(run=(1, 2)), _lib.EINVAL),
        "an IN term past the values": (_table(flags=IN, lo=2, hi=3), _lib.EINVAL),
        "a column the space cannot have": (_table(col=_lib.MAX_COLUMNS), _lib.EINVAL),
        "too many terms": (_table(n_terms=9), _lib.EINVAL),
        "an unknown flag bit": (_table(flags=4), _lib.EINVAL),
        "65 filters": (_table(n_filters=65), _lib.EUNSUPPORTED),
        "129 clauses": (_table(n_clauses=129), _lib.EUNSUPPORTED),
        "4097 values": (_table(n_clauses=1, n_values=5000, flags=IN, lo=0, hi=4097), _lib.EUNSUPPORTED),
    }
    for hole in ("clauses", "filters", "values"):
        t = _table(flags=IN, lo=0, hi=4)
        setattr(t[0], hole, None)
        bad["NULL " + hole] = (t, _lib.EINVAL)
    limits = marshal_filter_table(*fc.limits(), pack=False)
    for name, call in forms.items():
        pof = P(of, C.c_uint32)
        assert call(s._h, nq, None, pof) == _lib.EINVAL, name                                     # a NULL table
        for why, ((t, keep), code) in bad.items():
            assert call(s._h, nq, C.byref(t), pof) == code, (name, why)
        assert call(s._h, nq, C.byref(good), P(np.array([0, 2, 1], dtype=np.uint32), C.c_uint32)) == _lib.EINVAL, name
        assert b"mask_of[1]" in L.ehx_last_error(), name
        assert call(sh._h, nq, C.byref(good), pof) == _lib.EUNSUPPORTED and b"sharded" in L.ehx_last_error(), name
        for hole in range(3):                                                                     # the bitmap form's NULLs
            a = list(out)
            a[hole] = None
            assert call(s._h, nq, C.byref(good), pof, a) == _lib.EINVAL, name
        assert (o_ids == 7).all() and (o_dist == 7).all() and (o_cnt == 7).all() and (o_tot == 7).all(), name   # unwritten
        assert call(s._h, 0, None, None) == _lib.OK, name                                         # no queries
        assert call(s._h, nq, C.byref(limits.struct), pof) == _lib.OK, name                       # the limits are served
        assert (o_cnt == k).all(), name     # (filter 0 holds A IN {0, 5, ...}: the even rows; filter 1 a NOT IN over a column never written: every row)
        o_ids[:], o_dist[:], o_cnt[:], o_tot[:] = 7, 7, 7, 7
    g = C.byref(good)
    assert L.ehx_knn_filter(s._h, nq, P(Q, C.c_float), k, g, None, *out) == _lib.EINVAL            # NULL filter_of, as mask_of
    assert L.ehx_graph_knn_filter(s._h, nq, P(Q, C.c_float), k, g, None, 0, *out) == _lib.EINVAL
    assert L.ehx_graph_knn_filter(s._h, nq, P(Q, C.c_float), k, g, P(of, C.c_uint32), 3, *out) == _lib.EINVAL   # no such route
    assert L.ehx_knn_filter(s._h, nq, P(Q, C.c_float), 0, g, P(of, C.c_uint32), *out) == _lib.EINVAL
    assert L.ehx_knn_grouped_filter(s._h, nq, P(Q, C.c_float), k, 1, _lib.MAX_COLUMNS, g, P(of, C.c_uint32), *out) == _lib.EINVAL
    assert L.ehx_knn_grouped_filter(s._h, nq, P(Q, C.c_float), k, 0, 1, g, P(of, C.c_uint32), *out) == _lib.EINVAL
    assert (o_ids == 7).all() and (o_cnt == 7).all()
    # the device forms read d_filter_of back in the compaction's wait: an entry at n_filters is EINVAL, the outputs untouched
    filters = [[[(0, "in", [0])]], [[(0, 1, 1)], [(0, "in", [])]]]
    wrong = np.array([0, 2, 1], dtype=np.uint32)
    got = []
    with pytest.raises(ehx.EhxError) as e:
        _device(s, s.knn_filter_device, Q, wrong, k, k, filters, fill=got)
    assert e.value.code == _lib.EINVAL and "mask_of[1]" in str(e.value)
    assert (got[0].view(np.int64) == -7).all() and (got[1] == -7).all() and (got[2].view(np.int32) == 77).all()
    import torch
    dr = torch.tensor(r, device="cuda")
    for method, args, kw in ((s.knn_grouped_filter_device, (k, 1, filters), {}), (s.range_filter_device, (dr, k, filters), {"total": True}),
                             (s.graph_knn_filter_device, (k, filters), {"route": ehx.WALK_GRAPH}),
                             (s.graph_knn_filter_device, (k, filters), {"route": ehx.WALK_AUTO})):
        got = []
        with pytest.raises(ehx.EhxError) as e:
            _device(s, method, Q, wrong, k, *args, fill=got, **kw)
        assert e.value.code == _lib.EINVAL
        assert (got[0].view(np.int64) == -7).all() and (got[2].view(np.int32) == 77).all()
    # the Python side: what marshal_filters refuses, a table without filter_of, filter_of of the wrong length
    for bad_filters in ([], [[[(4, 0, 0)]]], [[[(0, 0, 0)] * 9]], [[[(0, "in", [-1])]]]):
        with pytest.raises(ValueError):
            s.knn_filter(Q, k, bad_filters, of)
    with pytest.raises(ValueError):
        s.knn_filter(Q, k, filters)
    with pytest.raises(ValueError):
        s.range_filter(Q, r, k, filters, of[:2])
    with pytest.raises(ehx.EhxError) as e:
        s.knn_filter(Q, k, [[[(0, 0, 0)]]] * 65, of)
    assert e.value.code == _lib.EUNSUPPORTED
    ids, dist, cnt = s.knn_filter(Q, k, filters, of)                          # ... and the call still serves
    assert (cnt == k).all() and ((ids % np.uint64(2)) == of[:, None].astype(np.uint64)).all()
    h = s._h
    s.drop()   # the tombstone answers for the dropped handle
    assert L.ehx_knn_filter(h, nq, P(Q, C.c_float), k, g, P(of, C.c_uint32), *out) == _lib.ENOTFOUND
    sh.drop()
    del keep_good
