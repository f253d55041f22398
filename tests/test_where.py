"""GPU tests of the predicate searches on stored columns (ehx_knn_where*, ehx_knn_grouped_where*, ehx_range_where*) and of
the kernel that builds their bitmaps (k_where.hip, through the hook ehx_test_where_bitmaps).

The bitmaps are checked against numpy (where_cases.holds: unsigned compares, a column never written reading as 0xFFFFFFFF).
The kNN answers against the oracle as tests/test_knn_masked_multi.py takes its truth — pyoracle.exhaustive over the rows numpy
allows, ids equal and distance BYTES equal, tails the sentinels — and, byte for byte and counter for counter, against the
bitmap forms given the numpy bitmaps; the grouped answers against the model tests/test_knn_grouped_masked.py uses.  Columns,
predicates and their counts: tests/where_cases.py."""
import ctypes as C
import threading

import numpy as np
import pytest

import column_cases as cc
import grouped_masked_model as gmm
import grouped_model as gm
import masked_multi_cases as mmc
import range_cases as rc
import where_cases as wc
from oracle import pyoracle
from test_knn_grouped_masked import _assert_rows as _assert_grouped_rows
from test_knn_masked import METRICS, NO_ID, _assert_rows, _i8_space, _keys, _same_bytes
from test_knn_masked_multi import _cut, _want

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402
from embeddinghub_amd.space import marshal_preds  # noqa: E402

f32 = np.float32
NONE = wc.NONE


def _raw():
    return C.CDLL(_lib.LIB_PATH)


def _hook5(s, name):
    out = (C.c_uint64 * 5)()
    getattr(_raw(), name)(s._h, out)
    return np.array(list(out), dtype=np.int64)


def _stored(name, X, metric, cols, cap=None, **kw):
    """a space whose rows were written WITH their column values: cols maps column number -> values"""
    s = ehx.Space.unique(name, X.shape[1], metric=METRICS[metric][0], initial_capacity=cap or len(X), **kw)
    s.set_batch_cols(_keys(len(X)), X, {c: np.asarray(v)[:len(X)] for c, v in cols.items()})
    return s


def _built(s, preds):
    """the builder alone -> (words u32 [n_preds, ceil(n / 32)], the snapshot n)"""
    table, n_preds = marshal_preds(preds)
    rows = len(s)
    words = np.full((n_preds, max((rows + 31) // 32, 1)), 0xA5A5A5A5, dtype=np.uint32)
    got_n = C.c_uint64(12345)
    L = _raw()
    L.ehx_test_where_bitmaps.restype = C.c_int
    rc_ = L.ehx_test_where_bitmaps(s._h, table, C.c_uint32(n_preds), words.ctypes.data_as(C.POINTER(C.c_uint32)),
                                   C.byref(got_n))
    assert rc_ == 0, "ehx_test_where_bitmaps: %d %s" % (rc_, _lib.load().ehx_last_error())
    return words[:, :(rows + 31) // 32], int(got_n.value)


def _assert_built(s, preds, cols, what):
    n = len(s)
    words, got_n = _built(s, preds)
    assert got_n == n, what
    truth = wc.bitmaps(preds, cols, n)
    want = wc.packed(truth)
    assert words.shape == want.shape, what
    bad = np.nonzero((words != want).any(axis=1))[0]
    assert bad.size == 0, "%s: predicates %s differ from numpy" % (what, bad.tolist())
    if n % 32:
        assert (words[:, -1] >> np.uint32(n % 32) == 0).all(), what + ": the last word's tail"
    assert np.array_equal(np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool), truth), what


def _torch_outputs(nq, k, total=False):
    import torch
    o = [torch.full((nq, k), -7, dtype=torch.int64, device="cuda"), torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda"),
         torch.full((nq,), 77, dtype=torch.int32, device="cuda")]
    if total:
        o.append(torch.full((nq,), -7, dtype=torch.int64, device="cuda"))
    return o


def _host(o):
    out = [o[0].cpu().numpy().view(np.uint64), o[1].cpu().numpy(), o[2].cpu().numpy().view(np.uint32)]
    return tuple(out + [o[3].cpu().numpy().view(np.uint64)] if len(o) == 4 else out)


def _device_args(Q, of):
    import torch
    dq = torch.tensor(np.ascontiguousarray(Q, dtype=f32), device="cuda")
    dof = torch.tensor(np.asarray(of, dtype=np.uint32).view(np.int32), device="cuda")
    return dq, dof


def _knn_where_device(s, Q, k, preds, of, fill=None):
    import torch
    dq, dof = _device_args(Q, of)
    o = _torch_outputs(len(Q), k)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    try:
        s.knn_where_device(dq, k, preds, dof, *o, stream=st.cuda_stream)
    finally:
        torch.cuda.synchronize()
        if fill is not None:
            fill.extend(_host(o))
    return _host(o)


# ---- 1. the bitmaps against numpy ----

@pytest.mark.parametrize("n", wc.BITMAP_ROWS)
def test_bitmaps_against_numpy(n):
    rng = np.random.default_rng(n)
    extra = 37
    X = rng.standard_normal((n + extra, 4)).astype(f32)
    cols = {c: v[:n] for c, v in wc.columns().items()}
    s = _stored("where-bits", X[:n], "l2", cols, cap=n + extra)
    for name, pred in wc.PREDS:                                             # every kind alone ...
        _assert_built(s, [pred], cols, "n=%d %s" % (n, name))
    _assert_built(s, wc.TABLE, cols, "n=%d the table" % n)
    _assert_built(s, wc.sixty_four(), cols, "n=%d 64 predicates" % n)       # ... and 64 at once
    # rows appended by a plain Set after the columns exist hold the default
    s.set_batch(_keys(extra, n), X[n:])
    grown = {c: np.concatenate([v, np.full(extra, NONE, dtype=np.uint32)]) for c, v in cols.items()}
    _assert_built(s, wc.TABLE, grown, "n=%d + %d plain rows" % (n, extra))
    _assert_built(s, [[(wc.A, NONE, NONE)], [(wc.B, 0, n - 1)]], grown, "n=%d the plain rows' default" % n)
    s.drop()
    # 0, 2^31 - 1, 2^31 and 2^32 - 1 at the range ends
    e = {0: wc.edge_column(n)}
    s = _stored("where-edges", X[:n], "l2", e)
    _assert_built(s, wc.edge_preds(), e, "n=%d edge values" % n)
    s.drop()


def test_bitmaps_of_an_empty_space():
    s = ehx.Space.unique("where-empty", 4, metric=ehx.METRIC_L2SQ)
    words, n = _built(s, wc.TABLE)
    assert n == 0 and words.shape == (len(wc.TABLE), 0)
    got = s.knn_where(np.zeros((3, 4), dtype=f32), 5, wc.TABLE, [0, 6, 11])
    assert (got[2] == 0).all() and (got[0] == NO_ID).all() and np.isposinf(got[1]).all()
    s.drop()


# ---- 2. kNN ----

def _masked_counters(s):
    return _hook5(s, "ehx_test_masked_counters")


@pytest.mark.parametrize("metric", mmc.METRICS)
def test_knn_where_is_the_oracle_s_and_the_bitmap_form_s_answer(metric):
    om = METRICS[metric][1]
    X, Q = rc.i8_data(128)
    Q = Q[:wc.NQ]
    tab, of = wc.table_truth(), wc.pred_of()
    s = _stored("where-knn", X, metric, wc.columns())
    twin = _i8_space("where-twin", 128, metric, X)                          # no column: the bitmap form under numpy's bitmaps
    assert s.scan_engine() == "i8"
    want_all = _want(X, Q, 60, om, tab, of)                                  # every query, under its own predicate's rows
    assert all(w is not None for w in want_all)
    for k in (1, 10, 48, 60):
        what = "%s k=%d" % (metric, k)
        c0 = _masked_counters(s)
        got = s.knn_where(Q, k, wc.TABLE, of)
        dc = _masked_counters(s) - c0
        _assert_rows(got, _cut(want_all, k), what)
        t0 = _masked_counters(twin)
        ref = twin.knn_masked_multi(Q, k, tab, of)
        dt = _masked_counters(twin) - t0
        assert _same_bytes(got, ref), what + ": differs from knn_masked_multi under numpy's bitmaps"
        assert dc.tolist() == dt.tolist(), (what, dc, dt)                     # the routes, the passes, the calls
        if k <= 48:                                                           # one batch holds both routes
            n_scan = int(mmc.scans(tab)[of].sum())
            assert 0 < n_scan < wc.NQ and dc[0] + dc[1] >= wc.NQ and dc[0] > 0 and dc[1] >= wc.NQ - n_scan, (what, dc)
        for name in ("a_is_3_and_not", "lo_above_hi", "never_is_0"):         # empty: for ITS queries only
            assert (got[2][of == wc.NAMES.index(name)] == 0).all(), (what, name)
        assert (got[2][of == wc.NAMES.index("no_terms")] == k).all(), what
        assert _same_bytes(got, _knn_where_device(s, Q, k, wc.TABLE, of)), what + ": host and device forms differ"
    # one predicate, pred_of=None: every query under it
    one = s.knn_where(Q, 10, [wc.TABLE[0]])
    assert _same_bytes(one, twin.knn_masked_multi(Q, 10, tab[:1], np.zeros(wc.NQ, dtype=np.uint32)))
    assert (wc.columns()[wc.A][one[0].astype(np.int64)] == 3).all()
    assert s.stats()["n_uncertified"] == 0
    s.drop()
    twin.drop()


@pytest.mark.parametrize("kind", ["flat_f16", "graph_f32"])
def test_f16_and_graph_spaces_answer_from_their_stored_rows(kind):
    n, d, nq, k = 1000, 16, 21, 10
    rng = np.random.default_rng(77)
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    kw = {"mode": ehx.MODE_GRAPH, "M": 16} if kind == "graph_f32" else {"dtype": ehx.DTYPE_F16}
    cols = {c: v[:n] for c, v in wc.columns().items()}
    s = _stored("where-small", X, "l2", cols, **kw)
    Xs = X.astype(np.float16).astype(f32) if kind == "flat_f16" else X
    tab = wc.table_truth(n)
    of = wc.pred_of(nq)[::-1].copy()
    c0 = _masked_counters(s)
    got = s.knn_where(Q, k, wc.TABLE, of)
    assert (_masked_counters(s) - c0).tolist() == [0, nq, 0, 0, 1]
    _assert_rows(got, _want(Xs, Q, k, METRICS["l2"][1], tab, of), kind)
    assert _same_bytes(got, s.knn_masked_multi(Q, k, tab, of)) and _same_bytes(got, _knn_where_device(s, Q, k, wc.TABLE, of))
    s.drop()


# ---- 3. the wrong predicate ----

@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_no_query_is_judged_by_another_query_s_predicate(metric):
    """masked_multi_cases.parity: every vector stored at rows 2 j and 2 j + 1, a column holding row & 1, predicates == 0 and
    == 1, queries alternating — the wrong predicate shows as an id of the wrong parity at the right distance"""
    om = METRICS[metric][1]
    X, Q, tab, of = mmc.parity()
    s = _stored("where-parity", X, metric, {2: (np.arange(len(X)) & 1).astype(np.uint32)})
    preds = [[(2, 0, 0)], [(2, 1, 1)]]
    for k in mmc.KS:
        what = "parity %s k=%d" % (metric, k)
        got = s.knn_where(Q, k, preds, of)
        _assert_rows(got, _want(X, Q, k, om, tab, of), what)
        assert (got[2] == k).all() and ((got[0] % np.uint64(2)) == of[:, None].astype(np.uint64)).all(), what
        assert _same_bytes(got, _knn_where_device(s, Q, k, preds, of)), what
    s.drop()


# ---- 4. grouped ----

GROUPED = ("a_is_3", "late", "c_middle", "a_is_3_c_low", "not_a_2_13", "a_is_3_and_not", "no_terms")   # none names column 3


def _grouped_device(s, Q, k, group_col, preds, of, m):
    import torch
    dq, dof = _device_args(Q, of)
    o = _torch_outputs(len(Q), k)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    try:
        s.knn_grouped_where_device(dq, k, group_col, preds, dof, *o, per_group=m, stream=st.cuda_stream)
    finally:
        torch.cuda.synchronize()
    return _host(o)


@pytest.mark.parametrize("groups", ["stored", "never_written"])
def test_grouped_where(groups):
    metric, k = "cosine", 10
    X, Q = rc.i8_data(128)
    Q = Q[:wc.NQ]
    pick = [wc.NAMES.index(name) for name in GROUPED]
    preds, tab = [wc.TABLE[i] for i in pick], wc.table_truth()[pick]
    of = mmc.interleaved(wc.NQ, len(pick))
    cols = dict(wc.columns())
    labels = np.full(wc.N, NONE, dtype=np.uint32)                             # never written: every row a group of its own
    if groups == "stored":
        labels = (np.arange(wc.N) // 4).astype(np.uint32)
        cols[3] = labels
    s = _stored("where-grouped", X, metric, cols)
    full = gm.oracle_all(X, Q, metric)
    for m in (1, 3):
        what = "%s per_group=%d" % (groups, m)
        c0 = _hook5(s, "ehx_test_grouped_masked_counters")
        got = s.knn_grouped_where(Q, k, 3, preds, of, per_group=m)
        c1 = _hook5(s, "ehx_test_grouped_masked_counters")
        _assert_grouped_rows(got, gmm.expected(full, labels, tab, of, k, m), k, what)
        ref = s.knn_grouped_masked(Q, k, labels, tab, of, per_group=m)
        c2 = _hook5(s, "ehx_test_grouped_masked_counters")
        assert _same_bytes(got, ref), what + ": differs from knn_grouped_masked under numpy's bitmaps"
        assert (c1 - c0).tolist() == (c2 - c1).tolist() and (c1 - c0)[4] == 1, (what, c1 - c0, c2 - c1)
        assert _same_bytes(got, _grouped_device(s, Q, k, 3, preds, of, m)), what + ": host and device forms differ"
        if groups == "stored":   # at most m rows of a group
            for i in range(wc.NQ):
                assert np.unique(got[0][i, :got[2][i]] // np.uint64(4), return_counts=True)[1].max(initial=0) <= m, (what, i)
    one = s.knn_grouped_where(Q, k, 3, [preds[0]], per_group=1)               # one predicate, pred_of=None
    assert _same_bytes(one, s.knn_grouped_masked(Q, k, labels, tab[0], per_group=1))
    s.drop()


# ---- 5. range ----

def _range_device(s, Q, r, mr, preds, of):
    import torch
    dq, dof = _device_args(Q, of)
    dr = torch.tensor(np.ascontiguousarray(r, dtype=f32), device="cuda")
    o = _torch_outputs(len(Q), mr, total=True)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    try:
        s.range_where_device(dq, dr, mr, preds, dof, *o, stream=st.cuda_stream)
    finally:
        torch.cuda.synchronize()
    return _host(o)


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_range_where(metric):
    om = METRICS[metric][1]
    mr = 256
    X, Q = rc.i8_data(128)
    Q = Q[:wc.NQ]
    tab, of = wc.table_truth(), wc.pred_of()
    s = _stored("where-range", X, metric, wc.columns())
    lists = _want(X, Q, 300, om, tab, of)
    for rank in (10, 300):
        what = "%s rank=%d" % (metric, rank)
        r = np.array([(d[min(rank, len(d)) - 1] if len(d) else 1.0) for _, d in lists], dtype=f32)
        c0 = _hook5(s, "ehx_test_range_masked_counters")
        got = s.range_where(Q, r, mr, wc.TABLE, of)
        c1 = _hook5(s, "ehx_test_range_masked_counters")
        ref = s.range_masked(Q, r, mr, tab, of)
        c2 = _hook5(s, "ehx_test_range_masked_counters")
        assert _same_bytes(got, ref), what + ": differs from range_masked under numpy's bitmaps"
        assert (c1 - c0).tolist() == (c2 - c1).tolist() and (c1 - c0)[4] == 1, (what, c1 - c0, c2 - c1)
        assert _same_bytes(got, _range_device(s, Q, r, mr, wc.TABLE, of)), what + ": host and device forms differ"
        for i, (wi, wd) in enumerate(lists):                                  # ... and the oracle's list up to the radius
            c = int(got[2][i])
            assert c == min(mr, int(got[3][i])) and int(got[3][i]) >= min(rank, len(wi)), (what, i)
            assert [int(v) for v in got[0][i, :c]] == wi[:c] and got[1][i, :c].tobytes() == wd[:c].tobytes(), (what, i)
            assert (got[0][i, c:] == NO_ID).all() and np.isposinf(got[1][i, c:]).all(), (what, i)
    one = s.range_where(Q, 0.5, mr, [wc.TABLE[1]])                            # one predicate, pred_of=None
    assert _same_bytes(one, s.range_masked(Q, 0.5, mr, tab[1]))
    s.drop()


# ---- 6. freshness ----

def test_relabelled_and_appended_rows_are_seen_by_the_next_call():
    n0, n1, d, nq, k = 2500, 3000, 16, 12, 10
    om = METRICS["l2"][1]
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n1, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    col = (np.arange(n1) % 4).astype(np.uint32)
    preds = [[(0, 1, 1)], [(0, 2, 3)], [(0, 1, 1, True)]]
    of = mmc.interleaved(nq, 3)
    s = _stored("where-fresh", X[:n0], "l2", {0: col[:n0]}, cap=n1)

    def check(n, what):
        tab = wc.bitmaps(preds, {0: col}, n)
        got = s.knn_where(Q, k, preds, of)
        _assert_rows(got, _want(X[:n], Q, k, om, tab, of), what)
        assert _same_bytes(got, _knn_where_device(s, Q, k, preds, of)), what
        return got

    before = check(n0, "as written")
    moved = np.unique(before[0][of == 0][:, :4].astype(np.int64))[:100]       # rows the first predicate returned ...
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


def test_where_searches_beside_appends_with_labels():
    """writers append chunks with set_batch_cols while searchers call knn_where (host and device form) under equality
    predicates: every answer is the oracle's answer over the labelled rows of ONE published prefix between the search's start
    and its return (column_cases.LabelledPrefixOracle, as tests/test_columns.py builds its own run)"""
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
    preds = [[(0, v, v)] for v in labels]
    of = (np.arange(len(Q)) % 4).astype(np.uint32)
    want = np.array(labels, dtype=np.uint32)[of]
    s = ehx.Space.unique("where-stream", d, metric=ehx.METRIC_COSINE, initial_capacity=len(X) + 256)
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
                ans = s.knn_where(Q, k, preds, of)
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
                s.knn_where_device(dq, k, preds, dof, *o, stream=st.cuda_stream)
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
    final = s.knn_where(Q, k, preds, of)
    assert oracle.assert_is_some_prefix(*final, len(X), len(X)) == len(X)
    s.drop()


def test_grouped_where_on_a_never_written_group_column_beside_appends_that_grow_the_space():
    """The array that stands in for a group column never written is allocated by the FIRST grouped search, at the capacity of
    that moment; the appends that follow grow the space beside the searches, and every later search must find the array as
    long as the capacity it runs under — whatever row count its plan then reads.  Every row is a group of its own, so the
    answer is knn_where's: the oracle's over the labelled rows of ONE published prefix."""
    d, base, n_chunks, m, k = 16, 3000, 6, 517, 10
    rng = np.random.default_rng(19)
    X = rng.standard_normal((base + n_chunks * m, d)).astype(f32)
    Q = rng.standard_normal((12, d)).astype(f32)
    col = rng.integers(1, 4, size=len(X)).astype(np.uint32)
    bounds = [base + j * m for j in range(n_chunks + 1)]
    labels = [1, 2, 3]
    preds = [[(0, v, v)] for v in labels]
    of = (np.arange(len(Q)) % 3).astype(np.uint32)
    want = np.array(labels, dtype=np.uint32)[of]
    s = ehx.Space.unique("where-grow", d, metric=ehx.METRIC_L2SQ, initial_capacity=base)   # full: the first append grows it
    s.set_batch_cols(_keys(base), X[:base], {0: col[:base]})
    oracle = cc.LabelledPrefixOracle(X, col, Q, want, k, pyoracle.METRIC_L2, bounds)
    first = s.knn_grouped_where(Q, k, 3, preds, of, per_group=1)            # column 3 is never written: the array is made here
    assert oracle.assert_is_some_prefix(*first, base, base) == base
    errs, records, tick = [], [], threading.Condition()

    def record(r):
        with tick:
            records.append(r)
            tick.notify_all()

    def writer():
        try:
            for j in range(n_chunks):   # paced by the searcher: a chunk lands after another answer has come back
                with tick:
                    seen = len(records)
                    assert tick.wait_for(lambda: len(records) > seen or errs, timeout=120), "no search returned"
                s.set_batch_cols(_keys(m, bounds[j]), X[bounds[j]:bounds[j + 1]], {0: col[bounds[j]:bounds[j + 1]]})
        except Exception as e:  # noqa: BLE001
            errs.append("writer: %r" % (e,))

    w = threading.Thread(target=writer)
    w.start()
    try:
        while w.is_alive() and not errs:
            lo = len(s)
            ans = s.knn_grouped_where(Q, k, 3, preds, of, per_group=1)
            record((lo, ans, len(s)))
    except Exception as e:  # noqa: BLE001
        errs.append("searcher: %r" % (e,))
        record(None)
    w.join(timeout=300)
    assert not w.is_alive() and not errs, errs
    assert len(s) == len(X)
    for lo, ans, hi in records:
        oracle.assert_is_some_prefix(*ans, lo, hi)
    final = s.knn_grouped_where(Q, k, 3, preds, of, per_group=3)            # (groups of one: the cap changes nothing)
    assert oracle.assert_is_some_prefix(*final, len(X), len(X)) == len(X)
    assert _same_bytes(final, s.knn_where(Q, k, preds, of))
    s.drop()


# ---- 7. errors ----

def _pred_table(n, n_terms=0, col=0, lo=0, hi=0, flags=0):
    t = (_lib.Pred * n)()
    for p in t:
        p.n_terms = n_terms
        for j in range(min(n_terms, _lib.PRED_MAX_TERMS)):
            p.terms[j] = _lib.Term(col, lo, hi, flags)
    return t


def test_error_returns():
    rng = np.random.default_rng(8)
    n, d, nq, k = 200, 8, 3, 4
    X = rng.standard_normal((n, d)).astype(f32)
    Q = np.ascontiguousarray(rng.standard_normal((nq, d)).astype(f32))
    s = _stored("where-err", X, "l2", {0: (np.arange(n) % 2).astype(np.uint32)})
    L = _lib.load()
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    of = np.array([0, 1, 0], dtype=np.uint32)
    r = np.full(nq, 1e9, dtype=f32)
    good = _pred_table(2, 1, col=0, lo=0, hi=0)
    o_ids, o_dist, o_cnt = np.full((nq, k), 7, dtype=np.uint64), np.full((nq, k), 7, dtype=f32), np.full(nq, 7, dtype=np.uint32)
    o_tot = np.full(nq, 7, dtype=np.uint64)
    out = [P(o_ids, C.c_uint64), P(o_dist, C.c_float), P(o_cnt, C.c_uint32)]
    forms = {
        "knn": lambda h, q_n, preds, n_preds, a_of, a=out: L.ehx_knn_where(h, q_n, P(Q, C.c_float), k, preds, n_preds, a_of, *a),
        "grouped": lambda h, q_n, preds, n_preds, a_of, a=out: L.ehx_knn_grouped_where(h, q_n, P(Q, C.c_float), k, 1, 1, preds,
                                                                                         n_preds, a_of, *a),
        "range": lambda h, q_n, preds, n_preds, a_of, a=out: L.ehx_range_where(h, q_n, P(Q, C.c_float), P(r, C.c_float), k, preds,
                                                                               n_preds, a_of, *a, P(o_tot, C.c_uint64)),
    }
    sh = ehx.Space.unique("where-sh", d, metric=ehx.METRIC_L2SQ, shards=2)
    sh.set_batch(_keys(n), X)
    for name, call in forms.items():
        pof = P(of, C.c_uint32)
        assert call(s._h, nq, None, 2, pof) == _lib.EINVAL, name                                  # NULL preds
        assert call(s._h, nq, good, 0, pof) == _lib.EINVAL, name                                  # no predicate
        assert call(s._h, nq, _pred_table(2, 1, col=_lib.MAX_COLUMNS), 2, pof) == _lib.EINVAL, name
        assert call(s._h, nq, _pred_table(2, 9), 2, pof) == _lib.EINVAL, name                     # too many terms
        assert call(s._h, nq, _pred_table(2, 1, flags=2), 2, pof) == _lib.EINVAL, name            # an unknown flag bit
        assert call(s._h, nq, _pred_table(65), 65, pof) == _lib.EUNSUPPORTED, name                # the bitmap table's limit
        assert call(s._h, nq, good, 2, P(np.array([0, 2, 1], dtype=np.uint32), C.c_uint32)) == _lib.EINVAL, name
        assert b"mask_of[1]" in L.ehx_last_error(), name
        assert call(sh._h, nq, good, 2, pof) == _lib.EUNSUPPORTED and b"sharded" in L.ehx_last_error(), name
        for hole in range(3):                                                                     # the bitmap form's NULLs
            a = list(out)
            a[hole] = None
            assert call(s._h, nq, good, 2, pof, a) == _lib.EINVAL, name
        assert (o_ids == 7).all() and (o_dist == 7).all() and (o_cnt == 7).all() and (o_tot == 7).all(), name   # unwritten
        assert call(s._h, 0, None, 0, None) == _lib.OK, name                                      # no queries
        assert call(s._h, nq, _pred_table(64, 8, col=3, lo=5, hi=4, flags=1), 64, pof) == _lib.OK, name   # the limits are served
        assert (o_cnt == k).all(), name
        o_ids[:], o_dist[:], o_cnt[:], o_tot[:] = 7, 7, 7, 7
    assert L.ehx_knn_where(s._h, nq, P(Q, C.c_float), k, good, 2, None, *out) == _lib.EINVAL        # NULL pred_of, as mask_of
    assert L.ehx_knn_where(s._h, nq, P(Q, C.c_float), 0, good, 2, P(of, C.c_uint32), *out) == _lib.EINVAL
    assert L.ehx_knn_grouped_where(s._h, nq, P(Q, C.c_float), k, 1, _lib.MAX_COLUMNS, good, 2, P(of, C.c_uint32), *out) == _lib.EINVAL
    assert L.ehx_knn_grouped_where(s._h, nq, P(Q, C.c_float), k, 0, 1, good, 2, P(of, C.c_uint32), *out) == _lib.EINVAL
    assert (o_ids == 7).all() and (o_cnt == 7).all()
    # the device forms read d_pred_of back in the compaction's wait: an entry at n_preds is EINVAL, the outputs untouched
    preds = [[(0, 0, 0)], [(0, 1, 1)]]
    bad = np.array([0, 2, 1], dtype=np.uint32)
    got = []
    with pytest.raises(ehx.EhxError) as e:
        _knn_where_device(s, Q, k, preds, bad, fill=got)
    assert e.value.code == _lib.EINVAL and "mask_of[1]" in str(e.value)
    assert (got[0].view(np.int64) == -7).all() and (got[1] == -7).all() and (got[2].view(np.int32) == 77).all()
    with pytest.raises(ehx.EhxError) as e:
        _grouped_device(s, Q, k, 1, preds, bad, 1)
    assert e.value.code == _lib.EINVAL
    with pytest.raises(ehx.EhxError) as e:
        _range_device(s, Q, r, k, preds, bad)
    assert e.value.code == _lib.EINVAL
    # the Python side: what marshal_preds refuses, a table without pred_of, pred_of of the wrong length
    for bad_preds in ([], [[(4, 0, 0)]], [[(0, 0, 0)] * 9]):
        with pytest.raises(ValueError):
            s.knn_where(Q, k, bad_preds, of)
    with pytest.raises(ValueError):
        s.knn_where(Q, k, preds)
    with pytest.raises(ValueError):
        s.range_where(Q, r, k, preds, of[:2])
    with pytest.raises(ehx.EhxError) as e:
        s.knn_where(Q, k, [[(0, 0, 0)]] * 65, of)
    assert e.value.code == _lib.EUNSUPPORTED
    ids, dist, cnt = s.knn_where(Q, k, preds, of)                             # ... and the call still serves
    assert (cnt == k).all() and ((ids % np.uint64(2)) == of[:, None].astype(np.uint64)).all()
    h = s._h
    s.drop()   # the tombstone answers for the dropped handle
    assert L.ehx_knn_where(h, nq, P(Q, C.c_float), k, good, 2, P(of, C.c_uint32), *out) == _lib.ENOTFOUND
    sh.drop()
