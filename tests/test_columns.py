"""GPU tests of stored label columns: labels written with the rows (set_batch_cols, column_set / _get, column_load_device /
_read_device), the index built over a column on the device (k_colindex.hip), and the label searches that take a column number
(knn_by_label*, knn_grouped_by_label*).

Truth comes from the oracle exactly as tests/test_knn_labeled.py takes it: pyoracle.exhaustive over the rows that carry the
wanted label, ids equal and distance BYTES equal, tails the sentinels; the grouped answers from the model
tests/test_knn_grouped_labeled.py uses (grouped_labeled_cases.expected).  The index is checked against numpy's stable argsort
and np.unique.  Columns, sizes and the labelled prefix oracle: tests/column_cases.py."""
import ctypes as C
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import column_cases as cc  # noqa: E402
import grouped_labeled_cases as glc  # noqa: E402
import grouped_model as gm  # noqa: E402
import labeled_cases as lbc  # noqa: E402
import largek_cases as lc  # noqa: E402
import masked_multi_cases as mmc  # noqa: E402
import range_cases as rc  # noqa: E402
from oracle import pyoracle  # noqa: E402

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402
from embeddinghub_amd.space import marshal_keys  # noqa: E402

f32 = np.float32
NONE = cc.NONE
PAUSE_US = 3000


def _t():
    """helpers of the label searches' own tests (imported late: the child process of the pause run needs none of them)"""
    import test_knn_grouped_masked as tg
    import test_knn_labeled as tl
    import test_knn_masked as tm
    return tm, tl, tg


def _L():
    return cc.raw(_lib.LIB_PATH)


def _keys(n, first=0):
    return ["k%d" % i for i in range(first, first + n)]


def _stored(name, X, metric, cols, dtype=None, cap=None, **kw):
    """a space whose rows were written WITH their labels: cols maps column number -> values"""
    tm = _t()[0]
    s = ehx.Space.unique(name, X.shape[1], metric=tm.METRICS[metric][0], initial_capacity=cap or len(X),
                         dtype=ehx.DTYPE_F32 if dtype is None else dtype, **kw)
    s.set_batch_cols(_keys(len(X)), X, cols)
    return s


def _device_by_label(s, Q, k, col, want):
    import torch
    dq = torch.tensor(np.ascontiguousarray(Q, dtype=f32), device="cuda")
    dw = torch.tensor(np.ascontiguousarray(want, dtype=np.uint32).view(np.int32), device="cuda")
    o_ids = torch.full((len(Q), k), -7, dtype=torch.int64, device="cuda")
    o_dist = torch.full((len(Q), k), -7.0, dtype=torch.float32, device="cuda")
    o_cnt = torch.full((len(Q),), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    try:
        s.knn_by_label_device(dq, k, col, dw, o_ids, o_dist, o_cnt, stream=st.cuda_stream)
    finally:
        torch.cuda.synchronize()
    return (o_ids.cpu().numpy().view(np.uint64), o_dist.cpu().numpy(), o_cnt.cpu().numpy().view(np.uint32))


def _device_grouped_by_label(s, Q, k, gcol, lcol, want, m):
    import torch
    dq = torch.tensor(np.ascontiguousarray(Q, dtype=f32), device="cuda")
    dw = torch.tensor(np.ascontiguousarray(want, dtype=np.uint32).view(np.int32), device="cuda")
    o_ids = torch.full((len(Q), k), -7, dtype=torch.int64, device="cuda")
    o_dist = torch.full((len(Q), k), -7.0, dtype=torch.float32, device="cuda")
    o_cnt = torch.full((len(Q),), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    try:
        s.knn_grouped_by_label_device(dq, k, gcol, lcol, dw, o_ids, o_dist, o_cnt, per_group=m, stream=st.cuda_stream)
    finally:
        torch.cuda.synchronize()
    return (o_ids.cpu().numpy().view(np.uint64), o_dist.cpu().numpy(), o_cnt.cpu().numpy().view(np.uint32))


# ---- 1. the index against numpy ----

@pytest.mark.parametrize("n", cc.INDEX_ROWS)
@pytest.mark.parametrize("kind", cc.INDEX_KINDS)
def test_index_against_numpy(kind, n):
    d, c = 4, 1
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, d)).astype(f32)
    col = cc.index_column(kind, n)
    s = _stored("col-index", X, "l2", {c: col})
    L = _L()
    assert cc.column_counters(L, s, c).tolist() == [0, 0, 0]
    ids, _, cnt = s.knn_by_label(X[:1], 1, c, [col[0]])   # the first search builds the index
    assert cnt[0] == 1 and col[int(ids[0, 0])] == col[0]
    perm, labels, start, got_n = cc.column_index(L, s, c)
    e_perm, e_labels, e_start = cc.expected_index(col)
    assert got_n == n
    assert np.array_equal(labels, e_labels) and np.array_equal(start, e_start), (kind, n)
    assert np.array_equal(perm, e_perm), (kind, n)            # stable: row ids ascend inside a label
    builds, fresh, passes = cc.column_counters(L, s, c).tolist()
    assert (builds, fresh) == (1, 0) and passes == cc.expected_passes(col), (kind, n, passes)
    if kind == "one_label":
        assert passes <= 1
    if kind == "random32" and n >= 4097:
        assert passes == 4
    if kind == "top_byte" and n > 1:
        assert passes == 1
    s.drop()


@pytest.mark.parametrize("kind", ["random32", "tenants16"])
def test_index_against_numpy_past_the_carry_loops(kind):
    """cc.BIG_ROWS rows: more than 256 sort tiles (colindex_scan_kernel carries between chunks of 256 tiles) and more than
    1024 boundary tiles (rows_prefix_kernel carries between chunks of 1024).  Rows by the generator, the column loaded
    from device memory: no key is marshalled."""
    import torch
    n, d, c = cc.BIG_ROWS, 4, 0
    col = cc.big_column(kind)
    s = ehx.Space.unique("col-index-big", d, metric=ehx.METRIC_L2SQ, initial_capacity=n)
    s.fill_synthetic(ehx.SEED_CORPUS, 0, n, False)
    s.column_load_device(c, 0, torch.tensor(col.view(np.int32), device="cuda"))
    L = _L()
    ids, _, cnt = s.knn_by_label(np.zeros((1, d), dtype=f32), 1, c, [col[5]])
    assert cnt[0] == 1 and col[int(ids[0, 0])] == col[5]
    perm, labels, start, got_n = cc.column_index(L, s, c)
    e_perm, e_labels, e_start = cc.expected_index(col)
    assert got_n == n and np.array_equal(labels, e_labels) and np.array_equal(start, e_start), kind
    assert np.array_equal(perm, e_perm), kind
    assert cc.column_counters(L, s, c).tolist() == [1, 0, cc.expected_passes(col)]
    back = torch.zeros(n, dtype=torch.int32, device="cuda")
    s.column_read_device(c, 0, back)
    assert np.array_equal(back.cpu().numpy().view(np.uint32), col)
    s.drop()


# ---- 2. answers: the oracle, knn_labeled given the same column, host and device forms ----

def _check_by_label(s, Q, k, c, col, want, expect, what):
    tm, tl, _ = _t()
    c0 = tl._counters(s)
    got = s.knn_by_label(Q, k, c, want)
    dc = tl._counters(s) - c0
    tm._assert_rows(got, expect, what)
    assert dc[0] + dc[1] == len(Q) and dc[4] == 1, (what, dc)      # scan + list == queries
    assert tm._same_bytes(got, s.knn_labeled(Q, k, col, want)), what + ": knn_labeled given the same column differs"
    assert tm._same_bytes(got, _device_by_label(s, Q, k, c, want)), what + ": host and device forms differ"
    return got, dc


@pytest.mark.parametrize("rows", ["f32", "f16"])
@pytest.mark.parametrize("d", rc.I8_DIMS)
@pytest.mark.parametrize("metric", mmc.METRICS)
def test_mixed_batch(metric, d, rows):
    tm, tl, _ = _t()
    om = tm.METRICS[metric][1]
    X, Q = rc.i8_data(d)
    Q = Q[:lbc.NQ]
    col, want = lbc.column(), lbc.mixed_batch()
    s = _stored("col-mixed", X, metric, {2: col}, dtype=ehx.DTYPE_F16 if rows == "f16" else ehx.DTYPE_F32)
    assert s.scan_engine() == "i8"
    Xs = X.astype(np.float16).astype(f32) if rows == "f16" else X
    expect_all = tl._want(Xs, Q, max(lbc.KS), om, col, want)
    scanned = 0
    for k in lbc.KS:
        what = "%s d=%d %s k=%d" % (metric, d, rows, k)
        got, dc = _check_by_label(s, Q, k, 2, col, want, tl._cut(expect_all, k), what)
        assert (got[2][want == lbc.ABSENT] == 0).all() and (got[2][want == lbc.ALL_ONES] == 1).all(), what
        scanned += dc[0]
        if k > 48:
            assert dc[0] == 0 and dc[3] == 0, (what, dc)
    assert scanned > 0                                              # the dense labels took the scan route
    builds, fresh, _ = cc.column_counters(_L(), s, 2).tolist()
    assert builds == 1 and fresh == 2 * len(lbc.KS) - 1             # host and device form of every k, one build in all
    assert s.stats()["n_uncertified"] == 0
    s.drop()


def test_two_device_batches():
    tm, tl, _ = _t()
    metric, d, k = "cosine", 128, 10
    om = tm.METRICS[metric][1]
    X, Q0 = rc.i8_data(d)
    col, want = lbc.column(), lbc.two_batches()
    Q = np.ascontiguousarray(Q0[np.arange(len(want)) % len(Q0)])
    assert len(Q) == lbc.SIDE_CHUNK + 64
    s = _stored("col-two", X, metric, {0: col})
    _check_by_label(s, Q, k, 0, col, want, tl._want(X, Q, k, om, col, want), "two batches")
    assert cc.column_counters(_L(), s, 0)[0] == 1
    s.drop()


@pytest.mark.parametrize("kind", ["flat_f32", "graph_f32"])
def test_small_and_graph_spaces_answer_from_their_stored_rows(kind):
    tm, tl, _ = _t()
    metric, om = "l2", tm.METRICS["l2"][1]
    n, d, nq = 3000, 24, 21
    rng = np.random.default_rng(410)
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    kw = {"mode": ehx.MODE_GRAPH, "M": 16} if kind == "graph_f32" else {}
    col = np.where(rng.random(n) < 0.5, 1, 2 + rng.integers(0, 30, size=n)).astype(np.uint32)
    col[77] = NONE
    want = np.array([1] * 9 + [NONE, 999] + [2 + i for i in range(10)], dtype=np.uint32)[::-1].copy()
    s = _stored("col-small", X, metric, {3: col}, **kw)
    for k in (1, 10, 100):
        _, dc = _check_by_label(s, Q, k, 3, col, want, tl._want(X, Q, k, om, col, want), "%s k=%d" % (kind, k))
        assert dc.tolist() == [0, nq, 0, 0, 1], dc
    s.drop()


# ---- 3. grouped answers: the model of tests/test_knn_grouped_labeled.py, and knn_grouped_labeled itself ----

def _check_grouped(s, Q, k, m, groups, col, want, expect, what):
    tm, _, tg = _t()
    c0 = tg._hook(s, "ehx_test_grouped_labeled_counters")
    got = s.knn_grouped_by_label(Q, k, 0, 1, want, per_group=m)
    dc = tg._hook(s, "ehx_test_grouped_labeled_counters") - c0
    tg._assert_rows(got, expect, k, what)
    assert dc[0] + dc[1] == len(Q) and dc[4] == 1, (what, dc)
    assert tm._same_bytes(got, s.knn_grouped_labeled(Q, k, groups, col, want, per_group=m)), what + ": the column form differs"
    assert tm._same_bytes(got, _device_grouped_by_label(s, Q, k, 0, 1, want, m)), what + ": host and device forms differ"
    return got, dc


@pytest.mark.parametrize("lab", sorted(gm.LABELINGS))
@pytest.mark.parametrize("metric", glc.METRICS)
def test_grouped_scan_cases(metric, lab):
    tm = _t()[0]
    X, Q = lc.gauss(20000, 64, 64, 1)
    full = gm.scan_oracle(metric)
    groups = gm.LABELINGS[lab](len(X))
    col, want = glc.tenant_column(), glc.scan_want()
    s = _stored("col-gscan", X, metric, {0: groups, 1: col})
    assert s.scan_engine() == "i8"
    cases = [c for c in glc.scan_cases() if c[0] == metric and c[1] == lab]
    assert len(cases) == 6
    for _, _, k, m in cases:
        what = "%s %s k=%d m=%d" % (metric, lab, k, m)
        got, dc = _check_grouped(s, Q, k, m, groups, col, want, glc.expected(full, groups, col, want, k, m), what)
        assert dc.tolist() == [64, 0, 0, glc.PASSES, 1], (what, dc)
    assert cc.column_counters(_L(), s, 1)[0] == 1
    s.drop()


def test_grouped_mixed_batch_and_a_group_column_never_written():
    tm = _t()[0]
    X, Q64 = lc.gauss(20000, 64, 64, 1)
    groups = gm.labels_scattered(len(X))
    col = glc.tenant_column()
    index = np.concatenate([np.arange(64), np.arange(36)])
    wants = np.concatenate([glc.scan_want(), glc.small_want(36)])
    shuffle = np.random.default_rng(6).permutation(100)
    index, wants = index[shuffle], wants[shuffle]
    Q = np.ascontiguousarray(Q64[index])
    full = tuple(np.ascontiguousarray(a[index]) for a in gm.scan_oracle("cosine"))
    s = _stored("col-gmixed", X, "cosine", {0: groups, 1: col})
    k, m = 10, 1
    got, dc = _check_grouped(s, Q, k, m, groups, col, wants, glc.expected(full, groups, col, wants, k, m), "mixed batch")
    assert dc.tolist() == [64, 36, 0, glc.PASSES, 1], dc
    # column 3 was never written: every row a group of its own — the kNN under the label column
    for kk in (10, 48):
        plain = s.knn_by_label(Q, kk, 1, wants)
        assert tm._same_bytes(s.knn_grouped_by_label(Q, kk, 3, 1, wants, per_group=1), plain), kk
    s.drop()


# ---- 4. freshness ----

def test_freshness_every_state_against_the_oracle():
    tm, tl, _ = _t()
    metric, d, k, c = "cosine", 128, 10, 0
    om = tm.METRICS[metric][1]
    X0, Q = rc.i8_data(d)
    Q = Q[:lbc.NQ]
    col0, want = lbc.column(), lbc.mixed_batch()
    L = _L()
    s = _stored("col-fresh", X0, metric, {c: col0}, cap=rc.I8_ROWS + 4096)
    X, col = X0.copy(), col0.copy()

    def state(what, wants=want):
        _check_by_label(s, Q, k, c, col, wants, tl._want(X, Q, k, om, col, wants), what)
        return cc.column_counters(L, s, c)

    # two searches with no write between them: one build, everything after it served fresh
    c1 = state("as written")
    assert c1[0] == 1 and c1[1] >= 1
    c2 = state("again")
    assert c2[0] == 1 and c2[1] > c1[1]
    # an append with labels: the new rows (the queries themselves: nearer than any old row) are found under THEIR labels
    n_new = 300
    new_rows = np.ascontiguousarray(Q[np.arange(n_new) % lbc.NQ])
    new_labels = want[np.arange(n_new) % lbc.NQ].copy()
    new_labels[new_labels == lbc.ABSENT] = lbc.FEW
    s.set_batch_cols(_keys(n_new, len(X)), new_rows, {c: new_labels})
    X, col = np.concatenate([X, new_rows]), np.concatenate([col, new_labels])
    c3 = state("appended with labels")
    assert c3[0] == 2                                              # one more build, then fresh again
    ids = s.knn_by_label(Q, 1, c, want)[0][:, 0]
    found = want != lbc.ABSENT
    assert (ids[found] >= rc.I8_ROWS).all() and (col[ids[found].astype(np.int64)] == want[found]).all()
    # a plain append: the rows carry EHX_GROUP_NONE — found by the queries that want it and by no others
    n_plain = lbc.NQ
    plain = np.ascontiguousarray(Q[:n_plain] * f32(1.0001))
    s.set_batch(_keys(n_plain, len(X)), plain)
    n_before = len(X)
    X, col = np.concatenate([X, plain]), np.concatenate([col, np.full(n_plain, NONE, dtype=np.uint32)])
    c4 = state("appended without labels")
    assert c4[0] == 3
    got = s.knn_by_label(Q, k, c, want)
    assert all((got[0][i, :got[2][i]] < n_before).all() for i in np.nonzero(want != NONE)[0])
    assert all(n_before + i in got[0][i] for i in np.nonzero(want == NONE)[0])
    assert (s.column_get(c, _keys(n_plain, n_before)) == NONE).all()
    # column_set moves rows between tenants
    moved = np.nonzero(col == lbc.TENTH)[0][:500]
    s.column_set(c, ["k%d" % r for r in moved], np.full(len(moved), lbc.FEW, dtype=np.uint32))
    col[moved] = lbc.FEW
    c5 = state("rows moved between tenants")
    assert c5[0] == 4
    assert (s.column_get(c, ["k%d" % r for r in moved[:7]]) == lbc.FEW).all()
    # a Set on a known key changes the vector and keeps the label
    r = int(np.nonzero(col == lbc.FEW)[0][3])
    s.set_batch(["k%d" % r], Q[:1] * f32(1.00001))
    X[r] = Q[0] * f32(1.00001)
    state("a vector rewritten in place")
    assert s.column_get(c, ["k%d" % r])[0] == lbc.FEW
    assert int(s.knn_by_label(Q[:1], 1, c, [lbc.FEW])[0][0, 0]) == r
    # a duplicate key in one set_batch_cols keeps the last value (and the last row)
    r2 = int(np.nonzero(col == lbc.HALF)[0][5])
    s.set_batch_cols(["k%d" % r2, "k%d" % r2], np.stack([Q[1], Q[2]]), {c: [lbc.TENTH, lbc.LAST]})
    X[r2], col[r2] = Q[2], lbc.LAST
    state("a key given twice")
    assert s.column_get(c, ["k%d" % r2])[0] == lbc.LAST
    s.drop()


def test_a_column_that_was_never_written():
    tm = _t()[0]
    d = 128
    X, Q = rc.i8_data(d)
    Q = Q[:lbc.NQ]
    s = tm._i8_space("col-never", d, "cosine", X)
    for k in (1, 10, 48):
        got = s.knn_by_label(Q, k, 1, np.full(lbc.NQ, NONE, dtype=np.uint32))
        assert tm._same_bytes(got, s.knn(Q, k)), k                  # wanting EHX_GROUP_NONE: the unfiltered kNN
        assert tm._same_bytes(got, _device_by_label(s, Q, k, 1, np.full(lbc.NQ, NONE, dtype=np.uint32))), k
    other = s.knn_by_label(Q, 10, 1, np.full(lbc.NQ, 5, dtype=np.uint32))
    assert (other[2] == 0).all() and (other[0] == tm.NO_ID).all()
    assert (s.column_get(1, _keys(5)) == NONE).all()
    s.drop()


# ---- 5. growth ----

def test_growth_keeps_every_label():
    tm, tl, _ = _t()
    n, d, step = 2600, 16, 371
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((24, d)).astype(f32)
    col = rng.integers(0, 9, size=n).astype(np.uint32)
    grp = rng.integers(0, 50, size=n).astype(np.uint32)
    s = ehx.Space.unique("col-grow", d, metric=ehx.METRIC_L2SQ, initial_capacity=300)
    cap0 = s.stats()["capacity"]
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        s.set_batch_cols(_keys(r1 - r0, r0), X[r0:r1], {0: col[r0:r1], 2: grp[r0:r1]})
        assert np.array_equal(s.column_get(0, _keys(r1)), col[:r1]), r1   # every label written before the growth
        assert np.array_equal(s.column_get(2, _keys(r1)), grp[:r1]), r1
    assert s.stats()["capacity"] > cap0 and len(s) == n
    want = (np.arange(len(Q)) % 10).astype(np.uint32)                     # label 9: nobody carries it
    om = tm.METRICS["l2"][1]
    _check_by_label(s, Q, 10, 0, col, want, tl._want(X, Q, 10, om, col, want), "after growth")
    # the device forms of the bulk load and read-back
    import torch
    back = torch.zeros(n, dtype=torch.int32, device="cuda")
    s.column_read_device(0, 0, back)
    assert np.array_equal(back.cpu().numpy().view(np.uint32), col)
    s.column_load_device(1, 100, torch.tensor(col[100:900].view(np.int32), device="cuda"))
    s.column_read_device(1, 0, back)
    exp1 = np.full(n, NONE, dtype=np.uint32)
    exp1[100:900] = col[100:900]
    assert np.array_equal(back.cpu().numpy().view(np.uint32), exp1)
    _check_by_label(s, Q, 10, 1, exp1, want, tl._want(X, Q, 10, om, exp1, want), "a loaded column")
    s.drop()


# ---- 6. under streamed appends ----

def case_stream(paused=False):
    """writers append chunks with set_batch_cols while searchers call knn_by_label (host and device form): every answer is
    the oracle's labelled answer over ONE published prefix between the search's start and its return"""
    import torch
    from test_append_under_search import _centres, _chunk_rows, _queries
    d, base, n_chunks, per, k = 128, 20000, 5 if paused else 10, 60, 10   # (paused: every search sleeps, fewer chunks)
    cen = _centres(41, 16, d)
    rng = np.random.default_rng(3)
    Xb = (rng.standard_normal((base, d)).astype(f32) / np.sqrt(f32(d))).astype(f32)
    m = 16 * per - 37                                                   # no boundary on a 256-row tile
    chunks = [_chunk_rows(cen, j, per, lambda j, m, r: 1.0, 9)[:m] for j in range(n_chunks)]
    X = np.concatenate([Xb] + chunks)
    col = rng.integers(1, 4, size=len(X)).astype(np.uint32)             # three tenants, above the scan route's cut
    col[rng.random(len(X)) < 0.1] = 50                                  # ... and a small one on the list route
    bounds = [base + j * m for j in range(n_chunks + 1)]
    Q = _queries(cen, 4, 2)
    want = np.array([1, 2, 3, 50], dtype=np.uint32)[np.arange(len(Q)) % 4]
    # (the capacity holds every chunk: growth under appends is test_growth_keeps_every_label's, and an appending writer that
    # must grow waits for the space's lock behind the searchers for as long as they overlap)
    s = ehx.Space.unique("col-stream", d, metric=ehx.METRIC_COSINE, initial_capacity=len(X) + 256)
    s.set_batch_cols(_keys(base), Xb, {0: col[:base]})
    assert s.scan_engine() == "i8"
    errs, records, stop = [], [], threading.Event()

    def writer():
        try:
            time.sleep(0.05)
            for j in range(n_chunks):
                s.set_batch_cols(_keys(m, bounds[j]), chunks[j], {0: col[bounds[j]:bounds[j + 1]]})
                time.sleep(0.01)
        except Exception as e:  # noqa: BLE001
            errs.append("writer: %r" % (e,))

    def host_searcher():
        try:
            while not stop.is_set():
                lo = len(s)
                ans = s.knn_by_label(Q, k, 0, want)
                records.append((lo, ans, len(s)))
        except Exception as e:  # noqa: BLE001
            errs.append("searcher: %r" % (e,))

    def device_searcher():
        try:
            st = torch.cuda.Stream()
            dq = torch.from_numpy(Q).cuda()
            dw = torch.from_numpy(want.view(np.int32)).cuda()
            ids = torch.empty((len(Q), k), dtype=torch.int64, device="cuda")
            dst = torch.empty((len(Q), k), dtype=torch.float32, device="cuda")
            cnt = torch.empty((len(Q),), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            while not stop.is_set():
                lo = len(s)
                s.knn_by_label_device(dq, k, 0, dw, ids, dst, cnt, stream=st.cuda_stream)
                st.synchronize()
                records.append((lo, (ids.cpu().numpy().astype(np.uint64), dst.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32)),
                                len(s)))
        except Exception as e:  # noqa: BLE001
            errs.append("device searcher: %r" % (e,))

    th = [threading.Thread(target=f) for f in (host_searcher, device_searcher)]
    w = threading.Thread(target=writer)
    for t in th + [w]:
        t.start()
    w.join(timeout=300)
    assert not w.is_alive(), "the writer hung"
    time.sleep(0.05)
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
    final = s.knn_by_label(Q, k, 0, want)
    assert oracle.assert_is_some_prefix(*final, len(X), len(X)) == len(X)
    assert np.array_equal(s.column_get(0, _keys(len(X))), col)
    s.drop()


def test_searches_beside_appends_with_labels():
    case_stream()


def test_searches_beside_appends_with_labels_and_the_pause_knob():
    """the same with EHX_TEST_PAUSE_US set, in a fresh child process (the knob is read once per process)"""
    env = dict(os.environ, EHX_TEST_PAUSE_US=str(PAUSE_US))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "stream"], env=env, cwd=ROOT, timeout=400,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, "the streamed case with the pause knob failed (rc %d):\n%s" % (r.returncode, r.stderr[-6000:])


# ---- 7. errors ----

def test_error_returns():
    rng = np.random.default_rng(8)
    n, d, nq = 200, 8, 3
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    col = (np.arange(n) % 3).astype(np.uint32)
    want = np.array([0, 1, 5], dtype=np.uint32)
    s = ehx.Space.unique("col-err", d, metric=ehx.METRIC_L2SQ, initial_capacity=n)
    s.set_batch_cols(_keys(n), X, {0: col})
    L = _lib.load()
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    code = lambda f: pytest.raises(ehx.EhxError, f).value.code  # noqa: E731
    # the searches: knn_labeled's codes, then the column number
    assert code(lambda: s.knn_by_label(Q, 0, 0, want)) == _lib.EINVAL
    assert code(lambda: s.knn_by_label(Q, 1025, 0, want)) == _lib.EUNSUPPORTED
    assert code(lambda: s.knn_by_label(Q, 4, cc.MAX_COLUMNS, want)) == _lib.EINVAL
    assert code(lambda: s.knn_grouped_by_label(Q, 4, 0, cc.MAX_COLUMNS, want)) == _lib.EINVAL
    assert code(lambda: s.knn_grouped_by_label(Q, 4, cc.MAX_COLUMNS, 0, want)) == _lib.EINVAL
    assert code(lambda: s.knn_grouped_by_label(Q, 4, 1, 0, want, per_group=0)) == _lib.EINVAL
    assert code(lambda: s.knn_grouped_by_label(Q, 257, 1, 0, want)) == _lib.EUNSUPPORTED
    assert s.knn_by_label(Q, 4, 0, want)[2].tolist() == [4, 4, 0]
    assert s.knn_by_label(np.zeros((0, d), dtype=f32), 4, 0, np.zeros(0, dtype=np.uint32))[2].shape == (0,)
    q = np.ascontiguousarray(Q)
    o_ids, o_dist, o_cnt = np.full((nq, 4), 7, dtype=np.uint64), np.full((nq, 4), 7, dtype=f32), np.full(nq, 7, dtype=np.uint32)
    args = [P(o_ids, C.c_uint64), P(o_dist, C.c_float), P(o_cnt, C.c_uint32)]
    for hole in range(3):
        a = list(args)
        a[hole] = None
        assert L.ehx_knn_by_label(s._h, nq, P(q, C.c_float), 4, 0, P(want, C.c_uint32), *a) == _lib.EINVAL
    assert L.ehx_knn_by_label(s._h, nq, None, 4, 0, P(want, C.c_uint32), *args) == _lib.EINVAL
    assert L.ehx_knn_by_label(s._h, nq, P(q, C.c_float), 4, 0, None, *args) == _lib.EINVAL           # NULL want
    assert (o_ids == 7).all() and (o_cnt == 7).all()
    # the writes
    keys = _keys(4)
    assert code(lambda: s.set_batch_cols(keys, X[:4], {cc.MAX_COLUMNS: [1, 2, 3, 4]})) == _lib.EINVAL
    n_, arr, lens, keep = marshal_keys(keys)
    two = (C.POINTER(C.c_uint32) * 2)(P(col, C.c_uint32), P(col, C.c_uint32))
    twice = np.array([1, 1], dtype=np.uint32)
    assert L.ehx_set_batch_cols(s._h, 4, arr, lens, P(np.ascontiguousarray(X[:4]), C.c_float), 2, P(twice, C.c_uint32),
                                two) == _lib.EINVAL                                                   # a column named twice
    assert code(lambda: s.column_set(cc.MAX_COLUMNS, keys, [1, 2, 3, 4])) == _lib.EINVAL
    assert code(lambda: s.column_get(cc.MAX_COLUMNS, keys)) == _lib.EINVAL
    with pytest.raises(ehx.EhxError) as e:                                                           # an unknown key ...
        s.column_set(0, ["k0", "k1", "nobody", "k3"], [9, 9, 9, 9])
    assert e.value.code == _lib.ENOTFOUND and e.value.bad_index == 2
    assert s.column_get(0, ["k0", "k1", "k3"]).tolist() == col[[0, 1, 3]].tolist()                   # ... and nothing written
    with pytest.raises(ehx.EhxError) as e:
        s.column_get(0, ["k0", "nobody"])
    assert e.value.code == _lib.ENOTFOUND and e.value.bad_index == 1
    import torch
    vals = torch.zeros(50, dtype=torch.int32, device="cuda")
    assert code(lambda: s.column_load_device(1, n - 49, vals)) == _lib.EINVAL                        # not below the row count
    assert code(lambda: s.column_read_device(1, n - 49, vals)) == _lib.EINVAL
    assert code(lambda: s.column_load_device(cc.MAX_COLUMNS, 0, vals)) == _lib.EINVAL
    s.column_load_device(1, n - 50, vals)
    # a frozen space refuses the writes and answers the reads and the searches
    s.freeze()
    assert code(lambda: s.set_batch_cols(["new"], X[:1], {0: [1]})) == _lib.EIMMUTABLE
    assert code(lambda: s.column_set(0, ["k0"], [1])) == _lib.EIMMUTABLE
    assert code(lambda: s.column_load_device(1, 0, vals)) == _lib.EIMMUTABLE
    assert s.column_get(0, ["k4"]).tolist() == [int(col[4])] and s.knn_by_label(Q, 4, 0, want)[2].tolist() == [4, 4, 0]
    # a NULL space, before the device is looked for
    assert L.ehx_knn_by_label(None, nq, P(q, C.c_float), 4, 0, P(want, C.c_uint32), *args) == _lib.EINVAL
    assert L.ehx_last_error() == b"space is NULL"
    assert L.ehx_column_set(None, 0, 1, arr, lens, P(col, C.c_uint32), None) == _lib.EINVAL
    assert L.ehx_last_error() == b"space is NULL"
    # a dropped space
    h = s._h
    s.drop()
    assert L.ehx_knn_by_label(h, nq, P(q, C.c_float), 4, 0, P(want, C.c_uint32), *args) == _lib.ENOTFOUND
    assert L.ehx_knn_by_label_device(h, None, nq, P(q, C.c_float), 4, 0, P(want, C.c_uint32), *args) == _lib.ENOTFOUND
    assert L.ehx_knn_grouped_by_label(h, nq, P(q, C.c_float), 4, 1, 1, 0, P(want, C.c_uint32), *args) == _lib.ENOTFOUND
    assert L.ehx_set_batch_cols(h, 4, arr, lens, P(np.ascontiguousarray(X[:4]), C.c_float), 1, P(twice, C.c_uint32),
                                two) == _lib.ENOTFOUND
    assert L.ehx_column_set(h, 0, 4, arr, lens, P(col, C.c_uint32), None) == _lib.ENOTFOUND
    assert L.ehx_column_get(h, 0, 4, arr, lens, P(o_cnt, C.c_uint32), None) == _lib.ENOTFOUND
    assert L.ehx_column_load_device(h, None, 0, 0, 1, vals.data_ptr()) == _lib.ENOTFOUND
    assert L.ehx_column_read_device(h, None, 0, 0, 1, vals.data_ptr()) == _lib.ENOTFOUND
    del keep
    # a row-sharded space
    sh = ehx.Space.unique("col-sh", d, metric=ehx.METRIC_L2SQ, shards=2)
    sh.set_batch(_keys(n), X)
    for f in (lambda: sh.knn_by_label(Q, 4, 0, want), lambda: sh.knn_grouped_by_label(Q, 4, 1, 0, want),
              lambda: sh.set_batch_cols(["x"], X[:1], {0: [1]}), lambda: sh.column_set(0, ["k0"], [1]),
              lambda: sh.column_get(0, ["k0"]), lambda: sh.column_load_device(0, 0, vals),
              lambda: sh.column_read_device(0, 0, vals)):
        with pytest.raises(ehx.EhxError) as e:
            f()
        assert e.value.code == _lib.EUNSUPPORTED and "sharded" in str(e.value)
    sh.drop()


if __name__ == "__main__":
    case_stream(paused=bool(os.environ.get("EHX_TEST_PAUSE_US")))
    print("case stream ok")
