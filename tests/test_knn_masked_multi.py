"""GPU tests of the exact kNN under a table of row bitmaps, one per query (ehx_knn_masked_multi, ehx_knn_masked_multi_device).

Truth comes from the oracle only: for every mask m of the table, with L_m the ascending list of the rows it allows (below
n_bits and the row count) and Q_m the queries searched under it, pyoracle.exhaustive(X[L_m], Q_m, k) answers and its local ids
are mapped back through L_m.  Ids must be equal and distance BYTES equal, tails the sentinels.  F16 spaces use the oracle on
X.astype(float16).astype(float32).  Shapes, table and queries' masks: tests/masked_multi_cases.py; the cases that pin the
route counters ("no query handed on") are the ones tests/test_masked_multi_model.py shows to stay within half a pool — the
non-finite cases pin none: whatever route a query takes there, its answer must be the oracle's."""
import ctypes as C

import numpy as np
import pytest

import masked_multi_cases as mmc
import range_cases as rc
import side_extreme_cases as sx
import test_masked_multi_model as model
from test_knn_masked import METRICS, NO_ID, _assert_rows, _counters, _expected, _i8_space, _keys, _same_bytes

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402
from embeddinghub_amd.space import marshal_mask_table  # noqa: E402

f32 = np.float32


def _want(X, Q, k, om, tab, mask_of):
    """per query (ids, dist) of the oracle over the rows its own mask allows; tab: bool [masks, <= rows]"""
    out = [None] * len(Q)
    for m in np.unique(mask_of):
        at = np.nonzero(mask_of == m)[0]
        for i, w in zip(at, _expected(X, np.ascontiguousarray(Q[at]), k, om, tab[m])):
            out[i] = w
    return out


def _cut(want, k):
    return [(ids[:k], dist[:k]) for ids, dist in want]


def _device_form(space, Q, k, allows, mask_of, n_bits=None, fill=None):
    import torch
    words, n_masks, n_bits = marshal_mask_table(allows, n_bits)
    dq = torch.tensor(np.ascontiguousarray(Q, dtype=f32), device="cuda")
    dm = torch.tensor(words.view(np.int32), device="cuda") if words.size else None
    dof = torch.tensor(np.asarray(mask_of, dtype=np.uint32).view(np.int32), device="cuda")
    o_ids = torch.full((len(Q), k), -7, dtype=torch.int64, device="cuda")
    o_dist = torch.full((len(Q), k), -7.0, dtype=torch.float32, device="cuda")
    o_cnt = torch.full((len(Q),), 77, dtype=torch.int32, device="cuda")
    try:
        space.knn_masked_multi_device(dq, k, dm, n_masks, n_bits, dof, o_ids, o_dist, o_cnt)
    finally:
        torch.cuda.synchronize()
        out = (o_ids.cpu().numpy().view(np.uint64), o_dist.cpu().numpy(), o_cnt.cpu().numpy().view(np.uint32))
        if fill is not None:
            fill.extend(out)
    return out


def _both_forms(s, Q, k, allows, mask_of, want, what, n_bits=None):
    """host form against the oracle, device form byte for byte the host form's; -> (answer, counter deltas of the host call)"""
    c0 = _counters(s)
    got = s.knn_masked_multi(Q, k, allows, mask_of, n_bits)
    dc = _counters(s) - c0
    _assert_rows(got, want, what)
    assert _same_bytes(got, _device_form(s, Q, k, allows, mask_of, n_bits)), what + ": host and device forms differ"
    return got, dc


# ---- the table of six: scan route, exact route and an empty bitmap in one batch ----

@pytest.mark.parametrize("rows", ["f32", "f16"])
@pytest.mark.parametrize("d", rc.I8_DIMS)
@pytest.mark.parametrize("metric", mmc.METRICS)
def test_table_of_six(metric, d, rows):
    om = METRICS[metric][1]
    X, Q = rc.i8_data(d)
    Q = Q[:mmc.NQ]
    tab, of = mmc.table(), mmc.interleaved(mmc.NQ, len(mmc.NAMES))
    s = _i8_space("maskedq-six", d, metric, X, dtype=ehx.DTYPE_F16 if rows == "f16" else ehx.DTYPE_F32)
    Xs = X.astype(np.float16).astype(f32) if rows == "f16" else X
    want_all = _want(Xs, Q, mmc.EXACT_K, om, tab, of)
    n_scan = int(mmc.scans(tab)[of].sum())
    assert n_scan == 64
    for k in mmc.KS + (mmc.EXACT_K,):
        what = "%s d=%d %s k=%d" % (metric, d, rows, k)
        got, dc = _both_forms(s, Q, k, tab, of, _cut(want_all, k), what)
        assert (got[2][of == 4] == 0).all() and (got[2][of == 3] == min(k, 300)).all(), what   # empty: ITS queries only
        if k <= 48:   # the model: nobody handed on, the batch's two passes
            assert dc.tolist() == [n_scan, mmc.NQ - n_scan, 0, len(mmc.passes(tab, of)), 1], (what, dc)
        else:
            assert dc.tolist() == [0, mmc.NQ, 0, 0, 1], (what, dc)
    assert s.stats()["n_uncertified"] == 0
    s.drop()


def test_every_row_is_knn_masked_s_answer_for_its_query_and_bitmap():
    d, k = 128, 10
    X, Q = rc.i8_data(d)
    Q = Q[:mmc.NQ]
    tab, of = mmc.table(), mmc.interleaved(mmc.NQ, len(mmc.NAMES))
    s = _i8_space("maskedq-rows", d, "cosine", X)
    got = s.knn_masked_multi(Q, k, tab, of)
    for m in range(len(mmc.NAMES)):
        at = np.nonzero(of == m)[0]
        alone = s.knn_masked(Q[at], k, tab[m])
        assert _same_bytes([g[at] for g in got], alone), mmc.NAMES[m]
    s.drop()


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_no_query_is_judged_by_another_query_s_bitmap(metric):
    """masked_multi_cases.parity: every vector stored at rows 2 j and 2 j + 1, mask A the even rows, mask B the odd ones,
    queries alternating — the wrong bitmap shows as an id of the wrong parity at the right distance"""
    om = METRICS[metric][1]
    X, Q, tab, of = mmc.parity()
    s = _i8_space("maskedq-parity", X.shape[1], metric, X)
    for k in mmc.KS:
        what = "parity %s k=%d" % (metric, k)
        got, dc = _both_forms(s, Q, k, tab, of, _want(X, Q, k, om, tab, of), what)
        assert (got[2] == k).all() and ((got[0] % np.uint64(2)) == of[:, None].astype(np.uint64)).all(), what
        assert dc.tolist() == [mmc.NQ, 0, 0, len(mmc.passes(tab, of)), 1], (what, dc)
    s.drop()


@pytest.mark.parametrize("d", [128, 768])
def test_one_mask_equals_knn_masked_byte_for_byte(d):
    X, Q = rc.i8_data(d)
    Q = Q[:mmc.NQ]
    s = _i8_space("maskedq-one", d, "cosine", X)
    zeros = np.zeros(mmc.NQ, dtype=np.uint32)
    for name in ("half", "few", "empty"):
        allowed = mmc.table()[mmc.NAMES.index(name)]
        for k in (10, 48, mmc.EXACT_K):
            c0 = _counters(s)
            one = s.knn_masked(Q, k, allowed)
            c1 = _counters(s)
            multi = s.knn_masked_multi(Q, k, allowed[None, :], zeros)
            c2 = _counters(s)
            assert _same_bytes(one, multi), (name, k)
            assert (c1 - c0).tolist() == (c2 - c1).tolist(), (name, k)
            assert _same_bytes(one, _device_form(s, Q, k, allowed[None, :], zeros)), (name, k)
    s.drop()


def test_two_identical_bitmaps_equal_knn_masked_byte_for_byte():
    """One mask runs the flush with the batch's ONE bitmap on both sides of the test above; a table of TWO identical bitmaps,
    the queries' masks interleaved, runs the flush with a bitmap per query (and the grouping by mask) against it.  Identical
    bitmaps give the identical pointwise maximum, so the passes — and every other counter — are knn_masked's too."""
    d = 128
    X, Q = rc.i8_data(d)
    Q = Q[:mmc.NQ]
    s = _i8_space("masked-twins", d, "cosine", X)
    of = mmc.interleaved(mmc.NQ, 2)
    for name in ("half", "few", "empty"):
        allowed = mmc.table()[mmc.NAMES.index(name)]
        twins = np.stack([allowed, allowed])
        for k in (10, 48, mmc.EXACT_K):
            c0 = _counters(s)
            one = s.knn_masked(Q, k, allowed)
            c1 = _counters(s)
            multi = s.knn_masked_multi(Q, k, twins, of)
            c2 = _counters(s)
            assert _same_bytes(one, multi), (name, k)
            assert (c1 - c0).tolist() == (c2 - c1).tolist(), (name, k)
            dev = _device_form(s, Q, k, twins, of)
            assert _same_bytes(one, dev), (name, k)
            assert (_counters(s) - c2).tolist() == (c1 - c0).tolist(), (name, k)
    s.drop()


# ---- rows the bitmaps do not cover ----

def test_n_bits_below_the_row_count_and_not_a_multiple_of_32():
    metric, d = "cosine", 128
    om = METRICS[metric][1]
    X, Q = rc.i8_data(d)
    Q = Q[:mmc.NQ]
    nb = model.N_BITS
    tab, of = mmc.table(), mmc.interleaved(mmc.NQ, len(mmc.NAMES))
    cut = tab[:, :nb]
    s = _i8_space("maskedq-bits", d, metric, X)
    # packed words whose last word still holds the bits of rows beyond n_bits, and whole words behind it
    words = marshal_mask_table(tab)[0][:, :(nb + 31) // 32 + 3]
    assert nb % 32 and (words[5, nb // 32] >> np.uint32(nb % 32)) != 0
    for k in (10, 48):
        what = "n_bits=%d k=%d" % (nb, k)
        want = _want(X, Q, k, om, cut, of)
        got, dc = _both_forms(s, Q, k, words, of, want, what + " packed", n_bits=nb)
        assert (got[0][got[0] != NO_ID] < nb).all(), what
        n_scan = int(mmc.scans(cut, len(X))[of].sum())
        assert n_scan == 48 and dc.tolist() == [n_scan, mmc.NQ - n_scan, 0, len(mmc.passes(cut, of)), 1], (what, dc)
        assert _same_bytes(got, s.knn_masked_multi(Q, k, tab, of, nb)), what + ": bool table with n_bits"
    s.drop()


def test_rows_appended_after_the_masks_were_built_never_appear():
    metric, d, k = "l2", 128, 10
    om = METRICS[metric][1]
    X, Q = rc.i8_data(d)
    Q = Q[:mmc.NQ]
    n0, n1 = model.APPEND_ROWS, rc.I8_ROWS
    of = mmc.interleaved(mmc.NQ, len(mmc.NAMES))
    built = mmc.table()[:, :n0]                                   # masks built while the space held n0 rows
    s = _i8_space("maskedq-append", d, metric, X[:n0], cap=n1)
    want = _want(X[:n0], Q, k, om, built, of)
    before, _ = _both_forms(s, Q, k, built, of, want, "before the append")
    s.set_batch(_keys(n1 - n0, n0), Q[np.arange(n1 - n0) % mmc.NQ])   # the queries themselves: nearer than any old row
    after, dc = _both_forms(s, Q, k, built, of, want, "after the append")
    assert _same_bytes(before, after) and (after[0][after[0] != NO_ID] < n0).all()
    assert dc.tolist() == [64, 32, 0, len(mmc.passes(built, of)), 1], dc
    grown = np.ones((1, n1), dtype=bool)                           # ... a bitmap that names them finds them
    ids = s.knn_masked_multi(Q, 1, grown, np.zeros(mmc.NQ, dtype=np.uint32))[0]
    assert (ids[:, 0] >= n0).all()
    s.drop()


# ---- spaces off the int8 engine ----

@pytest.mark.parametrize("kind", ["flat_f32", "flat_f16", "graph_f32"])
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_small_and_graph_spaces_answer_from_their_stored_rows(metric, kind):
    em, om = METRICS[metric]
    n, d, nq = 3000, 24, 21
    rng = np.random.default_rng(410)
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    kw = {"mode": ehx.MODE_GRAPH, "M": 16} if kind == "graph_f32" else {}
    s = ehx.Space.unique("maskedq-small", d, metric=em, initial_capacity=n,
                         dtype=ehx.DTYPE_F16 if kind == "flat_f16" else ehx.DTYPE_F32, **kw)
    s.set_batch(_keys(n), X)
    Xs = X.astype(np.float16).astype(f32) if kind == "flat_f16" else X
    tab = np.stack([rng.random(n) < 0.5, rng.random(n) < 0.02, np.zeros(n, dtype=bool), np.ones(n, dtype=bool)])
    of = mmc.interleaved(nq, 4)[::-1].copy()
    for k in (1, 10, 100):
        got, dc = _both_forms(s, Q, k, tab, of, _want(Xs, Q, k, om, tab, of), "%s %s k=%d" % (kind, metric, k))
        assert dc.tolist() == [0, nq, 0, 0, 1], dc
    s.drop()


# ---- values ----

@pytest.mark.parametrize("kind", ["g", "f"])
@pytest.mark.parametrize("metric", sx.METRICS)
def test_non_finite_rows_and_zero_rows(kind, metric):
    """side_extreme_cases.ladder: ordinary rows and a block of rows with one NaN / -NaN / +Inf / -Inf component (g: the space
    stays on the exact kernels) or of zero rows (f: an int8 space, the scan route), queries near block rows and a zero
    query among ordinary ones; bitmaps: sx.bitmaps' 50 % and <= 1024 rows with a part of the block, every row, none"""
    em, om = METRICS[metric]
    X, Q = sx.ladder(kind, metric)
    n = len(X)
    half, few = sx.bitmaps(n, 1)
    tab = np.stack([half, few, np.ones(n, dtype=bool), np.zeros(n, dtype=bool)])
    of = mmc.interleaved(len(Q), 4)
    s = ehx.Space.unique("maskedq-%s" % kind, X.shape[1], metric=em, initial_capacity=n)
    s.set_batch(_keys(n), X)
    assert s.scan_engine() == ("i8" if kind == "f" else "f32")
    for k in sx.MASKED_KS:
        what = "ladder %s %s k=%d" % (kind, metric, k)
        got, dc = _both_forms(s, Q, k, tab, of, _want(X, Q, k, om, tab, of), what)
        assert dc[0] + dc[1] == len(Q) and dc[4] == 1, (what, dc)
        if kind == "g":
            assert dc.tolist() == [0, len(Q), 0, 0, 1], (what, dc)
    assert s.stats()["n_uncertified"] == 0
    s.drop()


# ---- errors and accounting ----

def test_error_returns():
    rng = np.random.default_rng(8)
    n, d, nq = 200, 8, 3
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    tab = np.ones((2, n), dtype=bool)
    of = np.array([0, 1, 0], dtype=np.uint32)
    s = ehx.Space.unique("maskedq-err", d, metric=ehx.METRIC_L2SQ, initial_capacity=n)
    s.set_batch(_keys(n), X)
    for k, code in ((0, _lib.EINVAL), (1025, _lib.EUNSUPPORTED)):
        with pytest.raises(ehx.EhxError) as e:
            s.knn_masked_multi(Q, k, tab, of)
        assert e.value.code == code
    with pytest.raises(ehx.EhxError) as e:                           # 65 bitmaps
        s.knn_masked_multi(Q, 4, np.ones((65, n), dtype=bool), of)
    assert e.value.code == _lib.EUNSUPPORTED
    with pytest.raises(ehx.EhxError) as e:                           # no bitmap at all
        s.knn_masked_multi(Q, 4, np.ones((0, n), dtype=bool), of)
    assert e.value.code == _lib.EINVAL
    got = s.knn_masked_multi(Q, 4, np.ones((64, n), dtype=bool), np.array([63, 0, 31], dtype=np.uint32))   # 64 are served
    assert _same_bytes(got, s.knn(Q, 4))
    ids, dist, cnt = s.knn_masked_multi(np.zeros((0, d), dtype=f32), 4, tab, np.zeros(0, dtype=np.uint32))   # no queries
    assert ids.shape == (0, 4) and cnt.shape == (0,)
    with pytest.raises(ValueError):
        s.knn_masked_multi(Q, 4, tab, of[:2])
    # a mask_of entry equal to n_masks: EINVAL in both forms, the outputs untouched
    bad = np.array([0, 2, 1], dtype=np.uint32)
    L = _lib.load()
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    q = np.ascontiguousarray(Q)
    words = marshal_mask_table(tab)[0]
    o_ids, o_dist, o_cnt = np.full((nq, 4), 7, dtype=np.uint64), np.full((nq, 4), 7, dtype=f32), np.full(nq, 7, dtype=np.uint32)
    args = [P(o_ids, C.c_uint64), P(o_dist, C.c_float), P(o_cnt, C.c_uint32)]
    call = lambda a_q, a_w, a_of, a: L.ehx_knn_masked_multi(s._h, nq, a_q, 4, a_w, 2, n, a_of, a[0], a[1], a[2])  # noqa: E731
    assert call(P(q, C.c_float), P(words, C.c_uint32), P(bad, C.c_uint32), args) == _lib.EINVAL
    assert b"mask_of[1]" in L.ehx_last_error()
    assert (o_ids == 7).all() and (o_dist == 7).all() and (o_cnt == 7).all()
    out = []
    with pytest.raises(ehx.EhxError) as e:
        _device_form(s, Q, 4, tab, bad, fill=out)
    assert e.value.code == _lib.EINVAL and "mask_of[1]" in str(e.value)
    assert (out[0].view(np.int64) == -7).all() and (out[1] == -7).all() and (out[2].view(np.int32) == 77).all()
    # NULLs
    for hole in range(3):
        a = list(args)
        a[hole] = None
        assert call(P(q, C.c_float), P(words, C.c_uint32), P(of, C.c_uint32), a) == _lib.EINVAL
    assert call(None, P(words, C.c_uint32), P(of, C.c_uint32), args) == _lib.EINVAL
    assert call(P(q, C.c_float), None, P(of, C.c_uint32), args) == _lib.EINVAL           # NULL masks with n_bits > 0
    assert call(P(q, C.c_float), P(words, C.c_uint32), None, args) == _lib.EINVAL        # NULL mask_of
    assert L.ehx_knn_masked_multi_device(s._h, None, nq, None, 4, None, 2, n, None, None, None, None) == _lib.EINVAL
    assert call(P(q, C.c_float), P(words, C.c_uint32), P(of, C.c_uint32), args) == _lib.OK and (o_cnt == 4).all()
    h = s._h
    s.drop()   # the tombstone answers for the dropped handle
    assert L.ehx_knn_masked_multi(h, nq, P(q, C.c_float), 4, P(words, C.c_uint32), 2, n, P(of, C.c_uint32), *args) == _lib.ENOTFOUND
    sh = ehx.Space.unique("maskedq-sh", d, metric=ehx.METRIC_L2SQ, shards=2)
    sh.set_batch(_keys(n), X)
    with pytest.raises(ehx.EhxError) as e:
        sh.knn_masked_multi(Q, 4, tab, of)
    assert e.value.code == _lib.EUNSUPPORTED and "sharded" in str(e.value)
    sh.drop()


def test_stats_deltas():
    rng = np.random.default_rng(9)
    n, d, nq = 1000, 16, 12
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    tab = np.stack([rng.random(n) < 0.3, rng.random(n) < 0.6])
    of = mmc.interleaved(nq, 2)
    s = ehx.Space.unique("maskedq-stats", d, metric=ehx.METRIC_L2SQ, initial_capacity=n)
    s.set_batch(_keys(n), X)
    st0 = s.stats()
    s.knn_masked_multi(Q, 5, tab, of)
    st1 = s.stats()   # the exact route: every query against every row its own mask allows
    assert st1["n_queries"] - st0["n_queries"] == nq
    assert st1["n_dist"] - st0["n_dist"] == (nq // 2) * int(tab[0].sum() + tab[1].sum())
    assert st1["n_rerank"] == st0["n_rerank"] and st1["n_uncertified"] == 0
    s.drop()
    X8, Q8 = rc.i8_data(128)
    # the dense masks of the table of six with the queries the model paired them with: nobody takes the exact route
    at = np.array([i for i in range(mmc.NQ) if i % 6 in (0, 1, 5)])
    dense = mmc.table()[[0, 1, 5]]
    of = np.array([{0: 0, 1: 1, 5: 2}[i % 6] for i in at], dtype=np.uint32)
    s = _i8_space("maskedq-stats8", 128, "cosine", X8)
    st0, c0 = s.stats(), _counters(s)
    s.knn_masked_multi(Q8[at], 10, dense, of)
    st1, dc = s.stats(), _counters(s) - c0   # the scan route: every query once; samples and re-ranked rows, not list scans
    assert dc.tolist() == [len(at), 0, 0, 2, 1], dc
    assert st1["n_queries"] - st0["n_queries"] == len(at)
    lists = sum(int(dense[m].sum()) for m in of)
    assert len(at) * 200 < st1["n_dist"] - st0["n_dist"] < lists // 4
    assert st1["n_uncertified"] == 0 and st1["n_i8_queries"] == st0["n_i8_queries"]
    assert st1["n_i8_fallback"] == st0["n_i8_fallback"] and st1["n_rerank"] == st0["n_rerank"]
    s.drop()
