"""GPU tests of the exact range search under row bitmaps (ehx_range_masked, ehx_range_masked_device).

Truth comes from the oracle only: for every mask m of the table, with L_m the ascending list of the rows it allows (below
n_bits and the row count) and Q_m the queries under it, pyoracle.exhaustive(X[L_m], Q_m, k = len(L_m)) lists every allowed row
by (distance, id), its local ids are mapped back through L_m, and the list is cut at `dist <= radius` (range_cases.cut).
Ids must be equal, distance BYTES equal, counts and totals equal, tails the sentinels.  F16 spaces use the oracle on
X.astype(float16).astype(float32).  Shapes, table and the queries' masks: tests/masked_multi_cases.py; truth and radii:
tests/range_masked_cases.py; the cases that pin the route counters are the ones tests/test_range_masked_model.py shows to
stay within half a pool."""
import ctypes as C

import numpy as np
import pytest

import masked_multi_cases as mmc
import range_cases as rc
import range_masked_cases as rmc
from test_knn_masked import METRICS, NO_ID, _i8_space, _keys, _same_bytes
from test_range import _assert_range

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402
from embeddinghub_amd.space import marshal_mask_table  # noqa: E402

f32 = np.float32
MR = rmc.MAX_RESULTS


def _counters(s):
    out = (C.c_uint64 * 5)()
    C.CDLL(_lib.LIB_PATH).ehx_test_range_masked_counters(s._h, out)
    return np.array(list(out), dtype=np.int64)   # scan route, list route, pool overflows, truncated, calls


def _device_form(space, Q, radius, max_results, allows, mask_of, n_bits=None, fill=None):
    import torch
    a = np.asarray(allows)
    words, n_masks, n_bits = marshal_mask_table(a[None] if a.ndim == 1 else a, n_bits)
    nq = len(Q)
    dq = torch.tensor(np.ascontiguousarray(Q, dtype=f32), device="cuda")
    dr = torch.tensor(np.ascontiguousarray(radius, dtype=f32), device="cuda")
    dm = torch.tensor(words.view(np.int32), device="cuda") if words.size else None
    dof = None if mask_of is None else torch.tensor(np.asarray(mask_of, dtype=np.uint32).view(np.int32), device="cuda")
    o_ids = torch.full((nq, max_results), -7, dtype=torch.int64, device="cuda")
    o_dist = torch.full((nq, max_results), -7.0, dtype=torch.float32, device="cuda")
    o_cnt = torch.full((nq,), 77, dtype=torch.int32, device="cuda")
    o_tot = torch.full((nq,), -7, dtype=torch.int64, device="cuda")
    try:
        space.range_masked_device(dq, dr, max_results, dm, n_masks, n_bits, dof, o_ids, o_dist, o_cnt, o_tot)
    finally:
        torch.cuda.synchronize()
        out = (o_ids.cpu().numpy().view(np.uint64), o_dist.cpu().numpy(), o_cnt.cpu().numpy().view(np.uint32),
               o_tot.cpu().numpy().view(np.uint64))
        if fill is not None:
            fill.extend(out)
    return out


def _both_forms(s, Q, r, mr, allows, mask_of, want, what, n_bits=None):
    """host form against the oracle, device form byte for byte the host form's; -> (answer, counter deltas of the host call)"""
    c0 = _counters(s)
    got = s.range_masked(Q, r, mr, allows, mask_of, n_bits)
    dc = _counters(s) - c0
    _assert_range(got, want, mr, what)
    assert _same_bytes(got, _device_form(s, Q, r, mr, allows, mask_of, n_bits)), what + ": host and device forms differ"
    return got, dc


# ---- 1. the table of six: scan route, list route and an empty bitmap in one batch ----

@pytest.mark.parametrize("rows", ["f32", "f16"])
@pytest.mark.parametrize("d", rmc.DIMS)
@pytest.mark.parametrize("metric", mmc.METRICS)
def test_table_of_six(metric, d, rows):
    Xs, Q, tab, of, lists = rmc.six(d, metric, rows)
    X = rc.i8_data(d)[0]
    s = _i8_space("rangem-six", d, metric, X, dtype=ehx.DTYPE_F16 if rows == "f16" else ehx.DTYPE_F32)
    for rank in rmc.RANKS:
        what = "%s d=%d %s rank=%d" % (metric, d, rows, rank)
        r = rmc.radii_at(lists, len(Q), rank)
        got, dc = _both_forms(s, Q, r, MR, tab, of, rmc.want(lists, len(Q), r, MR), what)
        assert ((got[2] == 0) == (of == 4)).all() and ((got[3] == 0) == (of == 4)).all(), what   # empty: ITS queries only
        assert (got[3][of != 4] >= min(rank, 300)).all() and dc[4] == 1, what
        if rank == 300:
            assert (got[2][of != 4] == MR).all() and dc[3] == 80, (what, dc)   # truncated: everybody but the empty mask's
        if rows == "f32" and rmc.pinned(d, metric, rank):   # the model: nobody handed on
            assert dc[:3].tolist() == [64, 32, 0], (what, dc)
        else:
            assert dc[0] + dc[1] >= len(Q), (what, dc)
    assert s.stats()["n_uncertified"] == 0
    s.drop()


# ---- 2. an all-ones mask is the plain range search ----

@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_all_ones_is_range_search(metric):
    d, n = 128, rc.I8_ROWS
    X, Q = rc.i8_data(d)
    Q = Q[:mmc.NQ]
    oids, odist = rc.i8_oracle(d, metric)
    s = _i8_space("rangem-ones", d, metric, X)
    for rank in (1, 100, 300, 5000):   # 5000: the pool overflows on both sides
        r = np.ascontiguousarray(odist[:mmc.NQ, rank - 1])
        plain = s.range_search(Q, r, MR)
        assert (plain[3] >= rank).all()
        for bits in (n, n + 1000):
            got = s.range_masked(Q, r, MR, np.ones(bits, dtype=bool))
            assert _same_bytes(plain, got), (metric, rank, bits)
            assert _same_bytes(plain, _device_form(s, Q, r, MR, np.ones(bits, dtype=bool), None)), (metric, rank, bits)
        # n_bits = 10 000: rows at or above it are never members
        nb = 10000
        got = s.range_masked(Q, r, MR, np.ones(n, dtype=bool), n_bits=nb)
        lists = rmc.lists_under(X, Q, METRICS[metric][1], np.ones((1, nb), dtype=bool), np.zeros(mmc.NQ, dtype=np.uint32))
        _assert_range(got, rmc.want(lists, mmc.NQ, r, MR), MR, "n_bits=%d rank=%d" % (nb, rank))
        assert (got[0][got[0] != NO_ID] < nb).all() and (got[3] <= plain[3]).all()
    s.drop()


# ---- 3. a table matches the one-mask calls ----

def test_every_row_is_the_one_mask_answer_for_its_query_and_bitmap():
    d = 128
    Xs, Q, tab, of, lists = rmc.six(d, "cosine")
    s = _i8_space("rangem-rows", d, "cosine", Xs)
    for rank in (10, 300):
        r = rmc.radii_at(lists, len(Q), rank)
        got = s.range_masked(Q, r, MR, tab, of)
        for m in range(len(mmc.NAMES)):
            at = np.nonzero(of == m)[0]
            alone = s.range_masked(Q[at], r[at], MR, tab[m])   # one bitmap, mask_of None
            assert _same_bytes([g[at] for g in got], alone), (mmc.NAMES[m], rank)
            assert _same_bytes(alone, _device_form(s, Q[at], r[at], MR, tab[m], None)), (mmc.NAMES[m], rank)
    s.drop()


def test_both_routes_give_the_oracle_s_answer_for_every_mask():
    """the bench's hook sends every non-empty mask through the scan, or every mask through its list: the answer is the same"""
    d, metric = 128, "l2"
    Xs, Q, tab, of, lists = rmc.six(d, metric)
    s = _i8_space("rangem-routes", d, metric, Xs)
    hook = C.CDLL(_lib.LIB_PATH).ehx_test_range_masked_route
    hook.argtypes = [C.c_void_p, C.c_uint32]
    r = rmc.radii_at(lists, len(Q), 100)
    want = rmc.want(lists, len(Q), r, MR)
    try:
        hook(s._h, 2)
        _, dc = _both_forms(s, Q, r, MR, tab, of, want, "every mask listed")
        assert dc[:3].tolist() == [0, len(Q), 0], dc
        hook(s._h, 1)
        _, dc = _both_forms(s, Q, r, MR, tab, of, want, "every non-empty mask scanned")
        assert dc[0] > 64 and dc[0] + dc[1] >= len(Q) and dc[1] >= 16, dc   # (the empty mask has nothing to scan)
    finally:
        hook(s._h, 0)
    _, dc = _both_forms(s, Q, r, MR, tab, of, want, "the cut decides again")
    assert dc[:3].tolist() == [64, 32, 0], dc
    s.drop()


# ---- 4. no query is judged by another query's bitmap ----

@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_no_query_is_judged_by_another_query_s_bitmap(metric):
    """masked_multi_cases.parity: every vector stored at rows 2 j and 2 j + 1, mask A the even rows, mask B the odd ones,
    queries alternating; the radius is the exact distance of the query's nearest stored vector, so each answer is the ONE
    row of its own parity — the wrong bitmap shows as the twin's id at the same distance"""
    om = METRICS[metric][1]
    X, Q, tab, of = mmc.parity()
    lists = rmc.lists_under(X, Q, om, tab, of)
    r = rmc.radii_at(lists, len(Q), 1)
    want = rmc.want(lists, len(Q), r, 8)
    assert all(w[2] == 1 and w[0][0] % 2 == int(of[i]) for i, w in enumerate(want))
    s = _i8_space("rangem-parity", X.shape[1], metric, X)
    got, dc = _both_forms(s, Q, r, 8, tab, of, want, "parity " + metric)
    assert (got[2] == 1).all() and ((got[0][:, 0] % np.uint64(2)) == of.astype(np.uint64)).all()
    assert dc[0] + dc[1] >= len(Q) and dc[0] > 0
    s.drop()


# ---- 5. overflow and radii the scan does not serve ----

def test_overflow_and_unserved_radii():
    d, metric, nq = 128, "cosine", 8
    Xs, Q, tab, of, _ = rmc.six(d, metric)
    om = METRICS[metric][1]
    Q = np.ascontiguousarray(Q[:nq])
    zeros = np.zeros(nq, dtype=np.uint32)
    s = _i8_space("rangem-over", d, metric, Xs)
    inf = np.full(nq, np.inf, dtype=f32)
    # +Inf under "half": 10 000 > kPoolCap members — the scan does not serve the radius, the list's pool overflows
    half = tab[0]
    lists = rmc.lists_under(Xs, Q, om, half[None], zeros)
    n_half = int(half.sum())
    assert n_half > rmc.POOL
    got, dc = _both_forms(s, Q, inf, MR, half, None, rmc.want(lists, nq, inf, MR), "+Inf under half")
    assert (got[3] == n_half).all() and dc.tolist() == [0, nq, nq, nq, 1], dc
    # a finite radius at the 5 000th allowed distance under "ones": the scan route's pool overflows
    ones = tab[5]
    lists = rmc.lists_under(Xs, Q, om, ones[None], zeros)
    r = rmc.radii_at(lists, nq, 5000)
    got, dc = _both_forms(s, Q, r, MR, ones, None, rmc.want(lists, nq, r, MR), "5000th distance under ones")
    assert (got[3] >= 5000).all() and dc.tolist() == [0, nq, nq, nq, 1], dc
    # +Inf under "few": the list route, every allowed row returned, nothing overflows
    few = tab[3]
    lists = rmc.lists_under(Xs, Q, om, few[None], zeros)
    got, dc = _both_forms(s, Q, inf, 512, few, None, rmc.want(lists, nq, inf, 512), "+Inf under few")
    assert (got[2] == 300).all() and (got[3] == 300).all() and dc.tolist() == [0, nq, 0, 0, 1], dc
    # NaN and -Inf: empty answers, whatever the mask; a mixed batch keeps every query's own radius
    r = np.array([np.nan, -np.inf, np.nan, -np.inf, np.inf, np.inf, np.nan, -np.inf], dtype=f32)
    mo = np.array([0, 0, 1, 1, 0, 1, 1, 0], dtype=np.uint32)
    pair = np.stack([half, few])
    lists = rmc.lists_under(Xs, Q, om, pair, mo)
    got, dc = _both_forms(s, Q, r, MR, pair, mo, rmc.want(lists, nq, r, MR), "non-finite radii")
    assert got[3].tolist() == [0, 0, 0, 0, n_half, 300, 0, 0]
    assert dc[2] == 1 and dc[0] + dc[1] >= nq
    s.drop()


# ---- 6. spaces off the int8 engine ----

@pytest.mark.parametrize("kind", ["flat_f32", "flat_f16", "graph_f32"])
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_small_and_graph_spaces_answer_from_the_list_route(metric, kind):
    em, om = METRICS[metric]
    n, d, nq = 4000, 128, 21
    rng = np.random.default_rng(411)
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    kw = {"mode": ehx.MODE_GRAPH, "M": 16} if kind == "graph_f32" else {}
    s = ehx.Space.unique("rangem-small", d, metric=em, initial_capacity=n,
                         dtype=ehx.DTYPE_F16 if kind == "flat_f16" else ehx.DTYPE_F32, **kw)
    s.set_batch(_keys(n), X)
    Xs = rmc.rows_as_stored(X, "f16" if kind == "flat_f16" else "f32")
    tab = np.stack([rng.random(n) < 0.5, rng.random(n) < 0.02, np.zeros(n, dtype=bool), np.ones(n, dtype=bool)])
    of = mmc.interleaved(nq, 4)[::-1].copy()
    lists = rmc.lists_under(Xs, Q, om, tab, of)
    for rank, mr in ((1, 4), (10, 64), (70, 64), (300, 1024)):
        r = rmc.radii_at(lists, nq, rank)
        what = "%s %s rank=%d" % (kind, metric, rank)
        got, dc = _both_forms(s, Q, r, mr, tab, of, rmc.want(lists, nq, r, mr), what)
        assert dc[:3].tolist() == [0, nq, 0] and dc[4] == 1, (what, dc)
    s.drop()


# ---- 7. refusals ----

def test_error_returns():
    rng = np.random.default_rng(8)
    n, d, nq = 200, 8, 3
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    tab = np.ones((2, n), dtype=bool)
    of = np.array([0, 1, 0], dtype=np.uint32)
    s = ehx.Space.unique("rangem-err", d, metric=ehx.METRIC_L2SQ, initial_capacity=n)
    s.set_batch(_keys(n), X)
    for mr, code in ((0, _lib.EINVAL), (1025, _lib.EUNSUPPORTED)):
        with pytest.raises(ehx.EhxError) as e:
            s.range_masked(Q, 1.0, mr, tab, of)
        assert e.value.code == code
    with pytest.raises(ehx.EhxError) as e:                           # 65 bitmaps
        s.range_masked(Q, 1.0, 4, np.ones((65, n), dtype=bool), of)
    assert e.value.code == _lib.EUNSUPPORTED
    with pytest.raises(ehx.EhxError) as e:                           # no bitmap at all
        s.range_masked(Q, 1.0, 4, np.ones((0, n), dtype=bool), of)
    assert e.value.code == _lib.EINVAL
    got = s.range_masked(Q, np.inf, 4, np.ones((64, n), dtype=bool), np.array([63, 0, 31], dtype=np.uint32))   # 64 are served
    assert _same_bytes(got, s.range_search(Q, np.inf, 4))
    ids, dist, cnt, total = s.range_masked(np.zeros((0, d), dtype=f32), 1.0, 4, tab, np.zeros(0, dtype=np.uint32))   # no queries
    assert ids.shape == (0, 4) and cnt.shape == (0,) and total.shape == (0,)
    got = s.range_masked(Q, np.inf, 4, np.zeros((2, 0), dtype=bool), of)   # n_bits == 0: NULL masks, empty answers
    assert (got[2] == 0).all() and (got[3] == 0).all() and (got[0] == NO_ID).all() and np.isposinf(got[1]).all()
    with pytest.raises(ValueError):
        s.range_masked(Q, 1.0, 4, tab, of[:2])
    with pytest.raises(ValueError):
        s.range_masked(Q, 1.0, 4, tab)                               # a table of two needs mask_of
    # a mask_of entry equal to n_masks: EINVAL in both forms, the outputs untouched
    bad = np.array([0, 2, 1], dtype=np.uint32)
    L = _lib.load()
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    q, rad = np.ascontiguousarray(Q), np.full(nq, np.inf, dtype=f32)
    words = marshal_mask_table(tab)[0]
    o_ids, o_dist = np.full((nq, 4), 7, dtype=np.uint64), np.full((nq, 4), 7, dtype=f32)
    o_cnt, o_tot = np.full(nq, 7, dtype=np.uint32), np.full(nq, 7, dtype=np.uint64)
    args = [P(o_ids, C.c_uint64), P(o_dist, C.c_float), P(o_cnt, C.c_uint32), P(o_tot, C.c_uint64)]
    call = lambda a_q, a_r, a_w, a_of, a, n_masks=2: L.ehx_range_masked(s._h, nq, a_q, a_r, 4, a_w, n_masks, n, a_of, *a)  # noqa: E731
    pq, pr, pw, pof = P(q, C.c_float), P(rad, C.c_float), P(words, C.c_uint32), P(of, C.c_uint32)
    assert call(pq, pr, pw, P(bad, C.c_uint32), args) == _lib.EINVAL
    assert b"mask_of[1]" in L.ehx_last_error()
    assert (o_ids == 7).all() and (o_dist == 7).all() and (o_cnt == 7).all() and (o_tot == 7).all()
    out = []
    with pytest.raises(ehx.EhxError) as e:
        _device_form(s, Q, rad, 4, tab, bad, fill=out)
    assert e.value.code == _lib.EINVAL and "mask_of[1]" in str(e.value)
    assert (out[0].view(np.int64) == -7).all() and (out[1] == -7).all() and (out[2].view(np.int32) == 77).all()
    assert (out[3].view(np.int64) == -7).all()
    # NULLs
    for hole in range(3):
        a = list(args)
        a[hole] = None
        assert call(pq, pr, pw, pof, a) == _lib.EINVAL
    assert call(None, pr, pw, pof, args) == _lib.EINVAL
    assert call(pq, None, pw, pof, args) == _lib.EINVAL
    assert call(pq, pr, None, pof, args) == _lib.EINVAL              # NULL masks with n_bits > 0
    assert call(pq, pr, pw, None, args) == _lib.EINVAL               # NULL mask_of with two bitmaps
    assert call(pq, pr, pw, pof, args, n_masks=0) == _lib.EINVAL     # no bitmap, with queries
    assert L.ehx_range_masked(None, nq, pq, pr, 4, pw, 2, n, pof, *args) == _lib.EINVAL
    assert L.ehx_range_masked_device(s._h, None, nq, None, None, 4, None, 2, n, None, None, None, None, None) == _lib.EINVAL
    assert L.ehx_range_masked(s._h, 0, None, None, 4, None, 0, 0, None, *args) == _lib.OK   # no queries
    assert call(pq, pr, pw, None, args, n_masks=1) == _lib.OK and (o_cnt == 4).all() and (o_tot == n).all()   # a table of one
    assert call(pq, pr, pw, pof, args[:3] + [None]) == _lib.OK      # out_total may be NULL
    h = s._h
    s.drop()   # the tombstone answers for the dropped handle
    assert L.ehx_range_masked(h, nq, pq, pr, 4, pw, 2, n, pof, *args) == _lib.ENOTFOUND
    sh = ehx.Space.unique("rangem-sh", d, metric=ehx.METRIC_L2SQ, shards=2)
    sh.set_batch(_keys(n), X)
    with pytest.raises(ehx.EhxError) as e:
        sh.range_masked(Q, 1.0, 4, tab, of)
    assert e.value.code == _lib.EUNSUPPORTED and "sharded" in str(e.value)
    sh.drop()


def test_stats_deltas():
    rng = np.random.default_rng(9)
    n, d, nq = 1000, 16, 12
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    tab = np.stack([rng.random(n) < 0.3, rng.random(n) < 0.6])
    of = mmc.interleaved(nq, 2)
    s = ehx.Space.unique("rangem-stats", d, metric=ehx.METRIC_L2SQ, initial_capacity=n)
    s.set_batch(_keys(n), X)
    st0 = s.stats()
    s.range_masked(Q, 20.0, 5, tab, of)
    st1 = s.stats()   # the list route: every query against every row its own mask allows
    assert st1["n_queries"] - st0["n_queries"] == nq
    assert st1["n_dist"] - st0["n_dist"] == (nq // 2) * int(tab[0].sum() + tab[1].sum())
    assert st1["n_rerank"] == st0["n_rerank"] and st1["n_uncertified"] == 0
    s.drop()
