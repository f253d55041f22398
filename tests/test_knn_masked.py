"""GPU tests of the exact kNN under a row bitmap (ehx_knn_masked, ehx_knn_masked_device).

Expected answers come from the oracle only: with L the ascending list of allowed rows (below n_bits and the row count),
pyoracle.exhaustive(X[L], Q, k, metric) answers and its local ids are mapped back through L — tie order by local id is tie
order by global id.  Ids must be equal and distance BYTES equal, tails the sentinels.  F16 spaces use the oracle on
X.astype(float16).astype(float32).  The int8 cases (data: tests/range_cases.py, bitmaps: tests/masked_cases.py; the merge
cases: masked_cases.merge_cases) are the ones tests/test_masked_model.py shows to stay within half a pool."""
import ctypes as C

import numpy as np
import pytest

import largek_cases as lc
import masked_cases as mc
import range_cases as rc
from oracle import pyoracle

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402
from embeddinghub_amd.space import marshal_mask  # noqa: E402

METRICS = {"l2": (ehx.METRIC_L2SQ, pyoracle.METRIC_L2), "ip": (ehx.METRIC_IP, pyoracle.METRIC_IP),
           "cosine": (ehx.METRIC_COSINE, pyoracle.METRIC_COSINE)}
NO_ID = np.uint64(2**64 - 1)
f32 = np.float32


def _keys(n, first=0):
    return ["k%d" % i for i in range(first, first + n)]


def _raw():
    return C.CDLL(_lib.LIB_PATH)


def _counters(s):
    out = (C.c_uint64 * 5)()
    _raw().ehx_test_masked_counters(s._h, out)
    return np.array(list(out), dtype=np.int64)   # scan route, exact route, overflowed, scan passes, calls


def _live():
    out = (C.c_uint64 * 4)()
    _raw().ehx_test_live_resources(out)
    return list(out)


def _expected(X, Q, k, om, allowed):
    """(ids [nq, <= k] per query, dist) of the oracle over the allowed rows; allowed: bool over (a prefix of) the rows"""
    L = np.nonzero(np.asarray(allowed)[:X.shape[0]])[0]
    if L.size == 0:
        return [([], np.zeros(0, dtype=f32)) for _ in range(len(Q))]
    oi, od, oc = pyoracle.exhaustive(np.ascontiguousarray(X[L]), Q, k, om)
    return [([int(v) for v in L[oi[i, :int(oc[i])].astype(np.int64)]], od[i, :int(oc[i])].copy()) for i in range(len(Q))]


def _cut(want, nq, k):
    return [(ids[:k], dist[:k]) for ids, dist in want[:nq]]


def _assert_rows(got, want, what):
    ids, dist, cnt = got
    assert len(cnt) == len(want)
    k = ids.shape[1]
    for i, (wids, wdist) in enumerate(want):
        c = int(cnt[i])
        assert c == len(wids), "%s: query %d has %d results, the oracle %d" % (what, i, c, len(wids))
        assert [int(v) for v in ids[i, :c]] == wids, "%s: query %d ids differ" % (what, i)
        assert dist[i, :c].tobytes() == wdist.tobytes(), "%s: query %d distance bytes differ" % (what, i)
        assert (ids[i, c:k] == NO_ID).all() and np.isposinf(dist[i, c:k]).all(), "%s: query %d tail sentinels" % (what, i)


def _device_form(space, Q, k, allowed, n_bits=None):
    import torch
    words, n_bits = marshal_mask(allowed, n_bits)
    dq = torch.tensor(np.ascontiguousarray(Q, dtype=f32), device="cuda")
    dm = torch.tensor(words.view(np.int32), device="cuda") if len(words) else None
    o_ids = torch.full((len(Q), k), -7, dtype=torch.int64, device="cuda")
    o_dist = torch.full((len(Q), k), -7.0, dtype=torch.float32, device="cuda")
    o_cnt = torch.full((len(Q),), 77, dtype=torch.int32, device="cuda")
    space.knn_masked_device(dq, k, dm, n_bits, o_ids, o_dist, o_cnt)
    torch.cuda.synchronize()
    return (o_ids.cpu().numpy().view(np.uint64), o_dist.cpu().numpy(), o_cnt.cpu().numpy().view(np.uint32))


def _same_bytes(a, b):
    return all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes() for x, y in zip(a, b))


def _i8_space(name, d, metric, X, cap=None, **kw):
    s = ehx.Space.unique(name, d, metric=METRICS[metric][0], initial_capacity=cap or len(X), **kw)
    s.set_batch(_keys(len(X)), X)
    assert s.scan_engine() == "i8"
    return s


# ---- scan route ----

@pytest.mark.parametrize("d", rc.I8_DIMS)
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_scan_route(metric, d):
    om = METRICS[metric][1]
    X, Q = rc.i8_data(d)
    n = rc.I8_ROWS
    s = _i8_space("masked-i8", d, metric, X)
    for name, allowed in mc.masks(n).items():
        L = np.nonzero(allowed)[0].astype(np.uint64)
        want48 = _expected(X, Q, max(mc.KS), om, allowed)
        for nq in (1, rc.I8_QUERIES):
            for k in mc.KS:
                want = _cut(want48, nq, k)
                c0 = _counters(s)
                got = s.knn_masked(Q[:nq], k, allowed)
                dc = _counters(s) - c0
                what = "%s d=%d %s nq=%d k=%d" % (metric, d, name, nq, k)
                _assert_rows(got, want, what)
                # every query on the scan route, none overflowed (tests/test_masked_model.py), the passes of the plan
                assert dc.tolist() == [nq, 0, 0, mc.PASSES[name], 1], (what, dc)
                assert _same_bytes(got, s.knn_among(Q[:nq], k, L)), what + ": knn_among on the list differs"
                assert _same_bytes(got, _device_form(s, Q[:nq], k, allowed)), what + ": host and device forms differ"
                if name == "ones":
                    assert _same_bytes(got, s.knn(Q[:nq], k)), what + ": knn differs"
    assert s.stats()["n_uncertified"] == 0
    s.drop()


@pytest.mark.parametrize("where", ["last_pass", "first_pass"])
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_pool_overflow_falls_to_the_exact_route(metric, where):
    """allowed copies of one row, more than a pool of them inside ONE pass: the queries near that row meet them all at one
    distance.  last_pass: 5 000 copies behind the first 4096 allowed rows.  first_pass: row 5 and 4 096 copies are all the
    first pass sees (tile 0 allows row 5 only, the copies fill tiles 1-16) — the flag must stick and the query collect
    nothing in the pass behind it."""
    om = METRICS[metric][1]
    d, k, n = 128, 10, rc.I8_ROWS
    X0, Q0 = rc.i8_data(d)
    X = X0.copy()
    allowed = mc.masks(n)["half"].copy()
    c0, c1 = (10000, 15000) if where == "last_pass" else (256, 256 + 4096)
    X[c0:c1] = X[5]
    allowed[c0:c1] = True
    if where == "first_pass":
        allowed[:256] = False
    allowed[5] = True
    plan = mc.passes(allowed)
    assert len(plan) == 2 and plan[0][0] == 0
    rng = np.random.default_rng(77)
    near = (X[5][None, :] + f32(0.01) * rng.standard_normal((8, d)).astype(f32)).astype(f32)
    # the other queries: the 56 for which the copies lie farthest beyond the radius their pass runs under, by more than a
    # quarter of it (the int8 bound's slack is a few per cent of it).  That radius is at most the 10th distance among the
    # allowed rows of the first pass (last_pass), among the sample's rows other than the copies (first_pass)
    before = np.zeros(n, dtype=bool)
    if where == "last_pass":
        before[:plan[0][1] * mc.TILE] = allowed[:plan[0][1] * mc.TILE]
        assert plan[0][1] * mc.TILE <= c0
    else:
        assert plan[0][1] == 17
        before[mc.sample_ids(allowed)] = True
        before[c0:c1] = False
        assert before.sum() >= 100
    w1 = _expected(X, Q0, k, om, before)
    w5 = pyoracle.exhaustive(np.ascontiguousarray(X[5:6]), Q0, 1, om)[1][:, 0]
    ratio = np.array([w5[i] / w1[i][1][k - 1] for i in range(len(Q0))])
    far = [int(i) for i in np.argsort(-ratio)[:56]]
    assert ratio[far[-1]] > 1.25, ratio[far[-1]]
    Q = np.concatenate([Q0[far[:20]], near[:4], Q0[far[20:]], near[4:]]).astype(f32)
    is_near = np.array([False] * 20 + [True] * 4 + [False] * 36 + [True] * 4)
    s = _i8_space("masked-over", d, metric, X)
    want = _expected(X, Q, k, om, allowed)
    for i in np.nonzero(is_near)[0]:
        assert want[i][0] == [5] + list(range(c0, c0 + 9))     # the lowest ids win
    cn0 = _counters(s)
    got = s.knn_masked(Q, k, allowed)
    dc = _counters(s) - cn0
    _assert_rows(got, want, "overflow, " + where)
    assert dc.tolist() == [len(Q) - 8, 8, 8, 2, 1], dc
    assert _same_bytes(got, _device_form(s, Q, k, allowed))
    assert s.stats()["n_uncertified"] == 0
    s.drop()


# ---- the merge of a pass's hits into the carried keys ----

def _merge_case(name, check=None, **kw):
    """every bitmap and k of masked_cases.merge_cases()[name]: the oracle's answer, ehx_knn_among's bytes, both forms, every
    query served by the two passes of the scan route (tests/test_masked_model.py: no pool overflows)"""
    X, Q, metric, bitmaps, ks = mc.merge_cases()[name]
    om = METRICS[metric][1]
    s = _i8_space("masked-" + name, X.shape[1], metric, X, **kw)
    for bname, allowed in bitmaps.items():
        L = np.nonzero(allowed)[0].astype(np.uint64)
        for k in ks:
            what = "%s %s k=%d" % (name, bname, k)
            want = _expected(X, Q, k, om, allowed)
            c0 = _counters(s)
            got = s.knn_masked(Q, k, allowed)
            dc = _counters(s) - c0
            _assert_rows(got, want, what)
            assert dc.tolist() == [len(Q), 0, 0, 2, 1], (what, dc)
            assert _same_bytes(got, s.knn_among(Q, k, L)), what + ": knn_among on the list differs"
            assert _same_bytes(got, _device_form(s, Q, k, allowed)), what + ": host and device forms differ"
            if check:
                check(allowed, k, want)
    assert s.stats()["n_uncertified"] == 0
    s.drop()


def test_ties_across_passes_come_back_in_id_order():
    """300 copies of one row over the ids of both passes, the query that row: a pass's hits and the carried keys lie at ONE
    distance, and the rank merge must order them by id.  Where the bitmap clears a copy, the answer simply lacks it."""
    at = lc.ties()[2]

    def check(allowed, k, want):
        copies = at[allowed[at]]
        first_pass_rows = mc.passes(allowed)[0][1] * mc.TILE
        assert (copies < first_pass_rows).sum() > 0 and (copies >= first_pass_rows).sum() > 0
        assert want[0][0] == [int(v) for v in copies[:k]] and (want[0][1] == want[0][1][0]).all()

    _merge_case("ties", check)


def test_fewer_than_k_keys_carried_out_of_the_first_pass():
    """masked_cases.far_then_near: the first pass finds fewer than k rows within query 0's first radius — nothing, in fact —
    so fewer than k keys are carried, the radius stays where the sample put it, and the second pass brings the whole answer"""
    X, Q, metric, bitmaps, ks = mc.merge_cases()["short"]
    allowed, k = bitmaps["far_then_near"], ks[0]
    plan = mc.passes(allowed)
    assert len(plan) == 2 and k == mc.SCAN_MAX_K
    L = np.nonzero(allowed)[0]
    oi, od, oc = pyoracle.exhaustive(np.ascontiguousarray(X[L]), Q[:1], len(L), METRICS[metric][1])
    D0 = np.empty(len(X), dtype=f32)
    D0[L[oi[0].astype(np.int64)]] = od[0]
    r0 = np.sort(D0[mc.sample_ids(allowed)])[k - 1]
    first = L[L < plan[0][1] * mc.TILE]
    assert len(first) >= 4096 and (D0[first] <= r0).sum() < k
    _merge_case("short")


def test_binary16_rows_on_the_scan_route():
    _merge_case("f16", dtype=ehx.DTYPE_F16)


# ---- exact route ----

@pytest.mark.parametrize("kind", ["flat_f32", "flat_f16", "graph_f32"])
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_exact_route_small_spaces(metric, kind):
    em, om = METRICS[metric]
    n, d, nq = 700, 19, 5
    rng = np.random.default_rng(300)
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    kw = {"mode": ehx.MODE_GRAPH, "M": 16} if kind == "graph_f32" else {}
    s = ehx.Space.unique("masked-small", d, metric=em, initial_capacity=n,
                         dtype=ehx.DTYPE_F16 if kind == "flat_f16" else ehx.DTYPE_F32, **kw)
    s.set_batch(_keys(n), X)
    Xs = X.astype(np.float16).astype(f32) if kind == "flat_f16" else X
    allowed = rng.random(n) < 0.5
    for k in (1, 10, 100):
        c0 = _counters(s)
        got = s.knn_masked(Q, k, allowed)
        _assert_rows(got, _expected(Xs, Q, k, om, allowed), "%s %s k=%d" % (kind, metric, k))
        assert (_counters(s) - c0).tolist() == [0, nq, 0, 0, 1]
        assert _same_bytes(got, s.knn_among(Q, k, np.nonzero(allowed)[0].astype(np.uint64)))
        assert _same_bytes(got, _device_form(s, Q, k, allowed))
    s.drop()


def test_exact_route_on_an_int8_space_and_the_bitmap_s_edges():
    metric, d, nq = "cosine", 128, 33
    om = METRICS[metric][1]
    X, Q = rc.i8_data(d)
    Q = Q[:nq]
    n = rc.I8_ROWS
    s = _i8_space("masked-edges", d, metric, X)
    rng = np.random.default_rng(301)
    half = mc.masks(n)["half"]

    def run(k, allowed, n_bits, route, what, expect_mask=None):
        c0 = _counters(s)
        got = s.knn_masked(Q, k, allowed, n_bits)
        dc = _counters(s) - c0
        _assert_rows(got, _expected(X, Q, k, om, allowed if expect_mask is None else expect_mask), what)
        assert dc[:3].tolist() == ([nq, 0, 0] if route == "scan" else [0, nq, 0]) and dc[4] == 1, (what, dc)
        assert (dc[3] > 0) == (route == "scan")
        assert _same_bytes(got, _device_form(s, Q, k, allowed, n_bits)), what
        return got

    run(100, half, None, "exact", "k = 100 > 48")
    run(49, half, None, "exact", "k = 49")
    run(48, half, None, "scan", "k = 48")
    hundred = np.zeros(n, dtype=bool)
    hundred[rng.choice(n, size=100, replace=False)] = True
    run(10, hundred, None, "exact", "100 allowed rows")
    cut = mc.exact_cut(n)
    at_cut = np.zeros(n, dtype=bool)
    at_cut[rng.choice(n, size=cut, replace=False)] = True
    run(10, at_cut, None, "exact", "exactly the cut")
    at_cut[np.nonzero(~at_cut)[0][0]] = True
    run(10, at_cut, None, "scan", "one row above the cut")
    five = np.zeros(n, dtype=bool)
    five[[3, 4000, 4001, 19998, 19999]] = True
    got = run(10, five, None, "exact", "fewer allowed rows than k")
    assert (got[2] == 5).all()
    for empty, nb in ((np.zeros(n, dtype=bool), None), (np.zeros(0, dtype=bool), None), (np.ones(n, dtype=bool), 0)):
        got = run(10, empty, nb, "exact", "empty bitmap", expect_mask=np.zeros(n, dtype=bool))
        assert (got[2] == 0).all() and (got[0] == NO_ID).all() and np.isposinf(got[1]).all()
    # n_bits below the row count: the rows at or above it are not allowed, whatever the words hold
    ones = np.ones(n, dtype=bool)
    below = ones.copy()
    below[10001:] = False
    words = marshal_mask(ones)[0]
    run(10, words, 10001, "scan", "n_bits below the row count (packed words)", expect_mask=below)
    run(10, ones, 777, "exact", "n_bits = 777", expect_mask=np.arange(n) < 777)
    # ... and above it: bits at or above the row count name no row
    beyond = np.ones(n + 300, dtype=bool)
    beyond[:n] = half
    run(10, beyond, None, "scan", "n_bits above the row count", expect_mask=half)
    s.drop()


def test_a_space_without_the_int8_engine_takes_the_exact_route():
    metric, d, nq, k = "cosine", 128, 33, 10
    om = METRICS[metric][1]
    X, Q = rc.i8_data(d)
    s = ehx.Space.unique("masked-f32", d, metric=METRICS[metric][0], initial_capacity=rc.I8_ROWS)
    s.set_batch(_keys(rc.I8_ROWS), X)
    s.set_scan(ehx.SCAN_F32)
    assert s.scan_engine() != "i8"
    allowed = mc.masks(rc.I8_ROWS)["half"]
    got = s.knn_masked(Q[:nq], k, allowed)
    _assert_rows(got, _expected(X, Q[:nq], k, om, allowed), "SCAN_F32")
    assert _counters(s).tolist() == [0, nq, 0, 0, 1]
    assert _same_bytes(got, _device_form(s, Q[:nq], k, allowed))
    s.drop()


# ---- values and state ----

def test_nan_rows_nan_queries_and_ties():
    rng = np.random.default_rng(302)
    n, d = 600, 24
    X = rng.standard_normal((n, d)).astype(f32)
    X[10, 3] = np.nan                       # a NaN distance is never a neighbour
    X[[17, 230, 401]] = X[5]                # ties come back in id order
    Q = np.stack([X[5] + f32(0.25), rng.standard_normal(d).astype(f32), np.full(d, np.nan, dtype=f32)]).astype(f32)
    allowed = np.ones(n, dtype=bool)
    allowed[230] = False
    for metric in ("l2", "cosine"):
        em, om = METRICS[metric]
        s = ehx.Space.unique("masked-nan", d, metric=em, initial_capacity=n)
        s.set_batch(_keys(n), X)
        got = s.knn_masked(Q, 8, allowed)
        _assert_rows(got, _expected(X, Q, 8, om, allowed), "NaN, ties, " + metric)
        assert int(got[2][2]) == 0 and (metric != "l2" or [int(v) for v in got[0][0, :3]] == [5, 17, 401])
        assert 10 not in got[0][:2].astype(np.int64)
        s.drop()
    # on the scan route: a NaN query is one the bound does not serve — the exact route answers it, no overflow is counted
    X8, Q8 = rc.i8_data(128)
    X8 = X8.copy()
    X8[[17000, 18000]] = X8[7]
    Q = np.stack([X8[7] + f32(0.01), np.full(128, np.nan, dtype=f32), Q8[0]]).astype(f32)
    half = mc.masks(rc.I8_ROWS)["half"].copy()
    half[[7, 17000, 18000]] = True
    s = _i8_space("masked-nan8", 128, "l2", X8)
    got = s.knn_masked(Q, 10, half)
    _assert_rows(got, _expected(X8, Q, 10, pyoracle.METRIC_L2, half), "NaN query on the scan route")
    assert [int(v) for v in got[0][0, :3]] == [7, 17000, 18000] and int(got[2][1]) == 0
    assert _counters(s).tolist() == [2, 1, 0, mc.PASSES["half"], 1]
    s.drop()


def test_error_returns():
    rng = np.random.default_rng(8)
    n, d = 200, 8
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((3, d)).astype(f32)
    allowed = np.ones(n, dtype=bool)
    s = ehx.Space.unique("masked-err", d, metric=ehx.METRIC_L2SQ, initial_capacity=n)
    s.set_batch(_keys(n), X)
    for k, code in ((0, _lib.EINVAL), (1025, _lib.EUNSUPPORTED)):
        with pytest.raises(ehx.EhxError) as e:
            s.knn_masked(Q, k, allowed)
        assert e.value.code == code
    with pytest.raises(ValueError):
        s.knn_masked(Q, 4, np.zeros(3, dtype=np.uint32))   # packed words need n_bits
    ids, dist, cnt = s.knn_masked(np.zeros((0, d), dtype=f32), 4, allowed)   # no queries: EHX_OK, nothing written
    assert ids.shape == (0, 4) and cnt.shape == (0,)
    L = _lib.load()
    q = np.ascontiguousarray(Q)
    words = marshal_mask(allowed)[0]
    o_ids, o_dist, o_cnt = np.zeros((3, 4), dtype=np.uint64), np.zeros((3, 4), dtype=f32), np.zeros(3, dtype=np.uint32)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    args = [P(o_ids, C.c_uint64), P(o_dist, C.c_float), P(o_cnt, C.c_uint32)]
    for hole in range(3):
        a = list(args)
        a[hole] = None
        assert L.ehx_knn_masked(s._h, 3, P(q, C.c_float), 4, P(words, C.c_uint32), n, a[0], a[1], a[2]) == _lib.EINVAL
    assert L.ehx_knn_masked(s._h, 3, None, 4, P(words, C.c_uint32), n, *args) == _lib.EINVAL
    assert L.ehx_knn_masked(s._h, 3, P(q, C.c_float), 4, None, n, *args) == _lib.EINVAL       # a NULL mask with n_bits > 0
    assert L.ehx_knn_masked(s._h, 3, P(q, C.c_float), 4, None, 0, *args) == _lib.OK and (o_cnt == 0).all()
    assert L.ehx_knn_masked(s._h, 3, P(q, C.c_float), 4, P(words, C.c_uint32), n, *args) == _lib.OK and (o_cnt == 4).all()
    assert L.ehx_knn_masked_device(s._h, None, 3, None, 4, None, n, None, None, None) == _lib.EINVAL
    h = s._h
    s.drop()   # the tombstone answers for the dropped handle
    assert L.ehx_knn_masked(h, 3, P(q, C.c_float), 4, P(words, C.c_uint32), n, *args) == _lib.ENOTFOUND
    e0 = ehx.Space.unique("masked-empty", d, metric=ehx.METRIC_L2SQ)
    got = e0.knn_masked(Q, 4, allowed)
    assert (got[2] == 0).all() and (got[0] == NO_ID).all() and np.isposinf(got[1]).all()
    e0.drop()
    sh = ehx.Space.unique("masked-sh", d, metric=ehx.METRIC_L2SQ, shards=2)
    sh.set_batch(_keys(n), X)
    with pytest.raises(ehx.EhxError) as e:
        sh.knn_masked(Q, 4, allowed)
    assert e.value.code == _lib.EUNSUPPORTED and "sharded" in str(e.value)
    sh.drop()


def test_stats_deltas():
    rng = np.random.default_rng(9)
    n, d, nq = 1000, 16, 12
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    allowed = rng.random(n) < 0.3
    s = ehx.Space.unique("masked-stats", d, metric=ehx.METRIC_L2SQ, initial_capacity=n)
    s.set_batch(_keys(n), X)
    st0 = s.stats()
    s.knn_masked(Q, 5, allowed)
    st1 = s.stats()   # the exact route: every query against every allowed row
    assert st1["n_queries"] - st0["n_queries"] == nq and st1["n_dist"] - st0["n_dist"] == nq * int(allowed.sum())
    assert st1["n_rerank"] == st0["n_rerank"] and st1["n_uncertified"] == 0
    s.drop()
    X8, Q8 = rc.i8_data(128)
    half = mc.masks(rc.I8_ROWS)["half"]
    s = _i8_space("masked-stats8", 128, "cosine", X8)
    st0 = s.stats()
    s.knn_masked(Q8[:40], 10, half)
    st1 = s.stats()   # the scan route: every query once; the sample's rows and the rows re-ranked, far fewer than a list scan
    assert st1["n_queries"] - st0["n_queries"] == 40
    assert 40 * len(mc.sample_ids(half)) < st1["n_dist"] - st0["n_dist"] < 40 * int(half.sum()) // 4
    assert st1["n_uncertified"] == 0 and st1["n_i8_queries"] == st0["n_i8_queries"]
    s.drop()


def test_append_then_search_and_rewrite_then_search():
    metric, d, nq, k = "cosine", 128, 40, 10
    om = METRICS[metric][1]
    X, Q = rc.i8_data(d)
    Q = Q[:nq]
    n0, n1 = rc.I8_ROWS - 700, rc.I8_ROWS
    X = X.copy()
    s = _i8_space("masked-append", d, metric, X[:n0], cap=n1)
    half = mc.masks(n1)["half"]
    _assert_rows(s.knn_masked(Q, k, half), _expected(X[:n0], Q, k, om, half[:n0]), "before the append")
    s.set_batch(_keys(n1 - n0, n0), X[n0:])                      # append: the same bitmap now names 700 more rows
    got = s.knn_masked(Q, k, half)
    _assert_rows(got, _expected(X, Q, k, om, half), "after the append")
    assert _same_bytes(got, _device_form(s, Q, k, half))
    rows = np.nonzero(half)[0][::40]                             # rewrite allowed rows in place with the queries themselves
    X[rows[:nq]] = Q
    s.set_batch(["k%d" % i for i in rows[:nq]], Q)
    got = s.knn_masked(Q, k, half)
    want = _expected(X, Q, k, om, half)
    _assert_rows(got, want, "after the rewrite")
    assert all(want[i][0][0] == int(rows[i]) for i in range(nq))
    assert _counters(s)[2] == 0 and _counters(s)[0] == 4 * nq
    s.drop()


def test_a_dropped_space_leaves_nothing_behind():
    L = _lib.load()
    _lib.check(L.ehx_init(None, 0))
    base = _live()
    d = 128
    X0, Q0 = rc.i8_data(d)
    X = X0.copy()
    X[10000:15000] = X[5]
    allowed = mc.masks(rc.I8_ROWS)["half"].copy()
    allowed[10000:15000] = True
    Q = np.concatenate([Q0[:30], X[5:6] + f32(0.01)]).astype(f32)
    s = _i8_space("masked-life", d, "cosine", X)
    # the scan route, its overflow, the exact route and both forms all create their scratch
    got = s.knn_masked(Q, 10, allowed)
    assert _counters(s)[1] >= 1 and _counters(s)[2] >= 1 and _counters(s)[0] >= 1
    assert _same_bytes(got, _device_form(s, Q, 10, allowed))
    s.knn_masked(Q, 100, allowed)
    s.drop()
    assert _live() == base, "device allocations, pinned allocations, events, streams alive after the drop"
