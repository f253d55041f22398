"""The searches beside the plain kNN chain — range search, bitmap search, list search, the large-k route and the lookup by
stored key — against the oracle at extreme and non-finite values: what tests/test_extreme_values.py does for the chain.

Every expected answer comes from pyoracle.exhaustive alone (cut at the radius by range_cases.cut, or run over the allowed or
listed rows and mapped back).  Bar everywhere: ids equal, distance BYTES equal, counts (and the range search's totals)
equal, NO_ID / +Inf behind the count, no query uncertified.  On the spaces that keep the int8 engine the routes' counters
must move as the CPU model says (tests/side_extreme_cases.py, checked without a GPU by tests/test_side_extreme_model.py):
a served query is counted on its route, a marked one as handed on and not as overflowed, an overflowed one as both.  A row
outside the band the filters bound sends the space to the exact kernels (range_exact_kernel, the list kernels,
pool_rerank_sorted), which then walk whole blocks of subnormal, overflowing and non-finite rows in the fp32, binary16 and
block-permuted layouts.

Deliberate damage these cases catch (each tried once on a scratch build; none of it is in the tree):
  range_thr_kernel without its 1.001 m term    no answer changes — the int8 bound's own slack covers what the margin covers,
                                               as the model shows too — but queries that must overflow are served instead:
                                               the counters of test_row_magnitude_ladder[a_hi-l2],
                                               test_spaces_made_entirely_of_one_kind[a_lo-l2], test_cross_band_rows_and_queries
                                               [queries_huge-*], test_binary16_rows_at_their_limits[l2, ip] and
                                               test_odd_queries_inside_ordinary_batches[ip]
  prep_queries8 without u = NaN out of band    test_odd_queries_inside_ordinary_batches: wrong totals (inner product, cosine),
                                               a handed-on count below the marked queries (L2)
  radius_rerank_kernel emitting `merged` cut   counts below k on the bitmap and large-k routes of every case that serves a query
  at nh instead of n_out                       there, the sharded case included (19 cases)"""
import ctypes as C

import numpy as np
import pytest

import extreme_cases as xc
import largek_cases as lc
import masked_cases as mc
import range_cases as rc
import side_extreme_cases as sx
from oracle import pyoracle

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402

EM = {"l2": ehx.METRIC_L2SQ, "ip": ehx.METRIC_IP, "cosine": ehx.METRIC_COSINE}
NO_ID = np.uint64(2**64 - 1)
f32 = np.float32
D, MR = sx.D, sx.MAX_RESULTS


def _keys(n):
    return ["k%d" % i for i in range(n)]


def _hook(s, name, n):
    out = (C.c_uint64 * n)()
    getattr(C.CDLL(_lib.LIB_PATH), name)(s._h, out)
    return np.array(list(out), dtype=np.int64)


def _range_ctr(s):
    return _hook(s, "ehx_test_range_counters", 4)     # int8 path, exact path, pool overflows, truncated


def _masked_ctr(s):
    return _hook(s, "ehx_test_masked_counters", 5)    # scan route, exact route, overflowed, scan passes, calls


def _largek_ctr(s):
    return _hook(s, "ehx_test_largek_counters", 5)    # on the route, handed on, of those overflowed, scan passes, calls


def _space(name, X, metric, **kw):
    s = ehx.Space.unique(name, X.shape[1], metric=EM[metric], initial_capacity=len(X), **kw)
    s.set_batch(_keys(len(X)), X)
    return s


def _oracle(X, Q, k, metric):
    return pyoracle.exhaustive(np.ascontiguousarray(X), np.ascontiguousarray(Q), k, rc.OM[metric])


def _assert_rows(got, want, what):
    """want: [(ids, distances)] per query"""
    ids, dist, cnt = got
    assert len(cnt) == len(want), what
    for i, (wids, wdist) in enumerate(want):
        c = int(cnt[i])
        assert c == len(wids), "%s: query %d has %d results, the oracle %d" % (what, i, c, len(wids))
        assert [int(v) for v in ids[i, :c]] == [int(v) for v in wids], "%s: query %d ids differ" % (what, i)
        assert dist[i, :c].tobytes() == np.asarray(wdist, dtype=f32).tobytes(), "%s: query %d distance bytes differ" % (what, i)
        assert (ids[i, c:] == NO_ID).all() and np.isposinf(dist[i, c:]).all(), "%s: query %d tail sentinels" % (what, i)


def _assert_range(got, want, what):
    ids, dist, cnt, total = got
    assert [int(t) for t in total] == [w[2] for w in want], "%s: totals differ" % what
    _assert_rows((ids, dist, cnt), [(w[0], w[1]) for w in want], what)


def _lists(oracle, k):
    oids, odist, ocnt = oracle
    return [(oids[i, :min(int(ocnt[i]), k)], odist[i, :min(int(ocnt[i]), k)]) for i in range(len(ocnt))]


def _among(X, Q, k, metric, rows):
    """the oracle over the rows `rows` (ascending, unique), ids mapped back"""
    L = np.asarray(rows, dtype=np.int64)
    if L.size == 0:
        return [([], np.zeros(0, dtype=f32)) for _ in range(len(Q))]
    oi, od, oc = _oracle(X[L], Q, k, metric)
    return [(L[oi[i, :int(oc[i])].astype(np.int64)], od[i, :int(oc[i])]) for i in range(len(Q))]


def _drop_rule(oracle, own, k):
    """tests/test_knn_by_keys.py's rule over the oracle's (k + 1)-long lists"""
    out = []
    for i, (ids, dist) in enumerate(_lists(oracle, k + 1)):
        ids, dist = [int(v) for v in ids], list(dist)
        if ids:
            p = ids.index(own[i]) if own[i] in ids else len(ids) - 1
            del ids[p], dist[p]
        out.append((ids[:k], np.asarray(dist[:k], dtype=f32)))
    return out


# ---- one routine for every search of a case --------------------------------------------------------------------------

def _range(s, X, Q, metric, full, radius, verdict, what):
    """one range_search call: exact, and the counters as the model's verdicts say (verdict None: the exact path alone)"""
    want = rc.cut(*full, radius, MR)
    c0 = _range_ctr(s)
    got = s.range_search(Q, radius, MR)
    dc = _range_ctr(s) - c0
    _assert_range(got, want, what)
    totals = np.array([w[2] for w in want])
    assert dc[3] == (totals > MR).sum(), (what, dc)
    if verdict is None:
        assert dc[:3].tolist() == [0, len(Q), int((totals > sx.POOL_CAP).sum())], (what, dc)
    else:   # (a marked query with more than a pool of members overflows the EXACT path's pool: counted there, once)
        exact_over = int(((np.asarray(verdict) == sx.MARKED) & (totals > sx.POOL_CAP)).sum())
        sx.expect_counters(verdict, dc[0], dc[1], dc[2] - exact_over, what)
    return got


def _masked(s, X, Q, metric, k, allowed, verdict, what):
    """one knn_masked call; verdict None: the exact route"""
    want = _among(X, Q, k, metric, np.nonzero(allowed)[0])
    c0 = _masked_ctr(s)
    got = s.knn_masked(Q, k, allowed)
    dc = _masked_ctr(s) - c0
    _assert_rows(got, want, what)
    if verdict is None:
        assert dc.tolist() == [0, len(Q), 0, 0, 1], (what, dc)
    else:
        sx.expect_counters(verdict, dc[0], dc[1], dc[2], what)
        assert dc[3] == len(mc.passes(allowed)) and dc[4] == 1, (what, dc)
    return got


def _largek(s, call, nq, want, verdict, what):
    """one call that takes the large-k route on an int8 space (verdict None: it must not)"""
    c0, st0 = _largek_ctr(s), s.stats()
    got = call()
    dc, st1 = _largek_ctr(s) - c0, s.stats()
    _assert_rows(got, want, what)
    if verdict is None:
        assert dc.tolist() == [0, 0, 0, 0, 0], (what, dc)
    else:
        sx.expect_counters(verdict, dc[0], dc[1], dc[2], what)
        assert dc[3] == len(lc.passes(len(s))) and dc[4] == 1, (what, dc)
        assert st1["n_i8_queries"] - st0["n_i8_queries"] == nq and st1["n_i8_fallback"] - st0["n_i8_fallback"] == dc[1], what
    return got


def _every_search(s, X, Q, metric, key_rows, v, what, lists=True):
    """range search at the oracle's 1st, 10th and 100th distance, bitmap search (50 % and <= 1024 rows) at k 10 and 48,
    list search (shared and per-query lists), kNN at k = 100 and the by-key lookup at k = 48.  v: the model's verdicts
    (side_extreme_cases.route_verdicts) on an int8 space, None on a space that stays on the exact kernels."""
    n, nq = X.shape[0], Q.shape[0]
    half, few = sx.bitmaps(n, 1)
    full = v["model"].oracle if v else _oracle(X, Q, n, metric)
    out = {}
    for rank in sx.RANKS:
        r = sx.rank_radii(full, rank) if not (v and v.get("radii")) else v["radii"][rank]
        out["range", rank] = _range(s, X, Q, metric, full, r, v["range", rank][0] if v else None, "%s range@%d" % (what, rank))
    for k in sx.MASKED_KS:
        out["masked", k] = _masked(s, X, Q, metric, k, half, v["masked", k][0] if v else None, "%s bitmap 50 %% k=%d" % (what, k))
        _masked(s, X, Q, metric, k, few, None, "%s bitmap of %d rows k=%d" % (what, few.sum(), k))
    if lists:
        shared, per = sx.lists(n, nq, 2)
        _assert_rows(s.knn_among(Q, 10, shared), _among(X, Q, 10, metric, shared), what + " shared list")
        want = [_among(X, Q[i:i + 1], 10, metric, np.unique(per[i]))[0] for i in range(nq)]
        _assert_rows(s.knn_among(Q, 10, per), want, what + " per-query lists")
    k = sx.LARGE_K
    out["largek"] = _largek(s, lambda: s.knn(Q, k), nq, _lists(full, k), v["largek"][0] if v else None, "%s k=%d" % (what, k))
    if key_rows is not None:
        keys = ["k%d" % i for i in key_rows]
        want = _drop_rule(_oracle(X, X[key_rows], sx.BYKEYS_K + 1, metric), key_rows, sx.BYKEYS_K)
        _largek(s, lambda: s.knn_by_keys(keys, sx.BYKEYS_K), len(keys), want, v["bykeys"][0] if v else None, what + " by keys")
    assert s.stats()["n_uncertified"] == 0, what
    return out


def _print_tallies(name, v):
    for route in v:
        if route not in ("model", "radii"):
            print("%s %s: served %d marked %d overflowed %d undecided %d" % ((name, route) + sx.tally(v[route][0])))


# ---- a. the row-magnitude ladder -------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", sx.METRICS)
@pytest.mark.parametrize("kind", xc.KINDS)
def test_row_magnitude_ladder(kind, metric):
    """ordinary rows plus a block of 256 rows of one kind.  A kind the filters bound keeps the int8 engine: the radius routes
    run, and the model says which queries they serve; any other kind sends the space to the exact side kernels."""
    name = "ladder-%s-%s" % (kind, metric)
    safe = kind in xc.SAFE
    if safe:
        c, _, v = sx.case_verdicts(name)
        X, Q, key_rows = c["X"], c["Q"], c["key_rows"]
        _print_tallies(name, v)
    else:
        (X, Q), v = sx.ladder(kind, metric), None
        key_rows = sx.bykeys_rows(len(X), 5)
    s = _space("sx-ladder", X, metric)
    assert s.scan_engine() == ("i8" if safe else "f32"), (kind, s.scan_engine())
    out = _every_search(s, X, Q, metric, key_rows, v, name)
    if kind == "g":   # queries 20, 21 and 24 copy rows that hold a NaN: no neighbour, no member
        for rank in sx.RANKS:
            ids, dist, cnt, total = out["range", rank]
            assert cnt[[20, 21, 24]].tolist() == [0, 0, 0] and total[[20, 21, 24]].tolist() == [0, 0, 0]
        assert out["largek"][2][[20, 21, 24]].tolist() == [0, 0, 0]
    s.drop()


# ---- b. spaces made entirely of one kind -----------------------------------------------------------------------------

@pytest.mark.parametrize("metric", sx.METRICS)
@pytest.mark.parametrize("kind", ["a_lo", "a_hi", "f"])
def test_spaces_made_entirely_of_one_kind(kind, metric):
    name = "one-%s-%s" % (kind, metric)
    c, _, v = sx.case_verdicts(name)
    _print_tallies(name, v)
    s = _space("sx-one", c["X"], metric)
    assert s.scan_engine() == "i8"
    out = _every_search(s, c["X"], c["Q"], metric, c["key_rows"], v, name)
    if kind == "f" and metric == "l2":   # every distance of a query ties: the lowest ids
        ids, dist, cnt = out["largek"]
        assert (cnt == sx.LARGE_K).all() and (ids == np.arange(sx.LARGE_K, dtype=np.uint64)[None, :]).all()
    s.drop()


# ---- c. odd queries inside ordinary batches --------------------------------------------------------------------------

@pytest.mark.parametrize("metric", sx.METRICS)
def test_odd_queries_inside_ordinary_batches(metric):
    name = "odd-" + metric
    c, half, v = sx.case_verdicts(name)
    _print_tallies(name, v)
    X, Q = c["X"], c["Q"]
    s = _space("sx-odd", X, metric)
    assert s.scan_engine() == "i8"
    out = _every_search(s, X, Q, metric, None, v, name, lists=False)
    keep = c["ordinary"]
    for route, got in out.items():
        assert (got[2][[1, 2]] == 0).all(), (route, "NaN queries")
        if route[0] == "range":
            again = s.range_search(Q[keep], v["radii"][route[1]][keep], MR)
        elif route[0] == "masked":
            again = s.knn_masked(Q[keep], route[1], half)
        else:
            again = s.knn(Q[keep], sx.LARGE_K)
        for a, b in zip(again, got):   # the ordinary queries' rows do not depend on the odd ones beside them
            assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b[keep]).tobytes(), (name, route)
    # the range search once more, the odd queries under +Inf: marked whatever they are, every non-NaN row a member
    r = v["radii"][10].copy()
    r[xc.ODD_AT] = np.inf
    verdict, _ = v["model"].range(r)
    assert (np.asarray(verdict)[xc.ODD_AT] == sx.MARKED).all()
    got = _range(s, X, Q, metric, v["model"].oracle, r, verdict, name + " range, +Inf for the odd queries")
    assert (got[3][[1, 2]] == 0).all() and int(got[3][0]) == len(X)   # (the zero query: every row is a member)
    assert s.stats()["n_uncertified"] == 0
    s.drop()


# ---- d. cross-band: rows and queries of opposite extremes ------------------------------------------------------------

@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("which", ["rows_huge", "queries_huge"])
def test_cross_band_rows_and_queries(which, metric):
    name = "cross-%s-%s" % (which, metric)
    c, _, v = sx.case_verdicts(name)
    _print_tallies(name, v)
    s = _space("sx-cross", c["X"], metric)
    assert s.scan_engine() == "i8"
    _every_search(s, c["X"], c["Q"], metric, None, v, name, lists=False)
    s.drop()


# ---- e. extreme radii ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", sx.METRICS)
@pytest.mark.parametrize("space", ["a_hi", "ordinary"])
def test_extreme_radii(space, metric):
    """+-FLT_MAX, +-0, the smallest subnormal, a radius equal to a distance near 1e-24 and near 1e30 (the nearest the space
    has) and one ulp below each — side_extreme_cases.RADIUS_KINDS, one per query in turn"""
    X, Q, radius = sx.extreme_radii(space, metric)
    if metric == "l2":
        near = radius[5::9] if space == "ordinary" else radius[7::9]
        assert ((near > 5e-25) & (near < 2e-24)).all() if space == "ordinary" else ((near > 2e29) & (near < 4e30)).all()
    m = sx.Model(X, Q, metric)
    verdict, fill = m.range(radius)
    print("radii %s %s: served %d marked %d overflowed %d undecided %d" % ((space, metric) + sx.tally(verdict)))
    s = _space("sx-radii", X, metric)
    assert s.scan_engine() == "i8"
    got = _range(s, X, Q, metric, m.oracle, radius, verdict, "radii %s %s" % (space, metric))
    assert (got[3][1::9] == 0).all()              # -FLT_MAX: below every distance
    assert s.stats()["n_uncertified"] == 0
    s.drop()


# ---- f. binary16 storage ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", sx.METRICS)
def test_binary16_rows_at_their_limits(metric):
    """finite rows holding the binary16 edge values (the largest half, the smallest subnormal, values that round to them or to
    zero, -0): radius_rerank_kernel's and range_rerank_kernel's HALFX instantiations; the oracle runs on the rounded rows"""
    name = "f16-" + metric
    c, _, v = sx.case_verdicts(name)
    _print_tallies(name, v)
    s = _space("sx-f16", c["X_set"], metric, dtype=ehx.DTYPE_F16)
    assert s.scan_engine() == "i8"
    for r in (501, 600, 602, 606):
        assert s.get("k%d" % r).tobytes() == c["X"][r].tobytes()
    _every_search(s, c["X"], c["Q"], metric, c["key_rows"], v, name)
    s.drop()


# ---- g. the block-permuted layout ------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", sx.METRICS)
@pytest.mark.parametrize("kind", ["c", "d", "g"])
def test_graph_space_rows_of_one_kind(kind, metric):
    """a graph-mode space stores its fp32 rows once, block-permuted: the range, list and bitmap searches answer from them.
    (The graph itself is not built — build_batch = 0xFFFFFFFF, as test_extreme_values' graph cases over non-finite rows have
    it: none of these searches walks it, and what a graph built over NaN rows looks like is defined nowhere.)"""
    X, Q = xc._ladder(kind, D, seed=300 + xc.KINDS.index(kind) * 3 + sx.METRICS.index(metric), n=sx.N_GRAPH)
    n, nq = X.shape[0], Q.shape[0]
    what = "graph %s %s" % (kind, metric)
    s = _space("sx-graph", X, metric, mode=ehx.MODE_GRAPH, M=16, build_batch=0xFFFFFFFF)
    full = _oracle(X, Q, n, metric)
    for rank in sx.RANKS:
        _range(s, X, Q, metric, full, sx.rank_radii(full, rank), None, "%s range@%d" % (what, rank))
    half, few = sx.bitmaps(n, 3)
    for k in sx.MASKED_KS:
        _masked(s, X, Q, metric, k, half, None, "%s bitmap 50 %% k=%d" % (what, k))
        _masked(s, X, Q, metric, k, few, None, "%s bitmap of %d rows k=%d" % (what, few.sum(), k))
    shared, per = sx.lists(n, nq, 4)
    _assert_rows(s.knn_among(Q, 10, shared), _among(X, Q, 10, metric, shared), what + " shared list")
    want = [_among(X, Q[i:i + 1], 10, metric, np.unique(per[i]))[0] for i in range(nq)]
    _assert_rows(s.knn_among(Q, 10, per), want, what + " per-query lists")
    assert s.stats()["n_uncertified"] == 0
    s.drop()


# ---- h. a row-sharded space ------------------------------------------------------------------------------------------

def test_the_shards_of_a_sharded_space_take_the_large_k_route():
    """two shards of 20 000 rows just inside the band's high edge: both serve every query on the route
    (tests/test_side_extreme_model.py), asserted as tests/test_knn_largek.py asserts its sharded case"""
    X, Q = sx.sharded()
    s = ehx.Space.unique("sx-sharded", D, metric=ehx.METRIC_L2SQ, initial_capacity=len(X), shards=2)
    s.set_batch(_keys(len(X)), X)
    st0 = s.stats()
    _assert_rows(s.knn(Q, sx.LARGE_K), _lists(_oracle(X, Q, sx.LARGE_K, "l2"), sx.LARGE_K), "two shards")
    st1 = s.stats()
    assert st1["n_i8_queries"] - st0["n_i8_queries"] == 2 * len(Q) and st1["n_exhaustive"] == st0["n_exhaustive"]
    assert st1["n_uncertified"] == 0
    s.drop()
