"""GPU tests of the large-k scan route: flat searches with 48 < k <= 256 and at least 64 queries on a space whose first
engine is the int8 filter (ehx_largek.cpp, k_radius.hip).  Nothing but knn_device_locked decides the route, so the tests
call the ordinary entry points and read what happened from ehx_test_largek_counters and ehx_stats.

Expected answers come from the oracle only (pyoracle.exhaustive): ids equal, distance BYTES equal, sentinels behind the
count.  The cases that assert "no query handed on" are the ones tests/test_largek_model.py shows to stay within half a
pool at every pass (data: tests/largek_cases.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import largek_cases as lc
from oracle import pyoracle

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402

EM = {"l2": ehx.METRIC_L2SQ, "ip": ehx.METRIC_IP, "cosine": ehx.METRIC_COSINE}
NO_ID = np.uint64(2**64 - 1)
f32 = np.float32
PASSES = 3   # of a space of 16 385 .. 65 536 rows at the default growth (tests/test_largek_host.py)


def _keys(n, first=0):
    return ["k%d" % i for i in range(first, first + n)]


def _counters(s):
    out = (C.c_uint64 * 5)()
    C.CDLL(_lib.LIB_PATH).ehx_test_largek_counters(s._h, out)
    return np.array(list(out), dtype=np.int64)   # on the route, handed on, of those overflowed, scan passes, calls


def _space(name, X, metric, **kw):
    s = ehx.Space.unique(name, X.shape[1], metric=EM[metric], initial_capacity=len(X), **kw)
    s.set_batch(_keys(len(X)), X)
    return s


def _i8_space(name, X, metric, **kw):
    s = _space(name, X, metric, **kw)
    assert s.scan_engine() == "i8"
    return s


def _oracle(X, Q, k, metric):
    return pyoracle.exhaustive(np.ascontiguousarray(X), np.ascontiguousarray(Q), k, lc.OM[metric])


def _assert_exact(got, want, k, what):
    """want: the oracle's lists at some k' >= k (their first k columns are the oracle's at k)"""
    ids, dist, cnt = got
    oids, odist, ocnt = want
    assert ids.shape == (len(ocnt), k)
    wc = np.minimum(ocnt, k)
    assert np.array_equal(cnt, wc), "%s: counts differ" % what
    for i in range(len(ocnt)):
        c = int(wc[i])
        assert np.array_equal(ids[i, :c], oids[i, :c]), "%s: query %d ids differ" % (what, i)
        assert dist[i, :c].tobytes() == odist[i, :c].tobytes(), "%s: query %d distance bytes differ" % (what, i)
        assert (ids[i, c:] == NO_ID).all() and np.isposinf(dist[i, c:]).all(), "%s: query %d tail sentinels" % (what, i)


def _run(s, Q, k, want, what, route, handed=0, passes=PASSES, calls=1):
    """one knn call: exact, and the route's counters and the space's statistics moved as stated"""
    c0, st0 = _counters(s), s.stats()
    got = s.knn(Q, k)
    dc, st1 = _counters(s) - c0, s.stats()
    _assert_exact(got, want, k, what)
    assert dc[0] == route and dc[1] == handed and dc[3] == passes and dc[4] == calls, (what, dc)
    if route + handed:   # every query once in n_queries; the route's batch in n_i8_queries, what it handed on in both fall-backs
        assert st1["n_queries"] - st0["n_queries"] == len(Q), what
        assert st1["n_i8_queries"] - st0["n_i8_queries"] == route + handed, what
        assert st1["n_i8_fallback"] - st0["n_i8_fallback"] == handed, what
        assert st1["n_exhaustive"] - st0["n_exhaustive"] == handed, what
        assert st1["n_dist"] - st0["n_dist"] > len(Q) * len(s), what
    assert st1["n_uncertified"] == 0
    return got, dc


# ---- 1. the route, three metrics x every k at which something changes ----

@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_the_route_is_exact(metric):
    X, Q = lc.gauss(20000, 64, 64, 1)
    want = _oracle(X, Q, max(lc.KS), metric)
    s = _i8_space("largek-" + metric, X, metric)
    for k in lc.KS:
        _run(s, Q, k, want, "%s k=%d" % (metric, k), route=64)
    s.drop()


# ---- 2. the gates ----

def test_gates():
    X, Q = lc.gauss(20000, 64, 64, 1)
    want = _oracle(X, Q, 257, "l2")
    s = _i8_space("largek-gates", X, "l2")
    ex0 = s.stats()["n_exhaustive"]
    _run(s, Q[:63], 100, tuple(a[:63] for a in want), "63 queries", route=0, passes=0, calls=0)
    assert s.stats()["n_exhaustive"] - ex0 == 63
    _run(s, Q, 48, want, "k = 48", route=0, passes=0, calls=0)
    _run(s, Q, 257, want, "k = 257", route=0, passes=0, calls=0)
    assert s.stats()["n_exhaustive"] - ex0 == 63 + 64
    _run(s, Q, 100, want, "k = 100", route=64)          # ... and the same space does take it
    s.drop()
    small = _space("largek-small", X[:16000], "l2")          # below i8_min_rows
    assert small.scan_engine() != "i8"
    _run(small, Q, 100, _oracle(X[:16000], Q, 100, "l2"), "16 000 rows", route=0, passes=0, calls=0)
    small.drop()
    f32s = _space("largek-f32", X, "l2")
    f32s.set_scan(ehx.SCAN_F32)
    _run(f32s, Q, 100, want, "SCAN_F32", route=0, passes=0, calls=0)
    f32s.drop()
    g = ehx.Space.unique("largek-graph", 16, metric=ehx.METRIC_L2SQ, mode=ehx.MODE_GRAPH, M=16, initial_capacity=2000)
    g.set_batch(_keys(2000), np.random.default_rng(7).standard_normal((2000, 16)).astype(f32))
    g.knn(np.random.default_rng(8).standard_normal((64, 16)).astype(f32), 100)
    assert _counters(g).tolist() == [0, 0, 0, 0, 0]
    g.drop()


# ---- 3. ties ----

def test_ties_are_cut_by_id_across_passes():
    X, Q, at = lc.ties()
    want = _oracle(X, Q, 256, "l2")
    s = _i8_space("largek-ties", X, "l2")
    for k in (100, 256):
        got, _ = _run(s, Q, k, want, "ties k=%d" % k, route=64)
        # query 0 is the copied row: 300 rows at distance 0 in all three passes, the k lowest ids win
        assert np.array_equal(got[0][0].astype(np.int64), at[:k]) and (got[1][0] == 0).all()
    s.drop()


# ---- 4. shapes ----

@pytest.mark.parametrize("case", ["d200", "d768", "f16"])
def test_shapes(case):
    X, Q, metric, ks = lc.model_cases()[case]
    kw = {"dtype": ehx.DTYPE_F16} if case == "f16" else {}    # (the oracle runs on the rows rounded to binary16)
    s = _i8_space("largek-" + case, X, metric, **kw)
    for k in ks:
        _run(s, Q, k, _oracle(X, Q, k, metric), "%s k=%d" % (case, k), route=len(Q))
    s.drop()


# ---- 5. more queries than one device batch of the route ----

def test_two_chunks_of_queries():
    X, Q, metric, ks = lc.model_cases()["chunks"]
    assert 2048 < len(Q) <= 4096
    s = _i8_space("largek-chunks", X, metric)
    _run(s, Q, ks[0], _oracle(X, Q, ks[0], metric), "2100 queries", route=len(Q), passes=2 * PASSES)
    s.drop()


# ---- 6. queries handed to the exhaustive pass ----

def test_queries_the_bound_does_not_serve_are_handed_on():
    X, Q0 = lc.gauss(20000, 64, 64, 1)
    Q = Q0.copy()
    Q[3, 7] = np.nan
    Q[10] = 0
    s = _i8_space("largek-nan", X, "cosine")
    got, dc = _run(s, Q, 100, _oracle(X, Q, 100, "cosine"), "NaN and zero queries", route=62, handed=2)
    assert int(got[2][3]) == 0        # a NaN distance is never a neighbour
    s.drop()


def test_overflowed_pools_are_handed_on():
    """5 000 copies of row 5 inside the second pass's rows (4096 .. 16384): the queries near that row meet more than a
    pool of them at one distance there; the flag sticks, the exhaustive pass answers them"""
    X0, Q0 = lc.gauss(20000, 64, 64, 1)
    X, Q = X0.copy(), Q0.copy()
    X[6000:11000] = X[5]
    rng = np.random.default_rng(11)
    near = [2, 17, 40, 63]
    Q[near] = X[5][None, :] + f32(0.01) * rng.standard_normal((len(near), 64)).astype(f32)
    s = _i8_space("largek-over", X, "l2")
    want = _oracle(X, Q, 100, "l2")
    for i in near:
        assert [int(v) for v in want[0][i, :100]] == [5] + list(range(6000, 6099))
    c0 = _counters(s)
    _assert_exact(s.knn(Q, 100), want, 100, "overflow")
    dc = _counters(s) - c0
    assert dc[1] >= len(near) and dc[2] == dc[1] and dc[0] + dc[1] == 64, dc
    s.drop()


def test_clustered_rows_sorted_by_cluster():
    """rows sorted by cluster along the id, queries at the LAST cluster's centre: the strided sample still sees that
    cluster, the early passes find little, the last one much.  Pools may overflow: whatever is handed on overflowed."""
    rng = np.random.default_rng(12)
    n, d, n_cl = 20000, 64, 8
    cen = rng.standard_normal((n_cl, d)).astype(f32)
    X = (np.repeat(cen, n // n_cl, axis=0) + f32(0.3) * rng.standard_normal((n, d)).astype(f32)).astype(f32)
    Q = (cen[-1][None, :] + f32(0.05) * rng.standard_normal((64, d)).astype(f32)).astype(f32)
    s = _i8_space("largek-clustered", X, "l2")
    for k in (100, 256):
        c0, ex0 = _counters(s), s.stats()["n_exhaustive"]
        _assert_exact(s.knn(Q, k), _oracle(X, Q, k, "l2"), k, "clustered k=%d" % k)
        dc = _counters(s) - c0
        print("clustered k=%d: on the route %d, handed on %d, overflowed %d" % (k, dc[0], dc[1], dc[2]))
        assert dc[0] + dc[1] == 64 and dc[2] == dc[1] and dc[4] == 1, dc
        assert s.stats()["n_exhaustive"] - ex0 == dc[1]
    s.drop()


# ---- 7. neighbours of stored rows: k + 1 = 49 ----

def test_knn_by_keys_at_k_48_takes_the_route():
    X, Q, metric, ks = lc.model_cases()["bykeys"]
    s = _i8_space("largek-bykeys", X, metric)
    keys = ["k%d" % i for i in range(0, 64 * 300, 300)]
    c0 = _counters(s)
    ids, dist, cnt = s.knn_by_keys(keys, 48)
    dc = _counters(s) - c0
    assert dc.tolist() == [64, 0, 0, PASSES, 1], dc
    for i, key in enumerate(keys):       # (a single key: one query, the paged pass)
        i1, d1 = s.knn_by_key(key, 48)
        assert int(cnt[i]) == len(i1) == 48 and np.array_equal(ids[i], i1) and dist[i].tobytes() == d1.tobytes(), key
    assert (_counters(s) - c0)[4] == 1
    s.drop()


# ---- 8. a row-sharded space ----

def test_the_shards_of_a_sharded_space_take_the_route():
    X, Q = lc.gauss(40000, 64, 64, 6)
    s = ehx.Space.unique("largek-sharded", 64, metric=ehx.METRIC_L2SQ, initial_capacity=40000, shards=2)
    s.set_batch(_keys(40000), X)
    st0 = s.stats()
    _assert_exact(s.knn(Q, 100), _oracle(X, Q, 100, "l2"), 100, "two shards")
    st1 = s.stats()
    assert st1["n_i8_queries"] - st0["n_i8_queries"] == 2 * 64 and st1["n_exhaustive"] == st0["n_exhaustive"]
    assert st1["n_uncertified"] == 0
    s.drop()


# ---- 9. beside streamed appends ----

def test_searches_beside_appends_answer_for_a_published_prefix():
    """tests/test_append_under_search.py's case_c at 64 queries per call, k = 100: every answer is the oracle's over a prefix
    of completed Sets — the route plans its passes, seeds its sample and scans on ONE snapshot of the row count"""
    here = os.path.dirname(os.path.abspath(__file__))
    if here not in sys.path:
        sys.path.insert(0, here)
    import test_append_under_search as aus
    d, base, n_chunks, per = 128, 20000, 12, 40
    cen = aus._centres(31, 8, d)
    s = ehx.Space.unique("largek-aus", d, metric=ehx.METRIC_COSINE, initial_capacity=base + n_chunks * 8 * per)
    s.fill_synthetic(ehx.SEED_CORPUS, 0, base, True)
    Xb = pyoracle.gen_rows(ehx.SEED_CORPUS, 0, base, d, normalize=True)
    assert s.scan_engine() == "i8"
    c0 = _counters(s)
    chunks = [(aus._keys("c", j, 8 * per), aus._chunk_rows(cen, j, per, lambda j, m, r: r.uniform(0.97, 1.03, (m, 1)), 3))
              for j in range(n_chunks)]
    queries = {"k100": (aus._queries(cen, 8, 107), 100)}
    assert queries["k100"][0].shape[0] == 64
    X, bounds, rec = aus._stream(s, Xb, chunks, [aus._host_searcher(s, *queries["k100"], "k100")], pace=0.01)
    aus._check(X, bounds, rec, queries, pyoracle.METRIC_COSINE, False)
    dc = _counters(s) - c0
    assert dc[4] == len(rec) and dc[0] + dc[1] == 64 * len(rec) and dc[0] > 0, dc
    aus._final(s, X, queries, pyoracle.METRIC_COSINE)
    s.drop()
