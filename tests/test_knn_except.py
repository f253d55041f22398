"""GPU tests of the kNN with per-query exclusion lists (ehx_knn_except*, ehx_except.cpp, k_except.hip).

The reference is the CPU oracle alone: pyoracle.exhaustive at k + Lmax (Lmax: the case's longest de-duplicated in-range
list), every query's listed ids dropped in numpy, the first k of what remains — ids equal, distance BYTES equal, sentinels
behind the count.  Which route answered is read from ehx_test_except_counters."""
import ctypes as C
import functools

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
PASSES = 3   # of a space of 16 385 .. 65 536 rows at the default growth


def _counters(s):
    out = (C.c_uint64 * 5)()
    C.CDLL(_lib.LIB_PATH).ehx_test_except_counters(s._h, out)
    return np.array(list(out), dtype=np.int64)   # scan route, handed to the exact route, of those overflowed, scan passes, calls


def _space(name, X, metric, **kw):
    s = ehx.Space.unique(name, X.shape[1], metric=EM[metric], initial_capacity=len(X), **kw)
    s.set_batch(["k%d" % i for i in range(len(X))], X)
    return s


@functools.lru_cache(maxsize=None)
def _deep(case, metric, depth):
    """the oracle's lists of a named data set, computed once and shared"""
    X, Q = _data(case)
    return pyoracle.exhaustive(np.ascontiguousarray(X), np.ascontiguousarray(Q), min(depth, len(X)), lc.OM[metric])


def _data(case):
    if case == "gauss":
        return lc.gauss(20000, 64, 64, 1)
    if case == "ties":
        return lc.ties()[:2]
    return lc.model_cases()[case][:2]


def _mess(lists, n, seed=3):
    """every list as a caller may give it: unsorted, with repeats, with ids at or beyond the prefix; never above 4096 entries"""
    rng = np.random.default_rng(seed)
    out = []
    for l in lists:
        l = np.asarray(l, dtype=np.int64)
        room = _lib.EXCEPT_MAX_LIST - len(l)
        extra = np.concatenate([rng.choice(l, min(len(l), 3)) if len(l) else l, n + rng.integers(0, 2**40, 3)])[:room]
        out.append(rng.permutation(np.concatenate([l, extra])).astype(np.uint64))
    return out


def _expect(deep, lists, k, n):
    """the oracle's lists with every query's listed rows dropped, cut at k"""
    oids, odist, ocnt = deep
    nq = len(ocnt)
    ids, dist, cnt = np.full((nq, k), NO_ID), np.full((nq, k), np.inf, dtype=f32), np.zeros(nq, dtype=np.uint32)
    for i in range(nq):
        drop = np.unique(np.asarray(lists[i], dtype=np.uint64))
        drop = drop[drop < n]
        assert k + len(drop) <= oids.shape[1] or oids.shape[1] == n, "the oracle's depth"
        c = int(ocnt[i])
        keep = ~np.isin(oids[i, :c], drop)
        m = min(k, int(keep.sum()))
        ids[i, :m], dist[i, :m], cnt[i] = oids[i, :c][keep][:m], odist[i, :c][keep][:m], m
    return ids, dist, cnt


def _assert_exact(got, want, what):
    for g, w, name in zip(got, want, ("ids", "distance bytes", "counts")):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), "%s: %s differ" % (what, name)


def _run(s, Q, k, lists, deep, what, n=None):
    """one knn_except call against the reference -> how the counters moved"""
    c0, q0 = _counters(s), s.stats()["n_queries"]
    got = s.knn_except(Q, k, lists)
    _assert_exact(got, _expect(deep, lists, k, len(s) if n is None else n), what)
    assert s.stats()["n_queries"] - q0 == len(Q) and s.stats()["n_uncertified"] == 0, what
    return _counters(s) - c0


# ---- 1. the scan route: three metrics x the k on both sides of the certified chain's and the route's limits x four lists ----

_spaces = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_spaces():
    yield
    for s in _spaces.values():
        s.drop()


def _gauss_space(metric):
    if metric not in _spaces:
        _spaces[metric] = _space("except-" + metric, lc.gauss(20000, 64, 64, 1)[0], metric)
        assert _spaces[metric].scan_engine() == "i8"
    return _spaces[metric]


def _gauss_lists(kind, metric):
    near = _deep("gauss", metric, 256 + 4096)[0].astype(np.int64)
    rng = np.random.default_rng(5)
    return {"empty": [[] for _ in range(64)], "one": [near[i, :1] for i in range(64)],
            "near300": [near[i, :300] for i in range(64)],   # (they span all three passes' id ranges)
            "rand4096": [rng.choice(20000, 4090, replace=False) for _ in range(64)]}[kind]


@pytest.mark.parametrize("kind", ["empty", "one", "near300", "rand4096"])
@pytest.mark.parametrize("k", [10, 48, 49, 256])
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_the_scan_route_is_exact(metric, k, kind):
    X, Q = lc.gauss(20000, 64, 64, 1)
    lists = _mess(_gauss_lists(kind, metric), 20000)
    dc = _run(_gauss_space(metric), Q, k, lists, _deep("gauss", metric, 256 + 4096), "%s k=%d %s" % (metric, k, kind))
    assert dc[0] + dc[1] == 64 and dc[2] <= dc[1] and dc[3] == PASSES and dc[4] == 1, dc
    if k <= 48 and kind in ("empty", "one"):   # k + L <= 256: the radii lie at or below the large-k route's at k + L
        assert dc[1] == 0, dc


# ---- 2. shapes: wide rows, binary16 rows, two device batches; the query's 50 nearest as its list, k = 100 ----

@pytest.mark.parametrize("case", ["d768", "f16", "chunks"])
def test_shapes(case):
    X, Q, metric, _ = lc.model_cases()[case]
    deep = _deep(case, metric, 150)
    s = _space("except-" + case, X, metric, **({"dtype": ehx.DTYPE_F16} if case == "f16" else {}))
    assert s.scan_engine() == "i8"
    dc = _run(s, Q, 100, _mess([r[:50] for r in deep[0]], len(X)), deep, case)
    # (2100 queries: a device batch of 2048 on the scan route; the 52 left are below its gate and take the exact route)
    assert dc[0] + dc[1] == len(Q) and dc[0] > 0 and dc[3] == PASSES, dc
    s.drop()


# ---- 3. the exact route ----

@pytest.mark.parametrize("case", ["63 queries", "16000 rows", "scan_f32", "graph"])
def test_the_exact_route(case):
    X, Q = lc.gauss(20000, 64, 64, 1)
    kw = {}
    if case == "63 queries":
        Q = Q[:63]
    elif case == "16000 rows":
        X = X[:16000]            # below the int8 engine's row count
    elif case == "graph":
        X, Q = np.ascontiguousarray(X[:2000, :16]), np.ascontiguousarray(Q[:, :16])
        kw = {"mode": ehx.MODE_GRAPH, "M": 16}
    deep = pyoracle.exhaustive(np.ascontiguousarray(X), np.ascontiguousarray(Q), 400, lc.OM["l2"])
    s = _space("except-exact", X, "l2", **kw)
    if case == "scan_f32":
        s.set_scan(ehx.SCAN_F32)
    for k in (10, 100):
        dc = _run(s, Q, k, _mess([r[:300] for r in deep[0]], len(X)), deep, "%s k=%d" % (case, k))
        assert dc.tolist() == [0, len(Q), 0, 0, 1], dc
    s.drop()


# ---- 4. edges ----

def test_fewer_allowed_rows_than_k():
    X, Q = lc.gauss(20000, 64, 64, 1)
    X = X[:300]
    deep = pyoracle.exhaustive(np.ascontiguousarray(X), np.ascontiguousarray(Q), 300, lc.OM["l2"])
    rng = np.random.default_rng(9)
    s = _space("except-300", X, "l2")
    lists = _mess([rng.choice(300, 295, replace=False) for _ in range(64)], 300)
    _run(s, Q, 10, lists, deep, "295 of 300 rows listed")
    assert (s.knn_except(Q, 10, lists)[2] == 5).all()
    s.drop()


def test_a_list_of_the_4096_nearest_rows():
    X, Q = lc.gauss(20000, 64, 64, 1)
    deep = _deep("gauss", "l2", 256 + 4096)
    lists = [[] for _ in range(64)]
    lists[7] = np.random.default_rng(2).permutation(deep[0][7, :4096])   # whichever route answers query 7
    dc = _run(_gauss_space("l2"), Q, 10, lists, deep, "4096 nearest")
    assert dc[0] + dc[1] == 64 and dc[2] <= dc[1], dc


def test_queries_the_bound_does_not_serve_are_handed_on():
    X, Q0 = lc.gauss(20000, 64, 64, 1)
    Q = Q0.copy()
    Q[3, 7] = np.nan
    Q[10] = 0
    deep = pyoracle.exhaustive(np.ascontiguousarray(X), Q, 150, lc.OM["cosine"])
    lists = _mess([r[:50] for r in _deep("gauss", "cosine", 256 + 4096)[0]], 20000)
    s = _gauss_space("cosine")
    dc = _run(s, Q, 100, lists, deep, "NaN and zero queries")
    assert dc[1] >= 2 and dc[0] + dc[1] == 64, dc
    assert int(s.knn_except(Q, 100, lists)[2][3]) == 0        # a NaN distance is never a neighbour


def test_unlisted_copies_of_a_row_come_back_in_id_order():
    X, Q, at = lc.ties()
    s = _space("except-ties", X, "l2")
    lists = [at[::2] for _ in range(64)]   # half of the 300 copies of query 0's row
    _run(s, Q, 100, _mess(lists, 20000), _deep("ties", "l2", 256 + 4096), "ties")
    got = s.knn_except(Q, 100, lists)
    assert np.array_equal(got[0][0].astype(np.int64), at[1::2][:100]) and (got[1][0] == 0).all()
    s.drop()


# ---- 5. the contract's other statements: knn_masked under the complement bitmap; lists given as keys ----

def test_equals_knn_masked_under_the_complement_bitmap():
    X, Q = lc.gauss(20000, 64, 64, 1)
    s = _gauss_space("ip")
    seen = np.random.default_rng(4).choice(20000, 1000, replace=False)
    allow = np.ones(20000, dtype=bool)
    allow[seen] = False
    for k in (10, 48):
        _assert_exact(s.knn_except(Q, k, [seen] * 64), s.knn_masked(Q, k, allow), "complement k=%d" % k)


def test_lists_given_as_keys():
    X, Q = lc.gauss(20000, 64, 64, 1)
    s = _gauss_space("l2")
    near = _deep("gauss", "l2", 256 + 4096)[0][:, :40].astype(np.int64)
    keys = [["k%d" % r for r in row] + ["never-stored-%d" % i, "k20000"] for i, row in enumerate(near)]
    _assert_exact(s.knn_except_keys(Q, 10, keys), s.knn_except(Q, 10, list(near)), "keys")
