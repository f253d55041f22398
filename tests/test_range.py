"""GPU tests of the exact range search (ehx_range, ehx_range_device, ehx_range_keys).

Expected answers come from the oracle only: pyoracle.exhaustive(X, Q, k = n, metric) lists every row by (distance, id),
the list is cut at `dist <= radius` (tests/range_cases.py), and ids must be equal, distance BYTES equal, counts and totals
equal, tails the sentinels.  F16 spaces use the oracle on X.astype(float16).astype(float32).  The int8 cases take the
oracle's 6 000 nearest of 20 000 rows (every radius used lies below the 6 000th distance, asserted)."""
import ctypes as C

import numpy as np
import pytest

import range_cases as rc
from oracle import pyoracle

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402

METRICS = {"l2": (ehx.METRIC_L2SQ, pyoracle.METRIC_L2), "ip": (ehx.METRIC_IP, pyoracle.METRIC_IP),
           "cosine": (ehx.METRIC_COSINE, pyoracle.METRIC_COSINE)}
NO_ID = np.uint64(2**64 - 1)
f32 = np.float32


def _keys(n):
    return ["k%d" % i for i in range(n)]


def _raw():
    return C.CDLL(_lib.LIB_PATH)


def _counters(s):
    out = (C.c_uint64 * 4)()
    _raw().ehx_test_range_counters(s._h, out)
    return np.array(list(out), dtype=np.int64)   # int8 path, exact path, pool overflows, truncated


def _live():
    out = (C.c_uint64 * 4)()
    _raw().ehx_test_live_resources(out)
    return list(out)


def _assert_range(got, want, max_results, what):
    ids, dist, cnt, total = got
    assert ids.shape == (len(want), max_results) and dist.shape == ids.shape
    for i, (wids, wdist, wtotal) in enumerate(want):
        c = int(cnt[i])
        assert int(total[i]) == wtotal, "%s: query %d total %d, the oracle %d" % (what, i, int(total[i]), wtotal)
        assert c == len(wids) == min(wtotal, max_results), "%s: query %d count %d, the oracle %d" % (what, i, c, len(wids))
        assert [int(v) for v in ids[i, :c]] == wids, "%s: query %d ids differ" % (what, i)
        assert dist[i, :c].tobytes() == wdist.tobytes(), "%s: query %d distance bytes differ" % (what, i)
        assert (ids[i, c:] == NO_ID).all() and np.isposinf(dist[i, c:]).all(), "%s: query %d tail sentinels" % (what, i)


def _device_form(space, Q, radius, max_results, with_total=True):
    import torch
    nq = len(Q)
    dq = torch.tensor(np.ascontiguousarray(Q, dtype=np.float32), device="cuda")
    dr = torch.tensor(np.ascontiguousarray(radius, dtype=np.float32), device="cuda")
    o_ids = torch.full((nq, max_results), -7, dtype=torch.int64, device="cuda")
    o_dist = torch.full((nq, max_results), -7.0, dtype=torch.float32, device="cuda")
    o_cnt = torch.full((nq,), 77, dtype=torch.int32, device="cuda")
    o_tot = torch.full((nq,), -7, dtype=torch.int64, device="cuda") if with_total else None
    space.range_device(dq, dr, max_results, o_ids, o_dist, o_cnt, o_tot)
    torch.cuda.synchronize()
    return (o_ids.cpu().numpy().view(np.uint64), o_dist.cpu().numpy(), o_cnt.cpu().numpy().view(np.uint32),
            o_tot.cpu().numpy().view(np.uint64) if with_total else None)


def _same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _radii(dist, cnt, max_results):
    """one radius per query from the oracle's sorted distances: below the minimum; exactly the j-th distance and the float
    just below it, j in {1, 63, 64, 65, max_results, max_results + 1, n} (as far as the space has rows)"""
    nq = len(cnt)
    n = int(cnt.min())
    vals = []
    for j in (1, 63, 64, 65, max_results, max_results + 1, n):
        j = min(j, n)
        vals.append(lambda i, j=j: dist[i, j - 1])
        vals.append(lambda i, j=j: np.nextafter(dist[i, j - 1], f32(-np.inf)))
    vals.append(lambda i: np.nextafter(dist[i, 0], f32(-np.inf)))
    return np.array([vals[i % len(vals)](i) for i in range(nq)], dtype=f32)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_exact_path_flat(metric, dtype):
    em, om = METRICS[metric]
    nq = 15
    for n in (1, 255, 257, 1000):
        for d in (3, 19, 128, 130):
            rng = np.random.default_rng(1000 * n + d)
            X = rng.standard_normal((n, d)).astype(f32)
            Q = rng.standard_normal((nq, d)).astype(f32)
            Xs = X.astype(np.float16).astype(f32) if dtype == "f16" else X
            s = ehx.Space.unique("range", d, metric=em, initial_capacity=n,
                                 dtype=ehx.DTYPE_F16 if dtype == "f16" else ehx.DTYPE_F32)
            s.set_batch(_keys(n), X)
            oids, odist, ocnt = pyoracle.exhaustive(Xs, Q, n, om)
            for mr in (1, 64, 65, 1024):
                r = _radii(odist, ocnt, mr)
                want = rc.cut(oids, odist, ocnt, r, mr)
                host = s.range_search(Q, r, mr)
                _assert_range(host, want, mr, "n=%d d=%d max_results=%d" % (n, d, mr))
                if mr in (1, 65):
                    assert _same_bytes(host, _device_form(s, Q, r, mr)), "host and device forms differ"
            c = _counters(s)
            assert c[0] == 0 and c[1] == 4 * nq + 2 * nq and c[2] == 0
            assert s.stats()["n_uncertified"] == 0
            s.drop()


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_graph_space_answers_from_its_stored_rows(metric):
    em, om = METRICS[metric]
    rng = np.random.default_rng(20)
    n, d, nq = 2000, 20, 15
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    s = ehx.Space.unique("range-graph", d, metric=em, mode=ehx.MODE_GRAPH, M=16, initial_capacity=n)
    s.set_batch(_keys(n), X)
    oids, odist, ocnt = pyoracle.exhaustive(X, Q, n, om)
    for mr in (64, 1024):
        r = _radii(odist, ocnt, mr)
        host = s.range_search(Q, r, mr)
        _assert_range(host, rc.cut(oids, odist, ocnt, r, mr), mr, "graph max_results=%d" % mr)
        assert _same_bytes(host, _device_form(s, Q, r, mr))
    assert s.stats()["n_uncertified"] == 0
    s.drop()


@pytest.mark.parametrize("mode", ["flat", "graph"])
def test_more_members_than_a_pool(mode):
    """+Inf admits every row: 4 200 > kPoolCap members, the answer is the exact top max_results and the exact total"""
    rng = np.random.default_rng(21)
    n, d, nq = 4200, 20, 5
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    kw = dict(mode=ehx.MODE_GRAPH, M=16) if mode == "graph" else {}
    s = ehx.Space.unique("range-over", d, metric=ehx.METRIC_L2SQ, initial_capacity=n, **kw)
    s.set_batch(_keys(n), X)
    oids, odist, ocnt = pyoracle.exhaustive(X, Q, n, pyoracle.METRIC_L2)
    r = np.array([np.inf, odist[1, 4149], np.inf, odist[3, 9], np.inf], dtype=f32)
    for mr in (10, 64, 300):
        c0 = _counters(s)
        _assert_range(s.range_search(Q, r, mr), rc.cut(oids, odist, ocnt, r, mr), mr, "%s max_results=%d" % (mode, mr))
        dc = _counters(s) - c0
        assert dc.tolist() == [0, nq, 4, 4]
    assert s.stats()["n_uncertified"] == 0
    s.drop()


def test_ties_at_the_boundary_are_all_in():
    rng = np.random.default_rng(3)
    n, d = 500, 24
    X = rng.standard_normal((n, d)).astype(f32)
    X[[17, 230, 401]] = X[5]
    Q = np.stack([X[5] + f32(0.25), X[5] + f32(0.25)]).astype(f32)
    s = ehx.Space.unique("range-ties", d, metric=ehx.METRIC_L2SQ, initial_capacity=n)
    s.set_batch(_keys(n), X)
    oids, odist, ocnt = pyoracle.exhaustive(X, Q, n, pyoracle.METRIC_L2)
    j = [int(v) for v in oids[0]].index(5)
    r = np.array([odist[0, j], np.nextafter(odist[0, j], f32(-np.inf))], dtype=f32)
    for mr in (j + 2, 64):   # j + 2: the cut falls between the tied rows
        ids, dist, cnt, total = got = s.range_search(Q, r, mr)
        _assert_range(got, rc.cut(oids, odist, ocnt, r, mr), mr, "ties")
        assert int(total[0]) == j + 4 and int(total[1]) == j
        assert [int(v) for v in ids[0, j:j + 2]] == [5, 17]
    assert [int(v) for v in ids[0, j:j + 4]] == [5, 17, 230, 401]
    s.drop()


def test_non_finite_radii_and_values():
    rng = np.random.default_rng(4)
    n, d = 300, 24
    X = rng.standard_normal((n, d)).astype(f32)
    X[10, 3] = np.nan          # a NaN distance is no member, whatever the radius
    X[20] = 3.0e38             # (q - x)^2 overflows: +Inf is a distance, inside an infinite radius only
    Q = rng.standard_normal((4, d)).astype(f32)
    s = ehx.Space.unique("range-nf", d, metric=ehx.METRIC_L2SQ, initial_capacity=n)
    s.set_batch(_keys(n), X)
    oids, odist, ocnt = pyoracle.exhaustive(X, Q, n, pyoracle.METRIC_L2)
    r = np.array([np.nan, np.inf, -np.inf, odist[3, 40]], dtype=f32)
    got = s.range_search(Q, r, 512)
    _assert_range(got, rc.cut(oids, odist, ocnt, r, 512), 512, "non-finite")
    assert got[3].tolist() == [0, n - 1, 0, 41] and int(got[0][1, n - 2]) == 20
    assert _same_bytes(got, _device_form(s, Q, r, 512))
    assert _same_bytes(got[:3], _device_form(s, Q, r, 512, with_total=False)[:3])   # out_total may be NULL
    s.drop()
    # inner product: a dot product that overflows gives the distance -Inf, an ordinary member
    X = rng.standard_normal((n, d)).astype(f32)
    X[7] = 3.0e38
    Q = np.abs(rng.standard_normal((3, d))).astype(f32) * f32(1e3)
    s = ehx.Space.unique("range-ip", d, metric=ehx.METRIC_IP, initial_capacity=n)
    s.set_batch(_keys(n), X)
    oids, odist, ocnt = pyoracle.exhaustive(X, Q, n, pyoracle.METRIC_IP)
    assert np.isneginf(odist[:, 0]).all() and (oids[:, 0] == 7).all()
    r = np.array([-np.inf, odist[1, 5], np.inf], dtype=f32)
    got = s.range_search(Q, r, 16)
    _assert_range(got, rc.cut(oids, odist, ocnt, r, 16), 16, "inner product, -Inf distance")
    assert got[3].tolist() == [1, 6, n]
    s.drop()


def test_scalar_radius_and_keys_form():
    rng = np.random.default_rng(6)
    n, d, nq = 1500, 24, 20
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    s = ehx.Space.unique("range-keys", d, metric=ehx.METRIC_COSINE, initial_capacity=n)
    s.set_batch(_keys(n), X)
    oids, odist, ocnt = pyoracle.exhaustive(X, Q, n, pyoracle.METRIC_COSINE)
    r0 = f32(np.median(odist[:, 30]))
    got = s.range_search(Q, float(r0), 40)   # a scalar broadcasts
    _assert_range(got, rc.cut(oids, odist, ocnt, np.full(nq, r0, dtype=f32), 40), 40, "scalar radius")
    keys, kdist, kcnt, ktotal = s.range_search_keys(Q, float(r0), 40)
    assert kdist.tobytes() == got[1].tobytes() and np.array_equal(kcnt, got[2]) and np.array_equal(ktotal, got[3])
    for i in range(nq):
        assert keys[i] == [s.key_of(int(v)) for v in got[0][i, :int(got[2][i])]]
    s.drop()


@pytest.mark.parametrize("d", rc.I8_DIMS)
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_int8_path(metric, d):
    em, _ = METRICS[metric]
    X, Q = rc.i8_data(d)
    oids, odist = rc.i8_oracle(d, metric)
    s = ehx.Space.unique("range-i8", d, metric=em, initial_capacity=rc.I8_ROWS)
    s.set_batch(_keys(rc.I8_ROWS), X)
    assert s.scan_engine() == "i8"
    mr = rc.I8_MAX_RESULTS
    for nq in (1, rc.I8_QUERIES):
        depth = np.full(nq, odist.shape[1], dtype=np.uint32)
        for rank in rc.I8_RANKS:
            r = odist[:nq, rank - 1].copy()
            assert (odist[:nq, -1] > r).all()
            want = rc.cut(oids[:nq], odist[:nq], depth, r, mr)
            assert all(w[2] >= rank for w in want)
            c0 = _counters(s)
            got = s.range_search(Q[:nq], r, mr)
            dc = _counters(s) - c0
            _assert_range(got, want, mr, "int8 nq=%d rank=%d" % (nq, rank))
            # every query on the int8 path, none overflowed (tests/test_range_model.py: the bound alone stays within a pool)
            assert dc[0] == nq and dc[1] == 0 and dc[2] == 0, dc
            assert dc[3] == sum(w[2] > mr for w in want) and (rank < 300 or dc[3] == nq)
            if nq > 1 and rank == 100:
                assert _same_bytes(got, _device_form(s, Q[:nq], r, mr))
    assert s.stats()["n_uncertified"] == 0
    s.drop()


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_int8_pool_overflow_falls_to_the_exact_path(metric):
    em, _ = METRICS[metric]
    d, nq = 128, 64
    X, Q = rc.i8_data(d)
    oids, odist = rc.i8_oracle(d, metric)
    s = ehx.Space.unique("range-i8-over", d, metric=em, initial_capacity=rc.I8_ROWS)
    s.set_batch(_keys(rc.I8_ROWS), X)
    assert s.scan_engine() == "i8"
    r = odist[:nq, 9].copy()
    wide = np.arange(nq) % 8 == 3
    r[wide] = odist[:nq, 4999][wide]
    assert (odist[:nq, -1] > r).all()
    depth = np.full(nq, odist.shape[1], dtype=np.uint32)
    for mr in (256, 10):   # (10: the fall-back is the engine chain itself, 256: its paged exhaustive pass)
        want = rc.cut(oids[:nq], odist[:nq], depth, r, mr)
        assert all(want[i][2] >= 5000 for i in np.nonzero(wide)[0])
        c0 = _counters(s)
        got = s.range_search(Q[:nq], r, mr)
        dc = _counters(s) - c0
        _assert_range(got, want, mr, "overflow, max_results=%d" % mr)
        assert dc[0] == nq - 8 and dc[1] == 8 and dc[2] == 8, dc   # those 8 overflowed, the other 56 stayed
        assert _same_bytes(got, _device_form(s, Q[:nq], r, mr))
    # radii the bound does not map (+-Inf) go to the exact path; NaN has no members and stays
    r2 = odist[:nq, 9].copy()
    r2[5], r2[6], r2[7] = np.inf, np.nan, -np.inf
    want = rc.cut(oids[:nq], odist[:nq], depth, np.where(np.isinf(r2), f32(-1), r2), 16)
    want[5] = ([int(v) for v in oids[5, :16]], odist[5, :16].copy(), rc.I8_ROWS)
    c0 = _counters(s)
    _assert_range(s.range_search(Q[:nq], r2, 16), want, 16, "non-finite radii on an int8 space")
    assert (_counters(s) - c0).tolist()[:3] == [nq - 2, 2, 1]
    assert s.stats()["n_uncertified"] == 0
    s.drop()


@pytest.mark.parametrize("how", ["scan_f32", "small"])
def test_spaces_without_the_int8_engine_take_the_exact_path(how):
    d, nq, mr = 128, 33, 256
    X, Q = rc.i8_data(d)
    oids, odist = rc.i8_oracle(d, "cosine")
    n = rc.I8_ROWS if how == "scan_f32" else 3000   # (below i8_min_rows = 16 Ki rows)
    s = ehx.Space.unique("range-noi8", d, metric=ehx.METRIC_COSINE, initial_capacity=n)
    s.set_batch(_keys(n), X[:n])
    if how == "scan_f32":
        s.set_scan(ehx.SCAN_F32)
        r = odist[:nq, 99].copy()
        want = rc.cut(oids[:nq], odist[:nq], np.full(nq, odist.shape[1], dtype=np.uint32), r, mr)
    else:
        ids, dist, cnt = pyoracle.exhaustive(X[:n], Q[:nq], n, pyoracle.METRIC_COSINE)
        r = dist[:, 99].copy()
        want = rc.cut(ids, dist, cnt, r, mr)
    assert s.scan_engine() != "i8"
    got = s.range_search(Q[:nq], r, mr)
    _assert_range(got, want, mr, how)
    assert _counters(s).tolist()[:3] == [0, nq, 0]
    assert _same_bytes(got, _device_form(s, Q[:nq], r, mr))
    s.drop()


def test_error_returns():
    rng = np.random.default_rng(8)
    n, d = 200, 8
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((3, d)).astype(f32)
    s = ehx.Space.unique("range-err", d, metric=ehx.METRIC_L2SQ, initial_capacity=n)
    s.set_batch(_keys(n), X)
    for mr, code in ((0, _lib.EINVAL), (1025, _lib.EUNSUPPORTED)):
        with pytest.raises(ehx.EhxError) as e:
            s.range_search(Q, 1.0, mr)
        assert e.value.code == code
    with pytest.raises(ValueError):
        s.range_search(Q, [1.0, 2.0], 4)      # three queries, two radii
    ids, dist, cnt, total = s.range_search(np.zeros((0, d), dtype=f32), 1.0, 4)   # no queries: EHX_OK, nothing written
    assert ids.shape == (0, 4) and cnt.shape == (0,) and total.shape == (0,)
    L = _lib.load()
    q = np.ascontiguousarray(Q)
    rad = np.ones(3, dtype=f32)
    o_ids, o_dist, o_cnt = np.zeros((3, 4), dtype=np.uint64), np.zeros((3, 4), dtype=f32), np.zeros(3, dtype=np.uint32)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    args = [P(o_ids, C.c_uint64), P(o_dist, C.c_float), P(o_cnt, C.c_uint32)]
    for hole in range(3):
        a = list(args)
        a[hole] = None
        assert L.ehx_range(s._h, 3, P(q, C.c_float), P(rad, C.c_float), 4, a[0], a[1], a[2], None) == _lib.EINVAL
    assert L.ehx_range(s._h, 3, P(q, C.c_float), None, 4, args[0], args[1], args[2], None) == _lib.EINVAL
    assert L.ehx_range(s._h, 3, P(q, C.c_float), P(rad, C.c_float), 4, args[0], args[1], args[2], None) == _lib.OK
    assert L.ehx_range_device(s._h, None, 3, None, None, 4, None, None, None, None) == _lib.EINVAL
    h = s._h
    s.drop()   # the tombstone answers for the dropped handle
    assert L.ehx_range(h, 3, P(q, C.c_float), P(rad, C.c_float), 4, args[0], args[1], args[2], None) == _lib.ENOTFOUND
    e0 = ehx.Space.unique("range-empty", d, metric=ehx.METRIC_L2SQ)
    got = e0.range_search(Q, np.inf, 4)
    assert (got[2] == 0).all() and (got[3] == 0).all() and (got[0] == NO_ID).all() and np.isposinf(got[1]).all()
    e0.drop()
    sh = ehx.Space.unique("range-sh", d, metric=ehx.METRIC_L2SQ, shards=2)
    sh.set_batch(_keys(n), X)
    with pytest.raises(ehx.EhxError) as e:
        sh.range_search(Q, 1.0, 4)
    assert e.value.code == _lib.EUNSUPPORTED and "sharded" in str(e.value)
    sh.drop()


def test_stats_deltas():
    rng = np.random.default_rng(9)
    n, d, nq = 1000, 16, 12
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    s = ehx.Space.unique("range-stats", d, metric=ehx.METRIC_L2SQ, initial_capacity=n)
    s.set_batch(_keys(n), X)
    st0 = s.stats()
    s.range_search(Q, 20.0, 5)
    st1 = s.stats()
    assert st1["n_queries"] - st0["n_queries"] == nq and st1["n_dist"] - st0["n_dist"] == nq * n
    assert st1["n_rerank"] == st0["n_rerank"] and st1["n_uncertified"] == 0
    s.drop()


def test_a_dropped_space_leaves_nothing_behind():
    L = _lib.load()
    _lib.check(L.ehx_init(None, 0))
    base = _live()
    d = 128
    X, Q = rc.i8_data(d)
    oids, odist = rc.i8_oracle(d, "cosine")
    s = ehx.Space.unique("range-life", d, metric=ehx.METRIC_COSINE, initial_capacity=rc.I8_ROWS)
    s.set_batch(_keys(rc.I8_ROWS), X)
    r = odist[:40, 9].copy()
    r[3] = odist[3, 4999]    # the int8 path, its overflow, the exact path and the kNN fall-back all create their scratch
    got = s.range_search(Q[:40], r, 16)
    assert int(got[3][3]) >= 5000 and _counters(s).tolist()[:3] == [39, 1, 1]
    assert _same_bytes(got, _device_form(s, Q[:40], r, 16))
    s.drop()
    assert _live() == base, "device allocations, pinned allocations, events, streams alive after the drop"
