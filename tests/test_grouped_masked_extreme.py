"""The grouped kNN under row bitmaps (ehx_knn_grouped_masked*) against the oracle at extreme and non-finite values, in the
spirit of tests/test_filtered_searches_extreme.py: ALLOWED rows that hold NaN, +-Inf or FLT_MAX components, rows at the edges
of the band the int8 filter bounds, and queries that are not finite — on the list route (700 rows) and at the smallest shape
that reaches the scan route (20 000 rows).  A row whose distance is NaN is never returned and never counts toward a cap.

Every expected answer is the oracle's full list (grouped_model.oracle_all, which does not list NaN distances) with the rows
that are not allowed dropped, capped by the plain-Python greedy (grouped_masked_model.expected).  Bar: ids equal, distance
BYTES equal, counts equal, NO_ID / +Inf behind the count, the device form byte for byte the host form."""
import numpy as np
import pytest

import extreme_cases as xc
import grouped_masked_model as gmm
import grouped_model as gm
import test_knn_grouped_masked as t

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")

f32 = np.float32
FLT_MAX = np.finfo(f32).max
METRICS = ("l2", "ip", "cosine")


def _odd_rows(X, at):
    """rows at[0..7]: a NaN, a -NaN, a +Inf, a -Inf and a FLT_MAX component, a row of FLT_MAX, a zero row, a row of 1e19"""
    X[at[0], 1] = xc.POS_NAN
    X[at[1], 2] = xc.NEG_NAN
    X[at[2], 3] = np.inf
    X[at[3], 0] = -np.inf
    X[at[4], 1] = FLT_MAX
    X[at[5], :] = FLT_MAX
    X[at[6], :] = 0
    X[at[7], :] = f32(1e19)


def _odd_queries(rng, Q):
    """query 0 stays ordinary; 1: zero, 2: +NaN, 3: -NaN, 4: +Inf, 5: -Inf, 6-11: at the band edges, huge, tiny; 12: FLT_MAX"""
    for at, q in zip(range(1, 12), xc._odd_queries(rng, Q.shape[1])):
        Q[at] = q
    Q[12, 0] = FLT_MAX


@pytest.mark.parametrize("metric", METRICS)
def test_list_route_with_odd_allowed_rows(metric):
    n, d, nq = 700, 12, 16
    rng = np.random.default_rng(400 + METRICS.index(metric))
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    odd = [10, 47, 84, 121, 158, 195, 232, 269]            # all of group 10 (rows = 10 mod 37)
    _odd_rows(X, odd)
    X[306] = Q[0] + f32(0.5)                                # group 10's nearest finite row for query 0 ...
    X[10, :] = Q[0]
    X[10, 1] = xc.POS_NAN                                   # ... behind a NaN row that would be nearer still
    _odd_queries(rng, Q)
    labels = (np.arange(n) % 37).astype(np.uint32)
    labels[::13] = gm.NONE
    labels[odd] = 10
    labels[306] = 10
    allows = np.stack([rng.random(n) < 0.6, rng.random(n) < 0.6, np.zeros(n, dtype=bool)])
    allows[:2, odd] = True                                  # the odd rows are ALLOWED
    allows[:2, 306] = True
    mask_of = (np.arange(nq) % 3).astype(np.uint32)
    mask_of[0] = 0
    s = t._space("groupedm-odd", X, metric)
    full = gm.oracle_all(X, Q, metric)
    for k, m in ((8, 1), (8, 3), (256, 250)):
        c0 = t._counters(s)
        got = s.knn_grouped_masked(Q, k, labels, allows, mask_of, per_group=m)
        what = "odd rows %s k=%d m=%d" % (metric, k, m)
        t._assert_rows(got, gmm.expected(full, labels, allows, mask_of, k, m), k, what)
        assert (t._counters(s) - c0).tolist() == [0, nq, 0, 0, 1], what
        assert 10 not in got[0] and 47 not in got[0]        # a NaN row is never returned ...
        assert got[2][3] == 0                               # (query 3 holds a NaN under bitmap 0: nothing is returned for it)
    # ... and never counts toward its group's cap: at k = 256 every group is represented, group 10 by its nearest allowed row
    # that HAS a distance, although row 10 — the query itself but for a NaN — is allowed too
    got = s.knn_grouped_masked(Q, 256, labels, allows, mask_of, per_group=1)
    rep = next(int(x) for x in full[0][0, :int(full[2][0])] if labels[int(x)] == 10 and allows[0][int(x)])
    assert rep in got[0][0] and allows[0][10] and labels[10] == 10
    if metric == "l2":
        assert rep == 306
    assert t._same_bytes(got, t._device_form(s, Q, 256, labels, allows, mask_of, 1))
    s.drop()


@pytest.mark.parametrize("metric", METRICS)
def test_scan_route_with_rows_at_the_band_edges_and_odd_queries(metric):
    """an int8 space: every row inside the band the filter bounds — blocks just inside its low and high edge, zero rows —
    and queries that are not finite, which the bound does not serve: they are handed to the list route"""
    X0, Q0 = t.lc.gauss(20000, 64, 64, 1)
    X, Q = X0.copy(), Q0.copy()
    rng = np.random.default_rng(500 + METRICS.index(metric))
    X[3000:3064] = xc._kind_rows("a_lo", rng, 64, 64)
    X[9000:9064] = xc._kind_rows("a_hi", rng, 64, 64)
    X[17000:17016] = 0
    _odd_queries(rng, Q)
    labels = gm.labels_clustered(len(X))
    allows = gmm.scan_bitmaps(0.5).copy()
    for lo, hi in ((3000, 3064), (9000, 9064), (17000, 17016)):
        allows[:, lo:hi] = True
    mask_of = gmm.scan_mask_of(len(Q))
    s = t._i8_space("groupedm-band", X, metric)
    full = gm.oracle_all(X, Q, metric)
    for k, m in ((10, 1), (100, 4)):
        c0 = t._counters(s)
        got = s.knn_grouped_masked(Q, k, labels, allows, mask_of, per_group=m)
        dc = t._counters(s) - c0
        what = "band edges %s k=%d m=%d" % (metric, k, m)
        print(what, dc.tolist())
        t._assert_rows(got, gmm.expected(full, labels, allows, mask_of, k, m), k, what)
        assert dc[0] + dc[1] == 64 and dc[3] == t.PASSES and dc[4] == 1, (what, dc)   # the scan route was taken
        assert got[2][2] == 0                               # the NaN query
    assert t._same_bytes(got, t._device_form(s, Q, 100, labels, allows, mask_of, 4))
    s.drop()


def test_a_large_space_with_non_finite_rows_takes_the_list_route_over_several_slabs():
    """NaN, Inf and FLT_MAX rows take a space off the int8 engine: 20 000 rows, lists of about 10 000, three slabs"""
    X0, Q0 = t.lc.gauss(20000, 64, 64, 1)
    X, Q = X0.copy(), Q0.copy()
    odd = [5, 4100, 8200, 12300, 16400, 19990, 19995, 19999]
    _odd_rows(X, odd)
    labels = gm.labels_clustered(len(X))
    labels[odd] = 77                                        # one group: its NaN rows use up none of its cap
    allows = gmm.scan_bitmaps(0.5).copy()
    allows[:, odd] = True
    mask_of = gmm.scan_mask_of(len(Q))
    s = t._space("groupedm-nonfinite", X, "l2")
    assert s.scan_engine() != "i8"
    full = gm.oracle_all(X, Q, "l2")
    for k, m in ((10, 1), (256, 2)):
        c0 = t._counters(s)
        got = s.knn_grouped_masked(Q, k, labels, allows, mask_of, per_group=m)
        t._assert_rows(got, gmm.expected(full, labels, allows, mask_of, k, m), k, "non-finite rows k=%d m=%d" % (k, m))
        assert (t._counters(s) - c0).tolist() == [0, 64, 0, 0, 1]
        assert 5 not in got[0] and 4100 not in got[0]
    s.drop()
