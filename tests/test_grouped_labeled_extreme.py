"""The grouped kNN under a label column (ehx_knn_grouped_labeled*) against the oracle at extreme and non-finite values, built
on tests/extreme_cases.py the way tests/test_grouped_masked_extreme.py is: rows INSIDE a tenant that hold NaN, +-Inf or FLT_MAX
components, zero rows, rows at the edges of the band the int8 filter bounds, and queries that are not finite — on the list
route (700 rows) and at the smallest shape that reaches the scan route (20 000 rows).  A row whose distance is NaN is never
returned and never counts toward a cap.

Every expected answer is the oracle's full list (grouped_model.oracle_all, which does not list NaN distances) with the rows
of other tenants dropped, capped by the plain-Python greedy (grouped_labeled_cases.expected).  Bar: ids equal, distance BYTES
equal, counts equal, NO_ID / +Inf behind the count, the device form byte for byte the host form."""
import numpy as np
import pytest

import extreme_cases as xc
import grouped_labeled_cases as glc
import grouped_model as gm
import test_grouped_masked_extreme as gx
import test_knn_grouped_labeled as t

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")

f32 = np.float32
METRICS = ("l2", "ip", "cosine")


@pytest.mark.parametrize("metric", METRICS)
def test_list_route_with_odd_rows_inside_a_tenant(metric):
    n, d, nq = 700, 12, 16
    rng = np.random.default_rng(600 + METRICS.index(metric))
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    odd = [10, 47, 84, 121, 158, 195, 232, 269]            # all of group 10 (rows = 10 mod 37)
    gx._odd_rows(X, odd)
    X[306] = Q[0] + f32(0.5)                                # group 10's nearest finite row for query 0 ...
    X[10, :] = Q[0]
    X[10, 1] = xc.POS_NAN                                   # ... behind a NaN row that would be nearer still
    gx._odd_queries(rng, Q)
    groups = (np.arange(n) % 37).astype(np.uint32)
    groups[::13] = gm.NONE
    groups[odd] = 10
    groups[306] = 10
    col = np.where(rng.random(n) < 0.6, 20, 21).astype(np.uint32)
    col[odd] = 20                                           # the odd rows are tenant 20's
    col[306] = 20
    want = np.array([20, 21, 30], dtype=np.uint32)[np.arange(nq) % 3]   # (30: nobody)
    s = t._space("groupedl-odd", X, metric)
    full = gm.oracle_all(X, Q, metric)
    for k, m in ((8, 1), (8, 3), (256, 250)):
        c0 = t._counters(s)
        got = s.knn_grouped_labeled(Q, k, groups, col, want, per_group=m)
        what = "odd rows %s k=%d m=%d" % (metric, k, m)
        t._assert_rows(got, glc.expected(full, groups, col, want, k, m), k, what)
        assert (t._counters(s) - c0).tolist() == [0, nq, 0, 0, 1], what
        assert 10 not in got[0] and 47 not in got[0]        # a NaN row is never returned ...
        assert got[2][3] == 0                               # (query 3 holds a NaN and wants tenant 20: nothing is returned for it)
    # ... and never counts toward its group's cap: at k = 256 every group of the tenant is represented, group 10 by its
    # nearest row of the tenant that HAS a distance, although row 10 — the query itself but for a NaN — is the tenant's too
    got = s.knn_grouped_labeled(Q, 256, groups, col, want, per_group=1)
    rep = next(int(x) for x in full[0][0, :int(full[2][0])] if groups[int(x)] == 10 and col[int(x)] == 20)
    assert rep in got[0][0] and col[10] == 20 and groups[10] == 10
    if metric == "l2":
        assert rep == 306
    assert t._same_bytes(got, t._device_form(s, Q, 256, groups, col, want, 1))
    s.drop()


@pytest.mark.parametrize("metric", METRICS)
def test_scan_route_with_rows_at_the_band_edges_and_odd_queries(metric):
    """an int8 space: every row inside the band the filter bounds — blocks just inside its low and high edge, zero rows,
    each block inside one of the big tenants — and queries that are not finite, which the bound does not serve: they are
    handed to the list route under their own tenant"""
    X0, Q0 = t.lc.gauss(20000, 64, 64, 1)
    X, Q = X0.copy(), Q0.copy()
    rng = np.random.default_rng(700 + METRICS.index(metric))
    X[3000:3064] = xc._kind_rows("a_lo", rng, 64, 64)
    X[9000:9064] = xc._kind_rows("a_hi", rng, 64, 64)
    X[17000:17016] = 0
    gx._odd_queries(rng, Q)
    groups = gm.labels_clustered(len(X))
    col = glc.tenant_column().copy()
    for (lo, hi), tenant in zip(((3000, 3064), (9000, 9064), (17000, 17016)), glc.BIG):
        col[lo:hi] = tenant
    want = glc.scan_want()
    s = t._i8_space("groupedl-band", X, metric)
    full = gm.oracle_all(X, Q, metric)
    for k, m in ((10, 1), (100, 4)):
        c0 = t._counters(s)
        got = s.knn_grouped_labeled(Q, k, groups, col, want, per_group=m)
        dc = t._counters(s) - c0
        what = "band edges %s k=%d m=%d" % (metric, k, m)
        print(what, dc.tolist())
        t._assert_rows(got, glc.expected(full, groups, col, want, k, m), k, what)
        assert dc[0] + dc[1] == 64 and dc[3] == t.PASSES and dc[4] == 1, (what, dc)   # the scan route was taken
        assert got[2][2] == 0                               # the NaN query
    assert t._same_bytes(got, t._device_form(s, Q, 100, groups, col, want, 4))
    s.drop()


def test_a_large_space_with_non_finite_rows_takes_the_list_route_over_several_slabs():
    """NaN, Inf and FLT_MAX rows take a space off the int8 engine: 20 000 rows, tenants of about 6 000, two slabs"""
    X0, Q0 = t.lc.gauss(20000, 64, 64, 1)
    X, Q = X0.copy(), Q0.copy()
    odd = [5, 4100, 8200, 12300, 16400, 19990, 19995, 19999]
    gx._odd_rows(X, odd)
    groups = gm.labels_clustered(len(X))
    groups[odd] = 77                                        # one group: its NaN rows use up none of its cap
    col = glc.tenant_column().copy()
    col[odd] = 3                                            # ... inside one tenant
    want = glc.scan_want()
    s = t._space("groupedl-nonfinite", X, "l2")
    assert s.scan_engine() != "i8"
    full = gm.oracle_all(X, Q, "l2")
    for k, m in ((10, 1), (256, 2)):
        c0 = t._counters(s)
        got = s.knn_grouped_labeled(Q, k, groups, col, want, per_group=m)
        t._assert_rows(got, glc.expected(full, groups, col, want, k, m), k, "non-finite rows k=%d m=%d" % (k, m))
        assert (t._counters(s) - c0).tolist() == [0, 64, 0, 0, 1]
        assert 5 not in got[0] and 4100 not in got[0]
    assert t._same_bytes(got, t._device_form(s, Q, 256, groups, col, want, 2))
    s.drop()
