"""GPU tests of the grouped kNN under a label column (ehx_knn_grouped_labeled*, ehx_groupedl.cpp, k_grouped.hip): FILTER
FIRST, THEN CAP — the first k eligible rows among the rows of the query's own tenant — on the scan route (the falling-radius
int8 scan, "the row's label is the query's" in its flush, a cap per group in its re-rank, the first radius from a sample of
the tenant's rows) and on the list route (the tenant's rows in slabs of 4096 drawn from the compacted lists, any number of
tenants in one launch per slab).

Expected answers are never the code under test: the oracle's distances of every prefix row (grouped_model.oracle_all), the
rows of other tenants dropped, capped by the plain-Python greedy (grouped_masked_model.expected under the bitmap table
labeled_cases.as_table makes of the wanted labels): ids equal, distance BYTES equal, counts equal, sentinels behind the count;
the device form on its own stream byte for byte the host form.  The scan cases that assert "none handed on" are the ones
tests/test_knn_grouped_labeled_host.py clears on the CPU."""
import ctypes as C

import numpy as np
import pytest

import grouped_labeled_cases as glc
import grouped_model as gm
import largek_cases as lc
import test_knn_grouped_masked as t

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402
from embeddinghub_amd.space import marshal_groups  # noqa: E402

NO_ID = t.NO_ID
NONE = gm.NONE
ALL_ONES = 0xFFFFFFFF
f32 = np.float32
PASSES = glc.PASSES
_space, _i8_space, _assert_rows, _same_bytes, _keys = t._space, t._i8_space, t._assert_rows, t._same_bytes, t._keys


def _counters(s):
    return t._hook(s, "ehx_test_grouped_labeled_counters")   # on the scan route, on the list route, of those overflowed, passes, calls


def _device_form(space, Q, k, groups, col, want, per_group, n_labels=None, own_stream=True):
    import torch
    g, n = marshal_groups(groups)
    col = np.ascontiguousarray(col, dtype=np.uint32)
    n = min(n, len(col)) if n_labels is None else n_labels
    dq = torch.tensor(np.ascontiguousarray(Q, dtype=f32), device="cuda")
    dg = torch.tensor(g.view(np.int32), device="cuda") if len(g) else None
    dc = torch.tensor(col.view(np.int32), device="cuda") if len(col) else None
    dw = torch.tensor(np.ascontiguousarray(want, dtype=np.uint32).view(np.int32), device="cuda")
    o_ids = torch.full((len(Q), k), -7, dtype=torch.int64, device="cuda")
    o_dist = torch.full((len(Q), k), -7.0, dtype=torch.float32, device="cuda")
    o_cnt = torch.full((len(Q),), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream() if own_stream else None
    space.knn_grouped_labeled_device(dq, k, dg, dc, n, dw, o_ids, o_dist, o_cnt, per_group=per_group,
                                     stream=st.cuda_stream if st else None)
    torch.cuda.synchronize()
    return (o_ids.cpu().numpy().view(np.uint64), o_dist.cpu().numpy(), o_cnt.cpu().numpy().view(np.uint32))


def _rows_of(full, index):
    """the oracle's lists of the queries `index` (queries that repeat a point share its list)"""
    return tuple(np.ascontiguousarray(a[index]) for a in full)


# ---- 1. the list route, every layout ----

@pytest.mark.parametrize("kind", ["flat_f32", "flat_f16", "graph_f32"])
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
@pytest.mark.parametrize("d", [7, 129, 650])
def test_list_route_every_layout(d, metric, kind):
    n, nq = 700, 5
    rng = np.random.default_rng(2100 + d)
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    col = (np.arange(n) % 5).astype(np.uint32)
    want = np.array([0, 4, 9, 1, 4], dtype=np.uint32)                 # query 2 on a tenant nobody carries
    kw = {"mode": ehx.MODE_GRAPH, "M": 16} if kind == "graph_f32" else {}
    s = _space("groupedl-small", X, metric, dtype=ehx.DTYPE_F16 if kind == "flat_f16" else ehx.DTYPE_F32, **kw)
    Xs = X.astype(np.float16).astype(f32) if kind == "flat_f16" else X   # the oracle reads the rows as stored
    full = gm.oracle_all(Xs, Q, metric)
    groups = gm.labels_mod37(n)
    for k in (10, 100):
        for m in (1, 3):
            c0 = _counters(s)
            got = s.knn_grouped_labeled(Q, k, groups, col, want, per_group=m)
            what = "%s %s d=%d k=%d m=%d" % (kind, metric, d, k, m)
            _assert_rows(got, glc.expected(full, groups, col, want, k, m), k, what)
            assert (_counters(s) - c0).tolist() == [0, nq, 0, 0, 1], what
            assert got[2][2] == 0 and (got[0][2] == NO_ID).all() and np.isposinf(got[1][2]).all()   # the absent tenant's query
            assert (got[2][[0, 1, 3, 4]] > 0).all()                                              # ... and only its
    assert _same_bytes(got, _device_form(s, Q, 100, groups, col, want, 3))
    s.drop()


# ---- 2. more tenants than a table of bitmaps takes, ONE call ----

def test_more_tenants_than_a_bitmap_table_takes():
    n, d, n_tenants, k = 9000, 16, 300, 10
    rng = np.random.default_rng(77)
    X = rng.standard_normal((n, d)).astype(f32)
    col = rng.integers(0, n_tenants, n).astype(np.uint32)
    want = np.concatenate([np.arange(n_tenants), np.full(9, 41)]).astype(np.uint32)   # each on its own tenant, 9 on one
    Q = rng.standard_normal((len(want), d)).astype(f32)
    assert len(np.unique(want)) == n_tenants > 64
    groups = (np.arange(n) % 11).astype(np.uint32)
    groups[::17] = NONE
    s = _space("groupedl-300", X, "l2")
    full = gm.oracle_all(X, Q, "l2")
    for m in (1, 3):
        c0 = _counters(s)
        got = s.knn_grouped_labeled(Q, k, groups, col, want, per_group=m)
        assert (_counters(s) - c0).tolist() == [0, len(want), 0, 0, 1]
        _assert_rows(got, glc.expected(full, groups, col, want, k, m), k, "300 tenants m=%d" % m)
        assert (got[2] > 0).all()
    assert _same_bytes(got, _device_form(s, Q, k, groups, col, want, 3))
    # the same wants as a table of bitmaps: more than the 64 one call takes — the gap this search closes
    allows, mask_of = glc.as_table(col, want)
    with pytest.raises(ehx.EhxError) as e:
        s.knn_grouped_masked(Q, k, groups, allows, mask_of, per_group=3)
    assert e.value.code == _lib.EUNSUPPORTED
    s.drop()


# ---- 3. slab edges of a RANGE ----

@pytest.mark.parametrize("n_long", [8193, 4097, 4096])
def test_slab_edges_of_a_range(n_long):
    """tenant 1 holds n_long rows, tenant 2 4095: ranges that end in different slabs of one batch.  Group 7 has members at
    ranks 5, 6, 4090, 4096 and last of tenant 1's ascending ids (a tenant that does not scan is listed in any order, so the
    slab a member lands in is not fixed: what is fixed is the answer)"""
    n, d, nq, n_short = 13000, 16, 5, 4095
    rng = np.random.default_rng(n_long)
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    Q[1] = Q[0]                                                       # the same point under the other tenant
    pick = rng.permutation(n)
    long_ids, short_ids = np.sort(pick[:n_long]), np.sort(pick[n_long:n_long + n_short])
    col = np.full(n, 3, dtype=np.uint32)
    col[long_ids] = 1
    col[short_ids] = 2
    assert [int((col == w).sum()) for w in (1, 2)] == [n_long, n_short]
    near = [int(long_ids[p]) for p in (n_long - 1, 5, 6, 4090, min(4096, n_long - 2))]
    near2 = [int(short_ids[p]) for p in (n_short - 1, 0, 4000)]       # ... and three of the group under tenant 2
    for j, r in enumerate(near + near2):
        X[r] = Q[0]
        X[r, 0] += f32(0.01 * (j + 1))
    want = np.array([1, 2, 1, 2, 1], dtype=np.uint32)
    groups = (100 + np.arange(n) % 37).astype(np.uint32)
    groups[::11] = NONE
    groups[near + near2] = 7
    s = _space("groupedl-slab", X, "l2")
    full = gm.oracle_all(X, Q, "l2")
    assert [int(v) for v in full[0][0, :8]] == near + near2
    for k in (4, 10, 256):
        for m in (1, 2, 3):
            c0 = _counters(s)
            got = s.knn_grouped_labeled(Q, k, groups, col, want, per_group=m)
            assert (_counters(s) - c0).tolist() == [0, nq, 0, 0, 1]
            _assert_rows(got, glc.expected(full, groups, col, want, k, m), k, "long=%d k=%d m=%d" % (n_long, k, m))
            # the first m of group 7 OF THE TENANT, wherever its members lie in the range
            assert [int(v) for v in got[0][0, :m]] == near[:m] and near[m] not in got[0][0]
            assert [int(v) for v in got[0][1, :m]] == near2[:m] and not set(near) & set(int(v) for v in got[0][1])
    assert _same_bytes(got, _device_form(s, Q, 256, groups, col, want, 3))
    s.drop()


# ---- 4. filter before cap ----

def test_filter_before_cap():
    n, d, k = 700, 24, 37   # k = the number of groups: every group is represented, whatever belongs to another tenant
    rng = np.random.default_rng(33)
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((3, d)).astype(f32)
    groups = (np.arange(n) % 37).astype(np.uint32)
    s = _space("groupedl-filter", X, "l2")
    full = gm.oracle_all(X, Q, "l2")
    plain = s.knn_grouped(Q, k, groups, per_group=1)
    hit = [int(r) for r in plain[0][0, [0, 2, 5]]]                    # the rows that represent three groups for query 0 ...
    col = np.full(n, 1, dtype=np.uint32)
    col[hit] = 2                                                      # ... belong to another tenant
    want = np.array([1, 1, 1], dtype=np.uint32)
    got = s.knn_grouped_labeled(Q, k, groups, col, want, per_group=1)
    _assert_rows(got, glc.expected(full, groups, col, want, k, 1), k, "filter before cap")
    order = [int(v) for v in full[0][0]]
    for r in hit:                                                     # each group by its nearest row OF THE TENANT
        second = next(x for x in order if groups[x] == groups[r] and col[x] == 1)
        assert second in got[0][0] and r not in got[0][0]
    assert (got[2] == k).all()
    # grouped search first, the other tenant's rows dropped on the host: the three groups are lost
    host = [int(v) for v in plain[0][0] if col[int(v)] == 1]
    assert len(host) == k - 3 and host != [int(v) for v in got[0][0]]
    # ... and under the other tenant the three rows are all there is
    other = s.knn_grouped_labeled(Q[:1], k, groups, col, [2], per_group=1)
    assert other[2][0] == 3 and sorted(int(v) for v in other[0][0, :3]) == sorted(hit)
    s.drop()


# ---- 5. the scan route ----

@pytest.mark.parametrize("lab", sorted(gm.LABELINGS))
@pytest.mark.parametrize("metric", glc.METRICS)
def test_scan_route(metric, lab):
    X, Q = lc.gauss(20000, 64, 64, 1)
    full = gm.scan_oracle(metric)
    groups = gm.LABELINGS[lab](len(X))
    col, want = glc.tenant_column(), glc.scan_want()
    s = _i8_space("groupedl-scan", X, metric)
    cases = [c for c in glc.scan_cases() if c[0] == metric and c[1] == lab]
    assert len(cases) == 6
    for _, _, k, m in cases:
        c0, st0 = _counters(s), s.stats()
        got = s.knn_grouped_labeled(Q, k, groups, col, want, per_group=m)
        dc, st1 = _counters(s) - c0, s.stats()
        what = "%s %s k=%d m=%d" % (metric, lab, k, m)
        print(what, dc.tolist())
        _assert_rows(got, glc.expected(full, groups, col, want, k, m), k, what)
        assert glc.cleared(metric, lab, k, m)   # (the model leaves no case out)
        assert dc.tolist() == [64, 0, 0, PASSES, 1], (what, dc)
        assert st1["n_queries"] - st0["n_queries"] == 64, what
        assert st1["n_i8_queries"] - st0["n_i8_queries"] == 64 and st1["n_i8_fallback"] == st0["n_i8_fallback"], what
        assert st1["n_dist"] > st0["n_dist"]
    assert _same_bytes(got, _device_form(s, Q, k, groups, col, want, m))
    s.drop()


# ---- 6. a mixed batch ----

def test_mixed_batch_and_the_gate_of_64_scanning_queries():
    X, Q64 = lc.gauss(20000, 64, 64, 1)
    groups = gm.labels_scattered(len(X))
    col = glc.tenant_column()
    index = np.concatenate([np.arange(64), np.arange(36)])            # 36 further queries, at points of the first
    wants = np.concatenate([glc.scan_want(), glc.small_want(36)])
    shuffle = np.random.default_rng(6).permutation(100)
    index, wants = index[shuffle], wants[shuffle]
    Q = np.ascontiguousarray(Q64[index])
    full = _rows_of(gm.scan_oracle("cosine"), index)
    s = _i8_space("groupedl-mixed", X, "cosine")
    k, m = 10, 1
    exp = glc.expected(full, groups, col, wants, k, m)
    c0, st0 = _counters(s), s.stats()
    got = s.knn_grouped_labeled(Q, k, groups, col, wants, per_group=m)
    dc, st1 = _counters(s) - c0, s.stats()
    _assert_rows(got, exp, k, "mixed batch")
    assert dc.tolist() == [64, 36, 0, PASSES, 1], dc
    assert st1["n_queries"] - st0["n_queries"] == 100 and st1["n_i8_queries"] - st0["n_i8_queries"] == 64
    assert _same_bytes(got, _device_form(s, Q, k, groups, col, wants, m))
    # one scanning query fewer: 63 do not fill a query tile of the scan, the list route answers all 99
    keep = np.delete(np.arange(100), int(np.nonzero(wants < glc.SMALL0)[0][0]))
    c0 = _counters(s)
    fewer = s.knn_grouped_labeled(np.ascontiguousarray(Q[keep]), k, groups, col, wants[keep], per_group=m)
    assert (_counters(s) - c0).tolist() == [0, 99, 0, 0, 1]
    _assert_rows(fewer, [exp[i] for i in keep], k, "one scanning query fewer")
    assert _same_bytes(fewer, [a[keep] for a in got])                 # the same answer on either route
    # the answer does not depend on the order of the queries
    perm = np.random.default_rng(12).permutation(100)
    moved = s.knn_grouped_labeled(np.ascontiguousarray(Q[perm]), k, groups, col, wants[perm], per_group=m)
    back = [np.empty_like(a) for a in moved]
    for a, b in zip(moved, back):
        b[perm] = a
    assert _same_bytes(got, back)
    s.drop()


# ---- 7. handed on ----

def test_a_sample_without_k_groups_hands_every_query_on_under_its_own_tenant():
    X, Q = lc.gauss(20000, 64, 64, 1)
    full = gm.scan_oracle("l2")
    groups = (np.arange(len(X)) % 5).astype(np.uint32)
    col, want = glc.tenant_column(), glc.scan_want()
    s = _i8_space("groupedl-handed", X, "l2")
    c0, st0 = _counters(s), s.stats()
    got = s.knn_grouped_labeled(Q, 10, groups, col, want, per_group=1)
    dc, st1 = _counters(s) - c0, s.stats()
    # five groups exist: no sample reaches k = 10 capped rows, the radius stays +Inf, the bound serves no query
    assert dc.tolist() == [0, 64, 0, PASSES, 1], dc
    assert (got[2] == 5).all()
    _assert_rows(got, glc.expected(full, groups, col, want, 10, 1), 10, "handed on")
    assert (col[got[0][:, :5].astype(np.int64)] == want[:, None]).all()   # every query under ITS tenant
    assert st1["n_queries"] - st0["n_queries"] == 64 and st1["n_i8_fallback"] - st0["n_i8_fallback"] == 64
    s.drop()


# ---- 8. equivalences, byte for byte ----

def test_equivalences():
    X, Q = lc.gauss(20000, 64, 64, 1)
    n = len(X)
    full = gm.scan_oracle("cosine")
    groups = gm.labels_scattered(n)
    none = np.full(n, NONE, dtype=np.uint32)
    col, want = glc.tenant_column(), glc.scan_want()
    s = _i8_space("groupedl-eq", X, "cosine")
    # every group NONE, or per_group at least the largest group (clustered: ten rows): the kNN under the label column
    for k in (10, 48):
        labeled = s.knn_labeled(Q, k, col, want)
        for gr, m in ((none, 1), (groups, 2 ** 32 - 1), (gm.labels_clustered(n), 10)):
            c0 = _counters(s)
            got = s.knn_grouped_labeled(Q, k, gr, col, want, per_group=m)
            assert (_counters(s) - c0)[:2].sum() == 64
            assert _same_bytes(got, labeled), (k, m)
        few = s.knn_grouped_labeled(Q[:5], k, none, col, want[:5])   # (the list route)
        assert _same_bytes(few, s.knn_labeled(Q[:5], k, col, want[:5])), k
    # one tenant that every row carries and every query wants: the grouped kNN
    one, w1 = np.full(n, 77, dtype=np.uint32), np.full(64, 77, dtype=np.uint32)
    for k, m in ((10, 1), (100, 4)):
        c0 = _counters(s)
        got = s.knn_grouped_labeled(Q, k, groups, one, w1, per_group=m)
        assert (_counters(s) - c0)[:2].sum() == 64
        assert _same_bytes(got, s.knn_grouped(Q, k, groups, per_group=m)), (k, m)
        assert _same_bytes(s.knn_grouped_labeled(Q[:5], k, groups, one, w1[:5], per_group=m),
                           s.knn_grouped(Q[:5], k, groups, per_group=m))
    # the table of bitmaps that says what the three wanted tenants say: the grouped kNN under bitmaps
    allows, mask_of = glc.as_table(col, want)
    assert len(allows) == 3
    for k, m in ((10, 1), (100, 4), (256, 1)):
        got = s.knn_grouped_labeled(Q, k, groups, col, want, per_group=m)
        assert _same_bytes(got, s.knn_grouped_masked(Q, k, groups, allows, mask_of, per_group=m)), (k, m)
    # 0xFFFFFFFF is an ordinary tenant and EHX_GROUP_NONE as a group, in the same call
    col2 = col.copy()
    col2[col == 3] = ALL_ONES
    want2 = np.where(want == 3, ALL_ONES, want).astype(np.uint32)
    gr2 = groups.copy()
    gr2[::7] = NONE
    gr2[col2 == ALL_ONES] = np.where(np.arange((col2 == ALL_ONES).sum()) % 2, NONE, 5).astype(np.uint32)
    for q, w in ((Q, want2), (Q[:6], want2[:6])):
        got = s.knn_grouped_labeled(q, 10, gr2, col2, w, per_group=1)
        exp = glc.expected(_rows_of(full, np.arange(len(q))), gr2, col2, w, 10, 1)
        _assert_rows(got, exp, 10, "all ones, nq=%d" % len(q))
        mine = got[0][w == ALL_ONES]
        assert (col2[mine.astype(np.int64)] == ALL_ONES).all()
        assert ((gr2[mine.astype(np.int64)] == 5).sum(axis=1) == 1).all()   # group 5 once, the NONE rows each on its own
        assert _same_bytes(got, _device_form(s, q, 10, gr2, col2, w, 1))
    s.drop()


# ---- 9. the prefix ----

def test_n_labels_below_the_row_count():
    X, Q = lc.gauss(20000, 64, 64, 1)
    full = gm.scan_oracle("cosine")
    groups = gm.labels_scattered(len(X))
    col, want = glc.tenant_column(), glc.scan_want()
    s = _i8_space("groupedl-prefix", X, "cosine")
    nl = 15000
    for k, m in ((10, 1), (100, 4)):
        got = s.knn_grouped_labeled(Q, k, groups, col, want, per_group=m, n_labels=nl)
        _assert_rows(got, glc.expected(full, groups, col, want, k, m, n_eff=nl), k, "n_labels=%d k=%d" % (nl, k))
        assert (got[0][got[0] != NO_ID] < nl).all() and (got[2] == k).all()
        assert _same_bytes(got, s.knn_grouped_labeled(Q, k, groups[:nl], col[:nl], want, per_group=m))   # shorter columns
        assert _same_bytes(got, _device_form(s, Q, k, groups, col, want, m, n_labels=nl))
    s.drop()
    # not a multiple of a tile, on the list route
    n, nl = 300, 257
    rng = np.random.default_rng(257)
    X = rng.standard_normal((n, 12)).astype(f32)
    Q = rng.standard_normal((7, 12)).astype(f32)
    col = (np.arange(n) % 3).astype(np.uint32)
    groups = (np.arange(n) % 13).astype(np.uint32)
    want = (np.arange(7) % 4).astype(np.uint32)                       # (tenant 3: nobody)
    s = _space("groupedl-257", X, "l2")
    full = gm.oracle_all(X, Q, "l2")
    for k, m in ((10, 1), (100, 2)):
        got = s.knn_grouped_labeled(Q, k, groups, col, want, per_group=m, n_labels=nl)
        _assert_rows(got, glc.expected(full, groups, col, want, k, m, n_eff=nl), k, "n_labels=257 k=%d" % k)
        assert (got[0][got[0] != NO_ID] < nl).all()
        assert _same_bytes(got, _device_form(s, Q, k, groups, col, want, m, n_labels=nl))
    s.drop()


def test_rows_appended_after_the_columns_were_built_never_appear():
    X, Q = lc.gauss(20000, 64, 64, 1)
    n0, n1, k, m = 19300, 20000, 10, 1
    groups, col, want = gm.labels_scattered(n0), glc.tenant_column()[:n0], glc.scan_want()
    s = _i8_space("groupedl-append", X[:n0], "l2", cap=n1)
    full = gm.oracle_all(X[:n0], Q, "l2")
    exp = glc.expected(full, groups, col, want, k, m)
    before = s.knn_grouped_labeled(Q, k, groups, col, want, per_group=m)
    _assert_rows(before, exp, k, "before the append")
    s.set_batch(_keys(n1 - n0, n0), Q[np.arange(n1 - n0) % 64])       # the queries themselves: nearer than any old row
    after = s.knn_grouped_labeled(Q, k, groups, col, want, per_group=m)
    assert _same_bytes(before, after) and (after[0][after[0] != NO_ID] < n0).all()
    assert _same_bytes(after, _device_form(s, Q, k, groups, col, want, m))
    grown = np.concatenate([col, np.full(n1 - n0, 99, dtype=np.uint32)])   # ... longer columns find them
    ids = s.knn_grouped_labeled(Q, 1, np.full(n1, NONE, dtype=np.uint32), grown, np.full(64, 99, dtype=np.uint32))[0]
    assert (ids[:, 0] >= n0).all()
    s.drop()


# ---- 10. two device batches ----

def test_two_device_batches_on_the_list_route():
    n, d, nq, k = 2000, 8, 2113, 10
    rng = np.random.default_rng(2113)
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    col = rng.integers(0, 300, n).astype(np.uint32)
    want = rng.integers(0, 310, nq).astype(np.uint32)                 # (300 .. 309: nobody)
    assert len(np.unique(want)) > 290
    groups = (np.arange(n) % 3).astype(np.uint32)
    groups[::5] = NONE
    s = _space("groupedl-two", X, "l2")
    full = gm.oracle_all(X, Q, "l2")
    c0 = _counters(s)
    got = s.knn_grouped_labeled(Q, k, groups, col, want, per_group=1)
    assert (_counters(s) - c0).tolist() == [0, nq, 0, 0, 1]
    _assert_rows(got, glc.expected(full, groups, col, want, k, 1), k, "two batches, list route")
    assert (got[2][want >= 300] == 0).all()
    assert _same_bytes(got, _device_form(s, Q, k, groups, col, want, 1))
    s.drop()


def test_two_device_batches_on_the_scan_route():
    X, Q64 = lc.gauss(20000, 64, 64, 1)
    groups = gm.labels_scattered(len(X))
    col = glc.tenant_column()
    k, m, tiles = 10, 1, 33
    # expected once, from the 64 x 3 (query, tenant) pairs
    pair_q = np.repeat(np.arange(64), 3)
    pair_w = np.tile(np.array(glc.BIG, dtype=np.uint32), 64)
    pairs = glc.expected(_rows_of(gm.scan_oracle("cosine"), pair_q), groups, col, pair_w, k, m)
    index = np.tile(np.arange(64), tiles)
    turn = (np.arange(64 * tiles) % 64 + np.arange(64 * tiles) // 64) % 3     # the wants rotated from tile to tile
    want = np.array(glc.BIG, dtype=np.uint32)[turn]
    Q = np.ascontiguousarray(Q64[index])
    assert len(Q) == 2112 > 2048
    s = _i8_space("groupedl-two-scan", X, "cosine")
    c0, st0 = _counters(s), s.stats()
    got = s.knn_grouped_labeled(Q, k, groups, col, want, per_group=m)
    dc, st1 = _counters(s) - c0, s.stats()
    _assert_rows(got, [pairs[3 * int(q) + int(w)] for q, w in zip(index, turn)], k, "two batches, scan route")
    assert dc[0] + dc[1] == 2112 and dc[3] == 2 * PASSES and dc[4] == 1, dc   # the scan route in BOTH batches
    assert st1["n_queries"] - st0["n_queries"] == 2112 and st1["n_i8_queries"] - st0["n_i8_queries"] == 2112
    assert _same_bytes(got, _device_form(s, Q, k, groups, col, want, m))
    s.drop()


# ---- 12. errors ----

def test_error_returns():
    rng = np.random.default_rng(8)
    n, d = 200, 8
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((3, d)).astype(f32)
    groups = (np.arange(n) % 5).astype(np.uint32)
    col = (np.arange(n) % 3).astype(np.uint32)
    want = np.array([0, 1, 5], dtype=np.uint32)
    s = _space("groupedl-err", X, "l2")
    for k, m, code in ((0, 1, _lib.EINVAL), (4, 0, _lib.EINVAL), (257, 1, _lib.EUNSUPPORTED)):
        with pytest.raises(ehx.EhxError) as e:
            s.knn_grouped_labeled(Q, k, groups, col, want, per_group=m)
        assert e.value.code == code
        with pytest.raises(ehx.EhxError) as e:
            _device_form(s, Q, k, groups, col, want, m)
        assert e.value.code == code
    ids, dist, cnt = s.knn_grouped_labeled(np.zeros((0, d), dtype=f32), 4, groups, col, np.zeros(0, dtype=np.uint32))
    assert ids.shape == (0, 4) and cnt.shape == (0,)                                        # no queries: EHX_OK
    got = s.knn_grouped_labeled(Q, 256, groups, col, want, per_group=1)                      # k = 256 is served; five groups exist
    assert got[2].tolist() == [5, 5, 0]                                                     # ... count 0 for ITS query only
    for got in (s.knn_grouped_labeled(Q, 4, groups[:0], col[:0], want), _device_form(s, Q, 4, groups[:0], col[:0], want, 1)):
        assert (got[2] == 0).all() and (got[0] == NO_ID).all() and np.isposinf(got[1]).all()   # n_labels == 0
    with pytest.raises(ValueError):
        s.knn_grouped_labeled(Q, 4, groups, col, want[:2])                                  # a wrong number of wanted labels
    with pytest.raises(ValueError):
        s.knn_grouped_labeled(Q, 4, groups, col[:-1], want)                                 # columns of two lengths
    with pytest.raises(ValueError):
        s.knn_grouped_labeled(Q, 4, groups, col, want, n_labels=n + 1)
    import torch
    dq = torch.tensor(Q, device="cuda")
    dg = torch.tensor(groups.view(np.int32), device="cuda")
    dc = torch.tensor(col.view(np.int32), device="cuda")
    o_ids = torch.full((3, 4), -7, dtype=torch.int64, device="cuda")
    o_dist = torch.full((3, 4), -7.0, dtype=torch.float32, device="cuda")
    o_cnt = torch.full((3,), 77, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):                                                         # a d_want shorter than the batch
        s.knn_grouped_labeled_device(dq, 4, dg, dc, n, torch.zeros(2, dtype=torch.int32, device="cuda"), o_ids, o_dist, o_cnt)
    with pytest.raises(ValueError):
        s.knn_grouped_labeled_device(dq, 4, dg, dc[:100], n, torch.zeros(3, dtype=torch.int32, device="cuda"), o_ids, o_dist, o_cnt)
    L = _lib.load()
    q = np.ascontiguousarray(Q)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731

    def fresh():
        return np.full((3, 4), 7, dtype=np.uint64), np.full((3, 4), 7, dtype=f32), np.full(3, 7, dtype=np.uint32)

    def untouched(o):
        return (o[0] == 7).all() and (o[1] == 7).all() and (o[2] == 7).all()

    def call(o, k=4, m=1, gr=groups, lb=col, nl=n, w=want, qq=q):
        return L.ehx_knn_grouped_labeled(s._h, 3, P(qq, C.c_float) if qq is not None else None, k, m,
                                         P(gr, C.c_uint32) if gr is not None else None,
                                         P(lb, C.c_uint32) if lb is not None else None, nl,
                                         P(w, C.c_uint32) if w is not None else None,
                                         P(o[0], C.c_uint64), P(o[1], C.c_float), P(o[2], C.c_uint32))
    # EHX_EINVAL with the outputs unwritten
    for kw in ({"k": 0}, {"m": 0}, {"gr": None}, {"lb": None}, {"w": None}, {"qq": None}):
        o = fresh()
        assert call(o, **kw) == _lib.EINVAL and untouched(o), kw
    o = fresh()
    assert call(o, k=257) == _lib.EUNSUPPORTED and untouched(o)
    assert call(o, k=0, m=0) == _lib.EINVAL and L.ehx_last_error() == b"k is 0"             # the parents' order of checks
    assert call(o, k=257, m=0) == _lib.EINVAL and call(o, k=257, gr=None) == _lib.EUNSUPPORTED
    for hole in range(3):
        o = fresh()
        a = [P(o[0], C.c_uint64), P(o[1], C.c_float), P(o[2], C.c_uint32)]
        a[hole] = None
        assert L.ehx_knn_grouped_labeled(s._h, 3, P(q, C.c_float), 4, 1, P(groups, C.c_uint32), P(col, C.c_uint32), n,
                                         P(want, C.c_uint32), *a) == _lib.EINVAL
        assert untouched(o)
    o = fresh()
    assert call(o) == _lib.OK and o[2].tolist() == [4, 4, 0]
    assert call(o, gr=None, lb=None, nl=0) == _lib.OK and (o[2] == 0).all()                 # NULL columns with n_labels == 0
    # the device form: a NULL d_want is refused before anything is enqueued, the outputs unwritten
    with pytest.raises(ehx.EhxError) as e:
        s.knn_grouped_labeled_device(dq, 4, dg, dc, n, None, o_ids, o_dist, o_cnt)
    torch.cuda.synchronize()
    assert e.value.code == _lib.EINVAL
    assert (o_ids == -7).all() and (o_dist == -7.0).all() and (o_cnt == 77).all()
    assert L.ehx_knn_grouped_labeled(None, 3, P(q, C.c_float), 4, 1, P(groups, C.c_uint32), P(col, C.c_uint32), n,
                                     P(want, C.c_uint32), None, None, None) == _lib.EINVAL
    assert L.ehx_last_error() == b"space is NULL"
    assert L.ehx_knn_grouped_labeled_device(None, None, 3, None, 4, 1, None, None, n, None, None, None, None) == _lib.EINVAL
    assert L.ehx_last_error() == b"space is NULL"
    h = s._h
    s.drop()   # the tombstone answers for the dropped handle
    o = fresh()
    args = [P(q, C.c_float), 4, 1, P(groups, C.c_uint32), P(col, C.c_uint32), n, P(want, C.c_uint32), P(o[0], C.c_uint64),
            P(o[1], C.c_float), P(o[2], C.c_uint32)]
    assert L.ehx_knn_grouped_labeled(h, 3, *args) == _lib.ENOTFOUND
    assert L.ehx_knn_grouped_labeled_device(h, None, 3, *args) == _lib.ENOTFOUND and untouched(o)
    e0 = ehx.Space.unique("groupedl-empty", d, metric=ehx.METRIC_L2SQ)
    got = e0.knn_grouped_labeled(Q, 4, groups, col, want)
    assert (got[2] == 0).all() and (got[0] == NO_ID).all() and np.isposinf(got[1]).all()
    e0.drop()
    sh = ehx.Space.unique("groupedl-sh", d, metric=ehx.METRIC_L2SQ, shards=2)
    sh.set_batch(_keys(n), X)
    with pytest.raises(ehx.EhxError) as e:
        sh.knn_grouped_labeled(Q, 4, groups, col, want)
    assert e.value.code == _lib.EUNSUPPORTED and "sharded" in str(e.value)
    with pytest.raises(ehx.EhxError) as e:
        _device_form(sh, Q, 4, groups, col, want, 1)
    assert e.value.code == _lib.EUNSUPPORTED and "sharded" in str(e.value)
    sh.drop()


def test_rows_too_long_are_refused():
    max_ld = 21728   # grouped_rerank_max_ld()
    rng = np.random.default_rng(31)
    n, nq = 40, 2
    X = rng.standard_normal((n, max_ld + 1)).astype(f32)
    Q = rng.standard_normal((nq, max_ld + 1)).astype(f32)
    s = _space("groupedl-long", X, "l2")
    with pytest.raises(ehx.EhxError) as e:
        s.knn_grouped_labeled(Q, 10, np.arange(n) % 7, np.arange(n) % 2, [0, 1], per_group=2)
    assert e.value.code == _lib.EUNSUPPORTED and "LDS" in str(e.value)
    s.drop()


def test_stats_deltas_on_the_list_route():
    rng = np.random.default_rng(9)
    n, d, nq = 1000, 16, 24
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    col = rng.integers(0, 7, size=n).astype(np.uint32)
    want = np.array([0] * 10 + [1, 2, 3, 4, 5, 6, 99] * 2, dtype=np.uint32)
    s = _space("groupedl-stats", X, "l2")
    st0, c0 = s.stats(), _counters(s)
    s.knn_grouped_labeled(Q, 5, np.arange(n) % 50, col, want, per_group=2)
    st1, dc = s.stats(), _counters(s) - c0   # every query once, against every row that carries its label
    assert dc.tolist() == [0, nq, 0, 0, 1], dc
    assert st1["n_queries"] - st0["n_queries"] == nq
    assert st1["n_dist"] - st0["n_dist"] == sum(int((col == w).sum()) for w in want)
    assert st1["n_i8_queries"] == st0["n_i8_queries"] and st1["n_i8_fallback"] == st0["n_i8_fallback"]
    s.drop()
