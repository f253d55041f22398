"""GPU tests of what the grouped searches share (grouped_answer / grouped_list, ehx_grouped.cpp; the two pool-fill kernels
of k_grouped.hip): the same rows named in the three ways a call can name them — nothing (ehx_knn_grouped), row bitmaps
(ehx_knn_grouped_masked: one bitmap, or a table), a label column (ehx_knn_grouped_labeled from the call,
ehx_knn_grouped_by_label from stored columns) — give the same BYTES on the list route and on the scan route, each form
counts on its own hook, and a batch whose queries alternate between scanning and listed filters is answered alike whether
the filters come as bitmaps (ordered by route, then by bitmap) or as labels (ordered by route alone).

Expected answers of the mixed batch: tests/grouped_masked_model.py's greedy over the oracle's distances."""
import numpy as np
import pytest

import grouped_masked_model as gmm
import grouped_model as gm
import largek_cases as lc
import test_knn_grouped_masked as t

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")

f32 = np.float32
PASSES = t.PASSES
HOOKS = ("ehx_test_grouped_counters", "ehx_test_grouped_masked_counters", "ehx_test_grouped_masked_counters",
         "ehx_test_grouped_labeled_counters", "ehx_test_grouped_labeled_counters")
FORMS = ("grouped", "one bitmap", "a table of two", "a label column", "stored columns")
GROUP_COL, LABEL_COL, TENANT = 0, 1, 77


def _stored(name, X, metric, groups, col, **kw):
    """a space whose rows were written with their group (column 0) and their tenant (column 1)"""
    s = ehx.Space.unique(name, X.shape[1], metric=t.EM[metric], initial_capacity=len(X), **kw)
    s.set_batch_cols(t._keys(len(X)), X, {GROUP_COL: groups, LABEL_COL: col})
    return s


def _five(s, Q, k, m, groups, n):
    """every row of the prefix n for every query, said five ways -> [(answer, the form's own counters' change)]"""
    nq = len(Q)
    every = np.ones(n, dtype=bool)
    one = np.full(n, TENANT, dtype=np.uint32)
    want = np.full(nq, TENANT, dtype=np.uint32)
    calls = (lambda: s.knn_grouped(Q, k, groups[:n], per_group=m),
             lambda: s.knn_grouped_masked(Q, k, groups, every, per_group=m),
             lambda: s.knn_grouped_masked(Q, k, groups, np.stack([every, every]), (np.arange(nq) % 2).astype(np.uint32), per_group=m),
             lambda: s.knn_grouped_labeled(Q, k, groups[:n], one, want, per_group=m),
             # (stored columns have no length of their own: n = 0 is a tenant no row carries — column 2 was never written)
             lambda: s.knn_grouped_by_label(Q, k, GROUP_COL, LABEL_COL if n else 2, want, per_group=m))
    out = []
    for call, hook in zip(calls, HOOKS):
        c0 = t._hook(s, hook)
        got = call()
        out.append((got, (t._hook(s, hook) - c0).tolist()))
    return out


# ---- 1. the list route: two full slabs and one row, a flat and a graph space ----

@pytest.mark.parametrize("kind", ["flat_f32", "graph_f32"])
def test_list_route_same_bytes_in_every_form(kind):
    n, d, nq, k, m = 2 * gm.POOL_CAP + 1, 7, 5, 10, 2
    rng = np.random.default_rng(8193)
    X = rng.standard_normal((n, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    groups = gm.labels_scattered(n)
    kw = {"mode": ehx.MODE_GRAPH, "M": 16, "build_batch": 4096} if kind == "graph_f32" else {}   # (linked on the device)
    s = _stored("forms-list", X, "l2", groups, np.full(n, TENANT, dtype=np.uint32), **kw)
    answers = _five(s, Q, k, m, groups, n)
    t._assert_rows(answers[0][0], gm.expected(gm.oracle_all(X, Q, "l2"), groups, k, m), k, kind)
    for (got, dc), form in zip(answers, FORMS):
        assert t._same_bytes(got, answers[0][0]), "%s: %s differs from the grouped kNN" % (kind, form)
        assert dc == [0, nq, 0, 0, 1], (kind, form, dc)
    # no row named: count 0, and the page written, in every form
    for (got, dc), form in zip(_five(s, Q, k, m, groups, 0), FORMS):
        ids, dist, cnt = got
        assert (cnt == 0).all() and (ids == t.NO_ID).all() and np.isposinf(dist).all(), (kind, form)
        assert dc == [0, nq, 0, 0, 1], (kind, form, dc)
    s.drop()


# ---- 2. the scan route: the same bytes, the same counters on each form's own hook ----

@pytest.mark.parametrize("m", [1, 4])
@pytest.mark.parametrize("k", [10, 256])
def test_scan_route_same_bytes_and_counters_in_every_form(k, m):
    X, Q = lc.gauss(20000, 64, 64, 1)
    n = len(X)
    groups = gm.labels_clustered(n)
    assert gm.cleared("clustered", k, m)   # (tests/test_grouped_model.py: no query is handed on)
    s = _stored("forms-scan", X, "cosine", groups, np.full(n, TENANT, dtype=np.uint32))
    assert s.scan_engine() == "i8"
    answers = _five(s, Q, k, m, groups, n)
    t._assert_rows(answers[0][0], gm.expected(gm.scan_oracle("cosine"), groups, k, m), k, "k=%d m=%d" % (k, m))
    for (got, dc), form in zip(answers, FORMS):
        print(form, dc)
        assert t._same_bytes(got, answers[0][0]), "k=%d m=%d: %s differs from the grouped kNN" % (k, m, form)
        assert dc == [64, 0, 0, PASSES, 1], (k, m, form, dc)
    s.drop()


# ---- 3. a mixed batch whose queries alternate between four filters: two scan, two are listed ----

def mixed_filters(n=20000, n_small=200):
    """four disjoint row sets: 2 and 3 hold n_small rows each, 0 and 1 share the rest by halves, all scattered over the ids"""
    order = np.random.default_rng(11).permutation(n)
    col = np.empty(n, dtype=np.uint32)
    col[order[:n_small]] = 2
    col[order[n_small:2 * n_small]] = 3
    rest = order[2 * n_small:]
    col[rest[:len(rest) // 2]] = 0
    col[rest[len(rest) // 2:]] = 1
    return col


def test_mixed_batch_interleaved_as_bitmaps_and_as_labels():
    X, Q64 = lc.gauss(20000, 64, 64, 1)
    n, nq, k, m = len(X), 128, 10, 2
    index = np.arange(nq) % 64
    Q = np.ascontiguousarray(Q64[index])
    full = tuple(np.ascontiguousarray(a[index]) for a in gm.scan_oracle("cosine"))
    groups = gm.labels_scattered(n)
    col = mixed_filters(n)
    of = (np.arange(nq) % 4).astype(np.uint32)   # query i under filter i % 4: no two neighbours on one filter
    allows = np.stack([col == f for f in range(4)])
    cut = max(1024, n // 128)
    assert [int(a.sum()) > cut for a in allows] == [True, True, False, False] and allows.sum() == n
    s = _stored("forms-mixed", X, "cosine", groups, col)
    assert s.scan_engine() == "i8"
    exp = gmm.expected(full, groups, allows, of, k, m)
    calls = (("ehx_test_grouped_masked_counters", lambda: s.knn_grouped_masked(Q, k, groups, allows, of, per_group=m)),
             ("ehx_test_grouped_labeled_counters", lambda: s.knn_grouped_labeled(Q, k, groups, col, of, per_group=m)),
             ("ehx_test_grouped_labeled_counters", lambda: s.knn_grouped_by_label(Q, k, GROUP_COL, LABEL_COL, of, per_group=m)))
    answers = []
    for hook, call in calls:
        c0 = t._hook(s, hook)
        got = call()
        dc = (t._hook(s, hook) - c0).tolist()
        print(hook, dc)
        t._assert_rows(got, exp, k, hook)
        assert dc == [64, 64, 0, PASSES, 1], (hook, dc)
        answers.append(got)
    assert t._same_bytes(answers[0], answers[1]) and t._same_bytes(answers[0], answers[2])
    s.drop()
