"""The grouped graph walk (ehx_graph_knn_grouped*, k_graphg.hip) on the GPU, compared for equality of ids, distance bytes,
counts and sentinels: with tests/grouped_walk_model.py (the rule in plain Python), with the strict walk where no cap bites,
with the exact grouped search where the list is never trimmed."""
import numpy as np
import pytest

from filtered_walk_model import walk_cap
from grouped_walk_model import GROUP_NONE, grouped_search
from oracle import pyoracle

pytestmark = pytest.mark.gpu
ehx = pytest.importorskip("embeddinghub_amd")

METRICS = {"l2": (ehx.METRIC_L2SQ, pyoracle.METRIC_L2), "ip": (ehx.METRIC_IP, pyoracle.METRIC_IP),
           "cosine": (ehx.METRIC_COSINE, pyoracle.METRIC_COSINE)}
NO_ID = np.uint64(2**64 - 1)
K, NQ, DIMS = 10, 14, 24
_cases = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_spaces():
    yield
    for v in _cases.values():
        v[0].drop()
    _cases.clear()


def _reaches_all(l0, entry):
    seen, todo = {int(entry)}, [int(entry)]
    while todo:
        row = l0[todo.pop()]
        for nb in row[1:1 + int(row[0])]:
            if int(nb) not in seen:
                seen.add(int(nb))
                todo.append(int(nb))
    return len(seen) == l0.shape[0]


def _case(metric, n=1200, kind="import"):
    """-> space, graph, queries, the oracle's distances [nq, n], labels [n] u32, rows.  Rows: n / 4 centres + 0.05 noise, 4
    rows each; the label is the centre's number, shuffled in id space; every 10th row GROUP_NONE.  kind: import (an oracle
    graph), f16 (fp16 rows), built (on the GPU), dense (30 rows a centre, every 40th GROUP_NONE: under per_group = 1 fewer than
    one entry in twelve is eligible and the list runs to its cap).  n <= 300: level 0 reaches every row from the entry point."""
    key = (metric, n, kind)
    if key in _cases:
        return _cases[key]
    em, om = METRICS[metric]
    for seed in range(n, n + 8):
        rng = np.random.default_rng(seed)
        per, none_every = (30, 40) if kind == "dense" else (4, 10)
        centre = np.repeat(np.arange(n // per), per)
        X = (rng.standard_normal((n // per, DIMS))[centre] + 0.05 * rng.standard_normal((n, DIMS))).astype(np.float32)
        perm = rng.permutation(n)
        X[perm] = X.copy()
        labels = np.empty(n, dtype=np.uint32)
        labels[perm] = centre
        labels[::none_every] = GROUP_NONE
        Q = rng.standard_normal((NQ, DIMS)).astype(np.float32)
        stored = X.astype(np.float16).astype(np.float32) if kind == "f16" else X   # the oracle reads the rows as stored
        h = pyoracle.Hnsw(DIMS, om, n, M=16)
        h.add_rows(stored)
        l0, lv, upper = h.export_graph()
        if n > 300 or _reaches_all(l0, h.enterpoint):
            break
    else:
        raise AssertionError("no seed gives a connected level-0 graph")
    s = ehx.Space.unique("gg", DIMS, metric=em, mode=ehx.MODE_GRAPH, M=16, initial_capacity=n,
                         dtype=ehx.DTYPE_F16 if kind == "f16" else ehx.DTYPE_F32,
                         **({} if kind == "built" else {"build_batch": 0xFFFFFFFF}))
    s.set_batch(["k%d" % i for i in range(n)], X)
    if kind == "built":
        l0, lv, upper, entry, maxlevel = s.graph_export()
    else:
        entry, maxlevel = h.enterpoint, h.maxlevel
        s.graph_import(l0, lv, upper, entry, maxlevel)
    s.set_search_width(1)
    order, dist, _ = pyoracle.exhaustive(stored, Q, n, om)
    D = np.empty((NQ, n), dtype=np.float32)
    np.put_along_axis(D, order.astype(np.int64), dist, axis=1)
    _cases[key] = (s, (l0, upper, int(entry), int(maxlevel)), Q, D, labels, X)
    return _cases[key]


def _same(a, b):
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[0], b[0])
    assert np.ascontiguousarray(a[1]).tobytes() == np.ascontiguousarray(b[1]).tobytes()


def _is_the_model(got, graph, D, labels, per_group, ef, k, rows=None):
    """the answer `got` against the model, query by query -> the models' counters"""
    ids, dist, cnt = got
    ctrs = []
    for i in (range(D.shape[0]) if rows is None else rows):
        m_ids, m_dist, c = grouped_search(*graph, D[i], labels, per_group, ef, walk_cap(max(ef, k)), k)
        ctrs.append(c)
        assert cnt[i] == len(m_ids), (i, cnt[i], len(m_ids))
        np.testing.assert_array_equal(ids[i, :cnt[i]], m_ids, err_msg="query %d" % i)
        assert dist[i, :cnt[i]].tobytes() == m_dist.tobytes(), i
        assert (ids[i, cnt[i]:] == NO_ID).all() and np.isposinf(dist[i, cnt[i]:]).all(), i
    return ctrs


@pytest.mark.parametrize("per_group", [1, 2])
@pytest.mark.parametrize("ef", [10, 64])
@pytest.mark.parametrize("metric", list(METRICS))
def test_walk_is_the_rule(metric, ef, per_group):
    s, graph, Q, D, labels, _ = _case(metric)
    s.set_ef(ef)
    got = s.graph_knn_grouped(Q, K, per_group, labels[:1150], route=ehx.WALK_GRAPH)
    ctrs = _is_the_model(got, graph, D, labels[:1150], per_group, ef, K)
    assert (got[0][got[0] != NO_ID] < 1150).all()   # the last 50 rows are walked through, never returned
    if ef == 10 and per_group == 1:   # (from the model alone) the case bites: the cap per group changed an answer
        free = [grouped_search(*graph, D[i], labels[:1150], 1200, ef, walk_cap(ef), K)[0] for i in range(NQ)]
        assert any(not np.array_equal(free[i], got[0][i, :got[2][i]]) for i in range(NQ))


@pytest.mark.parametrize("labels_kind", ["groups_fit", "all_none"])
@pytest.mark.parametrize("ef", [10, 64])
@pytest.mark.parametrize("metric", list(METRICS))
def test_no_cap_no_change(metric, ef, labels_kind):
    s, _, Q, _, labels, _ = _case(metric)
    s.set_ef(ef)
    lab, per_group = (labels, 4) if labels_kind == "groups_fit" else (np.full(1200, GROUP_NONE, dtype=np.uint32), 1)
    _same(s.graph_knn_grouped(Q, K, per_group, lab, route=ehx.WALK_GRAPH), s.knn(Q, K))


@pytest.mark.parametrize("per_group", [1, 3])
@pytest.mark.parametrize("metric", list(METRICS))
def test_never_trimmed_is_exact(metric, per_group):
    s, _, Q, _, labels, _ = _case(metric, n=300)
    s.set_ef(300)
    _same(s.graph_knn_grouped(Q, K, per_group, labels, route=ehx.WALK_GRAPH), s.knn_grouped(Q, K, labels, per_group=per_group))


@pytest.mark.parametrize("kind", ["f16", "built", "dense"])
def test_stored_row_kinds_and_a_list_at_cap(kind):
    s, graph, Q, D, labels, _ = _case("l2", kind=kind)
    s.set_ef(10)
    ctrs = _is_the_model(s.graph_knn_grouped(Q, K, 1, labels[:1150], route=ehx.WALK_GRAPH), graph, D, labels[:1150], 1, 10, K)
    if kind == "dense":   # (from the model alone) lists reached cap
        assert any(c["hit_cap"] for c in ctrs)


def test_routes():
    torch = pytest.importorskip("torch")
    s, graph, Q, D, labels, X = _case("l2")
    s.set_ef(10)
    exact = s.knn_grouped(Q, K, labels[:1150], per_group=2)
    _same(s.graph_knn_grouped(Q, K, 2, labels[:1150], route=ehx.WALK_EXACT), exact)
    walked = s.graph_knn_grouped(Q, K, 2, labels[:1150], route=ehx.WALK_GRAPH)
    _same(s.graph_knn_grouped(Q, K, 2, labels[:1150]), walked)   # WALK_AUTO walks on a graph space
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    out = (torch.zeros((NQ, K), dtype=torch.int64, device="cuda"), torch.zeros((NQ, K), dtype=torch.float32, device="cuda"),
           torch.zeros(NQ, dtype=torch.int32, device="cuda"))
    s.graph_knn_grouped_device(dev(Q), K, 2, dev(labels.view(np.int32)), 1150, *out, route=ehx.WALK_GRAPH)
    torch.cuda.synchronize()
    _same((out[0].cpu().numpy().view(np.uint64), out[1].cpu().numpy(), out[2].cpu().numpy().view(np.uint32)), walked)
    ids, dist, cnt = s.graph_knn_grouped(Q, K, 2, labels[:0], route=ehx.WALK_GRAPH)
    assert (cnt == 0).all() and (ids == NO_ID).all() and np.isposinf(dist).all()
    # k = 256 at ef 256: the suite's longest list
    s.set_ef(256)
    _is_the_model(s.graph_knn_grouped(Q[:4], 256, 1, labels[:1150], route=ehx.WALK_GRAPH), graph, D, labels[:1150], 1, 256, 256,
                  rows=range(4))
    # a flat space has no graph: every route is the exact grouped search
    f = ehx.Space.unique("gg-flat", DIMS, metric=ehx.METRIC_L2SQ, initial_capacity=1200)
    _cases["flat"] = (f,)
    f.set_batch(["k%d" % i for i in range(1200)], X)
    for route in (ehx.WALK_AUTO, ehx.WALK_GRAPH, ehx.WALK_EXACT):
        _same(f.graph_knn_grouped(Q, K, 2, labels[:1150], route=route), exact)
