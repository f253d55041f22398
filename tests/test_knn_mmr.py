"""GPU tests of the MMR search (ehx_mmr_select_device, ehx_knn_mmr*; k_mmr.hip) against the plain greedy of include/ehx.h's
contract, written here: candidates from pyoracle.exhaustive, pair distances from pyoracle.dist (it prepares the pivot as the
oracle prepares any query), the cost in np.float32, one operation per rounding.  No tolerance: ids and distance BYTES equal."""
import functools

import numpy as np
import pytest

from oracle import pyoracle
from test_knn_grouped import NO_ID, _assert_rows   # ids, distance bytes, counts, tail sentinels

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")

EM = {"l2": ehx.METRIC_L2SQ, "ip": ehx.METRIC_IP, "cosine": ehx.METRIC_COSINE}
OM = {"l2": pyoracle.METRIC_L2, "ip": pyoracle.METRIC_IP, "cosine": pyoracle.METRIC_COSINE}
KINDS, METRICS = ["flat_f32", "flat_f16", "graph_f32"], ["l2", "ip", "cosine"]
f32 = np.float32


@functools.lru_cache(maxsize=None)
def _rows(d, kind, n_centres=40):
    """n_centres x 8 jittered copies plus loose rows (700 in all; 7 for n_centres = 0), 3 queries near centres; as stored"""
    rng = np.random.default_rng(d)
    centres = rng.standard_normal((max(n_centres, 1), d))
    X = np.concatenate([np.repeat(centres[:n_centres], 8, axis=0) + 0.05 * rng.standard_normal((8 * n_centres, d)),
                        rng.standard_normal((700 - 8 * n_centres if n_centres else 4, d))])
    if not n_centres:   # 7 rows: three near-duplicates and four loose ones
        X = np.concatenate([centres + 0.05 * rng.standard_normal((3, d)), X])
    X = X[rng.permutation(len(X))].astype(f32)
    Q = (centres[[0, 0, 0] if not n_centres else [0, 5, 9]] + 0.02 * rng.standard_normal((3, d))).astype(f32)
    return (X.astype(np.float16).astype(f32) if kind == "flat_f16" else X), Q


def _space(X, metric, kind):
    kw = {"mode": ehx.MODE_GRAPH, "M": 16} if kind == "graph_f32" else {}
    s = ehx.Space.unique("mmr", X.shape[1], metric=EM[metric], initial_capacity=len(X),
                         dtype=ehx.DTYPE_F16 if kind == "flat_f16" else ehx.DTYPE_F32, **kw)
    s.set_batch(["k%d" % i for i in range(len(X))], X)
    return s


def _greedy(ids, dq, k, lam, pair, n_rows, ft=f32):
    """the contract: -> the picked ranks.  pair(a, b): distance of row a to row b as the query; ft: the cost's number type"""
    lam, mu = ft(lam), ft(1) - ft(lam)
    left = [j for j in range(len(ids)) if ids[j] < n_rows]
    near, picks = {j: ft(np.inf) for j in left}, []
    while left and len(picks) < k:
        best = None
        for j in left if picks else left[:1]:
            if picks:
                d = ft(pair(int(ids[j]), int(ids[picks[-1]])))
                near[j] = d if d < near[j] else near[j]
            with np.errstate(invalid="ignore"):
                cost = (ft(0) if lam == 0 else lam * ft(dq[j])) - (ft(0) if mu == 0 else mu * near[j])
            key = (1, 0, j) if np.isnan(cost) else (0, cost, j)
            best = key if best is None or key < best else best
        picks.append(best[2])
        left.remove(best[2])
    return picks


def _expected(X, metric, cand, k, lam):
    """-> per query (ids, dq) of the picks, in pick order"""
    pair = functools.lru_cache(maxsize=None)(lambda a, b: pyoracle.dist(OM[metric], X[b], X[a]))
    want = []
    for ids, dq, c in zip(*cand):
        r = _greedy(ids[:c], dq[:c], k, lam, pair, len(X))
        want.append((ids[r], dq[r]))
    return want


def _on_device(call, nq, k):
    """call(o_ids, o_dist, o_cnt) with poisoned outputs -> numpy (ids u64, dist, counts u32)"""
    import torch
    o = (torch.full((nq, k), -7, dtype=torch.int64, device="cuda"), torch.full((nq, k), -7.0, device="cuda"),
         torch.full((nq,), 77, dtype=torch.int32, device="cuda"))
    call(*o)
    torch.cuda.synchronize()
    return o[0].cpu().numpy().view(np.uint64), o[1].cpu().numpy(), o[2].cpu().numpy().view(np.uint32)


def _select(s, cand, k, lam):
    import torch
    d = [torch.tensor(a.view(t), device="cuda") for a, t in zip(cand, (np.int64, f32, np.int32))]
    got = _on_device(lambda *o: s.mmr_select_device(*d, k, lam, *o), len(cand[0]), k)
    assert all(np.array_equal(a.cpu().numpy(), b.view(t)) for a, b, t in zip(d, cand, (np.int64, f32, np.int32))), "candidates rewritten"
    return got


def _check(d, metric, kind, k, fetch_k, lam, n_centres=40):
    import torch
    X, Q = _rows(d, kind, n_centres)
    cand = pyoracle.exhaustive(X, Q, fetch_k, OM[metric])
    want = _expected(X, metric, cand, k, lam)
    if k > 1:   # diversity matters here, or the case proves nothing
        half = _expected(X, metric, cand, k, 0.5)
        assert all(not np.array_equal(h[0], ids[:len(h[0])]) for h, ids in zip(half, cand[0]))
    what = "%s %s d=%d k=%d fetch_k=%d lambda=%g" % (kind, metric, d, k, fetch_k, lam)
    s = _space(X, metric, kind)
    dq = torch.tensor(Q, device="cuda")
    _assert_rows(_select(s, cand, k, lam), want, k, what + " select")
    full = _on_device(lambda *o: s.knn_mmr_device(dq, k, fetch_k, lam, *o), len(Q), k)
    if kind == "graph_f32":   # the candidates are the walk's: the selection over what knn_device returns
        walk = _on_device(lambda *o: s.knn_device(dq, fetch_k, *o), len(Q), fetch_k)
        want = list(zip(*_select(s, walk, k, lam)[:2]))
        want = [(i[:c], x[:c]) for (i, x), c in zip(want, np.minimum(walk[2], k))]
    _assert_rows(full, want, k, what + " knn_mmr_device")
    _assert_rows(s.knn_mmr(Q, k, fetch_k, lam), want, k, what + " knn_mmr")
    s.drop()
    return want


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("metric", METRICS)
def test_every_layout_and_metric(metric, kind):
    _check(19 if (KINDS.index(kind) + METRICS.index(metric)) % 2 else 132, metric, kind, 10, 100, 0.5)


@pytest.mark.parametrize("lam", [0.0, 0.25, 0.5, 1.0])
@pytest.mark.parametrize("k,fetch_k", [(1, 1), (4, 20), (10, 100), (48, 256)])
def test_every_k_and_lambda(k, fetch_k, lam):
    _check(132, "cosine", "flat_f32", k, fetch_k, lam)


def test_a_space_smaller_than_k():
    assert all(len(w[0]) == 7 for w in _check(19, "cosine", "flat_f32", 10, 100, 0.5, n_centres=0))


@pytest.mark.parametrize("lam", [0.25, 0.5, 0.75])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_float64_greedy_picks_the_same_ids_on_exact_data(metric, lam):
    """integer components in [-4, 4]: every product, sum and cost is exact in fp32 and in float64, and ties are frequent"""
    import torch
    rng = np.random.default_rng(64)
    X, Q = (rng.integers(-4, 5, size=(n, 19)).astype(f32) for n in (600, 3))
    X64 = X.astype(np.float64)
    dist = (lambda q, x: ((q - x) ** 2).sum(-1)) if metric == "l2" else (lambda q, x: 1.0 - (q * x).sum(-1))
    s = _space(X, metric, "flat_f32")
    got = _on_device(lambda *o: s.knn_mmr_device(torch.tensor(Q, device="cuda"), 10, 100, lam, *o), 3, 10)
    for i, q in enumerate(Q.astype(np.float64)):
        dq = dist(q, X64)
        ids = np.lexsort((np.arange(len(X)), dq))[:100]
        r = _greedy(ids, dq[ids], 10, lam, lambda a, b: dist(X64[b], X64[a]), len(X), ft=np.float64)
        assert got[2][i] == 10 and np.array_equal(got[0][i], ids[r].astype(np.uint64)), "query %d" % i
        assert not np.array_equal(ids[r], ids[:10])
    s.drop()


def test_lambda_one_is_knn_at_k():
    import torch
    X, Q = _rows(132, "flat_f32")
    s = _space(X, "cosine", "flat_f32")
    dq = torch.tensor(Q, device="cuda")
    a = _on_device(lambda *o: s.knn_mmr_device(dq, 10, 100, 1.0, *o), len(Q), 10)
    b = _on_device(lambda *o: s.knn_device(dq, 10, *o), len(Q), 10)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    s.drop()


def test_the_primitive_on_foreign_lists():
    """over knn_masked_multi_device's output: two bitmaps, one of them empty (count 0), and an id at the row count planted"""
    import torch
    X, Q = _rows(19, "flat_f32")
    s = _space(X, "l2", "flat_f32")
    words = (len(X) + 31) // 32
    masks = np.zeros((2, words), dtype=np.uint32)
    masks[0] = 0x77777777
    dm, dof = torch.tensor(masks.view(np.int32), device="cuda"), torch.tensor([0, 1, 0], dtype=torch.int32, device="cuda")
    cand = _on_device(lambda *o: s.knn_masked_multi_device(torch.tensor(Q, device="cuda"), 100, dm, 2, len(X), dof, *o), 3, 100)
    cand[0][0, 0], cand[0][2, 3] = len(X), len(X) + 5   # rank 0 of query 0 is no row: its first pick is rank 1
    want = _expected(X, "l2", cand, 10, 0.5)
    assert cand[2].tolist() == [100, 0, 100] and len(want[1][0]) == 0 and want[0][0][0] == cand[0][0, 1]
    got = _select(s, cand, 10, 0.5)
    _assert_rows(got, want, 10, "masked lists")
    assert (got[0][got[0] != NO_ID] < len(X)).all()
    s.drop()
