"""GPU tests of the MaxSim search (ehx_maxsim_select_device, ehx_knn_maxsim*; k_maxsim.hip) against include/ehx.h's contract
written in plain numpy fp32 over pyoracle.exhaustive's canonical distances.  No tolerance: labels, score BYTES, counts and
sentinels equal."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import pyoracle
from test_knn_grouped import _assert_rows   # ids, distance bytes, counts, tail sentinels
from test_knn_mmr import EM, OM, KINDS, METRICS, _on_device

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib   # noqa: E402

f32 = np.float32
NONE, COL, N, T = 0xFFFFFFFF, 1, 700, 32
TCOUNT = np.array([1, 5, 8, 9, 32], dtype=np.uint32)   # one block, a partial block, a whole one, two, four
BIG = 2**31 + 12345
# entities of 1, 2, ..., 26 rows, one of 46, one of 300 (more than a workgroup's step) and 3 rows of no entity: 700 rows,
# 28 entities — with the loose rows no more than fetch_k = 32 groups, so the grouped step finds every entity
SIZES = list(range(1, 27)) + [46, 300]
ENTITIES = [7 + 1000003 * j for j in range(27)] + [BIG]


@functools.lru_cache(maxsize=None)
def _data(d, kind):
    """-> rows as stored, their labels (shuffled over the rows), tokens [5, 32, d]"""
    rng = np.random.default_rng(1000 + d)
    X = rng.standard_normal((N, d)).astype(f32)
    labels = np.concatenate([np.full(n, e, dtype=np.uint32) for n, e in zip(SIZES, ENTITIES)] + [np.full(3, NONE, dtype=np.uint32)])
    labels = labels[rng.permutation(N)]
    tokens = rng.standard_normal((len(TCOUNT), T, d)).astype(f32)
    return (X.astype(np.float16).astype(f32) if kind == "flat_f16" else X), labels, tokens


def _dists(X, V, metric):
    """[len(V), len(X)] canonical distances; NaN where the oracle reports no neighbour"""
    ids, dist, cnt = pyoracle.exhaustive(X, V, len(X), OM[metric])
    D = np.full((len(V), len(X)), np.nan, dtype=f32)
    for v in range(len(V)):
        D[v, ids[v, :cnt[v]].astype(np.int64)] = dist[v, :cnt[v]]
    return D


def _reference(D, tcount, labels, cands, k):
    """the contract: D [nq, T, rows]; cands: per query the candidate labels -> per query (labels, scores) of the answer"""
    want = []
    for i, cand in enumerate(cands):
        scored = []
        for e in sorted(set(int(c) for c in cand) - {NONE}):
            rows = np.flatnonzero(labels == e)
            if not len(rows) or tcount[i] == 0:
                continue
            m = np.fmin.reduce(D[i, :tcount[i]][:, rows], axis=1, initial=f32(np.inf))   # (fmin: a NaN never lowers it)
            score = m[0]
            with np.errstate(invalid="ignore"):
                for t in range(1, tcount[i]):
                    score = f32(score + m[t])
            if not np.isnan(score):
                scored.append((score + f32(0), e))
        scored.sort()
        want.append((np.array([e for _, e in scored[:k]], dtype=np.uint64), np.array([s for s, _ in scored[:k]], dtype=f32)))
    return want


def _labeled_space(X, labels, metric, kind):
    kw = {"mode": ehx.MODE_GRAPH, "M": 16} if kind == "graph_f32" else {}
    s = ehx.Space.unique("maxsim", X.shape[1], metric=EM[metric], initial_capacity=2 * len(X),
                         dtype=ehx.DTYPE_F16 if kind == "flat_f16" else ehx.DTYPE_F32, **kw)
    s.set_batch_cols(["k%d" % i for i in range(len(X))], X, {COL: labels})
    return s


def _select(s, tokens, tcount, cands, k):
    import torch
    n_cand = max(len(c) for c in cands)
    block = np.full((len(cands), n_cand), 12345, dtype=np.uint32)   # (entries behind a count are never read as labels)
    for i, c in enumerate(cands):
        block[i, :len(c)] = c
    dev = lambda a: torch.tensor(np.ascontiguousarray(a).view(np.int32), device="cuda")   # noqa: E731
    return _on_device(lambda *o: s.maxsim_select_device(torch.tensor(tokens, device="cuda"), None if tcount is None else dev(tcount),
                                                        COL, dev(block), dev(np.array([len(c) for c in cands], dtype=np.uint32)),
                                                        k, *o), len(cands), k)


def _counters(s):
    out = (C.c_uint64 * 4)()
    assert C.CDLL(_lib.LIB_PATH).ehx_test_maxsim_counters(s._h, out) == 0
    return list(out)   # calls, candidates scored, rows walked, index rebuilds


@pytest.mark.parametrize("d", [7, 129, 650])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("metric", METRICS)
def test_against_the_contract(metric, kind, d):
    X, labels, tokens = _data(d, kind)
    D = _dists(X, tokens.reshape(-1, d), metric).reshape(len(TCOUNT), T, N)
    what = "%s %s d=%d" % (kind, metric, d)
    s = _labeled_space(X, labels, metric, kind)
    # the select form: a duplicate, an absent label, EHX_GROUP_NONE; k below and above the number scored
    mixed = [[ENTITIES[3], BIG, ENTITIES[3], 999, NONE, ENTITIES[20], ENTITIES[0]][:n] for n in (7, 7, 4, 7, 2)]
    for k in (2, 6):
        _assert_rows(_select(s, tokens, TCOUNT, mixed, k), _reference(D, TCOUNT, labels, mixed, k), k, what + " select k=%d" % k)
    # ... and over every entity: the exhaustive MaxSim ranking
    full = _reference(D, TCOUNT, labels, [ENTITIES] * len(TCOUNT), 40)
    assert all(len(w[0]) == len(ENTITIES) for w in full)
    before = _counters(s)
    _assert_rows(_select(s, tokens, TCOUNT, [ENTITIES[::-1]] * len(TCOUNT), 40), full, 40, what + " select, every entity")
    after = _counters(s)
    assert [a - b for a, b in zip(after, before)] == [1, len(ENTITIES) * len(TCOUNT), (N - 3) * len(TCOUNT), 0]
    # knn_maxsim: the composition of the two public calls, byte for byte — and at fetch_k = 32 the exhaustive ranking
    live = np.concatenate([tokens[i, :c] for i, c in enumerate(TCOUNT)])
    for fetch_k, k in ((3, 4), (32, 40)):
        ids, _, cnt = s.knn_grouped(live, fetch_k, labels, per_group=1)
        at = np.concatenate([[0], np.cumsum(TCOUNT.astype(np.int64))])
        cands = [[int(labels[r]) for v in range(at[i], at[i + 1]) for r in ids[v, :cnt[v]].astype(np.int64)] for i in range(len(TCOUNT))]
        cands = [[e for e in c if e != NONE] for c in cands]
        composed = _select(s, tokens, TCOUNT, cands, k)
        got = s.knn_maxsim(tokens, k, COL, fetch_k=fetch_k, token_count=TCOUNT)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, composed)), what + " knn_maxsim fetch_k=%d" % fetch_k
        if fetch_k == 32:
            _assert_rows(got, full, k, what + " knn_maxsim, exhaustive")
    import torch
    dev = _on_device(lambda *o: s.knn_maxsim_device(torch.tensor(tokens, device="cuda"), torch.tensor(TCOUNT.view(np.int32), device="cuda"),
                                                    COL, 40, 32, *o), len(TCOUNT), 40)
    _assert_rows(dev, full, 40, what + " knn_maxsim_device")
    s.drop()


def test_non_finite_values():
    d = 7
    X, labels, tokens = _data(d, "flat_f32")
    # a query vector holding NaN: its term is +Inf for every entity, every score +Inf, the order by label
    tok = tokens[:1, :2].copy()
    tok[0, 1, 3] = np.nan
    s = _labeled_space(X, labels, "l2", "flat_f32")
    got = _select(s, tok, None, [ENTITIES[::-1]], 40)
    want = _reference(_dists(X, tok.reshape(-1, d), "l2").reshape(1, 2, N), [2], labels, [ENTITIES], 40)
    assert np.isposinf(want[0][1]).all() and list(want[0][0]) == sorted(ENTITIES)
    _assert_rows(got, want, 40, "NaN vector")
    s.drop()
    # inner product: a row of +Inf in one entity, a row of -Inf that is another entity's only row (and one more among a third's
    # rows); vectors of either sign hit both: +Inf + -Inf is a NaN score, dropped, and a -Inf score leads
    X = X.copy()
    A, B, C_ = ENTITIES[5], ENTITIES[0], ENTITIES[9]
    X[np.flatnonzero(labels == A)[0]] = np.inf
    X[np.flatnonzero(labels == B)[0]] = -np.inf
    X[np.flatnonzero(labels == C_)[0]] = -np.inf
    tok = np.abs(tokens[:1, :2]).copy()
    tok[0, 1] *= -1
    s = _labeled_space(X, labels, "ip", "flat_f32")
    got = _select(s, tok, None, [ENTITIES], 40)
    want = _reference(_dists(X, tok.reshape(-1, d), "ip").reshape(1, 2, N), [2], labels, [ENTITIES], 40)
    assert B not in want[0][0] and len(want[0][0]) == len(ENTITIES) - 1
    assert sorted(want[0][0][:2]) == sorted([A, C_]) and np.isneginf(want[0][1][:2]).all() and np.isfinite(want[0][1][2])
    _assert_rows(got, want, 40, "inner product, infinite rows")
    s.drop()


def test_the_index_follows_appends_and_column_writes():
    d = 19
    X, labels, tokens = _data(d, "flat_f32")
    s = _labeled_space(X, labels, "cosine", "flat_f32")
    cands = [ENTITIES[:4]] * len(TCOUNT)

    def check(X, labels, rebuilds):
        want = _reference(_dists(X, tokens.reshape(-1, d), "cosine").reshape(len(TCOUNT), T, len(X)), TCOUNT, labels, cands, 4)
        before = _counters(s)[3]
        _assert_rows(_select(s, tokens, TCOUNT, cands, 4), want, 4, "%d rows" % len(X))
        assert _counters(s)[3] - before == rebuilds
        return want

    first = check(X, labels, 1)
    check(X, labels, 0)
    # an append: entity 0 (one row so far) gains rows that are the queries' own vectors
    more = tokens[:, 0].copy()
    s.set_batch_cols(["new%d" % i for i in range(len(more))], more, {COL: np.full(len(more), ENTITIES[0], dtype=np.uint32)})
    X2, labels2 = np.concatenate([X, more]), np.concatenate([labels, np.full(len(more), ENTITIES[0], dtype=np.uint32)])
    second = check(X2, labels2, 1)
    assert any(a[1].tobytes() != b[1].tobytes() for a, b in zip(first, second))
    # a write to the column of committed rows: they move from entity 0 to entity 1
    s.column_set(COL, ["new0", "new1"], np.full(2, ENTITIES[1], dtype=np.uint32))
    labels3 = labels2.copy()
    labels3[len(X):len(X) + 2] = ENTITIES[1]
    third = check(X2, labels3, 1)
    assert any(a[1].tobytes() != b[1].tobytes() for a, b in zip(second, third))
    s.drop()


def test_errors():
    d = 19
    X, labels, tokens = _data(d, "flat_f32")
    s = _labeled_space(X, labels, "l2", "flat_f32")
    cases = [(lambda: s.knn_maxsim(np.zeros((1, 33, d), f32), 1, COL, fetch_k=1), _lib.EUNSUPPORTED),
             (lambda: s.knn_maxsim(np.zeros((1, 25, d), f32), 1, COL, fetch_k=41), _lib.EUNSUPPORTED),   # 1025 candidates
             (lambda: s.knn_maxsim(tokens, 1, COL, fetch_k=257), _lib.EUNSUPPORTED),
             (lambda: s.knn_maxsim(tokens, 1025, COL, fetch_k=4), _lib.EUNSUPPORTED),
             (lambda: s.knn_maxsim(tokens, 1, _lib.MAX_COLUMNS, fetch_k=4), _lib.EINVAL),
             (lambda: s.knn_maxsim(tokens, 0, COL, fetch_k=4), _lib.EINVAL),
             (lambda: s.knn_maxsim(tokens, 1, COL, fetch_k=0), _lib.EINVAL),
             (lambda: _select(s, tokens, None, [[1] * 1025] * len(tokens), 1), _lib.EUNSUPPORTED)]
    for call, code in cases:
        with pytest.raises(ehx.EhxError) as e:
            call()
        assert e.value.code == code
    # a column never written and a query of no vectors: no entity, count 0
    assert (s.knn_maxsim(tokens, 3, 2, fetch_k=4)[2] == 0).all()
    assert s.knn_maxsim(tokens, 3, COL, fetch_k=8, token_count=[0, 1, 1, 1, 1])[2].tolist() == [0, 3, 3, 3, 3]
    s.drop()
    sh = ehx.Space.unique("maxsim-sh", d, metric=ehx.METRIC_L2SQ, shards=2)
    sh.set_batch(["k%d" % i for i in range(N)], X)
    with pytest.raises(ehx.EhxError) as e:
        sh.knn_maxsim(tokens, 3, COL, fetch_k=4)
    assert e.value.code == _lib.EUNSUPPORTED and "sharded" in str(e.value)
    sh.drop()
