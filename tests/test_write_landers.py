"""The three ways rows land in a space must leave the same space: the generator (fill_synthetic), a Set from host memory
(set_batch) and a Set from device memory (set_batch_device).  The rows are those of the generator's dataset,
pyoracle.gen_rows(SEED_CORPUS, 0, n, d, normalize=True), written in two calls each way; the keys are "0" .. "n-1", which
are also the implicit keys of generated rows.

Asked of the three spaces: get_by_id of every row byte for byte, knn(Q, 10) ids, counts and distance bytes for 16 generated
queries, graph_export() for graph spaces, and — of the host-written space — the oracle's exhaustive answer.  A graph
space's knn is a walk, so its exact answer is asked through knn_masked under an all-ones bitmap (the exact route).

Shapes: 700 rows as 300 + 400 (the second write straddles a 256-row tile) at 20 and 136 dims; the int8 case 16 640 x 32 as
16 500 + 140 (above the int8 engine's 16 384-row floor; the second write straddles a tile of an ordered scan copy)."""
import functools

import numpy as np
import pytest

from oracle import pyoracle

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
torch = pytest.importorskip("torch")

GRAPH = dict(mode=ehx.MODE_GRAPH, M=8, ef_construction=40, build_batch=1)
KINDS = {   # space kind -> (Space keywords, the oracle's metric)
    "flat-f32-cos": (dict(metric=ehx.METRIC_COSINE), pyoracle.METRIC_COSINE),
    "flat-f16-l2": (dict(metric=ehx.METRIC_L2SQ, dtype=ehx.DTYPE_F16), pyoracle.METRIC_L2),
    "graph-f32-l2": (dict(metric=ehx.METRIC_L2SQ, **GRAPH), pyoracle.METRIC_L2),                          # single-copy, permuted
    "graph-f16-cos": (dict(metric=ehx.METRIC_COSINE, dtype=ehx.DTYPE_F16, **GRAPH), pyoracle.METRIC_COSINE),  # own search copy
}
K = 10


@functools.lru_cache(maxsize=None)
def _reference(n, d, half, om):
    """rows, queries and the oracle's answer over the rows as a space of this dtype stores them; computed once, read-only"""
    X = pyoracle.gen_rows(ehx.SEED_CORPUS, 0, n, d, normalize=True)
    Q = pyoracle.gen_rows(ehx.SEED_QUERY, 0, 16, d, normalize=True)
    stored = X.astype(np.float16).astype(np.float32) if half else X
    ans = pyoracle.exhaustive(stored, Q, K, om)
    for a in (X, Q, stored) + tuple(ans):
        a.setflags(write=False)
    return X, Q, stored, ans


def _land_three_ways(n, first, d, kw, om):
    X = _reference(n, d, kw.get("dtype") == ehx.DTYPE_F16, om)[0]
    keys = [str(i) for i in range(n)]
    cuts = [(0, first), (first, n)]
    gen, host, dev = (ehx.Space.unique("landers-" + w, d, **kw) for w in ("gen", "host", "dev"))
    d_X = torch.tensor(X, device="cuda")   # (a copy: the reference stays read-only)
    for a, b in cuts:
        gen.fill_synthetic(ehx.SEED_CORPUS, a, b - a, True)
        host.set_batch(keys[a:b], X[a:b])
        dev.set_batch_device(keys[a:b], d_X[a:b])
    return gen, host, dev


def _rows(s):
    return np.stack([s.get_by_id(i) for i in range(len(s))]).view(np.uint32)


def _same_answer(a, b):
    return np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and a[2].tolist() == b[2].tolist()


def _assert_identical(spaces, n, d, kw, om, graph):
    X, Q, stored, oracle = _reference(n, d, kw.get("dtype") == ehx.DTYPE_F16, om)
    gen, host, dev = spaces
    assert len(gen) == len(host) == len(dev) == n
    rows = _rows(host)
    assert np.array_equal(rows, stored.view(np.uint32)), "the host-written rows are not the input's"
    assert np.array_equal(_rows(gen), rows), "generated rows differ from the host-written ones"
    assert np.array_equal(_rows(dev), rows), "device-written rows differ from the host-written ones"
    ans = host.knn(Q, K)
    assert _same_answer(gen.knn(Q, K), ans), "knn of the generated space differs"
    assert _same_answer(dev.knn(Q, K), ans), "knn of the device-written space differs"
    exact = host.knn_masked(Q, K, np.ones(n, dtype=bool)) if graph else ans
    assert (exact[2] == K).all() and _same_answer(exact, oracle), "the host-written space differs from the exhaustive oracle"
    if graph:
        gh = host.graph_export()
        for other, name in ((gen, "generated"), (dev, "device-written")):
            g = other.graph_export()
            assert np.array_equal(g[0], gh[0]) and np.array_equal(g[1], gh[1]) and g[3:] == gh[3:], name
            assert sorted(g[2]) == sorted(gh[2]) and all(np.array_equal(g[2][k], gh[2][k]) for k in gh[2]), name


@pytest.mark.parametrize("d", [20, 136])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_three_landers_leave_identical_spaces(kind, d):
    kw, om = KINDS[kind]
    n = 700
    spaces = _land_three_ways(n, 300, d, kw, om)
    try:
        _assert_identical(spaces, n, d, kw, om, graph="mode" in kw)
    finally:
        for s in spaces:
            s.drop()


def test_three_landers_leave_identical_int8_scan_copies():
    kw, om = dict(metric=ehx.METRIC_COSINE), pyoracle.METRIC_COSINE
    n, d = 16640, 32
    spaces = _land_three_ways(n, 16500, d, kw, om)
    try:
        for s in spaces:
            assert s.scan_engine() == "i8"
        i8_0 = [s.stats()["n_i8_queries"] for s in spaces]
        _assert_identical(spaces, n, d, kw, om, graph=False)
        for s, before in zip(spaces, i8_0):
            assert s.stats()["n_i8_queries"] > before, "the int8 engine did not run"
    finally:
        for s in spaces:
            s.drop()
