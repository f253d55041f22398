"""The strict graph walk (k_graph.hip) on graphs the GPU BUILT, at the sizes the benchmark runs, against the oracle's
searchKnn on the very same graph.

tests/test_graph_parity.py pins the walk on graphs the oracle built (at most 10 k rows).  Every number at 1 M rows or
more comes from a graph the GPU built with bulk rounds, and only there do the batch visited log (on when
nq * ceil(n/32) * 4 >= 192 MiB and n >= 32000 * ef, ehx_graph.cpp knn_graph_locked), its overflow branch (a query that
marks more than 48 * ef + 256 rows clears its whole bitmap slice) and the hand-offs of the shared bitmaps between
memset-mode batches, log-mode batches, one-launch single queries, bulk inserts and updatePoint repair run.  Here the
engine builds the graph from rows it generates itself (fill_synthetic / fill_manifold), the export passes the shared
structural checks (tests/graph_checks.py), the oracle imports it over the same rows (pyoracle.gen_rows /
gen_manifold_rows are bit-identical to the device generators, tests/test_datagen.py), and the two searches must agree:
ids, distance bytes, counts, and the work counters (n_dist = oracle n_dist - nq, n_hops = n_hops0 + n_hops_up).

Exact fp32 distance ties may order two candidates differently in the engine's (distance, id) list and hnswlib's heaps
(test_graph_scale.py::test_exact_distance_ties_engine_order_vs_heap_order): at most max(1, nq // 500) queries of a batch
may differ, each is printed.  A query whose walk left hnswlib's path (its answer, or its whole ef-list, differs) must be
the engine's own (distance, id)-order walk exactly — oracle/wide_walk_model.py at width 1 — and the counters of all
other queries are asserted exactly on a batch of their own (see compare()).  Every
batch also runs twice in a row and must return the same bytes: a visited bit left set by earlier work would make the
second run skip a row even where a tie rule could hide it.

EHX_PARITY_REPORT=<file>: one JSON line per batch (shape, batch size, ef, log / memset mode, queries that differed).
"""
import json
import os
import time

import numpy as np
import pytest

from graph_checks import check_graph
from oracle import pyoracle
from oracle.wide_walk_model import wide_search

pytestmark = pytest.mark.gpu
ehx = pytest.importorskip("embeddinghub_amd")

T = 16          # CPUs one process may use on the GPU machines (os.cpu_count() reports the whole machine)
M = 16
K = 10
LATENT = 16     # bench.py's --structured-dim
EM = {"l2": (ehx.METRIC_L2SQ, pyoracle.METRIC_L2), "ip": (ehx.METRIC_IP, pyoracle.METRIC_IP),
      "cos": (ehx.METRIC_COSINE, pyoracle.METRIC_COSINE)}

# name: rows x dims, metric, generator, normalised rows, build_batch (0 = auto rounds), fp16 rows, (batch, ef) pairs
SHAPES = {
    "l2_gauss_2m": dict(n=2_000_000, d=128, metric="l2", gen="gauss", norm=False, build_batch=0, f16=False,
                        batches=[(1024, 10), (1024, 60), (1024, 200), (512, 60)]),
    "l2_manifold_2m": dict(n=2_000_000, d=128, metric="l2", gen="manifold", norm=False, build_batch=4096, f16=False,
                           batches=[(1024, 10), (1024, 60), (1024, 200)]),
    "cos_manifold_1m": dict(n=1_000_000, d=768, metric="cos", gen="manifold", norm=True, build_batch=4096, f16=False,
                            batches=[(1024, 10), (1024, 60), (1024, 200)]),
    "ip_gauss_300k": dict(n=300_000, d=768, metric="ip", gen="gauss", norm=False, build_batch=0, f16=False,
                          batches=[(1024, 10), (1024, 100)]),
    "cos_f16_400k": dict(n=400_000, d=1536, metric="cos", gen="gauss", norm=False, build_batch=0, f16=True,
                         batches=[(1024, 10), (1024, 100)]),
}


def vis_mode(n, nq, ef):
    """the engine's choice for a batch (ehx_graph.cpp knn_graph_locked): the visited log or a memset of the bitmaps"""
    return "log" if nq * ((n + 31) // 32) * 4 >= (192 << 20) and n >= 32000 * max(ef, K) else "memset"


def _report(rec):
    print(json.dumps(rec))
    out = os.environ.get("EHX_PARITY_REPORT")
    if out:
        with open(out, "a") as f:
            f.write(json.dumps(rec) + "\n")


def _rows(c, seed, row0, n):
    if c["gen"] == "manifold":
        return pyoracle.gen_manifold_rows(seed, row0, n, c["d"], LATENT, normalize=c["norm"], threads=T)
    return pyoracle.gen_rows(seed, row0, n, c["d"], normalize=c["norm"], threads=T)


def _fill(s, c, n):
    if c["gen"] == "manifold":
        s.fill_manifold(ehx.SEED_CORPUS, 0, n, LATENT, c["norm"])
    else:
        s.fill_synthetic(ehx.SEED_CORPUS, 0, n, c["norm"])


def _export_checked(s):
    exp = s.graph_export()
    return exp, check_graph(*exp, M)


def _oracle(X, exp, om):
    l0, lv, upper, ep, ml = exp
    h = pyoracle.Hnsw(X.shape[1], om, X.shape[0], M=M)
    h.import_graph(X, l0, lv, upper, ep, ml, threads=T)
    return h


def _same(a, b):
    """per query: the same count, ids and distance bytes"""
    return (a[2] == b[2]) & (a[0] == b[0]).all(axis=1) & (a[1].view(np.uint32) == b[1].view(np.uint32)).all(axis=1)


def compare(s, h, X, exp, om, Q, ef, tag, run=None, mode=None):
    """one batch of the engine (run twice) against the oracle's searchKnn on the same graph; returns the record.

    The answers (k = 10) may differ for at most max(1, nq // 500) queries.  The whole ef-list (k = ef) is compared too: a
    query whose walk left hnswlib's path shows there even when its first ten agree.  Every such query must be the walk
    of the engine's own order, (distance, id) — the model of oracle/wide_walk_model.py at width 1, on the same graph
    and distances — in its ids, distance bytes and work counters (an exact fp32 tie at the tail of the list admits the
    candidate of the smaller id, where hnswlib's `lowerBound > d` turns it away).  The counters of all other queries
    must be the oracle's."""
    run = run or (lambda q, k: s.knn(q, k))
    nq = Q.shape[0]
    s.set_ef(ef)
    h.set_ef(ef)
    s.stats_reset()
    got = run(Q, K)
    g = s.stats()
    again = run(Q, K)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), (tag, ef, "a second run of the batch differs")
    labels, dists, counts, _, st = h.search_batch(Q, K, threads=T)
    diff = np.nonzero(~_same(got, (labels, dists, counts)))[0]
    for i in diff:
        print("%s ef=%d query %d differs: engine %s %s / oracle %s %s" % (
            tag, ef, i, got[0][i].tolist(), got[1][i].tolist(), labels[i].tolist(), dists[i].tolist()))
    assert len(diff) <= max(1, nq // 500), (tag, ef, "queries that differ from the oracle", diff[:20].tolist())
    E = max(ef, K)
    full = run(Q, E) if E > K else got
    o_full = h.search_batch(Q, E, threads=T)[:3] if E > K else (labels, dists, counts)
    walk = np.union1d(diff, np.nonzero(~_same(full, o_full))[0]).astype(np.int64)
    if len(walk):
        l0, _, upper, ep, ml = exp
        tot = np.zeros(3, dtype=np.int64)
        for i in walk:
            m_ids, m_dist, c = wide_search(l0, upper, ep, ml, _LazyDist(X, Q[i], om), ef, 1, E)
            print("%s ef=%d query %d: walk off hnswlib's path, engine = (distance, id)-order model: %s" % (
                tag, ef, i, full[0][i][:full[2][i]].tolist() == m_ids.tolist()))
            assert full[2][i] == len(m_ids), (tag, ef, i)
            np.testing.assert_array_equal(full[0][i, :full[2][i]], m_ids, err_msg="%s ef %d query %d" % (tag, ef, i))
            assert full[1][i, :full[2][i]].tobytes() == m_dist.tobytes(), (tag, ef, i)
            tot += (c["n_dist"], c["n_hops0"], c["n_hops_up"])
        s.stats_reset()
        run(Q[walk], K)
        assert s.graph_counters()[:3] == tuple(tot.tolist()), (tag, ef, s.graph_counters()[:3], tot)
        keep = np.setdiff1d(np.arange(nq), walk)      # the counters of the other queries, as a batch of their own
        s.stats_reset()
        got2 = run(Q[keep], K)
        g = s.stats()
        labels2, dists2, counts2, _, st = h.search_batch(Q[keep], K, threads=T)
        assert _same(got2, (labels2, dists2, counts2)).all(), (tag, ef)
        nq = len(keep)
    assert g["n_dist"] == st["n_dist"] - nq, (tag, ef, g["n_dist"], st["n_dist"])
    assert g["n_hops"] == st["n_hops0"] + st["n_hops_up"], (tag, ef, g["n_hops"], st)
    rec = {"case": tag, "n": len(s), "nq": int(Q.shape[0]), "ef": ef, "mode": mode or vis_mode(len(s), Q.shape[0], ef),
           "differ": int(len(diff)), "walk_off_path": int(len(walk)), "rows_fetched_per_query": round(st["n_dist"] / nq - 1, 1)}
    _report(rec)
    return rec


class _LazyDist:
    """the oracle's canonical distance of one query to a row, computed when the model first asks for it"""

    def __init__(self, X, q, om):
        self.X, self.q, self.om, self.cache = X, q, om, {}

    def __getitem__(self, i):
        i = int(i)
        v = self.cache.get(i)
        if v is None:
            v = self.cache[i] = np.float32(pyoracle.dist(self.om, self.q, self.X[i]))
        return v


@pytest.fixture(scope="module")
def built(request):
    """a graph space the GPU built over generated rows, the same rows on the host (fp16 spaces: binary16-rounded), and
    its export, structurally checked"""
    name = request.param
    c = SHAPES[name]
    em, _ = EM[c["metric"]]
    t0 = time.perf_counter()
    s = ehx.Space.unique("gpubuilt-" + name, c["d"], metric=em, mode=ehx.MODE_GRAPH, M=M, initial_capacity=c["n"],
                         build_batch=c["build_batch"], dtype=ehx.DTYPE_F16 if c["f16"] else ehx.DTYPE_F32)
    _fill(s, c, c["n"])
    build_s = time.perf_counter() - t0
    X = _rows(c, ehx.SEED_CORPUS, 0, c["n"])
    if c["f16"]:
        X = X.astype(np.float16).astype(np.float32)
    exp, summary = _export_checked(s)
    _report({"case": name, "gpu_build_s": round(build_s, 1), **summary})
    yield name, c, s, X, exp
    s.drop()


@pytest.mark.parametrize("built", list(SHAPES), indirect=True)
def test_strict_walk_on_gpu_built_graph_is_the_oracles_search(built):
    name, c, s, X, exp = built
    _, om = EM[c["metric"]]
    if c["f16"]:      # the space holds the binary16-rounded rows, and the oracle gets exactly those
        for i in np.random.default_rng(1).integers(0, c["n"], 64).tolist() + [0, c["n"] - 1]:
            assert s.get_by_id(i).tobytes() == X[i].tobytes(), i
    h = _oracle(X, exp, om)
    Qall = _rows(c, ehx.SEED_QUERY, 0, max(b for b, _ in c["batches"]))
    for nq, ef in c["batches"]:
        Q = Qall[:nq]
        rec = compare(s, h, X, exp, om, Q, ef, "%s B%d" % (name, nq))
        if name == "l2_gauss_2m" and ef == 10:
            # this batch runs in log mode and reaches the log's overflow branch: some query marks more rows than the
            # log holds (a lower bound from the oracle's own walk: rows evaluated minus the upper levels' at most M each)
            assert rec["mode"] == "log"
            cap = 48 * ef + 256
            over = 0
            h.set_ef(ef)
            for i in range(nq):
                st = h.search_batch(Q[i:i + 1], K, threads=1)[4]
                over += (st["n_dist"] - 1 - st["n_hops_up"] * M) > cap
            _report({"case": rec["case"], "ef": ef, "log_cap": cap, "queries_over_the_log_at_least": int(over)})
            assert over >= 1
    modes = {vis_mode(c["n"], nq, ef) for nq, ef in c["batches"]}
    if name == "l2_gauss_2m":
        assert modes == {"log", "memset"}
    del h


@pytest.mark.parametrize("built", ["l2_manifold_2m", "cos_manifold_1m"], indirect=True)
def test_wide_walk_on_gpu_built_graph_is_the_models_walk(built):
    """k_graphw.hip at scale against oracle/wide_walk_model.py on the exported graph, fed the oracle's distances: a batch
    of 1024 queries (the log / memset rule that batch size selects), 32 of them compared with the model — ids and
    distance bytes — and those 32 again as a batch of their own, whose work counters must be the model's.  ef 64 and
    200 run at the full width; ef 60 (walked two wide, include/ehx.h) is the one batch of the 2 M index in log mode."""
    name, c, s, X, exp = built
    _, om = EM[c["metric"]]
    l0, lv, upper, ep, ml = exp
    Q = _rows(c, ehx.SEED_QUERY, 0, 1024)
    pick = np.arange(0, 1024, 32)
    D = [_LazyDist(X, Q[i], om) for i in pick]
    try:
        for width in (2, 4):
            s.set_search_width(width)
            for ef in (60, 64, 200):
                s.set_ef(ef)
                ids, dist, cnt = s.knn(Q, K)
                eff = min(width, 2) if ef < 64 else width    # (the width the engine walks, as test_graph_wide.py)
                tot = {"n_dist": 0, "n_hops0": 0, "n_hops_up": 0, "steps": 0}
                for j, i in enumerate(pick):
                    m_ids, m_dist, cc = wide_search(l0, upper, ep, ml, D[j], ef, eff, K)
                    assert cnt[i] == len(m_ids), (width, ef, i)
                    np.testing.assert_array_equal(ids[i, :cnt[i]], m_ids, err_msg="width %d ef %d query %d" % (width, ef, i))
                    assert dist[i, :cnt[i]].tobytes() == m_dist.tobytes(), (width, ef, i)
                    for f in tot:
                        tot[f] += cc[f]
                s.stats_reset()
                ids2, dist2, _ = s.knn(Q[pick], K)
                assert ids2.tobytes() == ids[pick].tobytes() and dist2.tobytes() == dist[pick].tobytes(), (width, ef)
                g = s.graph_counters()
                assert (g[0], g[1], g[2], g[4]) == (tot["n_dist"], tot["n_hops0"], tot["n_hops_up"], tot["steps"]), \
                    (width, ef, g, tot)
                _report({"case": name + " wide", "width": eff, "ef": ef, "mode": vis_mode(c["n"], 1024, ef),
                         "rows_fetched_per_query": round(tot["n_dist"] / len(pick), 1)})
    finally:
        s.set_search_width(1)


def test_sequence_of_operations_on_one_space():
    """One 2 M x 128 L2 space through every kind of work that shares the visited bitmaps, each step compared with the
    oracle on the graph as it then is (re-imported after every step that changed it), every batch run twice."""
    c = SHAPES["l2_gauss_2m"]
    n, d = c["n"], c["d"]
    em, om = EM["l2"]
    t0 = time.perf_counter()
    s = ehx.Space.unique("gpubuilt-seq", d, metric=em, mode=ehx.MODE_GRAPH, M=M, initial_capacity=n)
    _fill(s, c, n)
    X = _rows(c, ehx.SEED_CORPUS, 0, n)
    exp, _ = _export_checked(s)
    h = _oracle(X, exp, om)
    Q = _rows(c, ehx.SEED_QUERY, 0, 1500)
    tag = "seq"
    # 1. log-mode batch; 2. memset-mode batch (leaves the bitmaps marked: vis_dirty); 3. log batch of 1500
    assert compare(s, h, X, exp, om, Q[:1024], 60, tag + "1 B1024")["mode"] == "log"
    assert compare(s, h, X, exp, om, Q[:1024], 200, tag + "2 B1024")["mode"] == "memset"
    assert compare(s, h, X, exp, om, Q[:1500], 60, tag + "3 B1500")["mode"] == "log"
    # (a memset batch again, so that the single queries below start from marked bitmaps)
    assert compare(s, h, X, exp, om, Q[:512], 60, tag + "3b B512")["mode"] == "memset"
    # 4. sixteen single-query calls: the one-launch path (EHX_ONE_LAUNCH, on by default)

    def singles(q, k):
        r = [s.knn(q[i:i + 1], k) for i in range(q.shape[0])]
        return tuple(np.concatenate([x[j] for x in r]) for j in range(3))
    compare(s, h, X, exp, om, Q[1024:1040], 60, tag + "4 single", run=singles, mode="one-launch")
    # 5. log batch (ef 10: the log overflows for some queries)
    assert compare(s, h, X, exp, om, Q[:1024], 10, tag + "5 B1024")["mode"] == "log"
    # 6. 20 k fresh rows past the initial capacity: the space grows, bulk rounds run; then a log batch
    del h
    extra = 20_000
    Y = _rows(c, ehx.SEED_CORPUS, n, extra)
    s.set_batch(["%d" % i for i in range(n, n + extra)], Y)
    assert len(s) == n + extra and s.stats()["capacity"] > n
    X = np.concatenate([X, Y])
    del Y
    exp, _ = _export_checked(s)
    h = _oracle(X, exp, om)
    assert compare(s, h, X, exp, om, Q[:1024], 60, tag + "6 B1024")["mode"] == "log"
    # 7. re-Set 200 known keys (hnswlib updatePoint: the repair path), then batches at ef 10 and 60
    del h
    rng = np.random.default_rng(7)
    upd = rng.choice(n + extra, 200, replace=False)
    V = pyoracle.gen_rows(ehx.SEED_QUERY + 7, 0, 200, d, threads=T)
    for i, v in zip(upd.tolist(), V):
        s.set("%d" % i, v)
        X[i] = v
    assert len(s) == n + extra
    for i in upd[:8].tolist():
        assert s.get_by_id(i).tobytes() == X[i].tobytes(), i
    exp, _ = _export_checked(s)
    h = _oracle(X, exp, om)
    for ef in (10, 60):
        assert compare(s, h, X, exp, om, Q[:1024], ef, tag + "7 B1024")["mode"] == "log"
    _report({"case": "seq", "wall_s": round(time.perf_counter() - t0, 1)})
    del h
    s.drop()
