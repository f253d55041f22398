"""CPU-side checks of the graph walk under a row bitmap (ehx_graph_knn_masked*): the model the kernel is held to
(tests/filtered_walk_model.py) is more than a restatement of the kernel —
  (1) with every row allowed it IS the strict walk: the oracle's search_batch in ids, distance bytes and work counters;
  (2) with cap = infinity and distinct distances its answer is hnswlib >= 0.7's filtered searchBaseLayerST, written here
      independently in the two-heap form (candidate heap, result heap of allowed entries only, lowerBound from the results);
  (3) its own properties: only allowed ids, non-decreasing distances, the list never exceeds cap, an empty bitmap ends —
and the header, the binding and the library name the new entry points, and k_graphm.hip compiles for gfx950 with no
scratch and no spills."""
import ctypes as C
import heapq
import math
import os
import re
import subprocess

import numpy as np
import pytest

from embeddinghub_amd import _lib
from embeddinghub_amd import build as ehx_build
from oracle import pyoracle
from filtered_walk_model import WALK_LIST_FACTOR, WALK_LIST_MAX, allowed_rows, filtered_search, walk_cap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = [pyoracle.METRIC_L2, pyoracle.METRIC_IP, pyoracle.METRIC_COSINE]
HOOK = "ehx_test_graph_masked_counters"
_cache = {}


def _graph(n, d, om, seed):
    """an oracle-built graph over Gaussian rows, its export and the rows (built once per shape and metric)"""
    key = (n, d, om, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        X = rng.standard_normal((n, d)).astype(np.float32)
        h = pyoracle.Hnsw(d, om, n, M=16)
        h.add_rows(X)
        l0, _, upper = h.export_graph()
        _cache[key] = (X, h, l0, upper)
    return _cache[key]


def _all_distances(X, Q, om):
    n = X.shape[0]
    ids, dist, _ = pyoracle.exhaustive(X, Q, n, om)
    D = np.empty((Q.shape[0], n), dtype=np.float32)
    np.put_along_axis(D, ids.astype(np.int64), dist, axis=1)
    return D


# ---- (1) every row allowed: the strict walk ----
@pytest.mark.parametrize("om", METRICS)
@pytest.mark.parametrize("n,d,nq,k,efs", [(3000, 64, 6, 10, (10, 50, 200)), (500, 19, 7, 3, (16,))])
def test_all_allowed_is_the_strict_walk(n, d, nq, k, efs, om):
    X, h, l0, upper = _graph(n, d, om, n + d)
    Q = np.random.default_rng(7).standard_normal((nq, d)).astype(np.float32)
    D = _all_distances(X, Q, om)
    everything = np.ones(n, dtype=bool)
    for ef in efs:
        h.set_ef(ef)
        labels, dists, counts, _, st = h.search_batch(Q, k, threads=1)
        e = max(ef, k)
        for cap in (e, walk_cap(e), math.inf):     # any cap >= ef
            tot = {"n_dist": 0, "n_hops0": 0, "n_hops_up": 0}
            for i in range(nq):
                ids, dist, c = filtered_search(l0, upper, h.enterpoint, h.maxlevel, D[i], everything, ef, cap, k)
                assert counts[i] == len(ids)
                np.testing.assert_array_equal(ids, labels[i, :counts[i]])
                assert dist.tobytes() == dists[i, :counts[i]].tobytes(), (ef, cap, i)
                assert c["max_len"] <= e
                for f in tot:
                    tot[f] += c[f]
            # (hnswlib re-evaluates the level-0 entry point at the top of searchBaseLayerST; the engine, and so the model,
            # reuses the descent's final distance: one row fewer per query, as tests/test_graph_parity.py has it)
            assert tot == {"n_dist": st["n_dist"] - nq, "n_hops0": st["n_hops0"], "n_hops_up": st["n_hops_up"]}, (ef, cap)


# ---- (2) cap = infinity, distinct distances: hnswlib >= 0.7's filtered searchBaseLayerST ----
def _hnswlib_filtered_level0(level0, ep, dist_row, allowed, ef):
    """hnswlib 0.7's searchBaseLayerST with an isIdAllowed filter and no deletions, neighbour by neighbour: a candidate
    min-heap, a result max-heap of ALLOWED entries only, lowerBound from the results; a neighbour is admitted iff
    results.size() < ef || lowerBound > d; the search stops when the closest candidate is above lowerBound with ef
    results.  -> the results, ascending (distance, id)."""
    results, cand = [], []                       # (-d, id) max-heap; (d, id) min-heap
    d0 = float(dist_row[ep])
    if allowed[ep]:
        heapq.heappush(results, (-d0, ep))
        lower = d0
    else:
        lower = float(np.finfo(np.float32).max)
    heapq.heappush(cand, (d0, ep))
    visited = {ep}
    while cand:
        d, c = cand[0]
        if d > lower and len(results) == ef:
            break
        heapq.heappop(cand)
        row = level0[c]
        for nb in row[1:1 + int(row[0])]:
            nb = int(nb)
            if nb in visited:
                continue
            visited.add(nb)
            dn = float(dist_row[nb])
            if len(results) < ef or lower > dn:
                heapq.heappush(cand, (dn, nb))
                if allowed[nb]:
                    heapq.heappush(results, (-dn, nb))
                if len(results) > ef:
                    heapq.heappop(results)
                if results:
                    lower = -results[0][0]
    return sorted((-d, i) for d, i in results)


@pytest.mark.parametrize("om", METRICS)
@pytest.mark.parametrize("case", ["half", "tenth", "entry_disallowed"])
def test_uncapped_model_is_hnswlibs_filtered_search(case, om):
    n, d, nq, k = 2000, 32, 10, 10
    X, h, l0, upper = _graph(n, d, om, 99)
    rng = np.random.default_rng(11)
    # the equivalence is claimed for pairwise distinct distances: the queries are the first nq of a larger draw whose 2000
    # float32 distances are (a collision among them is an ordinary event)
    Q = rng.standard_normal((4 * nq, d)).astype(np.float32)
    D = _all_distances(X, Q, om)
    D = D[[i for i in range(4 * nq) if len(np.unique(D[i])) == n][:nq]]
    assert D.shape[0] == nq
    allowed = rng.random(n) < (0.1 if case == "tenth" else 0.5)
    ep = int(h.enterpoint)
    allowed[ep] = case != "entry_disallowed"
    for ef in (10, 40):
        for i in range(nq):
            assert len(np.unique(D[i])) == n
            # (level 0 only, from the same node: the descent is not what differs)
            ids, dist, _ = filtered_search(l0, {}, ep, 0, D[i], allowed, ef, math.inf, ef)
            want = _hnswlib_filtered_level0(l0, ep, D[i], allowed, ef)
            assert [int(v) for v in ids] == [w[1] for w in want], (case, ef, i)
            assert [float(v) for v in dist] == [w[0] for w in want]


# ---- (3) the model's own properties ----
@pytest.mark.parametrize("om", METRICS)
def test_model_properties(om):
    n, d, nq, k, ef = 2000, 32, 6, 10, 20
    X, h, l0, upper = _graph(n, d, om, 99)
    rng = np.random.default_rng(13)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    D = _all_distances(X, Q, om)
    sparse = rng.random(n) < 0.02
    for allowed, cap in ((rng.random(n) < 0.3, walk_cap(ef)), (sparse, ef), (sparse, walk_cap(ef))):
        for i in range(nq):
            ids, dist, c = filtered_search(l0, upper, h.enterpoint, h.maxlevel, D[i], allowed, ef, cap, k)
            assert all(allowed[int(v)] for v in ids) and len(set(ids.tolist())) == len(ids) <= k
            assert np.all(np.diff(dist) >= 0)
            np.testing.assert_array_equal(dist, D[i][ids.astype(np.int64)])
            assert c["max_len"] <= cap and c["hit_cap"] == (c["max_len"] == cap)
    assert any(filtered_search(l0, upper, h.enterpoint, h.maxlevel, D[i], sparse, ef, ef, k)[2]["hit_cap"] for i in range(nq))
    for i in range(nq):   # nothing allowed: the walk ends (the list is cut at cap) and returns nothing
        ids, dist, c = filtered_search(l0, upper, h.enterpoint, h.maxlevel, D[i], np.zeros(n, dtype=bool), ef, walk_cap(ef), k)
        assert len(ids) == 0 and len(dist) == 0 and c["n_hops0"] >= 1


def test_allowed_rows_is_the_engines_definition():
    words = np.array([0xFFFFFFFF, 0x5], dtype=np.uint32)
    a = allowed_rows(words, 34, 40)
    assert a[:32].all() and a[32] and not a[33] and not a[34:].any()      # bit 34 is set but n_bits = 34 cuts it
    assert allowed_rows(words, 64, 33).sum() == 33                        # ... and so does the row count
    np.testing.assert_array_equal(allowed_rows(np.array([True, False, True]), 3, 2), [True, False])


def test_walk_cap_and_constants_follow_the_header():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    assert int(re.search(r"#define EHX_WALK_LIST_FACTOR (\d+)u", header).group(1)) == _lib.WALK_LIST_FACTOR == WALK_LIST_FACTOR
    assert int(re.search(r"#define EHX_WALK_LIST_MAX (\d+)u", header).group(1)) == _lib.WALK_LIST_MAX == WALK_LIST_MAX
    for name, val in (("EHX_WALK_AUTO", _lib.WALK_AUTO), ("EHX_WALK_GRAPH", _lib.WALK_GRAPH), ("EHX_WALK_EXACT", _lib.WALK_EXACT)):
        assert int(re.search(r"\b%s = (\d+)" % name, header).group(1)) == val
    assert [walk_cap(e) for e in (1, 10, 60, 256, 400, 4096, 5000)] == [12, 120, 720, 3072, 4096, 4096, 5000]
    # the AUTO cut: a walk iff allowed * FACTOR >= rows covered, i.e. down to the share at which cap entries hold ef allowed
    assert walk_cap(10) // 10 == _lib.WALK_LIST_FACTOR


def test_entry_points_are_declared_bound_and_exported():
    import embeddinghub_amd as ehx
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    if not os.path.exists(_lib.LIB_PATH):
        ehx_build.build()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("ehx_graph_knn_masked", "ehx_graph_knn_masked_device"):
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS and hasattr(raw, name)
    assert HOOK not in header and HOOK not in _lib.SYMBOLS and hasattr(raw, HOOK)
    assert "k_graphm.hip" in ehx_build.SOURCES
    assert re.search(r"#define EHX_ABI_VERSION 5\b", header) or _lib.load().ehx_abi_version() == 5
    assert _lib.load().ehx_abi_version() == 5
    assert (ehx.WALK_AUTO, ehx.WALK_GRAPH, ehx.WALK_EXACT) == (0, 1, 2)
    assert hasattr(ehx.Space, "graph_knn_masked") and hasattr(ehx.Space, "graph_knn_masked_device")


def test_masked_walk_kernel_uses_no_scratch_and_spills_nothing(tmp_path):
    src = os.path.join(ehx_build.CSRC, "k_graphm.hip")
    flags = [f for f in ehx_build.FLAGS if f != "-shared"]
    r = subprocess.run([ehx_build.HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o",
                                                    str(tmp_path / "k_graphm.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert sum("graph_search_masked_kernel" in n for n in names) == 2, names
    for what in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"):
        vals = re.findall(what + r": (\d+)", r.stderr)
        assert len(vals) == len(names) and all(v == "0" for v in vals), (what, vals)
