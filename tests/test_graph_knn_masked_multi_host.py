"""CPU-side checks of the graph walk under a table of bitmaps, one per query (ehx_graph_knn_masked_multi*): the
declarations, what both entry points answer to a NULL space without a device, the resource usage of the walk kernels (the
one-bitmap pair and the pair that reads a bitmap per query), the model the GPU test compares against — filtered_search per
query under its own allowed set — and the restatement of the per-mask AUTO rule and of the bitmaps' word offsets
(tests/graph_masked_multi_cases.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import graph_masked_multi_cases as gc
from embeddinghub_amd import _lib
from embeddinghub_amd import build as ehx_build
from embeddinghub_amd.space import Space, marshal_mask_table
from filtered_walk_model import WALK_LIST_FACTOR, allowed_rows, filtered_search, walk_cap
from oracle import pyoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ehx_graph_knn_masked_multi", "ehx_graph_knn_masked_multi_device")


def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    if not os.path.exists(_lib.LIB_PATH):
        ehx_build.build()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS and hasattr(raw, name)
    assert re.search(r"#define EHX_ABI_VERSION 5\b", header)   # additive: the version stays
    assert _lib.load().ehx_abi_version() == 5
    for name in ("graph_knn_masked_multi", "graph_knn_masked_multi_device"):
        assert callable(getattr(Space, name))
    # the route is the argument behind mask_of, in both forms
    assert _lib.SYMBOLS[NEW[0]][1][8] is C.c_uint32 and _lib.SYMBOLS[NEW[1]][1][9] is C.c_uint32


def test_a_null_space_is_refused_with_or_without_a_device():
    lib = _lib.load()
    q = (C.c_float * 4)()
    masks = (C.c_uint32 * 2)(0xF, 0x3)
    of = (C.c_uint32 * 1)(1)
    ids, dist, cnt = (C.c_uint64 * 4)(), (C.c_float * 4)(), (C.c_uint32 * 1)()
    assert lib.ehx_graph_knn_masked_multi(None, 1, q, 4, masks, 2, 4, of, _lib.WALK_GRAPH, ids, dist, cnt) == _lib.EINVAL
    assert lib.ehx_last_error() == b"space is NULL"
    assert lib.ehx_graph_knn_masked_multi_device(None, None, 1, None, 4, None, 2, 4, None, _lib.WALK_AUTO, None, None,
                                                 None) == _lib.EINVAL
    assert lib.ehx_last_error() == b"space is NULL"


def test_walk_kernels_one_bitmap_pair_and_table_pair_without_scratch_or_spills(tmp_path):
    src = os.path.join(ehx_build.CSRC, "k_graphm.hip")
    flags = [f for f in ehx_build.FLAGS if f != "-shared"]
    r = subprocess.run([ehx_build.HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o",
                                                    str(tmp_path / "k_graphm.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert sum("graph_search_masked_kernel" in n for n in names) == 2, names
    assert sum("graph_search_tabled_kernel" in n for n in names) == 2, names
    assert len(names) == 4, names                      # the shared walk is inlined into its four kernels
    for what in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"):
        vals = re.findall(what + r": (\d+)", r.stderr)
        assert len(vals) == len(names) and all(v == "0" for v in vals), (what, vals)


# ---- the model of a batch: filtered_search per query under its own allowed set ----
@pytest.fixture(scope="module")
def small():
    n, d, nq = 1200, 24, 14
    rng = np.random.default_rng(n + d)
    X = rng.standard_normal((n, d)).astype(np.float32)
    h = pyoracle.Hnsw(d, pyoracle.METRIC_L2, n, M=16)
    h.add_rows(X)
    l0, _, upper = h.export_graph()
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    ids, dist, _ = pyoracle.exhaustive(X, Q, n, pyoracle.METRIC_L2)
    D = np.empty((nq, n), dtype=np.float32)
    np.put_along_axis(D, ids.astype(np.int64), dist, axis=1)
    return h, (l0, upper, int(h.enterpoint), int(h.maxlevel)), Q, D


def test_model_of_a_batch_is_the_one_bitmap_model_row_by_row(small):
    h, graph, Q, D = small
    n, nq, k, ef = D.shape[1], D.shape[0], 5, 20
    tab = gc.table(gc.KINDS, n, graph[2])
    for mask_of in (gc.interleaved(nq, len(gc.KINDS)), gc.shuffled(nq, len(gc.KINDS))):
        rows, tot = gc.model_rows("small", graph, D, tab, mask_of, ef, k)
        want_tot = {f: 0 for f in tot}
        for i, (ids, dist) in enumerate(rows):
            a = tab[mask_of[i]]
            w_ids, w_dist, c = filtered_search(graph[0], graph[1], graph[2], graph[3], D[i], a, ef, walk_cap(ef), k)
            np.testing.assert_array_equal(ids, w_ids)
            assert dist.tobytes() == w_dist.tobytes()
            assert a[ids.astype(np.int64)].all() and len(ids) <= min(k, int(a.sum()))
            for f in want_tot:
                want_tot[f] += int(c[f])
        assert tot == want_tot
    # every bitmap all ones: the oracle's own search, whatever mask_of says
    ones = np.ones((3, n), dtype=bool)
    h.set_ef(ef)
    labels, dists, counts, _, _ = h.search_batch(Q, k, threads=1)
    rows, _ = gc.model_rows("small", graph, D, ones, gc.interleaved(nq, 3), ef, k)
    for i, (ids, dist) in enumerate(rows):
        np.testing.assert_array_equal(ids, labels[i, :counts[i]])
        assert dist.tobytes() == dists[i, :counts[i]].tobytes()
    # the bitmap matters per query: the same query under two complementary bitmaps shares no row
    half = gc.bitmap("half", n, 0)
    two = np.stack([half, ~half])
    a, _ = gc.model_rows("small", graph, D, two, np.zeros(nq, dtype=np.uint32), ef, k)
    b, _ = gc.model_rows("small", graph, D, two, np.ones(nq, dtype=np.uint32), ef, k)
    for (ia, _), (ib, _) in zip(a, b):
        assert len(ia) == k and len(ib) == k and not set(ia.tolist()) & set(ib.tolist())


def test_auto_rule_is_per_mask_and_offsets_address_each_querys_bitmap():
    n = 3000
    tab = gc.counted_table(n, n, (250, 249, 1500, 0))
    assert WALK_LIST_FACTOR == _lib.WALK_LIST_FACTOR == 12
    assert gc.auto_walks(tab, n, n).tolist() == [True, False, True, False]       # 12 * 250 >= 3000 > 12 * 249
    # rows at or above n_bits, or above the row count, are neither counted nor covered
    tab = gc.counted_table(n, 2400, (200, 199, 1500, 0))
    assert tab[:, 2400:].all()
    assert gc.auto_walks(tab, 2400, n).tolist() == [True, False, True, False]    # 12 * 200 >= 2400
    assert gc.auto_walks(tab[:, :2400], 5000, 2400).tolist() == [True, False, True, False]
    mask_of = np.array([3, 0, 1, 2, 0, 0, 1], dtype=np.uint32)
    w, x = gc.split(mask_of, gc.auto_walks(tab, 2400, n))
    assert w.tolist() == [1, 3, 4, 5] and x.tolist() == [0, 2, 6]
    # offsets: mask_of[i] * words of the covered rows, into the table staged dense at that stride
    for n_bits, n_rows in ((3000, 3000), (2963, 3000), (3000, 2400), (70, 3000), (0, 3000)):
        c = gc.covered(n_bits, n_rows)
        words = (c + 31) // 32
        off = gc.allow_of(mask_of, n_bits, n_rows)
        assert off.tolist() == [int(m) * words for m in mask_of]
        tab = gc.table(("half", "tenth", "first_half", "ones"), 3000, 0)
        staged = gc.pack(tab)[:, :words].reshape(-1)     # what the engine stages: every bitmap's words below the row count
        rows = np.arange(c)
        for i, m in enumerate(mask_of):
            bits = (staged[off[i] + (rows >> 5)] >> (rows & 31).astype(np.uint32)) & 1 if c else np.zeros(0)
            np.testing.assert_array_equal(bits.astype(bool), tab[m, :c])
            np.testing.assert_array_equal(allowed_rows(gc.pack(tab)[m], n_bits, n_rows)[:c], tab[m, :c])
    # pack is the binding's packing
    np.testing.assert_array_equal(gc.pack(tab), marshal_mask_table(tab)[0])
    # short_bits: below n_bits the table's bits, at and above it everything set
    n_bits = 3000 - 37
    sw = gc.short_bits(tab, n_bits)
    for m in range(tab.shape[0]):
        bits = np.unpackbits(sw[m].view(np.uint8), bitorder="little")[:3008].astype(bool)
        np.testing.assert_array_equal(bits[:n_bits], tab[m, :n_bits])
        assert bits[n_bits:].all()
