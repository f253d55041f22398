"""CPU-side checks of the grouped kNN under a label column (ehx_knn_grouped_labeled*): the declarations, the ABI that stays
as it was, the hook outside it, what both entry points answer without a device, what the header promises, the tenant column
of the scan cases, the table of the cases the GPU test asserts "none handed on" for — re-derived from the model case by
case — and the resource usage of the two pool-fill kernels (k_grouped.hip) built for gfx950 beside the function lists of the
two files they stand next to."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import grouped_labeled_cases as glc
import grouped_model as gm
from embeddinghub_amd import _lib
from embeddinghub_amd import build as ehx_build
from embeddinghub_amd.space import Space

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ehx_knn_grouped_labeled", "ehx_knn_grouped_labeled_device")
HOOK = "ehx_test_grouped_labeled_counters"


def _header():
    return open(os.path.join(ROOT, "include", "ehx.h")).read()


def test_entry_points_are_declared_bound_and_exported():
    header = _header()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS and hasattr(raw, name)
    assert "k_grouped.hip" in ehx_build.SOURCES and "ehx_groupedl.cpp" in ehx_build.SOURCES
    assert re.search(r"#define EHX_ABI_VERSION 5\b", header)   # additive: the version stays
    for name in ("knn_grouped_labeled", "knn_grouped_labeled_device"):
        assert callable(getattr(Space, name))
    assert list(inspect.signature(Space.knn_grouped_labeled).parameters)[1:] == [
        "queries", "k", "group_of", "label_of", "want", "per_group", "n_labels"]
    # per_group sits behind k, then the two columns under ONE length, then the wanted labels
    u32p = C.POINTER(C.c_uint32)
    assert _lib.SYMBOLS[NEW[0]][1][3:9] == [C.c_uint32, C.c_uint32, u32p, u32p, C.c_uint64, u32p]
    assert _lib.SYMBOLS[NEW[1]][1][4:10] == [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]


def test_the_counters_hook_is_not_part_of_the_abi():
    assert HOOK not in _header() and HOOK not in _lib.SYMBOLS
    assert hasattr(C.CDLL(_lib.LIB_PATH), HOOK)


def test_a_null_space_is_refused_before_the_device_is_looked_for():
    lib = _lib.load()
    q = (C.c_float * 4)()
    groups, col, want = (C.c_uint32 * 4)(0, 1, 2, 3), (C.c_uint32 * 4)(1, 2, 1, 2), (C.c_uint32 * 1)(1)
    ids, dist, cnt = (C.c_uint64 * 4)(), (C.c_float * 4)(), (C.c_uint32 * 1)()
    for call in (lambda: lib.ehx_knn_grouped_labeled(None, 1, q, 4, 1, groups, col, 4, want, ids, dist, cnt),
                 lambda: lib.ehx_knn_grouped_labeled_device(None, None, 1, None, 4, 1, None, None, 4, None, None, None, None)):
        assert call() == _lib.EINVAL and lib.ehx_last_error() == b"space is NULL"   # with a device or without one


def test_the_header_states_the_contract():
    text = " ".join(_header().split())
    at = text.index("Partitioned grouped kNN")
    doc = text[at:text.index("int ehx_knn_grouped_labeled_device(", at)].replace(" * ", " ")
    assert "FILTER FIRST, THEN CAP" in doc
    assert "byte for byte, what ehx_knn_grouped_masked_device returns for query i alone under the bitmap" in doc
    assert "ONE acquire-load snapshot" in doc and "n_eff = min(snapshot, n_labels)" in doc
    assert "0xFFFFFFFF is an ordinary tenant" in doc and "EHX_GROUP_NONE" in doc
    assert "equals ehx_knn_labeled_device" in doc and "equals ehx_knn_grouped_device" in doc
    assert "count 0 for ITS queries" in doc and "n_labels == 0 gives count 0 for every query" in doc
    assert "n_queries == 0: EHX_OK" in doc and "not limited" in doc
    assert "NaN is never a neighbour and never counts toward a cap" in doc
    for code in ("EHX_EINVAL", "EHX_EUNSUPPORTED", "EHX_ENOTFOUND", "EHX_ENODEVICE"):
        assert code in doc
    host = text[text.index("Grouped kNN under a label column from host pointers"):text.index("int ehx_knn_grouped_labeled(")]
    assert "staged on EVERY call" in host.replace(" * ", " ")


def test_the_tenant_column_of_the_scan_cases():
    col = glc.tenant_column()
    assert col.dtype == np.uint32 and len(col) == 20000
    assert [int((col == t).sum()) for t in glc.BIG] == [6046, 5968, 6010]
    small = np.bincount(col[col >= glc.SMALL0] - glc.SMALL0)
    assert len(small) == 100 and small.min() == 11 and small.max() == 32
    want = glc.scan_want()
    assert len(want) == 64 and want[:4].tolist() == [3, 5, 8, 3]
    tab, of = glc.as_table(col, want)
    assert tab.shape == (3, 20000)
    for i, lab in enumerate(want):
        assert (tab[of[i]] == (col == lab)).all()
    assert len(glc.scan_cases()) == 36
    assert ((glc.small_want() >= glc.SMALL0) & (glc.small_want() < glc.SMALL0 + glc.N_SMALL)).all()


@pytest.mark.parametrize("lab", sorted(gm.LABELINGS))
@pytest.mark.parametrize("metric", glc.METRICS)
def test_the_scan_cases_that_assert_none_handed_on_clear_the_model(metric, lab):
    """the model is the implementation's: the sample by rank over the tenant's ascending list, largek_passes' ranges"""
    full = gm.scan_oracle(metric)
    col, want = glc.tenant_column(), glc.scan_want()
    groups = gm.LABELINGS[lab](len(col))
    cases = [c for c in glc.scan_cases() if c[0] == metric and c[1] == lab]
    assert len(cases) == 6
    worst = 0
    for _, _, k, m in cases:
        answers, fills, unserved = glc.scan_cascade(metric, lab, k, m)
        print("%s %s k=%d m=%d: worst pool fill per pass %s, unserved %d" % (metric, lab, k, m, fills, unserved))
        exp = glc.expected(full, groups, col, want, k, m)
        for q in range(len(want)):   # the algorithm is exact whether the case is cleared or not
            assert answers[q] == [int(v) for v in exp[q][0]], (metric, lab, k, m, q)
        assert len(fills) == glc.PASSES
        assert unserved == 0, (metric, lab, k, m)
        assert max(fills) <= gm.POOL_CAP // 2, (metric, lab, k, m, fills)
        assert glc.cleared(metric, lab, k, m)
        worst = max(worst, max(fills))
    print("%s %s: worst pool fill %d of %d" % (metric, lab, worst, gm.POOL_CAP))


def _functions(name, tmp_path):
    src = os.path.join(ehx_build.CSRC, name)
    flags = [f for f in ehx_build.FLAGS if f != "-shared"]
    r = subprocess.run([ehx_build.HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o",
                                                    str(tmp_path / (name + ".o"))], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return re.findall(r"Function Name: (\S+)", r.stderr), r.stderr


def test_groupedl_kernels_use_no_scratch_and_spill_no_vector_registers(tmp_path):
    """the range seed and the range slab kernel, once each in k_grouped.hip: no scratch, no spill, no LDS"""
    names, log = _functions("k_grouped.hip", tmp_path)
    blocks = log.split("Function Name: ")[1:]   # one block of remarks per kernel
    assert len(blocks) == len(names)
    for kern in ("grouped_range_seed_kernel", "grouped_range_slab_kernel"):
        mine = [b for b in blocks if kern in b.split()[0]]
        assert len(mine) == 1, names
        for what in ("ScratchSize \\[bytes/lane\\]", "VGPRs Spill", "LDS Size \\[bytes/block\\]"):
            assert re.findall(what + r": (\d+)", mine[0]) == ["0"], (kern, what)


def test_the_files_beside_it_hold_the_functions_they_held(tmp_path):
    names, _ = _functions("k_grouped.hip", tmp_path)
    held = (("grouped_rerank_kernel", 9), ("grouped_range_seed_kernel", 1), ("grouped_range_slab_kernel", 1))
    assert len(names) == 11 and all(sum(k in n for n in names) == c for k, c in held)
    names, _ = _functions("k_labeled.hip", tmp_path)
    kernels = ("labeled_count_kernel", "labeled_tiles_kernel", "labeled_fill_kernel", "labeled_sample_kernel")
    assert len(names) == len(kernels) and all(sum(k in n for n in names) == 1 for k in kernels)
