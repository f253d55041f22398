"""CPU-side checks of the grouped kNN (ehx_knn_grouped*): the declarations, the ABI that stays as it was, the hook outside
it, what both entry points answer without a device, the marshalling of the labels, and the resource usage of k_grouped.hip
built for gfx950."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from embeddinghub_amd import _lib
from embeddinghub_amd import build as ehx_build
from embeddinghub_amd.space import Space, marshal_groups

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ehx_knn_grouped", "ehx_knn_grouped_device")
HOOK = "ehx_test_grouped_counters"


def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS and hasattr(raw, name)
    assert "k_grouped.hip" in ehx_build.SOURCES and "ehx_grouped.cpp" in ehx_build.SOURCES
    assert re.search(r"#define EHX_ABI_VERSION 5\b", header)   # additive: the version stays
    assert re.search(r"#define EHX_GROUP_NONE 0xFFFFFFFFu\b", header) and _lib.GROUP_NONE == 0xFFFFFFFF
    assert re.search(r"#define EHX_MAX_K_GROUPED 256u\b", header) and _lib.MAX_K_GROUPED == 256
    for name in ("knn_grouped", "knn_grouped_device"):
        assert callable(getattr(Space, name))
    # per_group sits behind k, the labels and their number behind it
    assert _lib.SYMBOLS[NEW[0]][1][3:7] == [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint64]
    assert _lib.SYMBOLS[NEW[1]][1][4:8] == [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64]


def test_the_counters_hook_is_not_part_of_the_abi():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    assert HOOK not in header and HOOK not in _lib.SYMBOLS
    assert hasattr(C.CDLL(_lib.LIB_PATH), HOOK)


def test_a_null_space_is_refused_before_the_device_is_looked_for():
    lib = _lib.load()
    q = (C.c_float * 4)()
    labels = (C.c_uint32 * 4)(0, 1, 2, 3)
    ids, dist, cnt = (C.c_uint64 * 4)(), (C.c_float * 4)(), (C.c_uint32 * 1)()
    assert lib.ehx_knn_grouped(None, 1, q, 4, 1, labels, 4, ids, dist, cnt) == _lib.EINVAL
    assert lib.ehx_last_error() == b"space is NULL"
    assert lib.ehx_knn_grouped_device(None, None, 1, None, 4, 1, None, 4, None, None, None) == _lib.EINVAL
    assert lib.ehx_last_error() == b"space is NULL"


def test_label_marshalling():
    g, n = marshal_groups([3, 0, 7, 7])
    assert n == 4 and g.dtype == np.uint32 and g.flags.c_contiguous and g.tolist() == [3, 0, 7, 7]
    g, n = marshal_groups(np.array([5, -1, 2 ** 32 - 2, -1], dtype=np.int64))
    assert n == 4 and g.tolist() == [5, _lib.GROUP_NONE, 2 ** 32 - 2, _lib.GROUP_NONE]      # -1: a group of its own
    g, n = marshal_groups(np.array([1, -1], dtype=np.int32))
    assert g.tolist() == [1, _lib.GROUP_NONE]
    src = np.array([9, _lib.GROUP_NONE, 4], dtype=np.uint32)
    g, n = marshal_groups(src)
    assert n == 3 and g.tolist() == src.tolist()                                            # uint32 passes through
    assert marshal_groups(np.arange(10, dtype=np.uint32)[::2])[0].flags.c_contiguous        # a strided view
    assert marshal_groups(np.arange(6, dtype=np.uint64))[0].tolist() == list(range(6))
    for empty in ([], np.zeros(0, dtype=np.uint32)):
        g, n = marshal_groups(empty)
        assert n == 0 and g.shape == (0,) and g.dtype == np.uint32
    for rt in (np.arange(100, dtype=np.uint32), np.random.default_rng(1).integers(0, 2 ** 32, size=257, dtype=np.uint64)):
        g, n = marshal_groups(rt)
        assert n == len(rt) and np.array_equal(g.astype(np.uint64), rt.astype(np.uint64))   # round trip
    for bad in (np.array([0, -2]), np.array([2 ** 32], dtype=np.int64), np.array([2 ** 32], dtype=np.uint64),
                np.zeros(4, dtype=np.float32), np.zeros((2, 2), dtype=np.uint32), np.array([True, False])):
        with pytest.raises(ValueError):
            marshal_groups(bad)


def test_grouped_kernels_use_no_scratch_and_spill_no_vector_registers(tmp_path):
    """three layouts x three metrics of the re-rank, and the two kernels that fill a query's pool from its range"""
    src = os.path.join(ehx_build.CSRC, "k_grouped.hip")
    flags = [f for f in ehx_build.FLAGS if f != "-shared"]
    r = subprocess.run([ehx_build.HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o",
                                                    str(tmp_path / "k_grouped.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    for kern, count in (("grouped_rerank_kernel", 9), ("grouped_range_seed_kernel", 1), ("grouped_range_slab_kernel", 1)):
        assert sum(kern in n for n in names) == count, names
    assert len(names) == 11
    for what in ("ScratchSize \\[bytes/lane\\]", "VGPRs Spill"):
        vals = re.findall(what + r": (\d+)", r.stderr)
        assert len(vals) == len(names) and all(v == "0" for v in vals), (what, vals)
