"""CPU-side checks of the filtered search (ehx_knn_among*): the marshalling of candidate lists, the argument checks that
need no device, the declarations, and the resource usage of k_among.hip built for gfx950."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from embeddinghub_amd import _lib
from embeddinghub_amd import build as ehx_build
from embeddinghub_amd.space import Space, marshal_id_lists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ehx_knn_among", "ehx_knn_among_device", "ehx_knn_among_keys")


def test_list_of_lists_becomes_ids_and_offsets():
    ids, off = marshal_id_lists([[3, 1, 2], [], np.array([7], dtype=np.int32), (9, 8)])
    assert ids.dtype == np.uint64 and off.dtype == np.uint64
    assert ids.tolist() == [3, 1, 2, 7, 9, 8] and off.tolist() == [0, 3, 3, 4, 6]
    assert ids.flags.c_contiguous and off.flags.c_contiguous
    ids, off = marshal_id_lists([[], []])
    assert ids.shape == (0,) and ids.dtype == np.uint64 and off.tolist() == [0, 0, 0]
    ids, off = marshal_id_lists([np.zeros(0, dtype=np.int64)])
    assert ids.shape == (0,) and off.tolist() == [0, 0]


def test_flat_ids_are_coerced_and_offsets_passed_through():
    ids, off = marshal_id_lists(np.array([5, 4, 2**40], dtype=np.int64))
    assert off is None and ids.dtype == np.uint64 and ids.tolist() == [5, 4, 2**40]
    ids, off = marshal_id_lists([5, 4, 3])          # a flat Python list: ONE shared list
    assert off is None and ids.tolist() == [5, 4, 3]
    ids, off = marshal_id_lists(np.arange(6, dtype=np.uint32)[::2], [0, 1, 3])
    assert ids.tolist() == [0, 2, 4] and ids.flags.c_contiguous and off.dtype == np.uint64 and off.tolist() == [0, 1, 3]
    ids, off = marshal_id_lists(np.zeros(0, dtype=np.float64))   # (an empty array of any dtype is an empty list)
    assert ids.shape == (0,) and off is None


def test_bad_ids_are_refused():
    with pytest.raises(ValueError):
        marshal_id_lists([1, -2, 3])
    with pytest.raises(ValueError):
        marshal_id_lists([[1.5, 2.0]])
    with pytest.raises(ValueError):
        marshal_id_lists(np.array([1.0, 2.0]))


def test_space_has_the_methods():
    for name in ("knn_among", "knn_among_keys", "knn_among_device"):
        assert callable(getattr(Space, name))


def test_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS
    assert "k_among.hip" in ehx_build.SOURCES and "ehx_among.cpp" in ehx_build.SOURCES
    assert re.search(r"#define EHX_ABI_VERSION 5\b", header)   # additive: the version stays


def test_null_arguments_without_a_device():
    """no space exists without a device (ehx_space_create: EHX_ENODEVICE), so what can be checked here is that every entry
    point refuses a NULL space before it touches anything"""
    lib = _lib.load()
    q = (C.c_float * 4)()
    ids, dist, cnt = (C.c_uint64 * 4)(), (C.c_float * 4)(), (C.c_uint32 * 1)()
    cand = (C.c_uint64 * 2)(0, 1)
    assert lib.ehx_knn_among(None, 1, q, 2, cand, None, 2, ids, dist, cnt) == _lib.EINVAL
    assert lib.ehx_last_error() == b"space is NULL"
    assert lib.ehx_knn_among_device(None, None, 1, None, 2, None, None, 2, 0, None, None, None) == _lib.EINVAL
    assert lib.ehx_knn_among_keys(None, 1, q, 2, 0, None, None, ids, dist, cnt, None) == _lib.EINVAL
    import torch
    if not torch.cuda.is_available():
        h = C.c_void_p()
        assert lib.ehx_space_create(b"among-nodev", 11, 4, 0, 0, None, C.byref(h)) == _lib.ENODEVICE and not h.value


def test_among_kernels_use_no_scratch_and_spill_no_vector_registers(tmp_path):
    src = os.path.join(ehx_build.CSRC, "k_among.hip")
    flags = [f for f in ehx_build.FLAGS if f != "-shared"]
    r = subprocess.run([ehx_build.HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o",
                                                    str(tmp_path / "k_among.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    for kern, count in (("among_tile_kernel", 9), ("among_list_kernel", 9), ("among_emit_kernel", 1)):
        assert sum(kern in n for n in names) == count, names
    for what in ("ScratchSize \\[bytes/lane\\]", "VGPRs Spill"):
        vals = re.findall(what + r": (\d+)", r.stderr)
        assert len(vals) == len(names) and all(v == "0" for v in vals), (what, vals)
    # the shared-list kernel over fp32 and binary16 rows (the flat spaces' instantiations) spills nothing at all
    sg = dict(zip(names, re.findall(r"SGPRs Spill: (\d+)", r.stderr)))
    for n, v in sg.items():
        if "among_tile_kernelILi0" in n or "among_tile_kernelILi1" in n or "among_emit" in n:
            assert v == "0", (n, v)
