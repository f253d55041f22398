"""CPU-side checks of the kNN under a row bitmap (ehx_knn_masked*): the declarations, the ABI that stays as it was, what both
entry points answer without a device, the marshalling of the bitmap, and the resource usage of k_masked.hip built for gfx950."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from embeddinghub_amd import _lib
from embeddinghub_amd import build as ehx_build
from embeddinghub_amd.space import Space, marshal_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ehx_knn_masked", "ehx_knn_masked_device")
HOOK = "ehx_test_masked_counters"


def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS and hasattr(raw, name)
    assert "k_masked.hip" in ehx_build.SOURCES and "ehx_masked.cpp" in ehx_build.SOURCES
    assert re.search(r"#define EHX_ABI_VERSION 5\b", header)   # additive: the version stays
    for name in ("knn_masked", "knn_masked_device"):
        assert callable(getattr(Space, name))


def test_the_counters_hook_is_not_part_of_the_abi():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    assert HOOK not in header and HOOK not in _lib.SYMBOLS
    assert hasattr(C.CDLL(_lib.LIB_PATH), HOOK)


def test_both_entry_points_without_a_device():
    import torch
    lib = _lib.load()
    q = (C.c_float * 4)()
    mask = (C.c_uint32 * 1)(0xF)
    ids, dist, cnt = (C.c_uint64 * 4)(), (C.c_float * 4)(), (C.c_uint32 * 1)()
    calls = (lambda s: lib.ehx_knn_masked(s, 1, q, 4, mask, 4, ids, dist, cnt),
             lambda s: lib.ehx_knn_masked_device(s, None, 1, None, 4, None, 4, None, None, None))
    if torch.cuda.is_available():
        for call in calls:   # a NULL space is refused before anything is touched
            assert call(None) == _lib.EINVAL and lib.ehx_last_error() == b"space is NULL"
    else:
        h = C.c_void_p()
        assert lib.ehx_space_create(b"masked-nodev", 12, 4, 0, 0, None, C.byref(h)) == _lib.ENODEVICE and not h.value
        for call in calls:   # no device: that is the answer, whatever else is wrong with the call
            assert call(None) == _lib.ENODEVICE


def test_mask_marshalling():
    for n in (0, 1, 31, 32, 33, 63, 70, 257):
        rng = np.random.default_rng(n)
        b = rng.random(n) < 0.5
        words, n_bits = marshal_mask(b)
        assert n_bits == n and words.dtype == np.uint32 and words.flags.c_contiguous and words.shape == ((n + 31) // 32,)
        for r in range(n):   # bit r & 31 of word r >> 5
            assert bool((int(words[r >> 5]) >> (r & 31)) & 1) == bool(b[r])
        if n % 32:           # the bits of the last word beyond n_bits are packed as zero
            assert int(words[-1]) >> (n % 32) == 0
    b = np.zeros(70, dtype=bool)
    b[[0, 31, 32, 69]] = True
    assert marshal_mask(b)[0].tolist() == [0x80000001, 0x1, 0x20]
    assert marshal_mask(b, 33)[0].tolist() == [0x80000001, 0x1] and marshal_mask(b, 33)[1] == 33   # a shorter n_bits cuts
    assert marshal_mask(b[::2])[0].tolist() == [0x00010001, 0x0]                                      # a strided view
    assert marshal_mask([True, False, True])[0].tolist() == [5]
    packed = np.array([7, 0xFFFFFFFF, 1], dtype=np.uint32)
    words, n_bits = marshal_mask(packed, 70)
    assert n_bits == 70 and words.tolist() == packed.tolist()            # packed words pass through as they are
    assert marshal_mask(packed, 96)[1] == 96 and marshal_mask(packed[:0], 0)[1] == 0
    assert marshal_mask(np.arange(6, dtype=np.uint32)[::2], 96)[0].flags.c_contiguous
    for bad, nb in ((packed, None), (packed, 97), (packed, -1), (np.zeros((2, 32), dtype=bool), None), (b, 71),
                    (np.zeros(4, dtype=np.int64), 4), (np.zeros(4, dtype=np.float32), None), (np.uint32(5), 3)):
        with pytest.raises(ValueError):
            marshal_mask(bad, nb)


def test_masked_kernels_use_no_scratch_and_spill_no_vector_registers(tmp_path):
    """ONE kernel file serves one bitmap and a table of them: exactly five functions, each once"""
    src = os.path.join(ehx_build.CSRC, "k_masked.hip")
    flags = [f for f in ehx_build.FLAGS if f != "-shared"]
    r = subprocess.run([ehx_build.HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o",
                                                    str(tmp_path / "k_masked.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    for kern in ("masked_count_kernel", "rows_prefix_kernel", "masked_fill_kernel", "masked_sample_kernel",
                 "masked_radius_kernel"):
        assert sum(kern in n for n in names) == 1, names
    assert len(names) == 5
    for what in ("ScratchSize \\[bytes/lane\\]", "VGPRs Spill"):
        vals = re.findall(what + r": (\d+)", r.stderr)
        assert len(vals) == len(names) and all(v == "0" for v in vals), (what, vals)
    # the ONE tile prefix of every compaction (block_prefix<1024>): 16 wave sums and the carry
    lds = dict(zip(names, re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)))
    assert len(lds) == 5 and [v for n, v in lds.items() if "rows_prefix_kernel" in n] == ["68"], lds
