"""CPU-side checks of the kNN under a table of bitmaps, one per query (ehx_knn_masked_multi*): the declarations and sources,
what both entry points answer to a NULL space without a device, and the marshalling of the table.  (The kernels are
k_masked.hip's: tests/test_knn_masked_host.py has their resource usage.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from embeddinghub_amd import _lib
from embeddinghub_amd import build as ehx_build
from embeddinghub_amd.space import Space, marshal_mask, marshal_mask_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ehx_knn_masked_multi", "ehx_knn_masked_multi_device")


def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS and hasattr(raw, name)
    assert "k_masked.hip" in ehx_build.SOURCES and "ehx_masked.cpp" in ehx_build.SOURCES   # one bitmap is a table of one
    for f in ("k_masked.hip", "ehx_masked.cpp"):
        assert os.path.exists(os.path.join(ehx_build.CSRC, f))
    for f in ("k_maskedq.hip", "ehx_maskedq.cpp"):   # ... and not a second copy
        assert f not in ehx_build.SOURCES and not os.path.exists(os.path.join(ehx_build.CSRC, f))
    assert re.search(r"#define EHX_ABI_VERSION 5\b", header)   # additive: the version stays
    assert "limit of 64 bitmaps is a CHOICE" in header          # stated as one, beside the contract
    for name in ("knn_masked_multi", "knn_masked_multi_device"):
        assert callable(getattr(Space, name))


def test_a_null_space_is_refused_with_or_without_a_device():
    lib = _lib.load()
    q = (C.c_float * 4)()
    masks = (C.c_uint32 * 2)(0xF, 0x3)
    of = (C.c_uint32 * 1)(1)
    ids, dist, cnt = (C.c_uint64 * 4)(), (C.c_float * 4)(), (C.c_uint32 * 1)()
    assert lib.ehx_knn_masked_multi(None, 1, q, 4, masks, 2, 4, of, ids, dist, cnt) == _lib.EINVAL
    assert lib.ehx_last_error() == b"space is NULL"
    assert lib.ehx_knn_masked_multi_device(None, None, 1, None, 4, None, 2, 4, None, None, None, None) == _lib.EINVAL
    assert lib.ehx_last_error() == b"space is NULL"


def test_mask_table_marshalling():
    for n in (0, 1, 31, 32, 33, 70, 257):
        rng = np.random.default_rng(n)
        b = rng.random((3, n)) < 0.5
        words, n_masks, n_bits = marshal_mask_table(b)
        assert (n_masks, n_bits) == (3, n) and words.dtype == np.uint32 and words.flags.c_contiguous
        assert words.shape == (3, (n + 31) // 32)
        for m in range(3):   # every row packed as marshal_mask packs one bitmap
            assert words[m].tolist() == marshal_mask(b[m])[0].tolist()
    b = np.zeros((2, 70), dtype=bool)
    b[0, [0, 31, 32, 69]] = True
    b[1, 33] = True
    assert marshal_mask_table(b)[0].tolist() == [[0x80000001, 0x1, 0x20], [0, 0x2, 0]]
    w, m, nb = marshal_mask_table(b, 33)                                   # a shorter n_bits cuts every bitmap
    assert w.tolist() == [[0x80000001, 0x1], [0, 0]] and (m, nb) == (2, 33)
    assert marshal_mask_table(b[:, ::2])[0].tolist() == [[0x00010001, 0x0], [0, 0]]   # a strided view
    assert marshal_mask_table([[True, False, True]])[0].tolist() == [[5]]
    assert marshal_mask_table(np.zeros((0, 40), dtype=bool))[1:] == (0, 40)
    packed = np.array([[7, 0xFFFFFFFF, 1], [1, 2, 3]], dtype=np.uint32)
    w, m, nb = marshal_mask_table(packed, 70)
    assert (m, nb) == (2, 70) and w.tolist() == packed.tolist()              # packed words pass through as they are
    w, m, nb = marshal_mask_table(packed, 40)                                # the table is dense at ceil(n_bits / 32) words
    assert w.tolist() == [[7, 0xFFFFFFFF], [1, 2]] and w.flags.c_contiguous and nb == 40
    assert marshal_mask_table(packed, 96)[2] == 96
    for bad, nb in ((packed, None), (packed, 97), (packed, -1), (np.zeros(32, dtype=bool), None), (b, 71),
                    (np.zeros((2, 2, 2), dtype=bool), None), (np.zeros((2, 4), dtype=np.int64), 4),
                    (np.zeros((2, 4), dtype=np.float32), None), (np.uint32(5), 3)):
        with pytest.raises(ValueError):
            marshal_mask_table(bad, nb)
