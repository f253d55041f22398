"""CPU-side checks of the MMR search: the declarations, and the EHX_EINVAL cases decided before a device is looked for."""
import ctypes as C
import os
import re

import pytest

from embeddinghub_amd import _lib
from embeddinghub_amd import build as ehx_build
from embeddinghub_amd.space import Space

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ehx_mmr_select_device", "ehx_knn_mmr_device", "ehx_knn_mmr")


def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS and hasattr(raw, name)
    assert "k_mmr.hip" in ehx_build.SOURCES and "ehx_mmr.cpp" in ehx_build.SOURCES
    assert re.search(r"#define EHX_ABI_VERSION 5\b", header)   # additive: the version stays
    assert re.search(r"#define EHX_MMR_MAX_FETCH 256u\b", header) and _lib.MMR_MAX_FETCH == 256
    for name in ("mmr_select_device", "knn_mmr_device", "knn_mmr"):
        assert callable(getattr(Space, name))
    assert _lib.SYMBOLS[NEW[0]][1][7:9] == [C.c_uint32, C.c_float]   # lambda: a float behind k, or behind fetch_k
    assert _lib.SYMBOLS[NEW[1]][1][4:7] == [C.c_uint32, C.c_uint32, C.c_float]
    assert _lib.SYMBOLS[NEW[2]][1][3:6] == [C.c_uint32, C.c_uint32, C.c_float]


@pytest.mark.parametrize("k,fetch_k,lam,text", [(0, 4, 0.5, b"k is 0"), (5, 4, 0.5, b"k=5 exceeds fetch_k=4"),
                                                (2, 4, float("nan"), b"lambda=nan is not in [0, 1]"),
                                                (2, 4, -0.1, b"lambda=-0.1 is not in [0, 1]"),
                                                (2, 4, 1.5, b"lambda=1.5 is not in [0, 1]")])
def test_bad_arguments_are_refused_before_the_device_is_looked_for(k, fetch_k, lam, text):
    lib = _lib.load()
    space = C.cast(C.create_string_buffer(8), C.c_void_p)   # never read: these checks come first
    q = (C.c_float * 4)()
    ids, dist, cnt = (C.c_uint64 * 8)(), (C.c_float * 8)(), (C.c_uint32 * 1)()
    a = [C.addressof(x) for x in (q, ids, dist, cnt)]
    calls = [lambda s: lib.ehx_knn_mmr(s, 1, q, k, fetch_k, lam, ids, dist, cnt),
             lambda s: lib.ehx_knn_mmr_device(s, None, 1, a[0], k, fetch_k, lam, *a[1:]),
             lambda s: lib.ehx_mmr_select_device(s, None, 1, fetch_k, *a[1:], k, lam, *a[1:])]
    for call in calls:
        assert call(None) == _lib.EINVAL and lib.ehx_last_error() == b"space is NULL"
        assert call(space) == _lib.EINVAL and lib.ehx_last_error() == text
