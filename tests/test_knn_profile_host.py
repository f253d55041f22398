"""CPU-side checks of the profile search: the declarations, and the bad arguments refused before a device is looked for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from embeddinghub_amd import _lib
from embeddinghub_amd import build as ehx_build
from embeddinghub_amd.space import Space

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ehx_combine_rows_device", "ehx_knn_profile_device", "ehx_knn_profile", "ehx_knn_profile_keys")


def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS and hasattr(raw, name)
    assert "k_profile.hip" in ehx_build.SOURCES and "ehx_profile.cpp" in ehx_build.SOURCES
    assert re.search(r"#define EHX_ABI_VERSION 5\b", header)   # additive: the version stays
    assert re.search(r"#define EHX_PROFILE_MAX_LIST 4096u\b", header) and _lib.PROFILE_MAX_LIST == 4096
    for name in ("combine_rows_device", "knn_profile_device", "knn_profile", "knn_profile_keys"):
        assert callable(getattr(Space, name))


@pytest.mark.parametrize("k,ptrs,off,n,code,text", [
    (0, True, [0, 0, 0], 0, _lib.EINVAL, b"k is 0"),
    (257, True, [0, 0, 0], 0, _lib.EUNSUPPORTED, b"k=257 exceeds 256"),
    (5, False, [0, 0, 0], 0, _lib.EINVAL, b"NULL argument"),
    (5, True, [0, 3, 2], 2, _lib.EINVAL, b"%s is not non-decreasing at query 1"),
    (5, True, [0, 1, 2], 3, _lib.EINVAL, b"%s ends at 2, not at %s = 3"),
    (5, True, [0, 4097, 4097], 4097, _lib.EINVAL, b"query 0 combines 4097 entries, more than EHX_PROFILE_MAX_LIST = 4096")])
def test_bad_arguments_are_refused_before_the_device_is_looked_for(k, ptrs, off, n, code, text):
    lib = _lib.load()
    space = C.cast(C.create_string_buffer(8), C.c_void_p)   # never read: these checks come first
    ids, dist, cnt = (C.c_uint64 * 514)() if ptrs else None, (C.c_float * 514)(), (C.c_uint32 * 2)()
    entries = np.zeros(4097, dtype=np.uint64).ctypes.data_as(C.POINTER(C.c_uint64))
    offs = (C.c_uint64 * 3)(*off)
    keys, klens = (C.c_char_p * 4097)(*([b"a"] * 4097)), (C.c_size_t * 4097)(*([1] * 4097))
    calls = [(lambda s: lib.ehx_knn_profile(s, 2, entries, offs, None, n, k, ids, dist, cnt), (b"off", b"n_entries")),
             (lambda s: lib.ehx_knn_profile_keys(s, 2, keys, klens, offs, None, n, k, ids, dist, cnt), (b"key_off", b"n_keys"))]
    for call, names in calls:
        assert call(None) == _lib.EINVAL and lib.ehx_last_error() == b"space is NULL"
        assert call(space) == code and lib.ehx_last_error() == (text % names[:text.count(b"%s")] if b"%s" in text else text)
    # the device forms decide what needs no offsets the same way
    assert lib.ehx_combine_rows_device(None, None, 2, None, None, None, 0, None, None) == _lib.EINVAL
    assert lib.ehx_last_error() == b"space is NULL"
    if off == [0, 0, 0]:
        assert lib.ehx_knn_profile_device(space, None, 2, None, offs, None, 0, k, ids, dist, cnt) == code and lib.ehx_last_error() == text
