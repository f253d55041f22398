"""CPU-side checks of the MaxSim search: the declarations, and the argument checks decided before a device is looked for."""
import ctypes as C
import os
import re

import pytest

from embeddinghub_amd import _lib
from embeddinghub_amd import build as ehx_build
from embeddinghub_amd.space import Space

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ehx_maxsim_select_device", "ehx_knn_maxsim_device", "ehx_knn_maxsim")


def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS and hasattr(raw, name)
    assert hasattr(raw, "ehx_test_maxsim_counters") and "ehx_test_maxsim_counters" not in header
    assert "k_maxsim.hip" in ehx_build.SOURCES and "ehx_maxsim.cpp" in ehx_build.SOURCES
    assert re.search(r"#define EHX_ABI_VERSION 5\b", header)   # additive: the version stays
    assert re.search(r"#define EHX_MAXSIM_MAX_TOKENS 32u\b", header) and _lib.MAXSIM_MAX_TOKENS == 32
    assert re.search(r"#define EHX_MAXSIM_MAX_CAND 1024u\b", header) and _lib.MAXSIM_MAX_CAND == 1024
    for name in ("maxsim_select_device", "knn_maxsim_device", "knn_maxsim"):
        assert callable(getattr(Space, name))


# (n_tokens, col, k, fetch_k or n_cand) -> code, text; the select form reads the last as n_cand
CASES = [((4, 0, 0, 4), _lib.EINVAL, b"k is 0"), ((0, 0, 2, 4), _lib.EINVAL, b"n_tokens is 0"),
         ((4, _lib.MAX_COLUMNS, 2, 4), _lib.EINVAL, None), ((33, 0, 2, 4), _lib.EUNSUPPORTED, b"n_tokens=33 exceeds 32"),
         ((4, 0, 1025, 4), _lib.EUNSUPPORTED, b"k=1025 exceeds 1024")]


@pytest.mark.parametrize("args,code,text", CASES)
def test_bad_arguments_are_refused_before_the_device_is_looked_for(args, code, text):
    lib = _lib.load()
    n_tokens, col, k, fk = args
    space = C.cast(C.create_string_buffer(8), C.c_void_p)   # never read: these checks come first
    q = (C.c_float * 8)()
    ids, score, cnt = (C.c_uint64 * 8)(), (C.c_float * 8)(), (C.c_uint32 * 1)()
    a = [C.addressof(x) for x in (q, ids, score, cnt)]
    calls = [lambda s: lib.ehx_knn_maxsim(s, 1, n_tokens, q, None, col, k, fk, ids, score, cnt),
             lambda s: lib.ehx_knn_maxsim_device(s, None, 1, n_tokens, a[0], None, col, k, fk, *a[1:]),
             lambda s: lib.ehx_maxsim_select_device(s, None, 1, n_tokens, a[0], None, col, fk, a[3], a[3], k, *a[1:])]
    for call in calls:
        assert call(None) == _lib.EINVAL and lib.ehx_last_error() == b"space is NULL"
        assert call(space) == code and (text is None or lib.ehx_last_error() == text)


def test_the_candidate_bounds_of_each_form():
    lib = _lib.load()
    space = C.cast(C.create_string_buffer(8), C.c_void_p)
    q = (C.c_float * 8)()
    ids, score, cnt = (C.c_uint64 * 8)(), (C.c_float * 8)(), (C.c_uint32 * 1)()
    a = [C.addressof(x) for x in (q, ids, score, cnt)]
    assert lib.ehx_knn_maxsim(space, 1, 25, q, None, 0, 2, 41, ids, score, cnt) == _lib.EUNSUPPORTED
    assert lib.ehx_last_error() == b"n_tokens * fetch_k = 25 * 41 exceeds 1024"
    assert lib.ehx_knn_maxsim_device(space, None, 1, 1, a[0], None, 0, 2, 257, *a[1:]) == _lib.EUNSUPPORTED
    assert lib.ehx_last_error() == b"fetch_k=257 exceeds 256"
    assert lib.ehx_knn_maxsim(space, 1, 4, q, None, 0, 2, 0, ids, score, cnt) == _lib.EINVAL
    assert lib.ehx_maxsim_select_device(space, None, 1, 4, a[0], None, 0, 1025, a[3], a[3], 2, *a[1:]) == _lib.EUNSUPPORTED
    assert lib.ehx_last_error() == b"n_cand=1025 exceeds 1024"
    assert lib.ehx_maxsim_select_device(space, None, 1, 4, a[0], None, 0, 8, None, a[3], 2, *a[1:]) == _lib.EINVAL
    assert lib.ehx_last_error() == b"NULL argument"
