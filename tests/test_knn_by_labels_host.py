"""CPU-side checks of the multi-probe label search's boundary: its two names are declared, bound and exported, its test hook
is exported and nothing more, and its first check needs no device."""
import ctypes as C
import os
import re

from embeddinghub_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ehx_knn_by_labels", "ehx_knn_by_labels_device"]
HOOK = "ehx_test_probe_counters"


def test_names_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SYMBOLS and hasattr(raw, name), name
    assert hasattr(raw, HOOK) and HOOK not in header and HOOK not in _lib.SYMBOLS
    assert re.search(r"#define EHX_MAX_WANT 64u\b", header) and _lib.MAX_WANT == 64


def test_null_space_is_refused_before_the_device_is_looked_for():
    lib = _lib.load()
    assert lib.ehx_knn_by_labels(None, 1, None, 1, 0, 1, None, None, None, None, None) == _lib.EINVAL
    assert lib.ehx_last_error() == b"space is NULL"
    assert lib.ehx_knn_by_labels_device(None, None, 1, None, 1, 0, 1, None, None, None, None, None) == _lib.EINVAL
    assert lib.ehx_last_error() == b"space is NULL"
