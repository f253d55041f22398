"""CPU-side checks of the graph walk under per-query exclusion lists (ehx_graph_knn_except*): the declarations, what the entry
points answer to a NULL space without a device, and the resource usage of the walk kernels.  The refusal of bad offsets is here
too, marked gpu: the call looks for the device in front of those checks, as ehx_graph_knn_masked_multi does."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from embeddinghub_amd import _lib
from embeddinghub_amd import build as ehx_build
from embeddinghub_amd.space import Space

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ehx_graph_knn_except_device", "ehx_graph_knn_except", "ehx_graph_knn_except_keys")


def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS and hasattr(raw, name)
        assert callable(getattr(Space, name[4:]))
    assert "k_graphx.hip" in ehx_build.SOURCES and "ehx_graphx.cpp" in ehx_build.SOURCES
    assert re.search(r"#define EHX_ABI_VERSION 5\b", header)   # additive: the version stays
    assert _lib.load().ehx_abi_version() == 5
    # the route is the argument behind the number of list entries, in every form
    assert [_lib.SYMBOLS[name][1][i] for name, i in zip(NEW, (8, 7, 8))] == [C.c_uint32] * 3


def _call_args(off, n_excl):
    q = (C.c_float * 8)()
    out = ((C.c_uint64 * 10)(), (C.c_float * 10)(), (C.c_uint32 * 2)())
    excl = np.zeros(4097, dtype=np.uint64).ctypes.data_as(C.POINTER(C.c_uint64))
    keys, klens = (C.c_char_p * 4097)(*([b"a"] * 4097)), (C.c_size_t * 4097)(*([1] * 4097))
    return q, (C.c_uint64 * 3)(*off), excl, keys, klens, n_excl, out


def test_a_null_space_is_refused_with_or_without_a_device():
    lib = _lib.load()
    q, offs, excl, keys, klens, n, out = _call_args([0, 1, 2], 2)
    for rc in (lib.ehx_graph_knn_except(None, 2, q, 5, excl, offs, n, _lib.WALK_GRAPH, *out),
               lib.ehx_graph_knn_except_keys(None, 2, q, 5, keys, klens, offs, n, _lib.WALK_AUTO, *out),
               lib.ehx_graph_knn_except_device(None, None, 2, None, 5, None, None, n, _lib.WALK_EXACT, None, None, None)):
        assert rc == _lib.EINVAL and lib.ehx_last_error() == b"space is NULL"


@pytest.mark.gpu
@pytest.mark.parametrize("off,n_excl,text", [
    ([0, 3, 2], 2, b"%s is not non-decreasing at query 1"),
    ([0, 1, 2], 3, b"%s ends at 2, not at %s = 3"),
    ([0, 4097, 4097], 4097, b"query 0 excludes 4097 entries, more than EHX_EXCEPT_MAX_LIST = 4096: "
                            b"use ehx_graph_knn_masked_multi with a bitmap per query")])
def test_bad_offsets_are_refused(off, n_excl, text):
    lib = _lib.load()
    s = Space.unique("gx-host", 4)
    q, offs, excl, keys, klens, n, out = _call_args(off, n_excl)
    calls = [(lambda: lib.ehx_graph_knn_except(s._h, 2, q, 5, excl, offs, n, _lib.WALK_GRAPH, *out), (b"excl_off", b"n_excl")),
             (lambda: lib.ehx_graph_knn_except_keys(s._h, 2, q, 5, keys, klens, offs, n, _lib.WALK_GRAPH, *out),
              (b"key_off", b"n_keys"))]
    for call, names in calls:
        assert call() == _lib.EINVAL
        assert lib.ehx_last_error() == (text % names[:text.count(b"%s")] if b"%s" in text else text)
    s.drop()


def test_walk_kernels_without_scratch_or_spills(tmp_path):
    src = os.path.join(ehx_build.CSRC, "k_graphx.hip")
    flags = [f for f in ehx_build.FLAGS if f != "-shared"]
    r = subprocess.run([ehx_build.HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o",
                                                    str(tmp_path / "k_graphx.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert len(names) == 2 and all("graph_search_except_kernel" in n for n in names), names   # the walk is inlined
    for what in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"):
        vals = re.findall(what + r": (\d+)", r.stderr)
        assert len(vals) == 2 and all(v == "0" for v in vals), (what, vals)
