"""CPU-side checks of the range search (ehx_range*): the declarations, the ABI that stays as it was, what every entry point
answers without a device, the marshalling of the radius, and the resource usage of k_range.hip built for gfx950."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from embeddinghub_amd import _lib
from embeddinghub_amd import build as ehx_build
from embeddinghub_amd.space import Space, marshal_radius

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ehx_range", "ehx_range_keys", "ehx_range_device")


def test_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS
    assert "k_range.hip" in ehx_build.SOURCES and "ehx_range.cpp" in ehx_build.SOURCES
    assert re.search(r"#define EHX_ABI_VERSION 5\b", header)   # additive: the version stays
    for name in ("range_search", "range_search_keys", "range_device"):
        assert callable(getattr(Space, name))


def test_stats_layout_is_unchanged():
    """ehx_stats_t as the parent commit declared it: same fields, same size"""
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    body = re.search(r"typedef struct ehx_stats_t \{(.*?)\} ehx_stats_t;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint64_t|double|uint32_t|float)\s+([^;]+);", body)
    names = [n.strip() for _, decl in fields for n in decl.split(",")]
    assert names == [f for f, _ in _lib.Stats._fields_]
    assert C.sizeof(_lib.Stats) == sum(8 if t in ("uint64_t", "double") else 4 for t, decl in fields for _ in decl.split(","))
    assert not any("range" in n for n in names)


def test_the_counters_hook_is_not_part_of_the_abi():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    assert "ehx_test_range_counters" not in header and "ehx_test_range_counters" not in _lib.SYMBOLS
    assert hasattr(C.CDLL(_lib.LIB_PATH), "ehx_test_range_counters")


def test_every_entry_point_without_a_device():
    import torch
    lib = _lib.load()
    q, r = (C.c_float * 4)(), (C.c_float * 1)()
    ids, dist, cnt, tot = (C.c_uint64 * 4)(), (C.c_float * 4)(), (C.c_uint32 * 1)(), (C.c_uint64 * 1)()
    off = (C.c_uint64 * 5)()
    calls = (lambda s: lib.ehx_range(s, 1, q, r, 4, ids, dist, cnt, tot),
             lambda s: lib.ehx_range_keys(s, 1, q, r, 4, ids, dist, cnt, tot, None, 0, off),
             lambda s: lib.ehx_range_device(s, None, 1, None, None, 4, None, None, None, None))
    if torch.cuda.is_available():
        for call in calls:   # a NULL space is refused before anything is touched
            assert call(None) == _lib.EINVAL and lib.ehx_last_error() == b"space is NULL"
    else:
        h = C.c_void_p()
        assert lib.ehx_space_create(b"range-nodev", 11, 4, 0, 0, None, C.byref(h)) == _lib.ENODEVICE and not h.value
        for call in calls:   # no device: that is the answer, whatever else is wrong with the call
            assert call(None) == _lib.ENODEVICE


def test_radius_marshalling():
    r = marshal_radius(0.25, 5)
    assert r.dtype == np.float32 and r.shape == (5,) and r.flags.c_contiguous and (r == np.float32(0.25)).all()
    assert marshal_radius(np.float64(2.0), 3).tolist() == [2.0, 2.0, 2.0]
    assert marshal_radius(np.array([1.5]), 4).tolist() == [1.5] * 4           # a one-element array broadcasts too
    assert np.isposinf(marshal_radius(np.inf, 2)).all() and np.isnan(marshal_radius(float("nan"), 2)).all()
    r = marshal_radius(np.arange(6, dtype=np.float64)[::2], 3)
    assert r.dtype == np.float32 and r.flags.c_contiguous and r.tolist() == [0.0, 2.0, 4.0]
    assert marshal_radius([], 0).shape == (0,)
    for bad in ([1.0, 2.0], np.zeros(4)):
        with pytest.raises(ValueError):
            marshal_radius(bad, 3)


def test_range_kernels_use_no_scratch_and_spill_no_vector_registers(tmp_path):
    src = os.path.join(ehx_build.CSRC, "k_range.hip")
    flags = [f for f in ehx_build.FLAGS if f != "-shared"]
    r = subprocess.run([ehx_build.HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o",
                                                    str(tmp_path / "k_range.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    for kern, count in (("range_exact_kernel", 9), ("range_rerank_kernel", 6), ("range_emit_kernel", 1),
                        ("range_thr_kernel", 1), ("range_iota_kernel", 1)):
        assert sum(kern in n for n in names) == count, names
    for what in ("ScratchSize \\[bytes/lane\\]", "VGPRs Spill"):
        vals = re.findall(what + r": (\d+)", r.stderr)
        assert len(vals) == len(names) and all(v == "0" for v in vals), (what, vals)
    # the hot small kernel of the int8 path, the sort and the threshold spill nothing at all
    sg = dict(zip(names, re.findall(r"SGPRs Spill: (\d+)", r.stderr)))
    for n, v in sg.items():
        if "range_rerank" in n or "range_emit" in n or "range_thr" in n:
            assert v == "0", (n, v)
