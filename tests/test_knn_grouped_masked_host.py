"""CPU-side checks of the grouped kNN under row bitmaps (ehx_knn_grouped_masked*): the declarations, the ABI that stays as
it was, the hook outside it, what both entry points answer without a device, and the resource usage of the two pool-fill
kernels (k_grouped.hip) built for gfx950."""
import ctypes as C
import inspect
import os
import re
import subprocess

from embeddinghub_amd import _lib
from embeddinghub_amd import build as ehx_build
from embeddinghub_amd.space import Space

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ehx_knn_grouped_masked", "ehx_knn_grouped_masked_device")
HOOK = "ehx_test_grouped_masked_counters"


def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS and hasattr(raw, name)
    assert "k_grouped.hip" in ehx_build.SOURCES and "ehx_groupedm.cpp" in ehx_build.SOURCES
    assert re.search(r"#define EHX_ABI_VERSION 5\b", header)   # additive: the version stays
    for name in ("knn_grouped_masked", "knn_grouped_masked_device"):
        assert callable(getattr(Space, name))
    assert list(inspect.signature(Space.knn_grouped_masked).parameters)[1:] == [
        "queries", "k", "group_of", "allows", "mask_of", "per_group", "n_bits"]
    # per_group sits behind k, the labels and their number behind it, then the table as ehx_knn_masked_multi's
    assert _lib.SYMBOLS[NEW[0]][1][3:11] == [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_uint32),
                                            C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32)]
    assert _lib.SYMBOLS[NEW[1]][1][4:12] == [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint64,
                                            C.c_void_p]
    # the header states the rule and the three equivalences
    doc = header[header.index("Grouped kNN under row bitmaps"):header.index("int ehx_knn_grouped_masked_device(")]
    for text in ("FILTER FIRST, THEN CAP", "equals ehx_knn_grouped_device", "equals ehx_knn_masked_multi_device",
                 "count 0 for ITS queries"):
        assert text in " ".join(doc.replace(" * ", " ").split()), text


def test_the_counters_hook_is_not_part_of_the_abi():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    assert HOOK not in header and HOOK not in _lib.SYMBOLS
    assert hasattr(C.CDLL(_lib.LIB_PATH), HOOK)


def test_a_null_space_is_refused_before_the_device_is_looked_for():
    lib = _lib.load()
    q = (C.c_float * 4)()
    labels = (C.c_uint32 * 4)(0, 1, 2, 3)
    mask = (C.c_uint32 * 1)(0xF)
    of = (C.c_uint32 * 1)(0)
    ids, dist, cnt = (C.c_uint64 * 4)(), (C.c_float * 4)(), (C.c_uint32 * 1)()
    assert lib.ehx_knn_grouped_masked(None, 1, q, 4, 1, labels, 4, mask, 1, 4, of, ids, dist, cnt) == _lib.EINVAL
    assert lib.ehx_last_error() == b"space is NULL"
    assert lib.ehx_knn_grouped_masked_device(None, None, 1, None, 4, 1, None, 4, None, 1, 4, None, None, None, None) == _lib.EINVAL
    assert lib.ehx_last_error() == b"space is NULL"


def test_groupedm_kernels_use_no_scratch_and_spill_no_vector_registers(tmp_path):
    """the seed and the slab kernel, which the three grouped searches share: once each in k_grouped.hip"""
    src = os.path.join(ehx_build.CSRC, "k_grouped.hip")
    flags = [f for f in ehx_build.FLAGS if f != "-shared"]
    r = subprocess.run([ehx_build.HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o",
                                                    str(tmp_path / "k_grouped.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    blocks = r.stderr.split("Function Name: ")[1:]   # one block of remarks per kernel
    for kern in ("grouped_range_seed_kernel", "grouped_range_slab_kernel"):
        mine = [b for b in blocks if kern in b.split()[0]]
        assert len(mine) == 1, [b.split()[0] for b in blocks]
        for what in ("ScratchSize \\[bytes/lane\\]", "VGPRs Spill"):
            assert re.findall(what + r": (\d+)", mine[0]) == ["0"], (kern, what)
