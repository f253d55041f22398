"""CPU-side checks of the range search under row bitmaps (ehx_range_masked*): the declarations and sources, the ABI that stays
as it was, the counters hook, what both entry points answer without a device, and the resource usage of k_rangem.hip built
for gfx950."""
import ctypes as C
import os
import re
import subprocess

from embeddinghub_amd import _lib
from embeddinghub_amd import build as ehx_build
from embeddinghub_amd.space import Space

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ehx_range_masked", "ehx_range_masked_device")
HOOK = "ehx_test_range_masked_counters"


def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS and hasattr(raw, name)
    for f in ("k_rangem.hip", "ehx_rangem.cpp"):
        assert f in ehx_build.SOURCES and os.path.exists(os.path.join(ehx_build.CSRC, f))
    assert re.search(r"#define EHX_ABI_VERSION 5\b", header)   # additive: the version stays
    for name in ("range_masked", "range_masked_device"):
        assert callable(getattr(Space, name))


def test_the_counters_hook_is_not_part_of_the_abi():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    assert HOOK not in header and HOOK not in _lib.SYMBOLS
    assert hasattr(C.CDLL(_lib.LIB_PATH), HOOK)


def test_one_int8_range_stage_and_one_compaction():
    """the new path calls the range search's int8 stage and the bitmap search's compaction: it holds no copy of either"""
    csrc = {f: open(os.path.join(ehx_build.CSRC, f)).read() for f in os.listdir(ehx_build.CSRC)}
    for fn in ("int range_i8_stage(", "int masked_plan(", "uint64_t masked_exact_cut("):
        defined = [f for f, src in csrc.items() if re.search(r"^%s[^;]*\{" % re.escape(fn), src, flags=re.M)]
        assert len(defined) == 1 and defined[0] != "ehx_rangem.cpp", (fn, defined)
        assert fn.split()[1] in csrc["ehx_rangem.cpp"] and fn.split()[1] in csrc["ehx_internal.h"]
    assert "getenv" not in csrc["ehx_rangem.cpp"] and "hipMalloc" not in csrc["ehx_rangem.cpp"]
    assert "range_list_kernel" not in csrc["k_range.hip"]


def test_both_entry_points_without_a_device():
    import torch
    lib = _lib.load()
    q, r = (C.c_float * 4)(), (C.c_float * 1)()
    masks, of = (C.c_uint32 * 1)(0xF), (C.c_uint32 * 1)(0)
    ids, dist, cnt, tot = (C.c_uint64 * 4)(), (C.c_float * 4)(), (C.c_uint32 * 1)(), (C.c_uint64 * 1)()
    calls = (lambda s: lib.ehx_range_masked(s, 1, q, r, 4, masks, 1, 4, of, ids, dist, cnt, tot),
             lambda s: lib.ehx_range_masked_device(s, None, 1, None, None, 4, None, 1, 4, None, None, None, None, None))
    if torch.cuda.is_available():
        for call in calls:   # a NULL space is refused before anything is touched
            assert call(None) == _lib.EINVAL and lib.ehx_last_error() == b"space is NULL"
    else:
        h = C.c_void_p()
        assert lib.ehx_space_create(b"rangem-nodev", 12, 4, 0, 0, None, C.byref(h)) == _lib.ENODEVICE and not h.value
        for call in calls:   # no device: that is the answer, whatever else is wrong with the call
            assert call(None) == _lib.ENODEVICE


def test_range_list_kernels_use_no_scratch_and_spill_no_vector_registers(tmp_path):
    src = os.path.join(ehx_build.CSRC, "k_rangem.hip")
    flags = [f for f in ehx_build.FLAGS if f != "-shared"]
    r = subprocess.run([ehx_build.HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o",
                                                    str(tmp_path / "k_rangem.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    for kern, count in (("range_list_kernel", 9), ("range_scan_radii_kernel", 1)):
        assert sum(kern in n for n in names) == count, names
    assert len(names) == 10 and not any("range_exact_kernel" in n for n in names), names
    for what in ("ScratchSize \\[bytes/lane\\]", "VGPRs Spill"):
        vals = re.findall(what + r": (\d+)", r.stderr)
        assert len(vals) == len(names) and all(v == "0" for v in vals), (what, vals)
