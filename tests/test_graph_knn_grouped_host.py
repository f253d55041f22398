"""CPU-side checks of the grouped graph walk: the entry points are declared and bound, a NULL space is refused before the
device is looked for, and k_graphg.hip compiles for gfx950 with no scratch and no spills."""
import ctypes as C
import os
import re
import subprocess

from embeddinghub_amd import _lib
from embeddinghub_amd import build as ehx_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ehx_graph_knn_grouped_device", "ehx_graph_knn_grouped")


def test_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS
    assert "k_graphg.hip" in ehx_build.SOURCES and "ehx_graphg.cpp" in ehx_build.SOURCES


def test_null_space_is_refused_before_the_device_is_looked_for():
    L = _lib.load()
    ids, dist, cnt = (C.c_uint64 * 4)(), (C.c_float * 4)(), (C.c_uint32 * 1)()
    q, lab = (C.c_float * 4)(), (C.c_uint32 * 4)()
    assert L.ehx_graph_knn_grouped(None, 1, q, 4, 1, lab, 4, _lib.WALK_GRAPH, ids, dist, cnt) == _lib.EINVAL
    assert L.ehx_graph_knn_grouped_device(None, None, 1, None, 4, 1, None, 4, _lib.WALK_GRAPH, None, None, None) == _lib.EINVAL
    assert b"space is NULL" in L.ehx_last_error()


def test_walk_kernel_uses_no_scratch_and_spills_nothing(tmp_path):
    src = os.path.join(ehx_build.CSRC, "k_graphg.hip")
    flags = [f for f in ehx_build.FLAGS if f != "-shared"]
    r = subprocess.run([ehx_build.HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o",
                                                    str(tmp_path / "k_graphg.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert sum("graph_search_grouped_kernel" in n for n in names) == 2, names
    for what in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"):
        vals = re.findall(what + r": (\d+)", r.stderr)
        assert len(vals) == len(names) and all(v == "0" for v in vals), (what, vals)
