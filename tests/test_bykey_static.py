"""CPU-side checks of the by-key feature: k_bykey.hip compiles for gfx950 with no scratch and no spills, and the header,
the binding and the C++ shim name the new entry points."""
import os
import re
import subprocess

from embeddinghub_amd import _lib
from embeddinghub_amd import build as ehx_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bykey_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    src = os.path.join(ehx_build.CSRC, "k_bykey.hip")
    flags = [f for f in ehx_build.FLAGS if f != "-shared"]
    r = subprocess.run([ehx_build.HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o",
                                                    str(tmp_path / "k_bykey.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert any("gather_rows_kernel" in n for n in names) and any("drop_self_kernel" in n for n in names), names
    for what in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"):
        vals = re.findall(what + r": (\d+)", r.stderr)
        assert len(vals) == len(names) and all(v == "0" for v in vals), (what, vals)


def test_new_entry_points_are_declared_bound_and_used():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    for name in ("ehx_knn_by_keys", "ehx_knn_by_keys_keys", "ehx_knn_by_ids_device"):
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS
    assert "k_bykey.hip" in ehx_build.SOURCES
    assert "ehx_knn_by_keys_keys(" in open(os.path.join(ROOT, "integration", "cpp", "ann_index.h")).read()
