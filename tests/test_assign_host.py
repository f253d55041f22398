"""CPU-side checks of the clustering calls: the three entry points are declared, bound and exported, the test hook is
exported and nothing else, k_assign.hip compiles for gfx950 with no scratch and no spills, and the strand restatement the
GPU tests compare the centroid sums with is itself pinned to a float64 sum."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from embeddinghub_amd import _lib
from embeddinghub_amd import build as ehx_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ehx_assign_device", "ehx_centroid_sums_device", "ehx_kmeans_device")


def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS and hasattr(raw, name)
    assert re.search(r"#define EHX_ASSIGN_MAX_CENTROIDS 4096u\b", header)
    assert re.search(r"#define EHX_ABI_VERSION 5\b", header)   # additive: the version stays
    assert "k_assign.hip" in ehx_build.SOURCES and "ehx_assign.cpp" in ehx_build.SOURCES
    assert hasattr(raw, "ehx_test_assign_counts")
    assert "ehx_test_assign_counts" not in header and "ehx_test_assign_counts" not in _lib.SYMBOLS


def test_assign_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    src = os.path.join(ehx_build.CSRC, "k_assign.hip")
    flags = [f for f in ehx_build.FLAGS if f != "-shared"] + ehx_build.EXTRA_FLAGS["k_assign.hip"]
    r = subprocess.run([ehx_build.HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o",
                                                    str(tmp_path / "k_assign.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    for kernel in ("assign_filter_kernel", "assign_exact_kernel", "centroid_stats_kernel", "lloyd_divide_kernel"):
        assert any(kernel in n for n in names), names
    for what in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"):
        vals = re.findall(what + r": (\d+)", r.stderr)
        assert len(vals) == len(names) and all(v == "0" for v in vals), (what, vals)


def test_strand_restatement_is_a_sum():
    """eight strands of at most ceil(L / 8) adds and seven joining adds: |t - sum| <= gamma_(ceil(L / 8) + 7) * sum |x|"""
    f32 = np.float32
    L = 1001
    R = np.random.default_rng(1).standard_normal((L, 9)).astype(f32)
    acc = np.zeros((8, 9), dtype=f32)
    for e in range(L):
        acc[e % 8] = acc[e % 8] + R[e]
    t = acc[0]
    for k in range(1, 8):
        t = t + acc[k]
    m = -(-L // 8) + 7
    gamma = m * 2.0 ** -24 / (1 - m * 2.0 ** -24)
    assert t.dtype == f32
    assert (np.abs(t.astype(np.float64) - R.astype(np.float64).sum(axis=0)) <= gamma * np.abs(R.astype(np.float64)).sum(axis=0)).all()
