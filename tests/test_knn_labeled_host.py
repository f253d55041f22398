"""CPU-side checks of the kNN under a label column (ehx_knn_labeled*): the declarations, the ABI that stays as it was, what
both entry points answer without a device, what the header promises, the batches of tests/labeled_cases.py, and the resource
usage of k_labeled.hip built for gfx950."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import labeled_cases as lbc
from embeddinghub_amd import _lib
from embeddinghub_amd import build as ehx_build
from embeddinghub_amd.space import Space

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ehx_knn_labeled", "ehx_knn_labeled_device")
HOOK = "ehx_test_labeled_counters"
KERNELS = ("labeled_count_kernel", "labeled_tiles_kernel", "labeled_fill_kernel", "labeled_sample_kernel")


def _header():
    return open(os.path.join(ROOT, "include", "ehx.h")).read()


def test_entry_points_are_declared_bound_and_exported():
    header = _header()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS and hasattr(raw, name)
    assert "k_labeled.hip" in ehx_build.SOURCES and "ehx_labeled.cpp" in ehx_build.SOURCES
    assert re.search(r"#define EHX_ABI_VERSION 5\b", header)   # additive: the version stays
    for name in ("knn_labeled", "knn_labeled_device"):
        assert callable(getattr(Space, name))


def test_the_counters_hook_is_not_part_of_the_abi():
    assert HOOK not in _header() and HOOK not in _lib.SYMBOLS
    assert hasattr(C.CDLL(_lib.LIB_PATH), HOOK)


def test_a_null_space_is_refused_before_the_device_is_looked_for():
    lib = _lib.load()
    q = (C.c_float * 4)()
    col, want = (C.c_uint32 * 4)(1, 2, 1, 2), (C.c_uint32 * 1)(1)
    ids, dist, cnt = (C.c_uint64 * 4)(), (C.c_float * 4)(), (C.c_uint32 * 1)()
    for call in (lambda: lib.ehx_knn_labeled(None, 1, q, 4, col, 4, want, ids, dist, cnt),
                 lambda: lib.ehx_knn_labeled_device(None, None, 1, None, 4, None, 4, None, None, None, None)):
        assert call() == _lib.EINVAL and lib.ehx_last_error() == b"space is NULL"   # with a device or without one


def test_the_header_states_the_contract():
    text = " ".join(_header().split())
    at = text.index("Partitioned kNN")
    doc = text[at:text.index("int ehx_knn_labeled_device(", at)].replace(" * ", " ")
    assert "byte for byte, what ehx_knn_masked_device returns for query i alone under the bitmap" in doc
    assert "0xFFFFFFFF is an ordinary label" in doc and "EHX_GROUP_NONE" in doc
    assert "count 0 for ITS queries" in doc
    assert "ONE acquire-load snapshot" in doc and "not limited" in doc
    assert re.search(r"at most TWICE per device batch", doc)   # the waits do not depend on the number of labels


def test_the_batches_of_the_gpu_tests():
    col = lbc.column()
    assert col.dtype == np.uint32 and len(col) == 20000
    assert len(np.unique(lbc.mixed_batch())) > 64 >= len(np.unique(lbc.table_batch()))
    assert len(lbc.two_batches()) == lbc.SIDE_CHUNK + 64
    tab, of = lbc.as_table(col, lbc.table_batch())
    for i, lab in enumerate(lbc.table_batch()):
        assert (tab[of[i]] == (col == lab)).all()


def test_labeled_kernels_use_no_scratch_and_spill_no_vector_registers(tmp_path):
    """the compaction by label: exactly these five functions, each once"""
    src = os.path.join(ehx_build.CSRC, "k_labeled.hip")
    flags = [f for f in ehx_build.FLAGS if f != "-shared"]
    r = subprocess.run([ehx_build.HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o",
                                                    str(tmp_path / "k_labeled.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    for kern in KERNELS:
        assert sum(kern in n for n in names) == 1, names
    assert len(names) == len(KERNELS)
    for what in ("ScratchSize \\[bytes/lane\\]", "VGPRs Spill"):
        vals = re.findall(what + r": (\d+)", r.stderr)
        assert len(vals) == len(names) and all(v == "0" for v in vals), (what, vals)
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert max(lds) == 16384   # the table of 2048 labels and its counters: 8 KB each


def test_the_batch_asked_four_ways_names_labels_on_both_sides_of_the_cut():
    """tests/test_knn_labeled.py's four-ways batch, by the routing rule in numpy: at least 64 queries on scanning labels and at
    least 64 on listed ones (labeled_cases.both_routes_batch asserts the sizes where it makes the batch)"""
    want, scans = lbc.both_routes_batch()
    assert len(want) == len(scans) == 134 and scans.sum() >= 64 and (~scans).sum() >= 64
    assert set(want[scans].tolist()) == set(lbc.DENSE)
