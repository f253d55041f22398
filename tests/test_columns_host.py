"""CPU-side checks of stored label columns: the declarations, the ABI that stays as it was, the hooks that stay out of it, what
every new entry point answers to a NULL space without a device, what the header promises, the helper's own columns, and the
resource usage of k_colindex.hip built for gfx950."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import column_cases as cc
import labeled_cases as lbc
from embeddinghub_amd import _lib
from embeddinghub_amd import build as ehx_build
from embeddinghub_amd.space import Space, marshal_columns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ehx_set_batch_cols", "ehx_column_set", "ehx_column_get", "ehx_column_load_device", "ehx_column_read_device",
       "ehx_knn_by_label", "ehx_knn_by_label_device", "ehx_knn_grouped_by_label", "ehx_knn_grouped_by_label_device")
HOOKS = ("ehx_test_column_counters", "ehx_test_column_index")
METHODS = ("set_batch_cols", "column_set", "column_get", "column_load_device", "column_read_device", "knn_by_label",
           "knn_by_label_device", "knn_grouped_by_label", "knn_grouped_by_label_device")
# kernel -> LDS bytes per workgroup, as designed (k_colindex.hip's header)
KERNELS = {"colindex_digits_kernel": 4096, "colindex_tilehist_kernel": 1024, "colindex_scan_kernel": 20,
           "colindex_scatter_kernel": 4096, "colindex_bcount_kernel": 16,
           "colindex_bfill_kernel": 16, "colindex_tiles_kernel": 0, "colindex_sample_kernel": 0,
           "column_scatter_kernel": 0, "column_gather_kernel": 0}


def _header():
    return open(os.path.join(ROOT, "include", "ehx.h")).read()


def test_entry_points_are_declared_bound_and_exported():
    header = _header()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS and hasattr(raw, name), name
    assert "k_colindex.hip" in ehx_build.SOURCES and "ehx_columns.cpp" in ehx_build.SOURCES
    assert re.search(r"#define EHX_ABI_VERSION 5\b", header)   # additive: the version stays
    assert re.search(r"#define EHX_MAX_COLUMNS 4\b", header) and _lib.MAX_COLUMNS == 4 == cc.MAX_COLUMNS
    for name in METHODS:
        assert callable(getattr(Space, name)), name


def test_the_hooks_are_not_part_of_the_abi():
    raw = C.CDLL(_lib.LIB_PATH)
    for hook in HOOKS:
        assert hook not in _header() and hook not in _lib.SYMBOLS and hasattr(raw, hook), hook


def test_a_null_space_is_refused_before_the_device_is_looked_for():
    lib = _lib.load()
    q = (C.c_float * 4)()
    vals, want = (C.c_uint32 * 4)(1, 2, 1, 2), (C.c_uint32 * 1)(1)
    cols = (C.c_uint32 * 1)(0)
    ptrs = (C.POINTER(C.c_uint32) * 1)(vals)
    keys, lens = (C.c_char_p * 1)(b"k"), (C.c_size_t * 1)(1)
    ids, dist, cnt = (C.c_uint64 * 4)(), (C.c_float * 4)(), (C.c_uint32 * 1)()
    calls = (lambda: lib.ehx_set_batch_cols(None, 1, keys, lens, q, 1, cols, ptrs),
             lambda: lib.ehx_set_batch_cols(None, 1, keys, lens, q, 0, None, None),
             lambda: lib.ehx_column_set(None, 0, 1, keys, lens, vals, None),
             lambda: lib.ehx_column_get(None, 0, 1, keys, lens, vals, None),
             lambda: lib.ehx_column_load_device(None, None, 0, 0, 1, None),
             lambda: lib.ehx_column_read_device(None, None, 0, 0, 1, None),
             lambda: lib.ehx_knn_by_label(None, 1, q, 4, 0, want, ids, dist, cnt),
             lambda: lib.ehx_knn_by_label_device(None, None, 1, None, 4, 0, None, None, None, None),
             lambda: lib.ehx_knn_grouped_by_label(None, 1, q, 4, 1, 0, 1, want, ids, dist, cnt),
             lambda: lib.ehx_knn_grouped_by_label_device(None, None, 1, None, 4, 1, 0, 1, None, None, None, None))
    assert len(calls) == len(NEW) + 1
    for call in calls:
        assert call() == _lib.EINVAL and lib.ehx_last_error() == b"space is NULL"   # with a device or without one


def test_the_header_states_the_contract():
    text = " ".join(_header().split()).replace(" * ", " ")
    cols = text[text.index("stored label columns: labels written with the rows"):text.index("int ehx_column_read_device(")]
    assert "reads as EHX_GROUP_NONE (0xFFFFFFFF) for every row" in cols and "holds the default EHX_GROUP_NONE" in cols
    assert "The labels land before the row count is published" in cols
    assert "no search ever sees a new row with a stale or default label" in cols
    assert "keeps its last value" in cols and "nothing is written" in cols
    assert "keeps its column values" in cols
    by = text[text.index("Partitioned kNN on a STORED column"):text.index("int ehx_knn_by_label_device(")]
    assert "ONE acquire-load snapshot n_pub" in by
    assert "byte for byte, what ehx_knn_labeled_device returns when given the stored column of that prefix with n_labels = n_pub" in by
    assert "0xFFFFFFFF is an ordinary label" in by
    assert "A stale index costs one rebuild" in by and "makes no pass over the column" in by
    grouped = text[text.index("Partitioned grouped kNN on STORED columns"):text.index("int ehx_knn_grouped_by_label_device(")]
    assert "ONE snapshot n_pub" in grouped and "byte for byte what ehx_knn_grouped_labeled_device returns" in grouped
    assert "EHX_GROUP_NONE: a group of its own" in grouped


def test_the_columns_of_the_gpu_tests():
    assert cc.INDEX_ROWS == (1, 255, 256, 257, 4097, 20000)
    for kind in cc.INDEX_KINDS:
        for n in cc.INDEX_ROWS:
            col = cc.index_column(kind, n)
            assert col.dtype == np.uint32 and len(col) == n
            perm, labels, start = cc.expected_index(col)
            assert (np.diff(labels.astype(np.int64)) > 0).all() and start[0] == 0 and start[-1] == n
            for i, lab in enumerate(labels[:50]):                      # a label's rows, ascending
                rows = perm[start[i]:start[i + 1]]
                assert (col[rows.astype(np.int64)] == lab).all() and (np.diff(rows.astype(np.int64)) > 0).all()
    assert cc.expected_passes(cc.index_column("one_label", 20000)) == 0
    assert cc.expected_passes(cc.index_column("random32", 20000)) == 4
    assert cc.expected_passes(cc.index_column("top_byte", 20000)) == 1
    assert cc.expected_passes(cc.index_column("descending", 20000)) == 2   # 0x2D7881 .. 0x2DC6C0: the two upper bytes are one value
    assert np.array_equal(cc.index_column("tenants", 20000), lbc.column())
    r = cc.index_column("random32", 4097)
    assert r[0] == 0 and (r == cc.NONE).any()
    cols, vals = marshal_columns({2: [1, 2, 3], 0: np.array([7, 8, cc.NONE], dtype=np.uint64)}, 3)
    assert cols.tolist() == [2, 0] and vals[1].dtype == np.uint32 and vals[1][2] == cc.NONE
    for bad in ({0: [1, 2]}, {0: [1.5, 2, 3]}, {0: [-1, 2, 3]}, {0: [2 ** 32, 2, 3]}):
        try:
            marshal_columns(bad, 3)
        except ValueError:
            continue
        raise AssertionError(bad)


def test_the_labelled_prefix_oracle_agrees_with_the_oracle_over_the_labelled_rows():
    from oracle import pyoracle
    rng = np.random.default_rng(1)
    X = rng.standard_normal((400, 8)).astype(np.float32)
    Q = rng.standard_normal((6, 8)).astype(np.float32)
    col = rng.integers(1, 3, size=400).astype(np.uint32)
    want = np.array([1, 2, 1, 2, 1, 2], dtype=np.uint32)
    bounds = [200, 300, 400]
    po = cc.LabelledPrefixOracle(X, col, Q, want, 5, pyoracle.METRIC_L2, bounds)
    for b in bounds:
        ids = np.zeros((6, 5), dtype=np.uint64)
        dist = np.zeros((6, 5), dtype=np.float32)
        cnt = np.zeros(6, dtype=np.uint32)
        for lab in (1, 2):
            rows = np.nonzero(col[:b] == lab)[0]
            at = np.nonzero(want == lab)[0]
            oi, od, oc = pyoracle.exhaustive(np.ascontiguousarray(X[rows]), np.ascontiguousarray(Q[at]), 5, pyoracle.METRIC_L2)
            ids[at], dist[at], cnt[at] = rows[oi.astype(np.int64)], od, oc
        assert po.assert_is_some_prefix(ids, dist, cnt, bounds[0], bounds[-1]) == b
    wrong = ids.copy()
    wrong[0, 0], wrong[0, 1] = ids[0, 1], ids[0, 0]
    try:
        po.assert_is_some_prefix(wrong, dist, cnt, bounds[0], bounds[-1])
    except AssertionError:
        return
    raise AssertionError("a swapped pair passed")


def test_colindex_kernels_use_no_scratch_spill_no_vector_registers_and_the_lds_designed_for(tmp_path):
    """the index build and the column writes: exactly these kernels, each once"""
    src = os.path.join(ehx_build.CSRC, "k_colindex.hip")
    flags = [f for f in ehx_build.FLAGS if f != "-shared"]
    r = subprocess.run([ehx_build.HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o",
                                                    str(tmp_path / "k_colindex.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    for kern in KERNELS:
        assert sum(kern in n for n in names) == 1, names
    assert len(names) == len(KERNELS)
    for what in ("ScratchSize \\[bytes/lane\\]", "VGPRs Spill"):
        vals = re.findall(what + r": (\d+)", r.stderr)
        assert len(vals) == len(names) and all(v == "0" for v in vals), (what, vals)
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(lds) == len(names)
    for name, size in zip(names, lds):
        kern = next(k for k in KERNELS if k in name)
        assert size == KERNELS[kern], (kern, size)
