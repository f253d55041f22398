"""CPU-side checks of the predicate searches on stored columns: the declarations, the ABI that stays as it was, the hooks that
stay out of it, what every new entry point answers to a NULL space without a device, the validation's codes, marshal_preds, the
helper's own columns and counts, and the resource usage of k_where.hip built for gfx950."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import masked_cases as mc
import where_cases as wc
from embeddinghub_amd import _lib
from embeddinghub_amd import build as ehx_build
from embeddinghub_amd.space import Space, marshal_preds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ehx_knn_where", "ehx_knn_where_device", "ehx_knn_grouped_where", "ehx_knn_grouped_where_device", "ehx_range_where",
       "ehx_range_where_device")
HOOKS = ("ehx_test_where_bitmaps", "ehx_test_where_check", "ehx_test_where_build_ms")
METHODS = ("knn_where", "knn_where_device", "knn_grouped_where", "knn_grouped_where_device", "range_where", "range_where_device")
KERNELS = {"where_bitmaps_kernel": 16640}   # kernel -> LDS bytes per workgroup, as k_where.hip's header states


def _header():
    return open(os.path.join(ROOT, "include", "ehx.h")).read()


def _check(preds_array, n):
    raw = C.CDLL(_lib.LIB_PATH)
    raw.ehx_test_where_check.restype = C.c_int
    return raw.ehx_test_where_check(preds_array, C.c_uint32(n))


def _table(n, n_terms=0, **term):
    t = (_lib.Pred * n)()
    for p in t:
        p.n_terms = n_terms
        for j in range(min(n_terms, _lib.PRED_MAX_TERMS)):
            p.terms[j] = _lib.Term(term.get("col", 0), term.get("lo", 0), term.get("hi", 0), term.get("flags", 0))
    return t


def test_entry_points_are_declared_bound_and_exported():
    header = _header()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS and hasattr(raw, name), name
    assert "k_where.hip" in ehx_build.SOURCES and "ehx_where.cpp" in ehx_build.SOURCES
    assert re.search(r"#define EHX_ABI_VERSION 5\b", header)   # additive: the version stays
    assert re.search(r"#define EHX_PRED_MAX_TERMS 8\b", header) and _lib.PRED_MAX_TERMS == 8 == wc.MAX_TERMS
    assert re.search(r"#define EHX_TERM_NOT 1u", header) and _lib.TERM_NOT == 1
    for name in METHODS:
        assert callable(getattr(Space, name)), name


def test_the_hooks_are_not_part_of_the_abi():
    raw = C.CDLL(_lib.LIB_PATH)
    for hook in HOOKS:
        assert hook not in _header() and hook not in _lib.SYMBOLS and hasattr(raw, hook), hook


def test_a_null_space_is_refused_before_the_device_is_looked_for():
    lib = _lib.load()
    q, r = (C.c_float * 4)(), (C.c_float * 1)(1.0)
    preds, of = _table(1), (C.c_uint32 * 1)(0)
    ids, dist, cnt, tot = (C.c_uint64 * 4)(), (C.c_float * 4)(), (C.c_uint32 * 1)(), (C.c_uint64 * 1)()
    calls = (lambda: lib.ehx_knn_where(None, 1, q, 4, preds, 1, of, ids, dist, cnt),
             lambda: lib.ehx_knn_where_device(None, None, 1, None, 4, preds, 1, None, None, None, None),
             lambda: lib.ehx_knn_grouped_where(None, 1, q, 4, 1, 0, preds, 1, of, ids, dist, cnt),
             lambda: lib.ehx_knn_grouped_where_device(None, None, 1, None, 4, 1, 0, preds, 1, None, None, None, None),
             lambda: lib.ehx_range_where(None, 1, q, r, 4, preds, 1, of, ids, dist, cnt, tot),
             lambda: lib.ehx_range_where_device(None, None, 1, None, None, 4, preds, 1, None, None, None, None, None))
    assert len(calls) == len(NEW)
    for call in calls:
        assert call() == _lib.EINVAL and lib.ehx_last_error() == b"space is NULL"   # with a device or without one


def test_the_validation_s_codes():
    assert _check(None, 1) == _lib.EINVAL                                     # NULL preds
    assert _check(_table(1), 0) == _lib.EINVAL                                # no predicate
    assert _check(_table(65), 65) == _lib.EUNSUPPORTED                        # the bitmap table's limit
    assert _check(_table(2, 9), 2) == _lib.EINVAL                             # n_terms above the limit
    assert _check(_table(2, 1, col=_lib.MAX_COLUMNS), 2) == _lib.EINVAL       # a column the space cannot have
    assert _check(_table(2, 1, flags=2), 2) == _lib.EINVAL                    # a flag bit other than NOT
    assert _check(_table(2, 1, flags=3), 2) == _lib.EINVAL
    bad_last = _table(64, 8, col=3, flags=1)
    bad_last[63].terms[7].col = 4                                             # the very last term of the very last predicate
    assert _check(bad_last, 64) == _lib.EINVAL
    # the limits: 64 predicates of 8 terms, the highest column, NOT, an empty range
    assert _check(_table(64, 8, col=3, lo=5, hi=4, flags=1), 64) == _lib.OK
    assert _check(_table(1, 0), 1) == _lib.OK
    assert _check(_table(1, 1, lo=0xFFFFFFFF, hi=0), 1) == _lib.OK


def test_marshal_preds():
    assert C.sizeof(_lib.Pred) == 132 and C.sizeof(_lib.Term) == 16 and _lib.Pred.terms.offset == 4
    t, n = marshal_preds(wc.TABLE)
    assert n == len(wc.TABLE) == 12 and C.sizeof(t) == 132 * 12
    assert _check(t, n) == _lib.OK
    eight = t[wc.NAMES.index("eight_terms")]
    assert eight.n_terms == 8 and eight.terms[6].flags == _lib.TERM_NOT and eight.terms[6].lo == 7 and eight.terms[7].col == 3
    assert eight.terms[7].lo == eight.terms[7].hi == 0xFFFFFFFF and t[wc.NAMES.index("no_terms")].n_terms == 0
    raw = np.frombuffer(bytes(t), dtype="<u4").reshape(12, 33)               # n_terms | 8 x (col, lo, hi, flags)
    assert raw[0].tolist()[:5] == [1, wc.A, 3, 3, 0]
    for tab in (wc.edge_preds(), wc.sixty_four()):
        t, n = marshal_preds(tab)
        assert _check(t, n) == _lib.OK
    assert marshal_preds([[(0, 1, 2)]] * 65)[1] == 65                        # EHX_EUNSUPPORTED is the C side's to say
    for bad in ([], [[(0, 0, 0)] * 9], [[(4, 0, 0)]], [[(-1, 0, 0)]], [[(0, -1, 0)]], [[(0, 0, 2 ** 32)]], [[(0, 0)]],
                [[(0, 0, 0, True, 1)]]):
        with pytest.raises(ValueError):
            marshal_preds(bad)


def test_the_header_states_the_contract():
    text = " ".join(_header().split()).replace(" * ", " ")
    part = text[text.index("predicate filters on stored columns"):text.index("int ehx_range_where(")]
    assert "ONE acquire-load snapshot n_pub" in part and "compared UNSIGNED" in part
    assert "A column never written reads as EHX_GROUP_NONE (0xFFFFFFFF) for every row" in part
    assert "lo > hi is an empty range: it never holds, and always holds under EHX_TERM_NOT" in part
    assert "n_terms == 0 allows every row" in part and "order-preserving map" in part
    assert "ehx_merge_topk_device" in part and "n_preds > 64: EHX_EUNSUPPORTED" in part
    assert "the graph walk under predicates is NOT built" in part
    assert "typedef struct ehx_term { uint32_t col, lo, hi, flags;" in part


def test_the_columns_and_counts_of_the_gpu_tests():
    cols = wc.columns()
    assert all(c.dtype == np.uint32 and len(c) == wc.N for c in cols.values()) and wc.NEVER not in cols
    assert (cols[wc.A] == np.arange(wc.N) % 16).all() and (cols[wc.B] == np.arange(wc.N)).all()
    assert (cols[wc.CC] >> 31).any() and not (cols[wc.CC] >> 31).all()
    tab = wc.table_truth()
    cnt = dict(zip(wc.NAMES, tab.sum(axis=1).tolist()))
    cut = mc.exact_cut(wc.N)
    assert cut == 1024 and cnt["a_is_3"] == 1250 > cut >= cnt["a_is_3_c_low"] > 0   # one batch holds both routes
    # a signed comparison would get c_middle wrong: its rows straddle 2^31
    c = cols[wc.CC][tab[wc.NAMES.index("c_middle")]]
    assert (c >= 0x80000000).any() and (c < 0x80000000).any()
    signed = (cols[wc.CC].view(np.int32) >= np.int32(0x40000000)) & (cols[wc.CC].view(np.int32) <= np.uint32(0xBFFFFFFF).view(np.int32))
    assert not signed.any()
    assert len(np.unique(wc.pred_of())) == len(wc.PREDS) and len(wc.pred_of()) == wc.NQ
    # the packed words: little-endian bits, a zero tail
    w = wc.packed(np.ones((2, 33), dtype=bool))
    assert w.tolist() == [[0xFFFFFFFF, 1], [0xFFFFFFFF, 1]]
    e = wc.bitmaps(wc.edge_preds(), {0: wc.edge_column(64)}, 64)
    assert e[wc.EDGES.index(0) * 4 + 3].all() and not e[1 * 4 + 0].any() and e[16 + 1 * 4 + 0].all()   # [0, max] | lo > hi | NOT
    assert wc.bitmaps(wc.sixty_four(), cols, 1025).shape == (64, 1025)
    assert wc.holds([(wc.NEVER, wc.NONE, wc.NONE)], {}, 5).all() and not wc.holds([(wc.NEVER, 0, 0)], {}, 5).any()


def test_where_kernel_uses_no_scratch_no_spill_and_the_lds_designed_for(tmp_path):
    """the bitmap build: exactly this kernel, once"""
    src = os.path.join(ehx_build.CSRC, "k_where.hip")
    flags = [f for f in ehx_build.FLAGS if f != "-shared"]
    r = subprocess.run([ehx_build.HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o",
                                                    str(tmp_path / "k_where.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    for kern in KERNELS:
        assert sum(kern in n for n in names) == 1, names
    assert len(names) == len(KERNELS)
    for what in ("ScratchSize \\[bytes/lane\\]", "VGPRs Spill", "SGPRs Spill"):
        vals = re.findall(what + r": (\d+)", r.stderr)
        assert len(vals) == len(names) and all(v == "0" for v in vals), (what, vals)
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert lds == [KERNELS["where_bitmaps_kernel"]]
    assert "16 640 bytes per workgroup" in open(src).read()
