"""CPU-side checks of the Boolean filters on stored columns: the declarations, the ABI that stays as it was, the hooks that stay
out of it, what every new entry point answers to a NULL space without a device, the validation's codes, marshal_filters, the
helper's own counts, and the resource usage of k_filter.hip built for gfx950."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import filter_cases as fc
import masked_cases as mc
import where_cases as wc
from embeddinghub_amd import _lib
from embeddinghub_amd import build as ehx_build
from embeddinghub_amd.space import FilterTable, Space, marshal_filter_table, marshal_filters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ehx_knn_filter", "ehx_knn_filter_device", "ehx_knn_grouped_filter", "ehx_knn_grouped_filter_device", "ehx_range_filter",
       "ehx_range_filter_device", "ehx_graph_knn_filter", "ehx_graph_knn_filter_device")
HOOKS = ("ehx_test_filter_bitmaps", "ehx_test_filter_check", "ehx_test_filter_build_ms")
METHODS = ("knn_filter", "knn_filter_device", "knn_grouped_filter", "knn_grouped_filter_device", "range_filter",
           "range_filter_device", "graph_knn_filter", "graph_knn_filter_device")
KERNELS = {"filter_bitmaps_kernel": 50176}   # kernel -> LDS bytes per workgroup, as k_filter.hip's header states
IN, NOT = _lib.TERM_IN, _lib.TERM_NOT


def _header():
    return open(os.path.join(ROOT, "include", "ehx.h")).read()


def _check(ft):
    raw = C.CDLL(_lib.LIB_PATH)
    raw.ehx_test_filter_check.restype = C.c_int
    raw.ehx_test_filter_check.argtypes = [C.POINTER(_lib.Filters)]
    return raw.ehx_test_filter_check(C.byref(ft) if ft is not None else None)


def _raw(n_clauses=1, n_terms=0, n_filters=1, run=(0, 1), n_values=0, **term):
    """an ehx_filters of n_clauses equal clauses of n_terms equal terms and n_filters equal runs; -> (struct, what it points into)"""
    cl = (_lib.Pred * max(n_clauses, 1))()
    for p in cl:
        p.n_terms = n_terms
        for j in range(min(n_terms, _lib.PRED_MAX_TERMS)):
            p.terms[j] = _lib.Term(term.get("col", 0), term.get("lo", 0), term.get("hi", 0), term.get("flags", 0))
    vals = (C.c_uint32 * max(n_values, 1))()
    fl = (_lib.Filter * max(n_filters, 1))()
    for f in fl:
        f.first_clause, f.n_clauses = run
    return _lib.Filters(cl, n_clauses, vals, n_values, fl, n_filters), (cl, vals, fl)


def test_entry_points_are_declared_bound_and_exported():
    header = _header()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS and hasattr(raw, name), name
    assert "k_filter.hip" in ehx_build.SOURCES and "ehx_filter.cpp" in ehx_build.SOURCES
    assert re.search(r"#define EHX_ABI_VERSION 5\b", header)   # additive: the version stays
    assert re.search(r"#define EHX_TERM_IN 2u", header) and _lib.TERM_IN == 2
    assert re.search(r"#define EHX_FILTER_MAX_CLAUSES 128\b", header) and _lib.FILTER_MAX_CLAUSES == 128 == fc.MAX_CLAUSES
    assert re.search(r"#define EHX_FILTER_MAX_VALUES 4096\b", header) and _lib.FILTER_MAX_VALUES == 4096 == fc.MAX_VALUES
    assert "typedef struct ehx_filter {" in header and "typedef struct ehx_filters {" in header
    # the new block stands behind ehx_range_where; the predicates' block keeps its sentences (tests/test_where_host.py)
    assert header.index("int ehx_range_where(") < header.index("#define EHX_TERM_IN") < header.index("int ehx_merge_topk_device(")
    for name in METHODS:
        assert callable(getattr(Space, name)), name


def test_the_hooks_are_not_part_of_the_abi():
    raw = C.CDLL(_lib.LIB_PATH)
    for hook in HOOKS:
        assert hook not in _header() and hook not in _lib.SYMBOLS and hasattr(raw, hook), hook


def test_a_null_space_is_refused_before_the_device_is_looked_for():
    lib = _lib.load()
    q, r = (C.c_float * 4)(), (C.c_float * 1)(1.0)
    ft, keep = _raw()
    f, of = C.byref(ft), (C.c_uint32 * 1)(0)
    ids, dist, cnt, tot = (C.c_uint64 * 4)(), (C.c_float * 4)(), (C.c_uint32 * 1)(), (C.c_uint64 * 1)()
    calls = (lambda: lib.ehx_knn_filter(None, 1, q, 4, f, of, ids, dist, cnt),
             lambda: lib.ehx_knn_filter_device(None, None, 1, None, 4, f, None, None, None, None),
             lambda: lib.ehx_knn_grouped_filter(None, 1, q, 4, 1, 0, f, of, ids, dist, cnt),
             lambda: lib.ehx_knn_grouped_filter_device(None, None, 1, None, 4, 1, 0, f, None, None, None, None),
             lambda: lib.ehx_range_filter(None, 1, q, r, 4, f, of, ids, dist, cnt, tot),
             lambda: lib.ehx_range_filter_device(None, None, 1, None, None, 4, f, None, None, None, None, None),
             lambda: lib.ehx_graph_knn_filter(None, 1, q, 4, f, of, 0, ids, dist, cnt),
             lambda: lib.ehx_graph_knn_filter_device(None, None, 1, None, 4, f, None, 0, None, None, None))
    assert len(calls) == len(NEW)
    for call in calls:
        assert call() == _lib.EINVAL and lib.ehx_last_error() == b"space is NULL"   # with a device or without one
    del keep


def test_the_validation_s_codes():
    ok, inval, unsup = _lib.OK, _lib.EINVAL, _lib.EUNSUPPORTED
    assert _check(None) == inval                                                # a NULL table
    for hole in ("clauses", "filters", "values"):                               # NULL where a count says there are some
        ft, keep = _raw(1, 1, 1, n_values=4, flags=IN, lo=0, hi=4)
        assert _check(ft) == ok
        setattr(ft, hole, None)
        assert _check(ft) == inval, hole
    ft, keep = _raw(0, 0, 1, run=(0, 0))                                        # ... and none where it says there are none
    ft.clauses, ft.values = None, None
    assert _check(ft) == ok
    assert _check(_raw(1, 0, 0)[0]) == inval                                    # no filter
    assert _check(_raw(1, 0, 64)[0]) == ok and _check(_raw(1, 0, 65)[0]) == unsup          # the bitmap table's limit
    assert _check(_raw(128, 0, 1, run=(0, 128))[0]) == ok and _check(_raw(129, 0, 1)[0]) == unsup
    assert _check(_raw(4, 0, 2, run=(3, 1))[0]) == ok                           # a run that ends at n_clauses
    assert _check(_raw(4, 0, 2, run=(3, 2))[0]) == inval                        # ... and one past it
    assert _check(_raw(4, 0, 2, run=(5, 0))[0]) == inval
    assert _check(_raw(4, 0, 2, run=(0xFFFFFFFF, 2))[0]) == inval               # (no wrap-around)
    assert _check(_raw(2, 8)[0]) == ok and _check(_raw(2, 9)[0]) == inval        # n_terms
    assert _check(_raw(2, 1, col=_lib.MAX_COLUMNS - 1)[0]) == ok
    assert _check(_raw(2, 1, col=_lib.MAX_COLUMNS)[0]) == inval                  # a column the space cannot have
    for flags, code in ((0, ok), (NOT, ok), (IN, ok), (IN | NOT, ok), (4, inval), (IN | 4, inval), (0x80000000, inval)):
        assert _check(_raw(2, 1, flags=flags)[0]) == code, flags
    # an IN term's values: inside, at the end, one past it, wrapping
    assert _check(_raw(1, 1, n_values=8, flags=IN, lo=3, hi=5)[0]) == ok
    assert _check(_raw(1, 1, n_values=8, flags=IN, lo=8, hi=0)[0]) == ok
    assert _check(_raw(1, 1, n_values=8, flags=IN, lo=4, hi=5)[0]) == inval
    assert _check(_raw(1, 1, n_values=8, flags=IN, lo=9, hi=0)[0]) == inval
    assert _check(_raw(1, 1, n_values=8, flags=IN, lo=0xFFFFFFFF, hi=2)[0]) == inval
    assert _check(_raw(1, 1, n_values=8, flags=0, lo=0xFFFFFFFF, hi=2)[0]) == ok   # (a range term's ends are no indices)
    # the values summed over the IN terms: 4096, and one more
    assert _check(_raw(128, 1, n_values=32, flags=IN, lo=0, hi=32)[0]) == ok
    assert _check(_raw(128, 8, n_values=4, flags=IN | NOT, lo=0, hi=4)[0]) == ok
    ft, keep = _raw(128, 1, n_values=33, flags=IN, lo=0, hi=32)
    ft.clauses[127].terms[0].hi = 33
    assert _check(ft) == unsup
    assert _check(_raw(1, 1, n_values=5000, flags=IN, lo=0, hi=4096)[0]) == ok
    assert _check(_raw(1, 1, n_values=5000, flags=IN, lo=0, hi=4097)[0]) == unsup
    # the very last term of the very last clause
    for field, bad in (("col", 4), ("flags", 4), ("hi", 5)):
        ft, keep = _raw(128, 8, 64, run=(126, 2), n_values=4, col=3, flags=IN | NOT, lo=0, hi=4)
        assert _check(ft) == ok
        setattr(ft.clauses[127].terms[7], field, bad)
        assert _check(ft) == inval, field
    # ehx_knn_where's own validation still refuses the new flag
    raw = C.CDLL(_lib.LIB_PATH)
    raw.ehx_test_where_check.restype = C.c_int
    t = (_lib.Pred * 1)()
    t[0].n_terms = 1
    t[0].terms[0] = _lib.Term(0, 0, 0, IN)
    assert raw.ehx_test_where_check(t, C.c_uint32(1)) == inval


def test_marshal_filters():
    assert C.sizeof(_lib.Filter) == 8 and _lib.Filters.n_clauses.offset == 8 and _lib.Filters.n_filters.offset == 40
    assert C.sizeof(_lib.Filters) == 48
    ft = marshal_filters(fc.TABLE)
    assert isinstance(ft, FilterTable) and ft.n_filters == len(fc.TABLE) == 12 and _check(ft.struct) == _lib.OK
    assert ft.n_clauses == sum(len(f) for f in fc.TABLE) == 77
    runs = [(r.first_clause, r.n_clauses) for r in ft.runs]
    assert runs[:3] == [(0, 1), (1, 2), (3, 1)] and runs[fc.NAMES.index("no_clause")][1] == 0
    assert runs[fc.NAMES.index("windows")][1] == 64
    # round trip: the struct reads back as the clauses given
    s = ft.struct
    assert (s.n_clauses, s.n_values, s.n_filters) == (ft.n_clauses, ft.n_values, 12)
    a_in = s.clauses[0]
    assert a_in.n_terms == 1 and a_in.terms[0].flags == IN and a_in.terms[0].col == fc.A
    t = a_in.terms[0]
    assert [s.values[t.lo + i] for i in range(t.hi)] == [3, 7, 11]            # packed: sorted and unique
    late = s.clauses[2].terms[0]
    assert (late.col, late.lo, late.hi, late.flags) == (fc.B, 18000, fc.NONE, 0)
    not_in = s.clauses[runs[fc.NAMES.index("not_in")][0]].terms[0]
    assert not_in.flags == IN | NOT and not_in.hi == 14
    empty = s.clauses[runs[fc.NAMES.index("in_empty")][0]].terms[0]
    assert empty.hi == 0 and empty.flags == IN
    # every set is sorted and strictly increasing, and the sets lie back to back
    at = 0
    for c in range(s.n_clauses):
        for j in range(s.clauses[c].n_terms):
            t = s.clauses[c].terms[j]
            if t.flags & IN:
                v = [s.values[t.lo + i] for i in range(t.hi)]
                assert t.lo == at and v == sorted(set(v))
                at += t.hi
    assert at == s.n_values
    # pack=False: as given
    raw = marshal_filters(fc.TABLE[:1], pack=False)
    assert raw.values.tolist() == [11, 3, 7, 3] and _check(raw.struct) == _lib.OK
    # shared clauses, and every limit at once
    ov = marshal_filter_table(*fc.overlapping())
    assert [(r.first_clause, r.n_clauses) for r in ov.runs] == [(0, 2), (1, 2)] and ov.n_clauses == 3 and _check(ov.struct) == _lib.OK
    lim = marshal_filter_table(*fc.limits(), pack=False)
    assert (lim.n_filters, lim.n_clauses, lim.n_values) == (64, 128, 4096) and lim.struct.clauses[127].n_terms == 8
    assert _check(lim.struct) == _lib.OK
    for tab in (fc.edge_filters(), [f for n in fc.SET_LENGTHS for f in fc.set_filters(n)]):
        assert _check(marshal_filters(tab).struct) == _lib.OK
    # EHX_EUNSUPPORTED is the C side's to say
    assert _check(marshal_filters([[[(0, 1, 2)]]] * 65).struct) == _lib.EUNSUPPORTED
    assert _check(marshal_filters([[[(0, 1, 2)]] * 129]).struct) == _lib.EUNSUPPORTED
    assert _check(marshal_filters([[[(0, "in", range(4097))]]]).struct) == _lib.EUNSUPPORTED
    for bad in ([], [[[(0, 0, 0)] * 9]], [[[(4, 0, 0)]]], [[[(-1, 0, 0)]]], [[[(0, -1, 0)]]], [[[(0, 0, 2 ** 32)]]], [[[(0, 0)]]],
                [[[(0, 0, 0, True, 1)]]], [[[(0, "in", [2 ** 32])]]], [[[(0, "in", [-1])]]], [[[(0, "of", [1])]]],
                [[[(4, "in", [1])]]]):
        with pytest.raises(ValueError):
            marshal_filters(bad)
    for clauses, runs in (([[(0, 0, 0)]], [(0, 2)]), ([[(0, 0, 0)]], [(1, 1)]), ([[(0, 0, 0)]], [(-1, 1)]), ([[(0, 0, 0)]], [])):
        with pytest.raises(ValueError):
            marshal_filter_table(clauses, runs)


def test_the_header_states_the_contract():
    text = " ".join(_header().split()).replace(" * ", " ")
    part = text[text.index("Boolean filters on stored columns"):text.index("int ehx_graph_knn_filter(")]
    assert "ONE acquire-load snapshot n_pub" in part and "DISJUNCTION of clauses" in part
    assert "hi == 0 is the empty set: it never holds, and always holds under EHX_TERM_NOT" in part
    assert "need not be sorted or distinct" in part and "runs of different filters may overlap" in part
    assert "n_clauses == 0 is the empty disjunction: it allows no row" in part and "it is returned once" in part
    assert "ehx_graph_knn_masked_multi_device" in part and "n_filters > 64" in part and "EHX_EUNSUPPORTED" in part
    assert "ehx_knn_where* keep refusing every flag bit but EHX_TERM_NOT" in part


def test_the_counts_of_the_gpu_tests():
    cols = wc.columns()
    tab = fc.table_truth()                                                      # (asserts the stated counts itself)
    cnt = dict(zip(fc.NAMES, tab.sum(axis=1).tolist()))
    assert cnt == fc.COUNTS
    cut = mc.exact_cut(fc.N)
    assert cut == 1024 == cnt["b_1024"] and cnt["mixed_exact"] <= cut < cnt["mixed_scan"] and cnt["small_in"] == 3
    both = (cols[fc.A] == 3) & (cols[fc.B] >= 18000)
    assert both.sum() == fc.COMMON and (tab[fc.NAMES.index("a3_or_late")] == ((cols[fc.A] == 3) | (cols[fc.B] >= 18000))).all()
    assert len(np.unique(fc.filter_of())) == len(fc.FILTERS) and len(fc.filter_of()) == fc.NQ
    # one-clause filters without IN terms are where_cases' predicates
    assert (fc.bitmaps([[p] for p in wc.TABLE], cols, fc.N) == wc.table_truth()).all()
    # the membership test is unsigned, a never-written column reads as NONE, NOT inverts, an empty set never holds
    e = {0: wc.edge_column(64)}
    got = fc.bitmaps(fc.edge_filters(), e, 64)
    assert got[0].sum() == 8 and (got[0] == (e[0] == 0)).all() and (got[3] == (e[0] == 0xFFFFFFFF)).all()
    assert (got[12:] == ~got[:12]).all()
    assert fc.term_holds((3, "in", [fc.NONE]), {}, 5).all() and not fc.term_holds((3, "in", []), {}, 5).any()
    assert fc.term_holds((3, "in", [], True), {}, 5).all()
    cl, runs = fc.overlapping()
    ov = fc.run_bitmaps(cl, runs, cols, fc.N)
    cb = fc.clause_bitmaps(cl, cols, fc.N)
    assert (ov[0] == (cb[0] | cb[1])).all() and (ov[1] == (cb[1] | cb[2])).all() and cb[1].sum() == 5
    cl, runs = fc.limits()
    lim = fc.run_bitmaps(cl, runs, cols, 1025)
    assert lim.shape == (64, 1025) and lim.any(axis=1).all()
    for n in fc.SET_LENGTHS:
        a, b = fc.bitmaps(fc.set_filters(n), cols, fc.N)
        assert a.sum() <= n and (a ^ b).all() and (n == 0 or a.sum() > 0)


def test_filter_kernel_uses_no_scratch_no_spill_and_the_lds_designed_for(tmp_path):
    """the bitmap build: exactly this kernel, once"""
    src = os.path.join(ehx_build.CSRC, "k_filter.hip")
    flags = [f for f in ehx_build.FLAGS if f != "-shared"]
    r = subprocess.run([ehx_build.HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o",
                                                    str(tmp_path / "k_filter.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    for kern in KERNELS:
        assert sum(kern in n for n in names) == 1, names
    assert len(names) == len(KERNELS)
    for what in ("ScratchSize \\[bytes/lane\\]", "VGPRs Spill", "SGPRs Spill"):
        vals = re.findall(what + r": (\d+)", r.stderr)
        assert len(vals) == len(names) and all(v == "0" for v in vals), (what, vals)
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert lds == [KERNELS["filter_bitmaps_kernel"]] and lds[0] <= 65536
    assert "50 176 bytes per workgroup" in open(src).read()
