"""CPU-side checks of THE routing rule of the filtered searches (filter_routes_cut, filter_routes_gate: ehx_masked.cpp),
through the hook ehx_test_filter_routes, against the rule written out in numpy: a filter scans iff the scan serves and it
allows MORE than the cut's rows; with a gate, only if at least `min` queries of the batch name scanning filters — of all the
scanning filters together — else none scans; a null filter_of means every query is filter 0."""
import ctypes as C
import os

import numpy as np

from embeddinghub_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOK = "ehx_test_filter_routes"
CUT, MIN = 1024, 64


def model(scan_serves, cut, n_allowed, filter_of, nq, min_q):
    scans = np.logical_and(bool(scan_serves), np.asarray(n_allowed, dtype=np.uint64) > np.uint64(cut))
    if min_q and len(scans):
        of = np.zeros(nq, dtype=np.int64) if filter_of is None else np.asarray(filter_of, dtype=np.int64)
        if int(scans[of].sum()) < min_q:
            scans[:] = False
    return scans.astype(np.int8)


def routes(scan_serves, cut, n_allowed, filter_of, nq, min_q):
    _lib.load()   # (the library as every caller loads it: behind torch's HIP runtime where there is one)
    fn = getattr(C.CDLL(_lib.LIB_PATH), HOOK)
    fn.restype = None
    fn.argtypes = [C.c_int, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    a = np.ascontiguousarray(n_allowed, dtype=np.uint64)
    of = None if filter_of is None else np.ascontiguousarray(filter_of, dtype=np.uint32)
    assert of is None or len(of) == nq
    out = np.full(len(a) + 1, 7, dtype=np.int8)   # one guard byte behind the filters
    fn(int(scan_serves), cut, a.ctypes.data if len(a) else None, len(a), None if of is None else of.ctypes.data, nq, min_q,
       out.ctypes.data)
    assert out[-1] == 7
    return out[:-1]


def both(scan_serves, cut, n_allowed, filter_of, nq, min_q):
    got = routes(scan_serves, cut, n_allowed, filter_of, nq, min_q)
    assert got.tolist() == model(scan_serves, cut, n_allowed, filter_of, nq, min_q).tolist()
    return got.tolist()


def test_the_hook_is_not_part_of_the_abi():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    _lib.load()
    assert HOOK not in header and HOOK not in _lib.SYMBOLS and hasattr(C.CDLL(_lib.LIB_PATH), HOOK)


def test_the_cut_is_strict_and_the_scan_must_serve():
    sizes = [0, 1, CUT - 1, CUT, CUT + 1, 5 * CUT, 2**32 + 5]
    assert both(True, CUT, sizes, None, 0, 0) == [0, 0, 0, 0, 1, 1, 1]   # exactly the cut's rows: the list
    assert both(False, CUT, sizes, None, 0, 0) == [0] * len(sizes)
    assert both(True, 0, sizes, None, 0, 0) == [0, 1, 1, 1, 1, 1, 1]       # a forced scan route: every non-empty filter
    assert both(True, 2**64 - 1, sizes, None, 0, 0) == [0] * len(sizes)    # a forced list route


def test_the_gate_counts_the_queries_that_name_scanning_filters():
    sizes = [CUT + 1, CUT, 3 * CUT]   # filters 0 and 2 scan
    for n_naming, expect in ((MIN - 1, [0, 0, 0]), (MIN, [1, 0, 1])):
        of = np.array([0] * n_naming + [1] * 200, dtype=np.uint32)   # (however many queries name the listed one)
        assert both(True, CUT, sizes, of, len(of), MIN) == expect
        assert both(True, CUT, sizes, of[::-1], len(of), MIN) == expect
        assert both(True, CUT, sizes, of, len(of), 0) == [1, 0, 1]     # no gate
        assert both(False, CUT, sizes, of, len(of), MIN) == [0, 0, 0]
    # 63 queries on one scanning filter and 1 on another: 64 together, both scan
    of = np.array([0] * (MIN - 1) + [2] + [1] * 30, dtype=np.uint32)
    assert both(True, CUT, sizes, of, len(of), MIN) == [1, 0, 1]
    assert both(True, CUT, sizes, of[:-31], MIN - 1, MIN) == [0, 0, 0]


def test_a_null_filter_of_names_filter_0_for_every_query():
    for nq, expect in ((MIN - 1, 0), (MIN, 1), (MIN + 1, 1)):
        assert both(True, CUT, [CUT + 1], None, nq, MIN) == [expect]
        assert both(True, CUT, [CUT + 1, 9 * CUT], None, nq, MIN) == [expect, expect]   # (nobody names filter 1: it follows)
    assert both(True, CUT, [CUT, 9 * CUT], None, 500, MIN) == [0, 0]   # filter 0 is listed: no query names a scanning one


def test_no_filter_and_no_query():
    assert both(True, CUT, [], None, 0, 0) == [] and both(True, CUT, [], None, 0, MIN) == []
    assert both(True, CUT, [CUT + 1], None, 0, MIN) == [0] and both(True, CUT, [CUT + 1], None, 0, 0) == [1]


def test_seeded_batches_against_the_model():
    rng = np.random.default_rng(41)
    for _ in range(200):
        n_filters, nq = int(rng.integers(1, 65)), int(rng.integers(0, 200))
        sizes = rng.integers(CUT - 2, CUT + 3, size=n_filters)
        of = rng.integers(0, n_filters, size=nq).astype(np.uint32)
        both(bool(rng.integers(0, 4)), CUT, sizes, of, nq, int(rng.choice([0, 1, MIN])))
