"""Helper of the tests of the Boolean filters on stored columns (no test here): the numpy truth of a table of filters — OR of
clauses, a clause an AND of range terms (where_cases.holds) and IN terms — the table of twelve filters of the int8 cases with
the allowed counts checked on the CPU, a pair of filters whose runs overlap, and a table at every limit at once.  Shared by the
CPU checks (tests/test_filter_host.py) and the GPU tests (tests/test_filter.py).  Columns, rows and queries are
tests/where_cases.py's: 20 000 rows, A = row % 16, B = the row id, CC seeded random, NEVER unwritten; 96 queries.

A filter is a list of clauses, a clause a list of terms, a term (col, lo, hi[, negate]) or (col, "in", values[, negate])."""
import functools

import numpy as np

import masked_multi_cases as mmc
import where_cases as wc

NONE = wc.NONE
A, B, CC, NEVER = wc.A, wc.B, wc.CC, wc.NEVER
N, NQ = wc.N, wc.NQ
MAX_FILTERS, MAX_CLAUSES, MAX_VALUES, MAX_TERMS = 64, 128, 4096, 8
BITMAP_ROWS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 20000)
SET_LENGTHS = (0, 1, 2, 3, 63, 64, 65, 1024)

# name -> (filter, rows it allows of the 20 000)
FILTERS = (
    ("a_in", [[(A, "in", [11, 3, 7, 3])]], 3750),                            # unsorted and duplicated as given; scan route
    ("a3_or_late", [[(A, 3, 3)], [(B, 18000, NONE)]], 3125),                 # 125 rows satisfy both and must appear once
    ("small_in", [[(B, "in", [5, 19999, 20000, 77])]], 3),                   # exact route, count 3 < k
    ("not_in", [[(A, "in", list(range(14)), True)]], 2500),
    ("mixed_exact", [[(A, "in", [1]), (CC, 0, 0x3FFFFFFF)], [(A, 9, 9), (B, 0, 999)]], 398),   # exact beside scan in one batch
    ("mixed_scan", [[(A, "in", [1, 2]), (CC, 0, 0x7FFFFFFF)], [(A, 9, 9), (B, 0, 999)]], 1319),
    ("b_1024", [[(B, "in", [16 * j + 5 for j in range(1024)])]], 1024),      # exactly the cut; a 1024-value set
    ("windows", [[(B, 300 * j, 300 * j + 99)] for j in range(64)], 6400),
    ("no_clause", [], 0),                                                    # the empty disjunction
    ("in_empty", [[(A, "in", [])]], 0),
    ("not_in_empty", [[(A, "in", [], True)]], N),
    ("never_in", [[(NEVER, "in", [0, NONE])]], N),
)
NAMES = tuple(name for name, _, _ in FILTERS)
TABLE = [f for _, f, _ in FILTERS]
COUNTS = {name: cnt for name, _, cnt in FILTERS}
COMMON = 125   # rows both clauses of a3_or_late allow


def term_holds(term, cols, n):
    """bool [n]: one term; an IN term by membership (unsigned), a range term as where_cases.holds has it"""
    if not isinstance(term[1], str):
        return wc.holds([term], cols, n)
    col = int(term[0])
    v = np.asarray(cols[col][:n], dtype=np.uint32) if col in cols else np.full(n, NONE, dtype=np.uint32)
    inside = np.isin(v.astype(np.uint64), np.asarray([int(x) for x in term[2]], dtype=np.uint64))
    return ~inside if len(term) == 4 and term[3] else inside


def clause_holds(clause, cols, n):
    ok = np.ones(n, dtype=bool)
    for term in clause:
        ok &= term_holds(term, cols, n)
    return ok


def clause_bitmaps(clauses, cols, n):
    return np.stack([clause_holds(c, cols, n) for c in clauses]) if len(clauses) else np.zeros((0, n), dtype=bool)


def run_bitmaps(clauses, runs, cols, n):
    """bool [n_filters, n]: filter f the OR of clauses[first, first + cnt) of runs[f]"""
    cb = clause_bitmaps(clauses, cols, n)
    return np.stack([cb[first:first + cnt].any(axis=0) if cnt else np.zeros(n, dtype=bool) for first, cnt in runs])


def bitmaps(filters, cols, n):
    """bool [n_filters, n]: the numpy truth of a list of filters"""
    return np.stack([clause_bitmaps(f, cols, n).any(axis=0) if len(f) else np.zeros(n, dtype=bool) for f in filters])


@functools.lru_cache(maxsize=None)
def table_truth(n=N):
    """bool [12, n] of TABLE over where_cases.columns(), the stated counts asserted at the full size"""
    tab = bitmaps(TABLE, wc.columns(N), n)
    if n == N:
        cnt = dict(zip(NAMES, tab.sum(axis=1).tolist()))
        assert cnt == COUNTS, cnt
        cols = wc.columns(N)
        assert int(((cols[A] == 3) & (cols[B] >= 18000)).sum()) == COMMON
        assert cnt["a3_or_late"] == 1250 + 2000 - COMMON
    tab.setflags(write=False)
    return tab


def filter_of(nq=NQ, n_filters=len(FILTERS)):
    """neighbouring queries carry different filters"""
    return mmc.interleaved(nq, n_filters)


def overlapping():
    """(clauses, runs): two filters sharing the middle clause — runs (first 0, n 2) and (first 1, n 2)"""
    return [[(A, 3, 3)], [(B, "in", [7, 19, 4000, 4001, 19999])], [(CC, 0x80000000, NONE), (A, 0, 7, True)]], [(0, 2), (1, 2)]


def limits():
    """(clauses, runs) at every limit at once: 64 filters of two clauses each, 128 clauses, 4096 values in total (32 per clause,
    distinct within a set, given unsorted), 8 terms in the last clause"""
    rng = np.random.default_rng(6007)
    clauses = []
    for c in range(MAX_CLAUSES):
        if c % 2 == 0:   # two values of A that occur, thirty that cannot
            vals = [c % 16, (c + 5) % 16] + [int(v) for v in rng.choice(np.arange(16, 1 << 20), size=30, replace=False)]
            vals = [vals[i] for i in rng.permutation(32)]
            clauses.append([(A, "in", vals)])
        else:
            clauses.append([(B, "in", [int(v) for v in rng.choice(N + 500, size=32, replace=False)], c % 4 == 3)])
    every_a = [int(v) for v in rng.permutation(32)]   # holds for every written row
    clauses[-1] = [(A, "in", every_a), (A, 0, 14), (B, 1000, NONE), (B, 0, 19000), (CC, 0x10000000, NONE), (CC, 0, 0xF0000000),
                   (A, 7, 7, True), (NEVER, NONE, NONE)]
    runs = [(2 * f, 2) for f in range(MAX_FILTERS)]
    assert len(clauses) == MAX_CLAUSES and len(clauses[-1]) == MAX_TERMS
    assert sum(len(t[2]) for c in clauses for t in c if isinstance(t[1], str)) == MAX_VALUES
    return clauses, runs


def set_filters(length, seed=0):
    """B IN / NOT IN a set of `length` row ids (the first a row of every space of 1 row or more, some beyond the rows), as
    filters of one clause"""
    rng = np.random.default_rng(1000 + length + seed)
    vals = ([0] + [int(v) for v in rng.choice(np.arange(1, N + N // 4), size=length - 1, replace=False)]) if length else []
    return [[[(B, "in", vals)]], [[(B, "in", vals, True)]]]


def edge_filters(col=0):
    """IN and NOT IN over 0, 2^31 - 1, 2^31, 2^32 - 1 and their neighbours, on where_cases.edge_column"""
    near = [1, 0x7FFFFFFE, 0x80000001, 0xFFFFFFFE]
    sets = [[e] for e in wc.EDGES] + [[v] for v in near] + [list(wc.EDGES), near, list(wc.EDGES) + near, [0x80000000, 0x7FFFFFFF]]
    return [[[(col, "in", s)]] for s in sets] + [[[(col, "in", s, True)]] for s in sets]
