"""Helper of the tests of the predicate searches on stored columns (no test here): the columns and the predicate table of
the int8 cases, the numpy truth of a predicate (unsigned, a column never written reading as 0xFFFFFFFF), the packed words a
table of predicates must give, and the edge-value and 64-predicate tables of the bitmap test.  Shared by the CPU checks
(tests/test_where_host.py) and the GPU tests (tests/test_where.py).  Data and queries: tests/range_cases.py's int8 cases,
tests/masked_multi_cases.py's 96 queries."""
import functools

import numpy as np

import masked_multi_cases as mmc
import range_cases as rc

NONE = 0xFFFFFFFF
MAX_COLUMNS, MAX_TERMS, MAX_PREDS = 4, 8, 64
N = rc.I8_ROWS
NQ = mmc.NQ
COL_SEED = 7241
A, B, CC, NEVER = 0, 1, 2, 3   # the columns: row % 16 | the row id, a timestamp | seeded random 32-bit | never written
BITMAP_ROWS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1025, 20000)
EDGES = (0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)


@functools.lru_cache(maxsize=None)
def columns(n=N):
    """{column number: u32 [n]} of the three written columns"""
    rng = np.random.default_rng(COL_SEED)
    cols = {A: (np.arange(n) % 16).astype(np.uint32), B: np.arange(n, dtype=np.uint32),
            CC: rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)}
    for c in cols.values():
        c.setflags(write=False)
    return cols


# name -> predicate: a list of (col, lo, hi) or (col, lo, hi, True) for NOT
PREDS = (
    ("a_is_3", [(A, 3, 3)]),                                               # 1250 rows: the scan route
    ("late", [(B, 18000, NONE)]),                                          # 2000 rows, clustered late
    ("c_middle", [(CC, 0x40000000, 0xBFFFFFFF)]),                          # about half: a signed comparison gets this wrong
    ("a_is_3_c_low", [(A, 3, 3), (CC, 0, 0x7FFFFFFF)]),                    # about 625: the exact route, in the same batch
    ("not_a_2_13", [(A, 2, 13, True)]),                                    # 5000: negation of a range
    ("a_is_3_and_not", [(A, 3, 3), (A, 3, 3, True)]),                      # 0: empty, for its queries only
    ("no_terms", []),                                                      # everything
    ("lo_above_hi", [(A, 5, 4)]),                                          # 0: an empty range
    ("not_lo_above_hi", [(A, 5, 4, True)]),                                # everything: a negated empty range
    ("eight_terms", [(A, 1, NONE), (A, 0, 14), (B, 1000, NONE), (B, 0, 19000), (CC, 0x10000000, NONE), (CC, 0, 0xF0000000),
                     (A, 7, 7, True), (NEVER, NONE, NONE)]),               # the term limit
    ("never_is_none", [(NEVER, NONE, NONE)]),                              # a column never written matches its default
    ("never_is_0", [(NEVER, 0, 0)]),                                       # ... and nothing else
)
NAMES = tuple(name for name, _ in PREDS)
TABLE = [p for _, p in PREDS]


def holds(pred, cols, n):
    """bool [n]: the rows predicate `pred` allows.  cols: {column: u32 values, at least n}; a column that is missing reads as
    NONE for every row.  The comparison is unsigned: the values are widened to u64."""
    ok = np.ones(n, dtype=bool)
    for term in pred:
        col, lo, hi = int(term[0]), int(term[1]), int(term[2])
        v = (np.asarray(cols[col][:n], dtype=np.uint32) if col in cols else np.full(n, NONE, dtype=np.uint32)).astype(np.uint64)
        inside = (v >= np.uint64(lo)) & (v <= np.uint64(hi))
        ok &= ~inside if len(term) == 4 and term[3] else inside
    return ok


def bitmaps(preds, cols, n):
    """bool [n_preds, n]: the numpy truth of a table of predicates"""
    return np.stack([holds(p, cols, n) for p in preds]) if len(preds) else np.zeros((0, n), dtype=bool)


def packed(tab):
    """u32 [n_preds, ceil(n / 32)]: bit r & 31 of word r >> 5, the tail of the last word zero"""
    n_preds, n = tab.shape
    bits = np.zeros((n_preds, (n + 31) // 32 * 32), dtype=np.uint8)
    bits[:, :n] = tab
    return np.packbits(bits, axis=1, bitorder="little").view("<u4").astype(np.uint32).reshape(n_preds, -1)


@functools.lru_cache(maxsize=None)
def table_truth(n=N):
    """bool [12, n] of TABLE over columns(), with the allowed counts the issue states asserted"""
    tab = bitmaps(TABLE, columns(N), n)
    if n == N:
        cnt = dict(zip(NAMES, tab.sum(axis=1).tolist()))
        assert cnt["a_is_3"] == 1250 and cnt["late"] == 2000 and cnt["not_a_2_13"] == 5000
        assert cnt["a_is_3_and_not"] == 0 and cnt["lo_above_hi"] == 0 and cnt["never_is_0"] == 0
        assert cnt["no_terms"] == cnt["not_lo_above_hi"] == cnt["never_is_none"] == N
        assert 9000 < cnt["c_middle"] < 11000 and 500 < cnt["a_is_3_c_low"] <= 1024 < cnt["a_is_3"]   # both routes in one batch
        assert 0 < cnt["eight_terms"] < N
    tab.setflags(write=False)
    return tab


def pred_of(nq=NQ, n_preds=len(PREDS)):
    """neighbouring queries carry different predicates"""
    return mmc.interleaved(nq, n_preds)


def edge_column(n):
    """values at and beside 0, 2^31 and 2^32 - 1, cycling"""
    vals = np.array([0, 1, 0x7FFFFFFE, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)
    return vals[np.arange(n) % len(vals)]


def edge_preds(col=0):
    """every pair of EDGES as a range's ends (the empty ones included), plain and negated, and the values beside them"""
    out = [[(col, lo, hi)] for lo in EDGES for hi in EDGES]
    out += [[(col, lo, hi, True)] for lo in EDGES for hi in EDGES]
    out += [[(col, 1, 0xFFFFFFFE)], [(col, 0x7FFFFFFF, 0x7FFFFFFF), (col, 0x80000000, 0x80000000, True)]]
    assert len(out) <= MAX_PREDS
    return out


def sixty_four():
    """64 predicates at once: TABLE, equality on every value of A, and windows of B and C"""
    out = list(TABLE) + [[(A, v, v)] for v in range(16)]
    out += [[(B, 300 * j, 300 * j + 1000 + 7 * j)] for j in range(18)]
    out += [[(CC, j << 28, ((j + 3) << 28) - 1), (A, j % 16, 15)] for j in range(13)]
    out += [[(B, 31, 33), (A, 0, 1, True)]] * (MAX_PREDS - len(out))
    assert len(out) == MAX_PREDS
    return out
