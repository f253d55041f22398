"""Helper of the tests of the kNN under a table of bitmaps, one per query (no test here): the table and the queries' masks of
the int8 cases, shared by the CPU model (tests/test_masked_multi_model.py) and the GPU tests (tests/test_knn_masked_multi.py),
and a restatement of how ehx_masked.cpp routes the queries, orders them and cuts the ONE scan of a batch into passes.
Sample, exact cut and the pass cut are tests/masked_cases.py's."""
import functools

import numpy as np

import masked_cases as mc
import range_cases as rc

f32 = np.float32
MASK_SEED = 5211
NQ = 96                               # not a multiple of the 64 queries of a wave group
KS = (1, 10, 48)                      # the scan route's; EXACT_K takes every query to the exact route
EXACT_K = 60
NAMES = ("half", "tenth", "last_tenth", "few", "empty", "ones")
MAX_MASKS = 64
METRICS = ("cosine", "l2", "ip")


@functools.lru_cache(maxsize=None)
def table(n=rc.I8_ROWS):
    """bool [6, n]: density 0.5; density 0.1; only the last tenth of the ids; 300 rows (the exact route, in the same batch
    as scan-route queries); empty; all ones"""
    rng = np.random.default_rng(MASK_SEED)
    t = np.zeros((len(NAMES), n), dtype=bool)
    t[0] = rng.random(n) < 0.5
    t[1] = rng.random(n) < 0.1
    t[2] = np.arange(n) >= n - n // 10
    t[3, rng.choice(n, size=300, replace=False)] = True
    t[5] = True
    t.setflags(write=False)
    return t


def interleaved(nq, n_masks):
    """mask_of: neighbouring queries carry different masks"""
    return (np.arange(nq) % n_masks).astype(np.uint32)


def scans(tab, n_rows=None):
    """per mask: more allowed rows than the exact cut of a space of n_rows rows (default: the rows the bitmaps cover) —
    the scan route, where the space and k allow it"""
    return tab.sum(axis=1) > mc.exact_cut(tab.shape[1] if n_rows is None else n_rows)


def order(tab, mask_of):
    """the order ehx_masked.cpp answers the queries in: the scan route's first, then by mask; stable"""
    s = scans(tab)
    place = np.where(s[mask_of], 0, MAX_MASKS) + mask_of
    return np.argsort(place, kind="stable")


def passes(tab, mask_of):
    """[(first tile, tiles)] of the batch's ONE scan: pass j ends at the first tile where some scanned mask has seen
    256 * 16^j allowed rows — the pass cut of masked_cases over the pointwise maximum of the scanned masks' running counts"""
    used = [m for m in np.unique(mask_of) if scans(tab)[m]]
    assert used
    return mc.passes_over(np.max([mc.running(tab[m]) for m in used], axis=0))


def parity():
    """The wrong-mask case: every vector stored twice, at rows 2 j and 2 j + 1; mask A allows the even rows, mask B the odd
    ones; queries alternate A / B.  A flush or a re-rank that consults another query's bitmap returns an id of the wrong
    parity — at the very distance of the right one.  -> (rows [20 000, 128], queries [96, 128], table [2, 20 000], mask_of)"""
    X0, Q0 = rc.i8_data(128)
    n = rc.I8_ROWS
    X = np.repeat(X0[:n // 2], 2, axis=0)
    tab = np.zeros((2, n), dtype=bool)
    tab[0, 0::2] = True
    tab[1, 1::2] = True
    for a in (X, tab):
        a.setflags(write=False)
    return X, Q0[:NQ], tab, interleaved(NQ, 2)
