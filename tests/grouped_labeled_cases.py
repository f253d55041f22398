"""Helper of the tests of the grouped kNN under a label column (no test here): the tenant column of the scan cases over
largek_cases.gauss(20000, 64, 64, 1) — three big tenants that take the scan route beside a hundred small ones — the wanted
tenants of its 64 queries, the cases the GPU test asserts "none handed on" for, and the model that clears them: the grouped
kNN under bitmaps' cascade (tests/grouped_masked_model.py) under the bitmap table that says what the wanted labels say — the
sample by rank over the tenant's ascending list, the unfiltered search's passes.  The sizes the tests rely on are asserted
here, where the column is made."""
import functools

import numpy as np

import grouped_masked_model as gmm
import grouped_model as gm
import labeled_cases as lbc
import masked_cases as mc

N_ROWS = 20000
BIG = (3, 5, 8)                       # the tenants that scan
BIG_ROWS = (6046, 5968, 6010)
SMALL0, N_SMALL = 1000, 100           # the small tenants: SMALL0 .. SMALL0 + N_SMALL - 1, 11 - 32 rows each
ABSENT = 7                            # no row carries it
METRICS = ("l2", "ip", "cosine")
SCAN_KS = (10, 100, 256)
SCAN_MS = (1, 4)
PASSES = 3                            # of a prefix of 16 385 .. 65 536 rows at the default growth


@functools.lru_cache(maxsize=None)
def tenant_column(n=N_ROWS):
    """uint32 [n]: tenants 3, 5 and 8 on about three tenths of the rows each, spread over the ids; every other row on one of
    N_SMALL small tenants"""
    rng = np.random.default_rng(23)
    u = rng.random(n)
    col = 1000 + rng.integers(0, 100, n)
    col[u < .3] = 3
    col[(.3 <= u) & (u < .6)] = 5
    col[(.6 <= u) & (u < .9)] = 8
    col = col.astype(np.uint32)
    if n == N_ROWS:
        cut = mc.exact_cut(n)
        assert cut == 1024
        assert tuple(int((col == t).sum()) for t in BIG) == BIG_ROWS and min(BIG_ROWS) > cut
        small = np.bincount(col[col >= SMALL0] - SMALL0, minlength=N_SMALL)
        assert len(small) == N_SMALL and small.min() == 11 and small.max() == 32
        assert not (col == ABSENT).any()
    col.setflags(write=False)
    return col


def scan_want(nq=64):
    """uint32 [nq]: scan query q wants BIG[q % 3]"""
    return np.array([BIG[q % 3] for q in range(nq)], dtype=np.uint32)


def small_want(n_more=36, seed=5):
    """uint32 [n_more]: further queries on small tenants (some of them on the same one)"""
    return (SMALL0 + np.random.default_rng(seed).integers(0, N_SMALL, n_more)).astype(np.uint32)


def as_table(col, want):
    """-> (bool [labels, rows], mask_of): labeled_cases.as_table — the bitmaps that allow what the wanted labels allow"""
    return lbc.as_table(np.asarray(col), np.asarray(want, dtype=np.uint32))


def expected(full, groups, col, want, k, m, n_eff=None):
    """The contract: the oracle's order, the rows of other tenants dropped, the plain-Python greedy over the rest"""
    col = np.asarray(col)
    allows, mask_of = as_table(col, want)
    if n_eff is None:
        n_eff = min(full[0].shape[1], len(groups), len(col))
    return gmm.expected(full, groups, allows, mask_of, k, m, n_eff=n_eff)


def scan_cases():
    return [(metric, lab, k, m) for metric in METRICS for lab in sorted(gm.LABELINGS) for k in SCAN_KS for m in SCAN_MS]


def scan_cascade(metric, lab, k, m):
    """-> (answers per query, worst pool fill per pass, unserved queries) of the scan route on the tenant column"""
    col, want = tenant_column(), scan_want()
    allows, mask_of = as_table(col, want)
    return gmm.scan_cascade(metric, gm.LABELINGS[lab](N_ROWS), allows, mask_of, k, m)


# The scan cases tests/test_knn_grouped_labeled.py asserts "all 64 on the scan route, none handed on, 3 passes" for: the
# ones the cascade clears — no unserved query and at most half a pool at every pass.  tests/test_knn_grouped_labeled_host.py
# re-derives this table from the model, case by case; none is left out.
NOT_CLEARED = set()


def cleared(metric, lab, k, m):
    return (metric, lab, k, m) not in NOT_CLEARED
