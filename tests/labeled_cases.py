"""Helper of the tests of the kNN under a label column (no test here): the seeded column over range_cases' int8 rows, the
batches of wanted labels, and the bitmap table that says the same as a batch (for the comparison with knn_masked_multi).
The sizes the tests rely on are asserted here, where the column is made."""
import functools

import numpy as np

import masked_cases as mc
import range_cases as rc

LABEL_SEED = 6121
NQ = 96                               # not a multiple of the 64 queries of a wave group
KS = (1, 10, 48, 60)                  # 60: above the scan route's k, every query takes the list route
HALF, TENTH, LAST, FEW = 7, 11, 13, 17
ABSENT = 5                            # no row carries it
ALL_ONES = 0xFFFFFFFF                 # an ordinary label here (EHX_GROUP_NONE elsewhere): ONE row carries it
ALL_ONES_ROW = 4321
SMALL0, N_SMALL = 1000, 200           # the small labels: SMALL0 .. SMALL0 + N_SMALL - 1
SPECIALS = (HALF, TENTH, LAST, FEW, ABSENT, ALL_ONES)
DENSE = (HALF, TENTH, LAST)
SHARED_RUN = 9                        # queries on ONE small label: at least the 8 that share a list-scan tile launch
SIDE_CHUNK = 2048                     # queries of one device batch (kSideChunk)


@functools.lru_cache(maxsize=None)
def column(n=rc.I8_ROWS):
    """uint32 [n]: HALF on about half of the rows and TENTH on about a tenth, both spread over the ids; LAST on the whole
    last tenth of the ids; FEW on 300 rows; ALL_ONES on one row; every other row on one of N_SMALL small labels"""
    rng = np.random.default_rng(LABEL_SEED)
    u = rng.random(n)
    col = (SMALL0 + rng.integers(0, N_SMALL, size=n)).astype(np.uint32)
    col[u < 0.5] = HALF
    col[(u >= 0.5) & (u < 0.6)] = TENTH
    col[n - n // 10:] = LAST
    rest = np.nonzero(col[:n - n // 10] >= SMALL0)[0]
    col[rng.choice(rest, size=300, replace=False)] = FEW
    assert col[ALL_ONES_ROW] != LAST
    col[ALL_ONES_ROW] = ALL_ONES
    if n == rc.I8_ROWS:
        cut = mc.exact_cut(n)
        assert cut == 1024
        size = lambda lab: int((col == lab).sum())  # noqa: E731
        assert 8500 < size(HALF) < 9500 and cut < size(TENTH) < 2200 and size(LAST) == n // 10 > cut
        assert 295 <= size(FEW) <= 300 and size(ALL_ONES) == 1 and size(ABSENT) == 0
        small = np.bincount(col[(col >= SMALL0) & (col < SMALL0 + N_SMALL)] - SMALL0, minlength=N_SMALL)
        assert small.min() >= 12 and small.max() <= 72   # a few dozen rows each
    col.setflags(write=False)
    return col


def _shuffled(want, seed):
    want = np.asarray(want, dtype=np.uint32)
    return want[np.random.default_rng(seed).permutation(len(want))]


def mixed_batch():
    """uint32 [NQ]: four queries on each of the six special labels, SHARED_RUN on one small label, every other query on a
    small label of its own — 70 distinct labels, more than a table of bitmaps takes; shuffled"""
    n_own = NQ - 4 * len(SPECIALS) - SHARED_RUN
    want = _shuffled(list(SPECIALS) * 4 + [SMALL0] * SHARED_RUN + [SMALL0 + 1 + i for i in range(n_own)], 1)
    assert len(want) == NQ and len(np.unique(want)) == len(SPECIALS) + 1 + n_own > 64
    return want


def table_batch():
    """uint32 [NQ] on at most 64 labels, the three dense ones among them: what a table of bitmaps can say too"""
    want = _shuffled(list(DENSE) * 12 + [FEW, ABSENT, ALL_ONES] * 4 + [SMALL0 + (i % 40) for i in range(NQ - 48)], 2)
    assert len(want) == NQ and len(np.unique(want)) == 46
    return want


def two_batches():
    """uint32 [SIDE_CHUNK + 64]: the specials, every small label and 100 labels nobody carries — about 300 distinct ones, the
    dense ones in both device batches"""
    nq = SIDE_CHUNK + 64
    pool = np.array(list(SPECIALS) + [SMALL0 + i for i in range(N_SMALL)] + [50000 + i for i in range(100)], dtype=np.uint32)
    base = pool[np.arange(nq) % len(pool)]
    tail = np.concatenate([np.repeat(np.array(DENSE, dtype=np.uint32), 3), base[SIDE_CHUNK:SIDE_CHUNK + 55]])
    want = np.concatenate([_shuffled(base[:SIDE_CHUNK], 3), _shuffled(tail, 4)])
    assert len(want) == nq and len(np.unique(want)) == len(pool) == 306
    for part in (want[:SIDE_CHUNK], want[SIDE_CHUNK:]):
        assert all((part == lab).any() for lab in DENSE)
    return want


def both_routes_batch():
    """uint32 [134]: 66 queries on the three dense labels (above the cut: they scan) and 68 on labels at or below it (FEW,
    ABSENT, ALL_ONES and 40 small ones: listed) — at least 64 on either side, so the grouped searches' 64-query gate lets
    the dense labels scan; shuffled.  -> (want, scans: bool per query, by the rule in numpy over column())"""
    want = _shuffled(list(DENSE) * 22 + [FEW] * 20 + [ABSENT, ALL_ONES] * 4 + [SMALL0 + i for i in range(40)], 5)
    col, cut = column(), mc.exact_cut(rc.I8_ROWS)
    assert cut == 1024
    rows = np.array([int((col == lab).sum()) for lab in want])
    scans = rows > cut
    assert sorted(set(want[scans].tolist())) == sorted(DENSE) and rows[~scans].max() <= 300 < cut
    assert int(scans.sum()) == 66 >= 64 and int((~scans).sum()) == 68 >= 64
    return want, scans


def as_table(col, want):
    """-> (bool [labels, rows], mask_of): the bitmaps that allow what the wanted labels allow, in ascending label order"""
    labs = np.unique(want)
    return col[None, :] == labs[:, None], np.searchsorted(labs, want).astype(np.uint32)
