"""Helper of the masked-kNN tests (no test here): the bitmaps of the int8 cases, shared by the CPU model
(tests/test_masked_model.py) and the GPU tests (tests/test_knn_masked.py), and a restatement of how ehx_masked.cpp samples
the allowed rows and cuts the scan into passes."""
import numpy as np

MASK_SEED = 4177                      # the random bitmaps of the cases below
SAMPLE = 256                          # allowed rows in the sample, at most (kMaskedSample)
GROWTH = 16                           # pass j ends where SAMPLE * GROWTH^j allowed rows have been seen
TILE = 256
POOL_CAP = 4096                       # kPoolCap
SCAN_MAX_K = 48
KS = (1, 10, 48)
# scan passes per query batch over range_cases.I8_ROWS = 20 000 rows: 10 000 allowed -> [0, 4096 seen) | the rest;
# 2 000 allowed -> one pass (4096 is never reached); 20 000 -> two
PASSES = {"half": 2, "tenth": 1, "tail": 2, "ones": 2}


def masks(n):
    """name -> bool [n]: 50 % random, 10 % random, the upper half of the ids, every row"""
    rng = np.random.default_rng(MASK_SEED)
    out = {"half": rng.random(n) < 0.5, "tenth": rng.random(n) < 0.1, "tail": np.arange(n) >= n // 2,
           "ones": np.ones(n, dtype=bool)}
    for m in out.values():
        m.setflags(write=False)
    return out


def exact_cut(n_rows):
    """at most this many allowed rows: the exact route"""
    return max(1024, n_rows // 128)


def sample_ids(allowed):
    """every ceil(n_allowed / 256)-th allowed id by rank"""
    L = np.nonzero(allowed)[0]
    stride = (len(L) + SAMPLE - 1) // SAMPLE
    return L[::stride]


def passes(allowed):
    """[(first tile, tiles)] of the scan passes (masked_passes, ehx_masked.cpp)"""
    n = len(allowed)
    n_tiles = (n + TILE - 1) // TILE
    pad = np.zeros(n_tiles * TILE, dtype=np.int64)
    pad[:n] = allowed
    cum = np.concatenate([[0], np.cumsum(pad.reshape(n_tiles, TILE).sum(axis=1))])
    out, t0, want = [], 0, SAMPLE * GROWTH
    while t0 < n_tiles:
        reach = np.nonzero(cum[t0 + 1:] >= want)[0]
        t1 = n_tiles if len(reach) == 0 or cum[n_tiles] <= want else t0 + 1 + int(reach[0])
        out.append((t0, t1 - t0))
        t0, want = t1, want * GROWTH
    return out
