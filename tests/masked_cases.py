"""Helper of the masked-kNN tests (no test here): the bitmaps of the int8 cases, shared by the CPU model
(tests/test_masked_model.py) and the GPU tests (tests/test_knn_masked.py), a restatement of how ehx_masked.cpp samples
the allowed rows and cuts the scan into passes, and the cases made for the merge of a pass's hits into the carried keys."""
import numpy as np

import largek_cases as lc

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


def running(allowed):
    """int64 [tiles + 1]: the allowed rows before every 256-row tile, the last entry their number"""
    n = len(allowed)
    n_tiles = (n + TILE - 1) // TILE
    pad = np.zeros(n_tiles * TILE, dtype=np.int64)
    pad[:n] = allowed
    return np.concatenate([[0], np.cumsum(pad.reshape(n_tiles, TILE).sum(axis=1))])


def passes_over(cum):
    """[(first tile, tiles)] of the scan passes over a running count (masked_passes, ehx_masked.cpp): THE statement of the
    pass cut — one bitmap passes its own counts, a table the pointwise maximum of its scanned masks'"""
    n_tiles = len(cum) - 1
    out, t0, want = [], 0, SAMPLE * GROWTH
    while t0 < n_tiles:
        reach = np.nonzero(cum[t0 + 1:] >= want)[0]
        t1 = n_tiles if len(reach) == 0 or cum[n_tiles] <= want else t0 + 1 + int(reach[0])
        out.append((t0, t1 - t0))
        t0, want = t1, want * GROWTH
    return out


def passes(allowed):
    """[(first tile, tiles)] of the scan passes under one bitmap"""
    return passes_over(running(allowed))


def far_then_near(X, q, n_far=4096, n_near=1500):
    """A bitmap made for ONE query q: of the ids below n / 2 the n_far rows FARTHEST from q, and of the ids from the next
    tile boundary up the n_near NEAREST.  The first pass ends where 4096 allowed rows have been seen — behind the last far
    row — while the sample, every 22nd allowed row by rank, holds more than 48 near rows: its 48th distance lies below every
    far row's, the first pass finds nothing for q and hands fewer than k keys on.  (The bitmaps above do not give that: every
    pass of theirs sees rows of every distance, hundreds of them within the first radius; a bitmap of the ids from 16 000
    up allows 4 000 rows, fewer than the 4096 a first pass ends at, so its scan is ONE pass.)"""
    n = len(X)
    d2 = ((X.astype(np.float64) - q.astype(np.float64)[None, :]) ** 2).sum(axis=1)
    lo, hi = n // 2, (n // 2 // TILE + 1) * TILE
    allowed = np.zeros(n, dtype=bool)
    allowed[np.argsort(-d2[:lo], kind="stable")[:n_far]] = True
    allowed[hi + np.argsort(d2[hi:], kind="stable")[:n_near]] = True
    allowed.setflags(write=False)
    return allowed


def merge_cases():
    """name -> (rows, queries, metric, {bitmap name: allowed}, ks): the GPU cases of the rank merge of a pass's hits into the
    carried keys.  Every one of them must pass tests/test_masked_model.py before its GPU test may assert "no query handed
    on".  ties: 300 copies of row 5 over the ids of both passes, query 0 that row — hits and carried keys at ONE distance,
    ordered by id.  short: far_then_near for query 0.  f16: binary16 rows, 96 columns, cosine."""
    m = masks(20000)
    Xt, Qt, _ = lc.ties()
    X, Q = lc.gauss(20000, 64, 64, 1)
    Xh, Qh = lc.f16_rows()
    return {"ties": (Xt, Qt, "l2", {"ones": m["ones"], "half": m["half"]}, KS),
            "short": (X, Q, "l2", {"far_then_near": far_then_near(X, Q[0])}, (48,)),
            "f16": (Xh, Qh, "cosine", {"half": m["half"]}, (48,))}
