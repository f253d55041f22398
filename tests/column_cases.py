"""Helper of the tests of stored label columns (no test here): the columns the index is checked on, the numpy statement of
what an index is, the hooks, and the labelled prefix oracle of the streamed-append test.  labeled_cases, grouped_labeled_cases
and range_cases are used as they are.  The sizes the tests rely on are asserted here, where the columns are made."""
import ctypes as C

import numpy as np

import labeled_cases as lbc
import range_cases as rc
from prefix_oracle import PrefixOracle

NONE = 0xFFFFFFFF
MAX_COLUMNS = 4
INDEX_ROWS = (1, 255, 256, 257, 4097, 20000)     # below, at and above a 256-key tile; one key above a 4096-key sort tile
INDEX_KINDS = ("one_label", "tenants", "random32", "top_byte", "descending")
assert rc.I8_ROWS == 20000 == INDEX_ROWS[-1]


def index_column(kind, n):
    """uint32 [n] of one of INDEX_KINDS"""
    rng = np.random.default_rng(4000 + n)
    if kind == "one_label":
        col = np.full(n, 77, dtype=np.uint32)
    elif kind == "tenants":
        col = lbc.column()[:n].copy()
    elif kind == "random32":
        col = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
        col[0] = 0
        col[n // 2] = NONE
        if n >= 4097:   # every byte varies: four passes
            assert all(len(np.unique((col >> s) & 255)) > 1 for s in (0, 8, 16, 24))
    elif kind == "top_byte":
        col = (rng.integers(0, 256, size=n).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00ABCDEF)
    elif kind == "descending":
        col = (np.uint32(3_000_000) - np.arange(n, dtype=np.uint32)).astype(np.uint32)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(col, dtype=np.uint32)


BIG_ROWS = 1_100_003    # 269 sort tiles of 4096 keys (> 256) and 4297 boundary tiles of 256 (> 1024), not a multiple of either
assert (BIG_ROWS + 4095) // 4096 > 256 and (BIG_ROWS + 255) // 256 > 1024 and BIG_ROWS % 256 and BIG_ROWS % 4096


def big_column(kind):
    """uint32 [BIG_ROWS]: random 32-bit values (four passes, about as many labels as rows), or 16 tenants in random order"""
    rng = np.random.default_rng(88)
    if kind == "random32":
        return rng.integers(0, 2 ** 32, size=BIG_ROWS, dtype=np.uint64).astype(np.uint32)
    assert kind == "tenants16"
    return rng.integers(0, 16, size=BIG_ROWS).astype(np.uint32)


def expected_passes(col):
    """digit passes the sort runs on this column: the bytes that take more than one value"""
    return sum(len(np.unique((col >> np.uint32(s)) & np.uint32(255))) > 1 for s in (0, 8, 16, 24))


def expected_index(col):
    """-> (perm u64 [n], labels u32 [L], start u32 [L + 1]) — numpy's stable sort and np.unique"""
    col = np.asarray(col, dtype=np.uint32)
    perm = np.argsort(col, kind="stable").astype(np.uint64)
    labels, first = np.unique(col[perm.astype(np.int64)], return_index=True)
    return perm, labels.astype(np.uint32), np.concatenate([first, [len(col)]]).astype(np.uint32)


def raw(lib_path):
    return C.CDLL(lib_path)


def column_counters(L, s, col):
    """index builds, searches served from a fresh index, digit passes of the last build"""
    out = (C.c_uint64 * 3)()
    L.ehx_test_column_counters(s._h, C.c_uint32(col), out)
    return np.array(list(out), dtype=np.int64)


def column_index(L, s, col):
    """the index as the device holds it -> (perm, labels, start) cut to their lengths"""
    n = len(s)
    perm = np.zeros(max(n, 1), dtype=np.uint64)
    labels = np.zeros(max(n, 1), dtype=np.uint32)
    start = np.zeros(n + 1, dtype=np.uint32)
    got_n, got_l = C.c_uint64(0), C.c_uint32(0)
    L.ehx_test_column_index.restype = C.c_int
    rc_ = L.ehx_test_column_index(s._h, C.c_uint32(col), perm.ctypes.data_as(C.POINTER(C.c_uint64)),
                                  labels.ctypes.data_as(C.POINTER(C.c_uint32)), start.ctypes.data_as(C.POINTER(C.c_uint32)),
                                  C.byref(got_n), C.byref(got_l))
    assert rc_ == 0, "ehx_test_column_index: %d" % rc_
    return perm[:got_n.value], labels[:got_l.value], start[:got_l.value + 1], got_n.value


class LabelledPrefixOracle:
    """The oracle's labelled answer for every published prefix: per wanted label T a PrefixOracle over the rows that carry T
    (in id order), its bounds the number of such rows below every publish boundary.  Every chunk must carry rows of every
    wanted label (asserted), so every boundary is one of each label's."""

    def __init__(self, X, col, Q, want, k, metric, bounds):
        self.want, self.bounds = np.asarray(want, dtype=np.uint32), [int(b) for b in bounds]
        self.parts = {}
        for lab in np.unique(self.want):
            rows = np.nonzero(col == lab)[0]
            local = [int(np.searchsorted(rows, b)) for b in self.bounds]
            assert all(a < b for a, b in zip(local, local[1:])) and local[0] > 0, "label %d: a chunk without its rows" % lab
            at = np.nonzero(self.want == lab)[0]
            self.parts[int(lab)] = (rows, local, at, PrefixOracle(X[rows], Q[at], k, metric, local))

    def assert_is_some_prefix(self, ids, dist, cnt, lo, hi):
        """ONE boundary lo <= b <= hi serves every label's queries"""
        ok = None
        for lab, (rows, local, at, po) in self.parts.items():
            gi = np.asarray(ids)[at].astype(np.uint64)
            c = np.asarray(cnt)[at]
            keep = np.arange(gi.shape[1])[None, :] < c[:, None]
            safe = np.where(keep, gi, np.uint64(rows[0])).astype(np.int64)
            pos = np.searchsorted(rows, safe)
            assert (rows[np.minimum(pos, len(rows) - 1)] == safe).all(), "label %d: a returned row does not carry it" % lab
            fits = set()
            for b, lb in zip(self.bounds, local):
                if lo <= b <= hi and po._equal((pos.astype(np.uint64), np.asarray(dist)[at], c), po.answer(lb)):
                    fits.add(b)
            ok = fits if ok is None else ok & fits
        assert ok, "the answer is the oracle's labelled top-k of no published prefix in [%d, %d]" % (lo, hi)
        return max(ok)
