"""GPU test of the ONE tile prefix of the compactions (rows_prefix_kernel, k_masked.hip, over block_prefix, k_prefix.h),
through the hook ehx_test_rows_prefix: host arrays in and out, a device but no space.  Every row of counts must come back as
numpy's exclusive cumulative sum with the total behind it, at the smallest sizes that cross a wave (64 lanes), a chunk of
1024 entries and two chunks — the carry between chunks, which the bitmap and label suites (79 tiles) never reach."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402

GUARD, UNWRITTEN = 0xC0FFEE11, 0xDEADBEEF


def _prefix(counts, rows, n):
    out = np.full(rows * (n + 1) + 1, UNWRITTEN, dtype=np.uint32)
    out[-1] = GUARD
    _lib.load()   # (torch's HIP runtime first: a process holds ONE runtime instance, _lib.load says why)
    fn = C.CDLL(_lib.LIB_PATH).ehx_test_rows_prefix
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    assert counts.size == rows * n
    assert fn(counts.ctypes.data if counts.size else None, rows, n, out.ctypes.data) == _lib.OK
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
@pytest.mark.parametrize("rows", [1, 3])
def test_every_row_is_numpy_s_exclusive_prefix_with_the_total_behind_it(rows, n):
    counts = np.random.default_rng(1000 * rows + n).integers(0, 257, size=(rows, n)).astype(np.uint32)
    assert counts.max() <= 256
    out = _prefix(counts, rows, n)
    want = np.zeros((rows, n + 1), dtype=np.uint64)
    want[:, 1:] = np.cumsum(counts.astype(np.uint64), axis=1)
    assert out[:-1].reshape(rows, n + 1).tolist() == want.tolist()
    assert out[-1] == GUARD


@pytest.mark.parametrize("rows", [0, 1, 3])
def test_no_entry_launches_nothing(rows):
    out = _prefix(np.zeros(0, dtype=np.uint32), rows, 0)   # rows words (the totals' places) and the guard
    assert (out[:-1] == UNWRITTEN).all() and out[-1] == GUARD
