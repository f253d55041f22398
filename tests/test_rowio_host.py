"""CPU-side checks of the device-resident Set and the batched Gets (ehx_set_batch_device, ehx_get_batch,
ehx_get_by_ids_device): the declarations, the ABI that stays as it was, what the entry points answer without a device, the
duplicate rule of the scatter and what a batch of row ids touches (WriteBatch; host functions behind test hooks), the
resource usage of k_rowio.hip built for gfx950, and the argument checks of Space.set_batch_device, which run in front of
the C call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from embeddinghub_amd import _lib
from embeddinghub_amd import build as ehx_build
from embeddinghub_amd.space import Space

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ehx_set_batch_device", "ehx_get_batch", "ehx_get_by_ids_device")
HOOK = "ehx_test_last_writers"
HOOKS = (HOOK, "ehx_test_write_batch")
NONE = 2**64 - 1


def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS and hasattr(raw, name)
    assert "k_rowio.hip" in ehx_build.SOURCES and "ehx_rowio.cpp" in ehx_build.SOURCES
    assert re.search(r"#define EHX_ABI_VERSION 5\b", header)   # additive: the version stays
    for name in ("set_batch_device", "get_batch", "get_by_ids_device"):
        assert callable(getattr(Space, name))


def test_the_duplicate_rule_hook_is_not_part_of_the_abi():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    for hook in HOOKS:
        assert hook not in header and hook not in _lib.SYMBOLS
        assert hasattr(C.CDLL(_lib.LIB_PATH), hook)


def test_the_entry_points_without_a_device():
    import torch
    lib = _lib.load()
    out = (C.c_float * 4)()
    calls = (lambda s: lib.ehx_set_batch_device(s, None, 1, None, None, None, 0),
             lambda s: lib.ehx_get_batch(s, 1, None, None, out, None),
             lambda s: lib.ehx_get_by_ids_device(s, None, 1, None, None, None))
    if torch.cuda.is_available():
        for call in calls:   # a NULL space is refused before anything is touched
            assert call(None) == _lib.EINVAL and lib.ehx_last_error() == b"space is NULL"
    else:
        h = C.c_void_p()
        assert lib.ehx_space_create(b"rowio-nodev", 11, 4, 0, 0, None, C.byref(h)) == _lib.ENODEVICE and not h.value
        for call in calls:   # no device: that is the answer, whatever else is wrong with the call
            assert call(None) == _lib.ENODEVICE


def _last_writers(ids):
    fn = getattr(C.CDLL(_lib.LIB_PATH), HOOK)
    fn.restype = None
    fn.argtypes = [C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(C.c_uint64)]
    a = np.asarray(ids, dtype=np.uint64)
    out = np.full(len(a) + 1, 12345, dtype=np.uint64)   # (one word more: nothing is written behind the n-th)
    fn(a.ctypes.data_as(C.POINTER(C.c_uint64)), len(a), out.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert out[-1] == 12345
    return out[:-1].tolist()


def test_last_writers():
    assert _last_writers([5, 6, 5, 7, 6, 5]) == [NONE, NONE, NONE, 7, 6, 5]
    distinct = [9, 0, 3, 2**40, 7, 1]
    assert _last_writers(distinct) == distinct
    assert _last_writers([]) == []
    assert _last_writers([4]) == [4]
    assert _last_writers([4, 4]) == [NONE, 4]
    # against a restatement: of every id the highest position keeps it
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 50, 400).tolist()
    last = {v: i for i, v in enumerate(ids)}
    assert _last_writers(ids) == [v if last[v] == i else NONE for i, v in enumerate(ids)]


def _write_batch(ids, old_n):
    fn = C.CDLL(_lib.LIB_PATH).ehx_test_write_batch
    fn.restype = None
    fn.argtypes = [C.POINTER(C.c_uint64), C.c_size_t, C.c_uint64, C.POINTER(C.c_uint64)]
    a = np.asarray(ids, dtype=np.uint64)
    out = np.full(6, 12345, dtype=np.uint64)
    fn(a.ctypes.data_as(C.POINTER(C.c_uint64)), len(a), old_n, out.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert out[-1] == 12345
    return tuple(int(v) for v in out[:5])


def _write_batch_numpy(ids, old_n):
    """(lo, hi, dense_run, touches_committed, all_appended) restated; an empty batch: the identities of min and max, a run,
    nothing touched, all of its (no) rows appended"""
    a = np.asarray(ids, dtype=np.uint64)
    if a.size == 0:
        return (NONE, 0, 1, 0, 1)
    dense = bool((a == a[0] + np.arange(a.size, dtype=np.uint64)).all())
    return (int(a.min()), int(a.max()), int(dense), int((a < old_n).any()), int(dense and int(a[0]) == old_n))


@pytest.mark.parametrize("name, ids, old_n, expect", [
    ("empty", [], 7, (NONE, 0, 1, 0, 1)),
    ("one id, appended", [7], 7, (7, 7, 1, 0, 1)),
    ("one id, rewritten", [3], 7, (3, 3, 1, 1, 0)),
    ("a dense append", list(range(100, 108)), 100, (100, 107, 1, 0, 1)),
    ("a dense run starting below old_n", list(range(96, 104)), 100, (96, 103, 1, 1, 0)),
    ("a run with one repeat", [100, 101, 102, 102, 103], 100, (100, 103, 0, 0, 0)),
    ("a permuted run", [100, 102, 101, 103], 100, (100, 103, 0, 0, 0)),
    ("ids all below old_n", [5, 9, 2, 9], 100, (2, 9, 0, 1, 0)),
    ("a mix with lo < old_n <= hi", [100, 4, 101, 102], 100, (4, 102, 0, 1, 0)),
    ("ids beyond 2^32", [2**40, 2**40 + 1], 2**40, (2**40, 2**40 + 1, 1, 0, 1)),
])
def test_write_batch(name, ids, old_n, expect):
    assert _write_batch_numpy(ids, old_n) == expect, "the restatement itself"
    assert _write_batch(ids, old_n) == expect


def test_write_batch_against_its_restatement():
    rng = np.random.default_rng(5)
    for _ in range(200):
        old_n = int(rng.integers(0, 40))
        n = int(rng.integers(0, 12))
        ids = (np.arange(n) + rng.integers(0, 45)).tolist() if rng.random() < 0.5 else rng.integers(0, 60, n).tolist()
        assert _write_batch(ids, old_n) == _write_batch_numpy(ids, old_n), (ids, old_n)


def test_scatter_kernel_uses_no_scratch_and_spills_no_vector_registers(tmp_path):
    src = os.path.join(ehx_build.CSRC, "k_rowio.hip")
    flags = [f for f in ehx_build.FLAGS if f != "-shared"]
    r = subprocess.run([ehx_build.HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o",
                                                    str(tmp_path / "k_rowio.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    assert len(names) == 1 and "scatter_rows_kernel" in names[0], names
    for what in ("ScratchSize \\[bytes/lane\\]", "VGPRs Spill"):
        vals = re.findall(what + r": (\d+)", r.stderr)
        assert len(vals) == 1 and vals[0] == "0", (what, vals)


class _Tensor:
    """a stand-in with what set_batch_device looks at; the checks run in front of the C call"""

    def __init__(self, shape, dtype="torch.float32", contiguous=True, is_cuda=True):
        self.shape, self.dtype, self._c, self.is_cuda = shape, dtype, contiguous, is_cuda

    def data_ptr(self):
        raise AssertionError("the pointer is taken only after the checks")

    def is_contiguous(self):
        return self._c


def test_set_batch_device_checks_its_arguments_before_the_call():
    s = Space.__new__(Space)   # (no engine behind it: every case is refused before the library is asked)
    s.dims, s._h, s._L = 8, None, None
    keys = ["a", "b", "c"]
    for bad in (np.zeros((3, 8), dtype=np.float32),              # host memory
                _Tensor((3, 8), dtype="torch.int64"),
                _Tensor((3, 8), dtype="torch.bfloat16"),
                _Tensor((3, 8), contiguous=False),
                _Tensor((3, 8), is_cuda=False),
                _Tensor((3, 4)),                                  # not the space's dims
                _Tensor((24,)),
                _Tensor((2, 8)),                                  # three keys, two rows
                [[0.0] * 8] * 3):
        with pytest.raises(ValueError):
            s.set_batch_device(keys, bad)
    import torch
    for bad in (torch.zeros((3, 8), dtype=torch.int64), torch.zeros((3, 16))[:, ::2], torch.zeros((3, 8), dtype=torch.float64)):
        with pytest.raises(ValueError):
            s.set_batch_device(keys, bad)
