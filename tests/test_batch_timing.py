"""Which batches of a search are timed, and what ehx_stats makes of them (the figures bench.py reports come from here).

After ehx_stats_reset, R batches through each pipeline leave a known number of scan windows in the ring behind
scan_ms_mean (scan_launches):
  - the fp32 / fp16 scans time every batch and put every one in the ring;
  - the exhaustive pass (k > EHX_MAX_K) is timed but never in the ring: scan_launches falls back to 1 (last_scan_ms);
  - the int8 chain (per scratch set) and the graph search time batch 0 and every EHX_STATS_EVERY-th batch; only the
    latter go into the ring, so R batches leave floor(R / N) entries (the fallback 1 when that is 0);
  - a graph query answered in one launch records nothing.
A reset restarts the count, so the batch right after it is a timed one.  EHX_STATS_EVERY is read once per process: the
N = 3 case runs in a fresh child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import pyoracle  # noqa: E402

pytestmark = pytest.mark.gpu

N_ROWS, DIMS, K = 20000, 128, 10


def _ehx():
    import embeddinghub_amd
    return embeddinghub_amd


def _every():
    return int(os.environ.get("EHX_STATS_EVERY", "2"))


def _launches(batches, every):
    """ring entries that `batches` batches of a sampled pipeline leave after a reset (at least the fallback 1)"""
    return max(1, batches // every)


def _queries(nq, seed=1):
    return pyoracle.gen_rows(_ehx().SEED_QUERY, seed * 100000, nq, DIMS, normalize=True)


def _flat_space():
    ehx = _ehx()
    s = ehx.Space.unique("timing", DIMS, metric=ehx.METRIC_COSINE, initial_capacity=N_ROWS)
    s.fill_synthetic(ehx.SEED_CORPUS, 0, N_ROWS, True)
    assert s.scan_engine() == "i8"
    return s


def _check_times(st):
    assert st["last_scan_ms"] > 0, st
    assert st["last_total_ms"] >= st["last_scan_ms"], st


def _flat_engines(s, R):
    ehx = _ehx()
    Q = _queries(64)
    for scan in (ehx.SCAN_F32, ehx.SCAN_F16):
        s.set_scan(scan)
        s.stats_reset()
        for _ in range(R):
            s.knn(Q, K)
        st = s.stats()
        assert st["n_filter_fallback"] == 0, st
        assert st["scan_launches"] == R, (scan, R, st)
        _check_times(st)
    s.set_scan(ehx.SCAN_AUTO)


def _exhaustive(s, R):
    s.stats_reset()
    Q = _queries(8, seed=2)
    for _ in range(R):
        _, _, cnt = s.knn(Q, 100)
        assert (cnt == 100).all()
    st = s.stats()
    assert st["n_exhaustive"] == 8 * R, st
    assert st["scan_launches"] == 1, st
    _check_times(st)


def _i8_device(s, R, pre=0):
    """int8 through ehx_knn_device on one torch stream: always scratch set 0; `pre` batches run before the reset"""
    import torch
    Q = torch.from_numpy(_queries(64, seed=3)).cuda()
    ids = torch.empty((64, K), dtype=torch.int64, device="cuda")
    dst = torch.empty((64, K), dtype=torch.float32, device="cuda")
    cnt = torch.empty(64, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    for i in range(pre + R):
        if i == pre:
            torch.cuda.synchronize()
            s.stats_reset()
        s.knn_device(Q, K, ids, dst, cnt, stream=st.cuda_stream)
    st.synchronize()
    stats = s.stats()
    assert stats["n_i8_queries"] == 64 * R and stats["n_i8_fallback"] == 0, stats
    assert stats["scan_launches"] == _launches(R, _every()), (R, pre, stats)
    _check_times(stats)


def _i8_host(s, R):
    """int8 through host ehx_knn at a batch above 32 KiB of queries: the slot path, consecutive batches alternate sets"""
    Q = _queries(256, seed=4)
    assert Q.nbytes > 32 << 10
    s.stats_reset()
    for _ in range(R):
        s.knn(Q, K)
    st = s.stats()
    assert st["n_i8_queries"] == 256 * R and st["n_i8_fallback"] == 0, st
    n = _every()
    per_set = (R + 1) // 2 // n + R // 2 // n
    assert st["scan_launches"] == max(1, per_set), (R, st)
    _check_times(st)


def _graph(R, pre=0):
    ehx = _ehx()
    n, d = 6000, 64
    g = ehx.Space.unique("timing-g", d, metric=ehx.METRIC_L2SQ, mode=ehx.MODE_GRAPH, initial_capacity=n, build_batch=4096)
    g.fill_synthetic(ehx.SEED_CORPUS, 0, n, False)
    Q = pyoracle.gen_rows(ehx.SEED_QUERY, 0, 32, d, normalize=False)
    for i in range(pre + R):
        if i == pre:
            g.stats_reset()
        g.knn(Q, K)
    st = g.stats()
    assert st["scan_launches"] == _launches(R, _every()), (R, pre, st)
    _check_times(st)
    g.knn(Q[:1], K)   # one query in one launch: no events
    st2 = g.stats()
    assert st2["scan_launches"] == st["scan_launches"], (st, st2)
    assert st2["last_scan_ms"] == st["last_scan_ms"], (st, st2)
    g.drop()


@pytest.mark.parametrize("R", [1, 4, 5])
def test_flat_engines_time_every_batch(R):
    s = _flat_space()
    _flat_engines(s, R)
    s.drop()


def test_exhaustive_pass_stays_out_of_the_ring():
    s = _flat_space()
    _exhaustive(s, 3)
    s.drop()


@pytest.mark.parametrize("R", [1, 2, 5, 8])
def test_i8_device_batches_sampled(R):
    s = _flat_space()
    _i8_device(s, R)
    s.drop()


@pytest.mark.parametrize("R", [4, 7])
def test_i8_host_batches_sampled_per_set(R):
    s = _flat_space()
    _i8_host(s, R)
    s.drop()


@pytest.mark.parametrize("R", [1, 5])
def test_graph_batches_sampled(R):
    _graph(R)


def test_reset_makes_the_next_batch_timed():
    # one batch before the reset: were the count not restarted, the sampled batches would fall on other indices
    s = _flat_space()
    _i8_device(s, 3, pre=1)
    s.drop()
    _graph(3, pre=1)


def _child():
    assert _every() == 3
    s = _flat_space()
    _flat_engines(s, 4)
    _i8_device(s, 7)
    _i8_device(s, 5, pre=1)
    _i8_host(s, 12)
    s.drop()
    _graph(7)
    _graph(5, pre=1)


def test_stats_every_three_in_a_child_process():
    env = dict(os.environ, EHX_STATS_EVERY="3")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, timeout=400,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, "EHX_STATS_EVERY=3 child failed (rc %d):\n%s" % (r.returncode, r.stderr[-6000:])


if __name__ == "__main__":
    _child()
    print("EHX_STATS_EVERY=3 ok")
