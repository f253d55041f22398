"""GPU: the flat int8 chain's long passes under the share planner's table (csrc/ehx_balance.h, k_flati8.hip TAB).

The partition of a pass's row tiles over the XCDs cannot change an answer.  Two test hooks (csrc/ehx_testhooks.cpp) force
eight factors — with the clamp and the 64-tiles-per-chunk gate lifted, so that the one pass of a 274-tile space takes the
table path — and read back the bounds, stamps and factors of the last batch.  70 000 cosine rows of 256 and of 768 dims (the
compile-time-slot loop), 300 queries (two query tiles), k = 10: ids and distance bytes are pyoracle.exhaustive's and those
of the uniform run under every forced split; the bounds cover every tile once; with the hook off the factors learnt over
six batches stay inside the clamp; with EHX_I8_BALANCE=0 (read once per process: a child) the split is the uniform one."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import pyoracle  # noqa: E402

pytestmark = pytest.mark.gpu

N_ROWS, NQ, K = 70000, 300, 10
N_TILES = (N_ROWS + 255) // 256   # 274
LO, HI = 0.85, 1.15               # the planner's clamp (ehx_balance.h)
CASES = {
    "uniform": [1.0] * 8,
    "one-xcd": [0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0],
    "zero-xcd": [1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 1.0],
    "alternating": [0.5, 1.5] * 4,
}
_RAW = []


def _ehx():
    import embeddinghub_amd
    return embeddinghub_amd


def _raw():
    if not _RAW:
        from embeddinghub_amd import _lib
        lib = C.CDLL(_lib.LIB_PATH)
        lib.ehx_test_i8_balance_force.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        lib.ehx_test_i8_balance_force.restype = C.c_int
        lib.ehx_test_i8_balance_read.argtypes = [C.c_void_p] * 6
        lib.ehx_test_i8_balance_read.restype = C.c_int
        _RAW.append(lib)
    return _RAW[0]


def _ok(rc):
    from embeddinghub_amd import _lib
    assert rc == 0, (rc, _lib.load().ehx_last_error())


def force(s, factors, min_tiles_per_chunk=1):
    f = None if factors is None else np.ascontiguousarray(factors, dtype=np.float64)
    _ok(_raw().ehx_test_i8_balance_force(s._h, None if f is None else f.ctypes.data, min_tiles_per_chunk))


def read(s):
    info = np.zeros(8, dtype=np.uint64)
    bounds = np.zeros(257, dtype=np.uint32)
    stamps = np.zeros(2 * 512, dtype=np.uint64)
    factors, rates = np.zeros(8), np.zeros(8)
    _ok(_raw().ehx_test_i8_balance_read(s._h, info.ctypes.data, bounds.ctypes.data, stamps.ctypes.data, factors.ctypes.data,
                                        rates.ctypes.data))
    batches, grid, q_tiles, n_tiles, n_chunks, tile0, table, khz = (int(v) for v in info)
    return dict(batches=batches, grid=grid, q_tiles=q_tiles, n_tiles=n_tiles, n_chunks=n_chunks, tile0=tile0, table=table,
                khz=khz, bounds=bounds[:n_chunks + 1].astype(np.int64), stamps=stamps[:2 * grid].reshape(grid, 2),
                factors=factors, rates=rates)


def xcd_tiles(r):
    cpx = r["n_chunks"] // 8
    return [int(r["bounds"][(x + 1) * cpx] - r["bounds"][x * cpx]) for x in range(8)]


def check_cover(r, n_tiles=N_TILES):
    b = r["bounds"]
    assert r["n_tiles"] == n_tiles and r["tile0"] == 0 and r["n_chunks"] % 8 == 0 and r["grid"] == r["q_tiles"] * r["n_chunks"]
    assert b[0] == 0 and b[-1] == n_tiles and np.all(np.diff(b) >= 0), b
    seen = np.zeros(n_tiles, dtype=np.int64)
    for c in range(r["n_chunks"]):
        seen[b[c]:b[c + 1]] += 1
    assert np.all(seen == 1), "tiles covered %s times" % sorted(set(seen.tolist()))
    st = r["stamps"]
    assert np.all(st[:, 0] > 0) and np.all(st[:, 1] >= st[:, 0]), "a workgroup's finish stamp precedes its start stamp"


def uniform_split(n_tiles, n_chunks):
    tpc = (n_tiles + n_chunks - 1) // n_chunks
    return np.minimum(np.arange(n_chunks + 1, dtype=np.int64) * tpc, n_tiles)


def make_space(dims, tag):
    ehx = _ehx()
    s = ehx.Space.unique("i8-balance-%s-%d" % (tag, dims), dims, metric=ehx.METRIC_COSINE, initial_capacity=N_ROWS)
    s.fill_synthetic(ehx.SEED_CORPUS, 0, N_ROWS, True)
    assert s.scan_engine() == "i8"
    return s


def data(dims):
    ehx = _ehx()
    X = pyoracle.gen_rows(ehx.SEED_CORPUS, 0, N_ROWS, dims, normalize=True)
    Q = pyoracle.gen_rows(ehx.SEED_QUERY, 0, NQ, dims, normalize=True)
    return X, np.ascontiguousarray(Q, dtype=np.float32)


def same(got, want, what):
    ids, dist, cnt = got
    oids, odist, ocnt = want
    assert np.array_equal(cnt, ocnt) and int(cnt.min()) == K, what
    assert np.array_equal(ids, oids), "%s: ids differ" % what
    assert np.ascontiguousarray(dist).tobytes() == np.ascontiguousarray(odist).tobytes(), "%s: distance bytes differ" % what


@pytest.fixture(scope="module", params=[256, 768])
def setup(request):
    dims = request.param
    X, Q = data(dims)
    truth = pyoracle.exhaustive(X, Q, K, pyoracle.METRIC_COSINE)
    s = make_space(dims, "forced")
    force(s, CASES["uniform"])
    uni = s.knn(Q, K)
    yield dict(dims=dims, s=s, Q=Q, truth=truth, uniform=uni, uniform_read=read(s))
    s.drop()


@pytest.mark.parametrize("case", list(CASES))
def test_forced_shares_leave_the_answers_alone(setup, case):
    s, Q = setup["s"], setup["Q"]
    st0 = s.stats()
    force(s, CASES[case])
    got = s.knn(Q, K)
    r = read(s)
    force(s, CASES["uniform"])
    same(got, setup["truth"], "%s against the oracle" % case)
    same(got, setup["uniform"], "%s against the uniform run" % case)
    st1 = s.stats()
    assert st1["n_i8_queries"] - st0["n_i8_queries"] == NQ and st1["n_i8_fallback"] == st0["n_i8_fallback"]
    assert r["table"] == 1 and r["q_tiles"] == 2
    check_cover(r)
    tiles = xcd_tiles(r)
    want = np.array(CASES[case]) / sum(CASES[case]) * N_TILES
    assert all(abs(t - w) <= 1.0 for t, w in zip(tiles, want)), (tiles, want)
    if case == "one-xcd":
        assert tiles == [0, 0, N_TILES, 0, 0, 0, 0, 0]
    if case == "zero-xcd":
        assert tiles[5] == 0 and min(tiles[:5] + tiles[6:]) > 0
    assert list(r["factors"]) == CASES[case]
    # an XCD without tiles has no rate; every other one has
    assert [x for x in range(8) if r["rates"][x] == 0.0] == [x for x in range(8) if tiles[x] == 0]


def test_learnt_factors_stay_inside_the_clamp_over_six_batches(setup):
    """the hook off (nothing forced), the gate at one tile per chunk so that this space's one pass is stamped and balanced"""
    s, Q = setup["s"], setup["Q"]
    force(s, None)
    before = read(s)["batches"]
    try:
        for i in range(6):
            got = s.knn(Q, K)
            r = read(s)
            assert r["batches"] == before + i + 1 and r["table"] == 1
            check_cover(r)
            assert np.all(r["factors"] >= LO) and np.all(r["factors"] <= HI), r["factors"]
            assert np.all(r["rates"] > 0.0), r["rates"]
            same(got, setup["truth"], "batch %d against the oracle" % i)
    finally:
        force(s, CASES["uniform"])


def child():
    """EHX_I8_BALANCE=0: no table — the kernel's own arithmetic, which the bounds read back restate; the stamps stay on"""
    dims = int(sys.argv[2])
    X, Q = data(dims)
    s = make_space(dims, "off")
    force(s, None)
    got = s.knn(Q, K)
    r = read(s)
    same(got, pyoracle.exhaustive(X, Q, K, pyoracle.METRIC_COSINE), "the switch off against the oracle")
    check_cover(r)
    print(json.dumps({"table": r["table"], "uniform": bool(np.array_equal(r["bounds"], uniform_split(N_TILES, r["n_chunks"])))}))
    s.drop()


def test_the_switch_gives_the_uniform_split():
    env = dict(os.environ, EHX_I8_BALANCE="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "child", "256"], env=env, cwd=ROOT, timeout=300,
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    assert json.loads(p.stdout.strip().splitlines()[-1]) == {"table": 0, "uniform": True}


if __name__ == "__main__":
    child()
