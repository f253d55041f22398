"""Searches beside streamed appends answer exactly as the oracle does on the rows of SOME published prefix.

Writers append chunks with set_prepared (rows a function of their key) while searchers run; every answer a search
returns mid-stream must be, in ids and distance bytes, the oracle's top-k over X[:b_j] for a publish boundary b_j with
lo <= b_j <= hi (lo = rows published before the search started, hi = rows published after it returned;
tests/prefix_oracle.py).  Every chunk puts rows near every query, spread over the distance range of the current top-k,
so a search that mixes two prefixes — a pass planned on one row count and masked by another, page 1 of one prefix and
page 2 of another, an engine picked for one prefix and run on another — answers for no prefix and fails.

The races are microseconds wide.  EHX_TEST_PAUSE_US (csrc/ehx_env.h, read once per process) makes a search sleep on the
host where a publish could slip in; the cases below run once more with it, each in a fresh child process."""
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import pyoracle  # noqa: E402
from prefix_oracle import PrefixOracle  # noqa: E402

pytestmark = pytest.mark.gpu

PAUSE_US = 3000   # the knob runs: long enough for a chunk's publish to land inside the window


def _ehx():
    import embeddinghub_amd
    return embeddinghub_amd


def _unit(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def _centres(seed, c, d):
    return _unit(np.random.default_rng(seed).standard_normal((c, d)).astype(np.float32))


def _queries(centres, per, seed, spread=0.05):
    r = np.random.default_rng(seed)
    c, d = centres.shape
    q = np.repeat(centres, per, axis=0) + np.float32(spread) * r.standard_normal((c * per, d)).astype(np.float32) / np.sqrt(d)
    return q.astype(np.float32)


def _chunk_rows(centres, j, per_centre, scale, seed):
    """chunk j: per_centre rows near each centre at radii spread over [0.25, 1.6] x a radius that shrinks with j (new rows
    land below and above any floor of the current top-k), shuffled; `scale` (per row) multiplies the rows"""
    r = np.random.default_rng(seed * 7919 + j)
    c, d = centres.shape
    rad = np.float32(0.55 * 0.96 ** j) * r.uniform(0.25, 1.6, (c * per_centre, 1)).astype(np.float32)
    x = np.repeat(centres, per_centre, axis=0) + rad * r.standard_normal((c * per_centre, d)).astype(np.float32) / np.float32(np.sqrt(d))
    x = x[r.permutation(len(x))]
    return (x * scale(j, len(x), r)).astype(np.float32)


def _stream(s, base_X, chunks, searchers, n_writers=1, pace=0.0):
    """chunks: list of (keys, rows); searchers: callables(stop_event) -> list of (lo, answer, hi, tag).  Returns X in id
    order, the publish boundaries, the search records."""
    ehx = _ehx()
    preps = [s.prepare_batch(k, v) for k, v in chunks]
    row_of = {}
    for ci, (keys, rows) in enumerate(chunks):
        for i, kk in enumerate(keys):
            row_of[kk] = (ci, i)
    base = len(s)
    assert base == len(base_X)
    errs, records = [], []
    stop = threading.Event()
    nxt = [0]
    lk = threading.Lock()

    def writer():
        try:
            time.sleep(0.05)    # (the searchers are running before the first publish)
            while True:
                with lk:
                    ci = nxt[0]
                    nxt[0] += 1
                if ci >= len(preps):
                    return
                s.set_prepared(preps[ci])
                if pace:
                    time.sleep(pace)
        except Exception as e:  # noqa: BLE001
            errs.append("writer: %r" % (e,))

    def run_searcher(fn):
        try:
            records.extend(fn(stop))
        except Exception as e:  # noqa: BLE001
            errs.append("searcher: %r" % (e,))

    ws = [threading.Thread(target=writer) for _ in range(n_writers)]
    ss = [threading.Thread(target=run_searcher, args=(fn,)) for fn in searchers]
    for t in ss + ws:
        t.start()
    for t in ws:
        t.join(timeout=600)
        assert not t.is_alive(), "a writer hung"
    time.sleep(0.05)
    stop.set()
    for t in ss:
        t.join(timeout=600)
        assert not t.is_alive(), "a searcher hung"
    assert not errs, errs
    # ids follow the commit order (several writers): X rebuilt from the keys, the boundaries from the chunks' sizes
    total = base + sum(len(k) for k, _ in chunks)
    assert len(s) == total
    X = np.empty((total, base_X.shape[1]), dtype=np.float32)
    X[:base] = base_X
    bounds, pos = [base], base
    while pos < total:
        ci, i = row_of[s.key_of(pos)]
        assert i == 0, "a chunk's rows are not one block of ids"
        keys, rows = chunks[ci]
        for j in range(1, len(keys)):
            assert s.key_of(pos + j) == keys[j], "row %d: not key %d of chunk %d" % (pos + j, j, ci)
        X[pos:pos + len(keys)] = rows
        pos += len(keys)
        bounds.append(pos)
    return X, bounds, records


def _host_searcher(s, Q, k, tag, clock=None):
    """clock: what lo / hi are read from (default: the published row count; test_rewrite_under_search.py counts batches)"""
    clock = clock or (lambda: len(s))

    def fn(stop):
        out = []
        while not stop.is_set():
            lo = clock()
            ans = s.knn(Q, k)
            hi = clock()
            out.append((lo, ans, hi, tag))
        return out
    return fn


def _device_searcher(s, Q, k, tag, clock=None):
    import torch
    clock = clock or (lambda: len(s))
    st = torch.cuda.Stream()
    q = torch.from_numpy(Q).cuda()
    B = Q.shape[0]

    def fn(stop):
        out = []
        ids = torch.empty((B, k), dtype=torch.int64, device="cuda")
        dst = torch.empty((B, k), dtype=torch.float32, device="cuda")
        cnt = torch.empty((B,), dtype=torch.int32, device="cuda")
        while not stop.is_set():
            lo = clock()
            s.knn_device(q, k, ids, dst, cnt, stream=st.cuda_stream)
            st.synchronize()
            hi = clock()
            out.append((lo, (ids.cpu().numpy().astype(np.uint64), dst.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32)),
                        hi, tag))
        return out
    return fn


def _check(X, bounds, records, queries, metric, paused):
    """every mid-stream answer is some prefix's; searches overlapped >= 3 publishes (a publish landed between a search's
    lo and hi), and the searches started under >= 3 different published counts"""
    oracles = {}
    for lo, ans, hi, tag in records:
        if tag not in oracles:
            Q, k = queries[tag]
            oracles[tag] = PrefixOracle(X, Q, k, metric, bounds)
        oracles[tag].assert_is_some_prefix(*ans, lo, hi)
    seen = {lo for lo, _, _, _ in records if lo < bounds[-1]}
    assert len(seen) >= 3, "the searches ran across %d publishes only" % len(seen)
    overlapped = {b for lo, _, hi, _ in records for b in bounds if lo < b <= hi}
    assert len(overlapped) >= 3, "searches overlapped %d publishes only (paused: %s)" % (len(overlapped), paused)
    return oracles


def _final(s, X, queries, metric, oracles=None):
    """the final state is the oracle's over every row (`oracles`: _check's, whose last prefix is all of X — the merge is
    exact, tests/test_prefix_oracle.py — instead of one more scan of a big X)"""
    for tag, (Q, k) in queries.items():
        ids, dist, cnt = s.knn(Q, k)
        if oracles is not None:
            oids, odist, _ = oracles[tag].answer(len(X))
        else:
            oids, odist, _ = pyoracle.exhaustive(X, Q, k, metric)
        np.testing.assert_array_equal(ids, oids)
        assert dist.tobytes() == odist.tobytes(), tag


def _keys(prefix, j, n):
    return ["%s%d_%d" % (prefix, j, i) for i in range(n)]


# ---- the cases -------------------------------------------------------------------------------------------------------

def case_a(paused=False):
    """f32 cosine, 65 536 x 256, the int8 filter: knn at B = 64 (k = 10, 48), knn_device at B = 256 on a torch stream"""
    ehx = _ehx()
    d, base, n_chunks, per = 256, 65536, 14, 80
    cen = _centres(11, 16, d)
    s = ehx.Space.unique("aus_a", d, metric=ehx.METRIC_COSINE, initial_capacity=base + n_chunks * 16 * per)
    s.fill_synthetic(ehx.SEED_CORPUS, 0, base, True)
    Xb = pyoracle.gen_rows(ehx.SEED_CORPUS, 0, base, d, normalize=True)
    assert s.scan_engine() == "i8"
    i8_0 = s.stats()["n_i8_queries"]
    # (chunks of 16 x 80 - 37 rows: no publish boundary after the base falls on a 256-row tile, so a pass planned on one count
    # and masked by a later one takes rows of a chunk it does not take whole)
    m = 16 * per - 37
    chunks = [(_keys("a", j, m), _chunk_rows(cen, j, per, lambda j, m, r: 1.0, 1)[:m]) for j in range(n_chunks)]
    queries = {"h10": (_queries(cen, 4, 2), 10), "h48": (_queries(cen, 4, 3), 48), "dev": (_queries(cen, 16, 4), 10)}
    X, bounds, rec = _stream(s, Xb, chunks, [_host_searcher(s, *queries["h10"], "h10"), _host_searcher(s, *queries["h48"], "h48"),
                                            _device_searcher(s, *queries["dev"], "dev")], pace=0.01)
    _check(X, bounds, rec, queries, pyoracle.METRIC_COSINE, paused)
    assert s.scan_engine() == "i8"
    assert s.stats()["n_i8_queries"] > i8_0, "the int8 engine did not run"
    _final(s, X, queries, pyoracle.METRIC_COSINE)
    s.drop()


def case_b(paused=False):
    """f32 L2^2, norms that fall chunk by chunk (every append lowers the straddling tile's min B) and spread by ~1 % inside
    every tile (lane groups with B margins): the int8 filter with group margins"""
    ehx = _ehx()
    d, base, n_chunks, per = 128, 32768, 12, 60
    cen = _centres(21, 16, d)
    r0 = np.random.default_rng(5)
    Xb = _unit(r0.standard_normal((base, d)).astype(np.float32)) * r0.uniform(1.9, 2.1, (base, 1)).astype(np.float32)
    s = ehx.Space.unique("aus_b", d, metric=ehx.METRIC_L2SQ, initial_capacity=base + n_chunks * 16 * per)
    s.set_batch(["b%d" % i for i in range(base)], Xb)
    assert s.scan_engine() == "i8"
    i8_0 = s.stats()["n_i8_queries"]
    chunks = [(_keys("b", j, 16 * per), _chunk_rows(cen, j, per, lambda j, m, r: (1.0 - 0.02 * j) * r.uniform(0.98, 1.02, (m, 1)), 2))
              for j in range(n_chunks)]
    queries = {"h10": (_queries(cen, 4, 5) * np.float32(0.9), 10), "dev": (_queries(cen, 8, 6) * np.float32(0.9), 10)}
    X, bounds, rec = _stream(s, Xb, chunks, [_host_searcher(s, *queries["h10"], "h10"), _device_searcher(s, *queries["dev"], "dev")],
                             pace=0.01)
    _check(X, bounds, rec, queries, pyoracle.METRIC_L2, paused)
    assert s.scan_engine() == "i8"
    assert s.stats()["n_i8_queries"] > i8_0, "the int8 engine did not run"
    _final(s, X, queries, pyoracle.METRIC_L2)
    s.drop()


def case_c(paused=False):
    """exhaustive pages (EHX_MAX_K < k): cosine and L2^2, k = 65, 100, 200"""
    ehx = _ehx()
    d, base, n_chunks, per = 128, 20000, 12, 40
    cen = _centres(31, 8, d)
    for metric, om in ((ehx.METRIC_COSINE, pyoracle.METRIC_COSINE), (ehx.METRIC_L2SQ, pyoracle.METRIC_L2)):
        s = ehx.Space.unique("aus_c", d, metric=metric, initial_capacity=base + n_chunks * 8 * per)
        s.fill_synthetic(ehx.SEED_CORPUS, 0, base, True)
        Xb = pyoracle.gen_rows(ehx.SEED_CORPUS, 0, base, d, normalize=True)
        ex0 = s.stats()["n_exhaustive"]
        chunks = [(_keys("c", j, 8 * per), _chunk_rows(cen, j, per, lambda j, m, r: r.uniform(0.97, 1.03, (m, 1)), 3))
                  for j in range(n_chunks)]
        queries = {"k%d" % k: (_queries(cen, 2, 7 + k), k) for k in (65, 100, 200)}
        X, bounds, rec = _stream(s, Xb, chunks, [_host_searcher(s, *queries[t], t) for t in queries], pace=0.01)
        _check(X, bounds, rec, queries, om, paused)
        assert s.stats()["n_exhaustive"] > ex0, "the exhaustive pages did not run"
        _final(s, X, queries, om)
        s.drop()


def case_d(paused=False):
    """f32 cosine below i8_min_rows: the fp16 filter"""
    ehx = _ehx()
    d, base, n_chunks, per = 256, 8000, 12, 30
    cen = _centres(41, 16, d)
    s = ehx.Space.unique("aus_d", d, metric=ehx.METRIC_COSINE, initial_capacity=base + n_chunks * 16 * per)
    s.fill_synthetic(ehx.SEED_CORPUS, 0, base, True)
    Xb = pyoracle.gen_rows(ehx.SEED_CORPUS, 0, base, d, normalize=True)
    assert s.scan_engine() == "f16"
    f16_0 = s.stats()["n_filter_queries"]
    chunks = [(_keys("d", j, 16 * per), _chunk_rows(cen, j, per, lambda j, m, r: 1.0, 4)) for j in range(n_chunks)]
    queries = {"h10": (_queries(cen, 4, 8), 10)}
    X, bounds, rec = _stream(s, Xb, chunks, [_host_searcher(s, *queries["h10"], "h10")], pace=0.01)
    _check(X, bounds, rec, queries, pyoracle.METRIC_COSINE, paused)
    assert s.scan_engine() == "f16" and len(s) < 16384
    assert s.stats()["n_filter_queries"] > f16_0, "the fp16 filter did not run"
    _final(s, X, queries, pyoracle.METRIC_COSINE)
    s.drop()


def case_e(paused=False):
    """single queries against a small shard (the one-launch exhaustive path) from four threads"""
    ehx = _ehx()
    d, base, n_chunks, per = 128, 4000, 16, 40     # (base and chunks not multiples of the 64-row blocks)
    cen = _centres(51, 8, d)
    s = ehx.Space.unique("aus_e", d, metric=ehx.METRIC_COSINE, initial_capacity=base + n_chunks * 8 * per)
    s.fill_synthetic(ehx.SEED_CORPUS, 0, base, True)
    Xb = pyoracle.gen_rows(ehx.SEED_CORPUS, 0, base, d, normalize=True)
    ex0 = s.stats()["n_exhaustive"]
    chunks = [(_keys("e", j, 8 * per - 3), _chunk_rows(cen, j, per, lambda j, m, r: 1.0, 5)[:8 * per - 3]) for j in range(n_chunks)]
    queries = {"q%d" % t: (_queries(cen[t:t + 1], 1, 9 + t), 10) for t in range(4)}
    X, bounds, rec = _stream(s, Xb, chunks, [_host_searcher(s, *queries[t], t) for t in queries], pace=0.01)
    _check(X, bounds, rec, queries, pyoracle.METRIC_COSINE, paused)
    # (ehx_stats does not count one-launch calls apart: n_exhaustive also grows on the three-launch single-query pass of
    # knn_device_locked, and calls the micro-batcher coalesces run the filter chain.  That the one-launch path runs is
    # ASSUMED from the shape — one query, k <= 64, a flat shard far below EHX_SMALL_EXACT_BYTES, one caller mostly
    # alone — not proven here; its pause-knob run fails on a tree that reads the row count twice there.)
    assert s.stats()["n_exhaustive"] > ex0, "the single-query exhaustive path did not run"
    _final(s, X, queries, pyoracle.METRIC_COSINE)
    s.drop()


def case_f(paused=False):
    """every chunk holds one row of tiny norm (sumsq in (0, 1e-24]) aligned with a query — the oracle ranks it first, no
    filter can bound it: from the first such chunk on every search must scan in fp32.  An engine picked before that chunk
    is published must not scan the rows it brings, so the case runs in three rounds, each on a fresh space (the window
    opens once per space: the unsafe-row count stays > 0 after the first such chunk).  The first row of every chunk is
    the tiny one and the base is not a whole number of 256-row tiles, so the chunk's first rows share a tile with
    published rows."""
    ehx = _ehx()
    d, base, n_chunks, per = 256, 32768 + 37, 6, 40
    cen = _centres(61, 16, d)
    Qh = _queries(cen, 4, 10)
    Xb = pyoracle.gen_rows(ehx.SEED_CORPUS, 0, base, d, normalize=True)
    for rnd in range(3):
        s = ehx.Space.unique("aus_f", d, metric=ehx.METRIC_COSINE, initial_capacity=base + n_chunks * 16 * per)
        s.fill_synthetic(ehx.SEED_CORPUS, 0, base, True)
        assert s.scan_engine() == "i8"
        i8_0 = s.stats()["n_i8_queries"]
        chunks, aligned = [], []
        for j in range(n_chunks):
            rows = _chunk_rows(cen, j + 10 * rnd, per, lambda j, m, r: 1.0, 6)
            qj = (5 * j + 17 * rnd) % len(Qh)
            tiny = _unit(Qh[qj]) * np.float32(1e-13)
            assert 0 < float(np.dot(tiny, tiny)) <= 1e-24
            rows[0] = tiny
            aligned.append(qj)
            chunks.append((_keys("f%d_" % rnd, j, len(rows)), rows))
        queries = {"h10": (Qh, 10)}
        X, bounds, rec = _stream(s, Xb, chunks, [_host_searcher(s, *queries["h10"], "h10"),
                                                 _host_searcher(s, *queries["h10"], "h10")], pace=0.01)
        _check(X, bounds, rec, queries, pyoracle.METRIC_COSINE, paused)
        assert s.stats()["n_i8_queries"] > i8_0, "no search ran on the int8 filter before the first tiny-norm chunk"
        assert s.scan_engine() == "f32"
        _final(s, X, queries, pyoracle.METRIC_COSINE)
        ids, _, _ = s.knn(Qh[aligned[0]:aligned[0] + 1], 10)
        tiny_ids = np.nonzero((X.astype(np.float64) ** 2).sum(axis=1) <= 1e-24)[0]
        assert len(tiny_ids) == n_chunks and ids[0, 0] in tiny_ids, "the tiny-norm row aligned with the query is not first"
        s.drop()


def case_g(paused=False):
    """DTYPE_F16, 1536 dims, cosine: 262 144 base rows by fill_synthetic, four writers append 8192-row chunks while two
    searchers run at B = 1024 (knn and knn_device), the initial capacity below the final count (the arrays grow
    mid-stream, under the space's lock held exclusively): the int8 filter, then the re-rank on the binary16 rows.  The
    oracle runs on the rows rounded to binary16 (test_flat_parity.py: test_fp16_rows_parity); the base rows come from
    pyoracle.gen_rows, the host twin of fill_synthetic.  The two searchers share one query set, so one prefix oracle
    serves both."""
    ehx = _ehx()
    d, base, n_chunks, per, n_cen = 1536, 262144, 12, 128, 64     # 64 centres x 128 rows = 8192 rows per chunk
    total = base + n_chunks * n_cen * per
    cen = _centres(71, n_cen, d)
    s = ehx.Space.unique("aus_g", d, metric=ehx.METRIC_COSINE, dtype=ehx.DTYPE_F16, initial_capacity=base + 3 * n_cen * per)
    s.fill_synthetic(ehx.SEED_CORPUS, 0, base, True)
    Xb = pyoracle.gen_rows(ehx.SEED_CORPUS, 0, base, d, normalize=True).astype(np.float16).astype(np.float32)
    assert s.scan_engine() == "i8"
    st0 = s.stats()
    assert st0["capacity"] < total, "the capacity must be below the final count: growth happens mid-stream"
    f16 = lambda x: x.astype(np.float16).astype(np.float32)     # (the engine rounds the same way: RNE)
    chunks = [(_keys("g", j, n_cen * per), f16(_chunk_rows(cen, j, per, lambda j, m, r: 1.0, 7))) for j in range(n_chunks)]
    Q = _queries(cen, 16, 12)
    queries = {"g": (Q, 10)}
    X, bounds, rec = _stream(s, Xb, chunks, [_host_searcher(s, Q, 10, "g"), _device_searcher(s, Q, 10, "g")],
                             n_writers=4, pace=0.01)
    del Xb
    oracles = _check(X, bounds, rec, queries, pyoracle.METRIC_COSINE, paused)
    st = s.stats()
    assert st["capacity"] > st0["capacity"] and st["n_rows"] == total
    assert s.scan_engine() == "i8"
    assert st["n_i8_queries"] > st0["n_i8_queries"], "the int8 filter did not run"
    _final(s, X, queries, pyoracle.METRIC_COSINE, oracles)
    s.drop()


CASES = {"a": case_a, "b": case_b, "c": case_c, "d": case_d, "e": case_e, "f": case_f, "g": case_g}


@pytest.mark.parametrize("case", sorted(CASES))
def test_searches_beside_appends_answer_for_a_published_prefix(case):
    CASES[case]()


@pytest.mark.parametrize("case", ["a", "c", "e", "f"])
def test_searches_beside_appends_with_the_pause_knob(case):
    """the same case with EHX_TEST_PAUSE_US set, in a fresh child process (the knob is read once per process)"""
    env = dict(os.environ, EHX_TEST_PAUSE_US=str(PAUSE_US))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case], env=env, cwd=ROOT, timeout=400,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, "case %s with the pause knob failed (rc %d):\n%s" % (case, r.returncode, r.stderr[-6000:])


if __name__ == "__main__":
    CASES[sys.argv[1]](paused=bool(os.environ.get("EHX_TEST_PAUSE_US")))
    print("case %s ok" % sys.argv[1])
