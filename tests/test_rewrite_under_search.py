"""Searches beside in-place rewrites (flat spaces) and beside any write on a graph space answer exactly as the oracle
does on ONE version of the space.

One writer thread sends batches 1..T with set_prepared while searchers run; version v is the state after batches
1..v.  A search that started after `lo` batches had returned and finished (host call returned, or the caller's stream
synchronised) when `hi` had returned must give, in ids, distance bytes and counts, the oracle's answer on version v for
one v with lo <= v <= min(hi + 1, T) (tests/version_oracle.py, which also explains why the versions are counted by the
writer and not marked by a row per batch).  The inputs come from version_oracle.CASE_INPUTS; tests/test_version_oracle.py
proves on the CPU that any two versions differ in at least two ids for every query, so a stale scan copy, a
half-applied batch or a batch applied in one shard and not in another is no version's answer.

Every answer every searcher collected is checked; no record is skipped."""
import os
import sys
import threading
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import version_oracle as vo  # noqa: E402
from test_append_under_search import _device_searcher, _ehx, _host_searcher  # noqa: E402

pytestmark = pytest.mark.gpu


def _keys(ids):
    return ["%d" % i for i in ids]      # (a space filled by fill_synthetic names its rows by their decimal id)


WRITER_S = 60      # all batches take a few seconds; beyond this the stream is ended and what was collected is checked
JOIN_S = 60        # ONE deadline for all threads after that: whoever has not come back by then is named, the case fails


def _stream(s, ci, make_searchers, pace=0.01):
    """one writer sends ci.batches in order, counting those that have returned; make_searchers(clock) -> callables(stop)
    -> [(lo, answer, hi, tag)].  Returns the records and the number of batches that had returned within WRITER_S (the
    caller checks every record first, then that number).  Progress (batches returned, clock reads of the searchers: two
    per search) goes to stderr every two seconds, so a stall names its thread."""
    preps = [s.prepare_batch(_keys(ids), rows) for ids, rows in ci.batches]
    done, reads = [0], [0]
    errs, records = [], []
    stop, quiet = threading.Event(), threading.Event()

    def clock():
        reads[0] += 1
        return done[0]

    def writer():
        try:
            time.sleep(0.05)    # (the searchers are running before the first batch)
            for prep in preps:
                s.set_prepared(prep)
                done[0] += 1
                time.sleep(pace)
        except Exception as e:  # noqa: BLE001
            errs.append("writer: %r" % (e,))

    def run_searcher(fn):
        try:
            records.extend(fn(stop))
        except Exception as e:  # noqa: BLE001
            errs.append("searcher: %r" % (e,))

    def progress():
        t0 = time.time()
        while not quiet.wait(2.0):
            print("[%s %.0f s] batches returned %d of %d, searches about %d" % (ci.name, time.time() - t0, done[0], len(preps),
                                                                               reads[0] // 2), file=sys.stderr, flush=True)

    w = threading.Thread(target=writer, name="writer")
    ss = [threading.Thread(target=run_searcher, args=(fn,), name="searcher-%d" % i) for i, fn in enumerate(make_searchers(clock))]
    pr = threading.Thread(target=progress, daemon=True)
    for t in ss + [w, pr]:
        t.start()
    w.join(timeout=WRITER_S)
    in_time = done[0]       # (fewer than all: the writer is starved or stuck — the searchers are stopped, so it can finish)
    time.sleep(0.05)
    stop.set()
    hung, deadline = [], time.time() + JOIN_S
    for t in ss + [w]:
        t.join(timeout=max(0.0, deadline - time.time()))
        if t.is_alive():
            hung.append(t.name)
    quiet.set()
    assert not hung, "hung after %d of %d batches and about %d searches: %s" % (done[0], len(preps), reads[0] // 2, hung)
    assert not errs, errs
    assert done[0] == len(preps)
    return records, in_time


def _inflight_device_searcher(s, Q, k, tag, clock, depth=4):
    """`depth` knn_device calls back to back on one stream, each into its own buffers, nothing waited for in between:
    lo is read before the first, hi after ONE stream.synchronize(), and every one of them is a record"""
    import torch
    st = torch.cuda.Stream()
    q = torch.from_numpy(Q).cuda()
    B = Q.shape[0]
    bufs = [(torch.empty((B, k), dtype=torch.int64, device="cuda"), torch.empty((B, k), dtype=torch.float32, device="cuda"),
             torch.empty((B,), dtype=torch.int32, device="cuda")) for _ in range(depth)]

    def fn(stop):
        out = []
        while not stop.is_set():
            lo = clock()
            for ids, dst, cnt in bufs:
                s.knn_device(q, k, ids, dst, cnt, stream=st.cuda_stream)
            st.synchronize()
            hi = clock()
            for ids, dst, cnt in bufs:
                out.append((lo, (ids.cpu().numpy().astype(np.uint64), dst.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32)),
                            hi, tag))
        return out
    return fn


def _check(ci, oracles, records):
    """every answer is some version's inside its window; the searches started under >= 3 different versions and >= 3
    batches committed between some search's lo and hi (the thresholds of test_append_under_search.py's _check)"""
    T = len(ci.batches)
    answered = {}
    for lo, ans, hi, tag in records:
        v = oracles[tag].assert_is_some_version(*ans, lo, hi)
        answered.setdefault(tag, set()).add(v)
    assert set(answered) == set(ci.queries), "a searcher collected nothing: %r" % sorted(answered)
    seen = {lo for lo, _, _, _ in records if lo < T}
    assert len(seen) >= 3, "the searches started under %d versions only" % len(seen)
    overlapped = {b for lo, _, hi, _ in records for b in range(lo + 1, hi + 1)}
    assert len(overlapped) >= 3, "searches overlapped %d batches only" % len(overlapped)
    return {"searches": len(records), "versions_seen_as_lo": len(seen), "batches_overlapped": len(overlapped),
            "versions_answered": {t: len(v) for t, v in sorted(answered.items())}}


def _final(s, ci, oracles, X, h=None):
    """the final state is the last version's answer; Get of rewritten keys returns the last vector written (as the space
    holds it); graph spaces: the graph is the oracle's after the last batch; nothing went uncertified"""
    T = len(ci.batches)
    for tag, (Q, k) in ci.queries.items():
        ids, dist, cnt = s.knn(Q, k)
        oids, odist, ocnt = oracles[tag].answer(T)
        np.testing.assert_array_equal(cnt, ocnt)
        np.testing.assert_array_equal(ids, oids)
        assert dist.tobytes() == odist.tobytes(), tag
    assert len(s) == len(X)
    for ids, _ in ci.batches:
        for i in list(ids[:6]) + list(ids[-3:]):
            assert s.get("%d" % i).tobytes() == X[int(i)].tobytes(), "Get of key %d is not the last vector written" % i
    if h is not None:
        from test_graph_parity import _same_graph
        _same_graph(s, h)
    assert s.stats()["n_uncertified"] == 0


def _report(name, summary, st, extra=""):
    keep = ("n_queries", "n_i8_queries", "n_i8_fallback", "n_filter_queries", "n_filter_fallback", "n_exhaustive",
            "n_rerank", "n_uncertified", "n_dist", "n_hops")
    print("%s: %s counters %s %s" % (name, summary, {f: st[f] for f in keep}, extra), flush=True)


def _flat(name, make_space, searchers, engine, counter, pace=0.01, also=None):
    ehx = _ehx()
    assert vo.SEED_CORPUS == ehx.SEED_CORPUS
    ci = vo.CASE_INPUTS[name]()
    s = make_space(ehx, ci)
    assert len(s) == ci.n
    if engine:
        assert s.scan_engine() == engine
    c0 = s.stats()[counter]
    oracles, X, _ = ci.versions()
    rec, in_time = _stream(s, ci, lambda clock: searchers(s, ci, clock), pace)
    summary = _check(ci, oracles, rec)
    assert in_time == len(ci.batches), "the writer got %d of %d batches through in %d s beside the searches" % (
        in_time, len(ci.batches), WRITER_S)
    if engine:
        assert s.scan_engine() == engine
    st = s.stats()
    assert st[counter] > c0, "%s did not grow: the engine the case names did not run" % counter
    # ... and it ANSWERED: a filter whose copy is stale after a rewrite loses its certificate, and the next engine answers in
    # its place, correctly — the answers alone would not show it.  The named filter must have answered the majority.
    if engine == "i8":
        assert 2 * st["n_i8_fallback"] < st["n_i8_queries"], "the int8 filter answered %d of %d queries only" % (
            st["n_i8_queries"] - st["n_i8_fallback"], st["n_i8_queries"])
    if engine == "f16":
        assert 2 * st["n_filter_fallback"] < st["n_filter_queries"], "the fp16 filter answered %d of %d queries only" % (
            st["n_filter_queries"] - st["n_filter_fallback"], st["n_filter_queries"])
    if also:
        also(st)
    _final(s, ci, oracles, X)
    _report(name, summary, s.stats())
    s.drop()


def _synthetic_space(prefix, metric, **kw):
    def make(ehx, ci):
        s = ehx.Space.unique(prefix, ci.d, metric=metric(ehx), **{k: v(ehx) for k, v in kw.items()})
        s.fill_synthetic(ehx.SEED_CORPUS, 0, ci.n, True)
        return s
    return make


def _set_space(prefix, metric, **kw):
    def make(ehx, ci):
        s = ehx.Space.unique(prefix, ci.d, metric=metric(ehx), **{k: v(ehx) for k, v in kw.items()})
        s.set_batch(_keys(range(ci.n)), ci.X0)
        return s
    return make


COS = lambda ehx: ehx.METRIC_COSINE     # noqa: E731
L2 = lambda ehx: ehx.METRIC_L2SQ        # noqa: E731


def _host_and_device(s, ci, clock):
    return [(_device_searcher if t == "dev" else _host_searcher)(s, *ci.queries[t], t, clock) for t in ci.queries]


# ---- the cases -------------------------------------------------------------------------------------------------------

def case_r_i8():
    """f32 cosine, 65 627 x 256, fill_synthetic base: the int8 filter, whole sorted tiles re-made under the exclusive
    writer; knn at B = 64 (k = 10, 48), knn_device at B = 256"""
    _flat("r_i8", _synthetic_space("rus_i8", COS), _host_and_device, "i8", "n_i8_queries")


def case_r_i8_l2():
    """f32 L2^2, 32 825 x 128, norms spread +-1 % inside the tiles; the rewrites make rows longer and shorter (lane-group
    margins, a tile's min B raised and lowered)"""
    _flat("r_i8_l2", _set_space("rus_l2", L2), _host_and_device, "i8", "n_i8_queries")


def case_r_f16rows():
    """DTYPE_F16 cosine, 32 898 x 512: the int8 copy made from the rounded rows, the re-rank on the binary16 rows"""
    _flat("r_f16rows", _synthetic_space("rus_h", COS, dtype=lambda ehx: ehx.DTYPE_F16), _host_and_device, "i8", "n_i8_queries")


def case_r_f16flt():
    """f32 cosine below i8_min_rows: the fp16 filter copy refreshed in place; knn at B = 64, knn_device at B = 128"""
    _flat("r_f16flt", _synthetic_space("rus_f", COS), _host_and_device, "f16", "n_filter_queries")


def case_r_f32_paged():
    """two small f32 cosine spaces (set_scan is a setting of the space): one fixed at SCAN_F32, one searched at k = 65 and
    200 and by knn_device at k = 100 (the paged exhaustive pass: no page of one version beside a page of another)"""
    _flat("r_f32", _synthetic_space("rus_32", COS, scan=lambda ehx: ehx.SCAN_F32), _host_and_device, "f32", "n_queries")
    _flat("r_paged", _synthetic_space("rus_pg", COS), _host_and_device, None, "n_exhaustive")


def case_r_one():
    """f32 cosine, 4 021 x 128, four threads each sending ONE query per call (the one-launch path; as in case e of
    test_append_under_search.py, that this path serves is assumed from the shape, n_exhaustive counts it with others)"""
    _flat("r_one", _synthetic_space("rus_one", COS), _host_and_device, None, "n_exhaustive")


def case_r_shards():
    """f32 L2^2, shards = 3, 9 000 x 96, every batch's rows spread over all three shards (test_version_oracle.py): no answer
    may mix shard states.  The parent counts a query once, its engine counters add up the shards': every query ran on all
    three shards when the engines' counts are three times the parent's."""
    def all_shards(st):
        assert st["n_rows"] == 9000
        assert st["n_i8_queries"] + st["n_filter_queries"] + st["n_exhaustive"] >= 3 * st["n_queries"] > 0, st
    _flat("r_shards", _set_space("rus_sh", L2, shards=lambda ehx: 3), _host_and_device, None, "n_queries", also=all_shards)


def _graph(name, dtype):
    ehx = _ehx()
    ci = vo.CASE_INPUTS[name]()
    cap = ci.n + ci.appends[2] + 50
    assert cap < ci.total, "the capacity must be below the final count: the arrays move mid-stream"
    s = ehx.Space.unique("rus_" + name, ci.d, metric=ehx.METRIC_L2SQ if ci.metric == "l2" else ehx.METRIC_COSINE,
                         mode=ehx.MODE_GRAPH, build_batch=1, ef=ci.ef, initial_capacity=cap, dtype=dtype(ehx))
    s.set_search_width(1)       # the strict walk: bit-identical to the oracle's searchKnn (test_graph_parity.py)
    s.set_batch(_keys(range(ci.n)), ci.X0)
    cap0 = s.stats()["capacity"]
    assert cap0 < ci.total
    oracles, X, h = ci.versions()
    hops0 = s.stats()["n_hops"]

    def searchers(clock):
        out = []
        for t, (Q, k) in ci.queries.items():
            out.append(_inflight_device_searcher(s, Q, k, t, clock) if t == "dev" else _host_searcher(s, Q, k, t, clock))
        return out

    rec, in_time = _stream(s, ci, searchers, pace=0.01)
    summary = _check(ci, oracles, rec)
    assert in_time == len(ci.batches), "the writer got %d of %d batches through in %d s beside the searches" % (
        in_time, len(ci.batches), WRITER_S)
    st = s.stats()
    assert st["n_hops"] > hops0, "the graph walk did not run"
    assert st["capacity"] > cap0 and st["n_rows"] == ci.total, "the arrays did not grow mid-stream"
    _final(s, ci, oracles, X, h)
    _report(name, summary, s.stats(), "capacity %d -> %d" % (cap0, st["capacity"]))
    s.drop()


def case_g_strict():
    """graph, L2^2, 6 500 x 64 growing to 8 000, build_batch = 1, ef 64: batches alternate updates of ~50 known keys (the
    entry point and one key twice among them) and appends of 300 fresh keys past the initial capacity; host B = 32, host
    one-query calls, and a device searcher with four batches in flight on its stream"""
    _graph("g_strict", lambda ehx: ehx.DTYPE_F32)


def case_g_cos16():
    """graph, cosine, DTYPE_F16, 3 000 x 100 growing to 4 000 (row length not a multiple of 16): the search copy re-made
    from the rounded rows on update"""
    _graph("g_cos16", lambda ehx: ehx.DTYPE_F16)


CASES = {"r_i8": case_r_i8, "r_i8_l2": case_r_i8_l2, "r_f16rows": case_r_f16rows, "r_f16flt": case_r_f16flt,
         "r_f32_paged": case_r_f32_paged, "r_one": case_r_one, "r_shards": case_r_shards, "g_strict": case_g_strict,
         "g_cos16": case_g_cos16}


@pytest.mark.parametrize("case", sorted(CASES))
def test_searches_beside_rewrites_answer_for_one_version(case):
    CASES[case]()


if __name__ == "__main__":
    import faulthandler
    faulthandler.dump_traceback_later(WRITER_S + JOIN_S + 90, exit=True)     # (every thread's stack, should a case outlive its joins)
    CASES[sys.argv[1]]()
    print("case %s ok" % sys.argv[1])
