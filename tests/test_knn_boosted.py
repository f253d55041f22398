"""Tests of the boosted kNN (ehx_knn_boosted*, ehx_knn_decay*, ehx_boost.cpp, k_boost.hip).

The reference is the CPU oracle alone: pyoracle.exhaustive at full depth gives every row's canonical distance bytes, the
score is numpy float32 arithmetic (d + w * p, each op rounded by numpy), the order a lexsort on (score, id) — ids equal,
score BYTES equal, counts and tail sentinels equal.  Which route answered is read from ehx_test_boost_counters."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import largek_cases as lc
from oracle import pyoracle

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402
from embeddinghub_amd import build as ehx_build  # noqa: E402

gpu = pytest.mark.gpu
EM = {"l2": ehx.METRIC_L2SQ, "ip": ehx.METRIC_IP, "cosine": ehx.METRIC_COSINE}
NO_ID = np.uint64(2**64 - 1)
f32 = np.float32
PASSES = 3   # of a space of 16 385 .. 65 536 rows at the default growth
NEW = ("ehx_knn_boosted_device", "ehx_knn_boosted", "ehx_knn_decay_device", "ehx_knn_decay")


@functools.lru_cache(maxsize=None)
def _deep(case, metric):
    """every row's canonical distance for a named data set, computed once and shared"""
    X, Q = _data(case)
    return pyoracle.exhaustive(np.ascontiguousarray(X), np.ascontiguousarray(Q), len(X), lc.OM[metric])


def _data(case):
    X, Q = lc.ties()[:2] if case == "ties" else lc.gauss(20000, 64, 64, 1)
    if case == "f16":
        return X[:2000, :32].astype(np.float16).astype(f32), Q[:, :32]
    return {"16000": (X[:16000], Q), "63": (X, Q[:63]), "graph": (X[:2000, :32], Q[:, :32])}.get(case, (X, Q))


def _reference(deep, p, w, k):
    oids, odist, ocnt = deep
    nq = len(ocnt)
    ids, score, cnt = np.full((nq, k), NO_ID), np.full((nq, k), np.inf, dtype=f32), np.zeros(nq, dtype=np.uint32)
    w = np.broadcast_to(np.asarray(1.0 if w is None else w, dtype=f32), (nq,))
    for i in range(nq):
        rid, d = oids[i, :int(ocnt[i])].astype(np.int64), odist[i, :int(ocnt[i])]
        rid, d = rid[rid < len(p)], d[rid < len(p)]          # rows without a penalty are not searched
        with np.errstate(all="ignore"):
            sc = d + w[i] * p[rid]                            # float32: two roundings
        rid, sc = rid[sc == sc], sc[sc == sc]                 # a NaN score is never a neighbour
        top = np.lexsort((rid, sc))[:k]
        ids[i, :len(top)], score[i, :len(top)], cnt[i] = rid[top], sc[top], len(top)
    return ids, score, cnt


def _counters(s):
    out = (C.c_uint64 * 5)()
    C.CDLL(_lib.LIB_PATH).ehx_test_boost_counters(s._h, out)
    return np.array(list(out), dtype=np.int64)   # scan route, handed to the exact route, of those overflowed, scan passes, calls


def _run(s, Q, k, p, w, deep, what, call=None):
    """one call against the reference -> how the counters moved"""
    c0, q0 = _counters(s), s.stats()["n_queries"]
    got = call() if call else s.knn_boosted(Q, k, p, w)
    for g, r, name in zip(got, _reference(deep, p, w, k), ("ids", "score bytes", "counts")):
        assert g.shape == r.shape and g.tobytes() == r.tobytes(), "%s: %s differ" % (what, name)
    assert s.stats()["n_queries"] - q0 == len(Q), what
    return _counters(s) - c0


_spaces = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_spaces():
    yield
    for s in _spaces.values():
        s.drop()


def _space(case, metric, **kw):
    if (case, metric) not in _spaces:
        X = _data(case)[0]
        s = ehx.Space.unique("boost-%s-%s" % (case, metric), X.shape[1], metric=EM[metric], initial_capacity=len(X), **kw)
        s.set_batch(["k%d" % i for i in range(len(X))], X)
        _spaces[(case, metric)] = s
    return _spaces[(case, metric)]


def _penalties(kind, n=20000):
    rng = np.random.default_rng(11)
    return {"zero": (np.zeros(n, dtype=f32), None), "const": (np.full(n, 0.25, dtype=f32), None),
            "uniform w=0.1": (rng.random(n, dtype=f32), 0.1), "uniform w=2": (rng.random(n, dtype=f32), 2.0),
            "signed": (rng.random(n, dtype=f32) * 2 - 1, None)}[kind]


@gpu
@pytest.mark.parametrize("kind", ["zero", "const", "uniform w=0.1", "uniform w=2", "signed"])
@pytest.mark.parametrize("k", [10, 48, 49, 256])
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_the_scan_route_is_exact(metric, k, kind):
    Q = lc.gauss(20000, 64, 64, 1)[1]
    s = _space("gauss", metric)
    assert s.scan_engine() == "i8"
    p, w = _penalties(kind)
    dc = _run(s, Q, k, p, w, _deep("gauss", metric), "%s k=%d %s" % (metric, k, kind))
    assert dc[0] + dc[1] == 64 and dc[2] <= dc[1] and dc[3] == PASSES and dc[4] == 1, "handed on %d: %s" % (dc[1], dc)
    if kind in ("zero", "const"):   # the distance radius is the large-k route's to a few ulps: worst pool 1325 of 4096
        ids, dist, cnt = s.knn(Q, k)
        got = s.knn_boosted(Q, k, p, w)
        assert np.array_equal(got[0], ids) and np.array_equal(got[1], dist + p[0]) and dc[0] == 64 and dc[1] == 0, dc


@gpu
def test_equal_scores_resolve_in_id_order():
    X, Q, at = lc.ties()
    s = _space("ties", "l2")
    p = np.random.default_rng(2).integers(0, 3, 20000).astype(f32)   # integer penalties over 300 copies of query 0's row
    _run(s, Q, 100, p, None, _deep("ties", "l2"), "ties")
    got = s.knn_boosted(Q, 100, p)
    first = at[np.lexsort((at, p[at]))][:100]   # the copies lie at distance 0, every other row some 100 away
    assert np.array_equal(got[0][0].astype(np.int64), first) and np.array_equal(got[1][0], p[first])


@gpu
def test_per_query_weights_and_a_short_penalty_array():
    Q = lc.gauss(20000, 64, 64, 1)[1]
    w = np.random.default_rng(3).random(64, dtype=f32)
    w[::5] = 0
    p = _penalties("uniform w=2", 17000)[0]
    dc = _run(_space("gauss", "ip"), Q, 49, p, w, _deep("gauss", "ip"), "17000 penalties")
    assert dc[0] + dc[1] == 64 and dc[3] == PASSES, dc
    assert (_space("gauss", "ip").knn_boosted(Q, 49, p, w)[0] < 17000).all()


@gpu
def test_nan_and_infinite_penalties():
    Q = lc.gauss(20000, 64, 64, 1)[1]
    deep = _deep("gauss", "l2")
    p = _penalties("uniform w=0.1")[0].copy()
    p[deep[0][:, 0]] = np.nan            # every query's nearest row
    p[deep[0][:, 1]] = np.inf            # ... and its second
    s = _space("gauss", "l2")
    _run(s, Q, 10, p, 0.1, deep, "NaN, +Inf")
    assert not np.isin(s.knn_boosted(Q, 10, p, 0.1)[0], deep[0][:, 0]).any()
    p[7] = -np.inf                       # the floor's flag sends the whole call to the exact route
    dc = _run(s, Q, 10, p, 0.1, deep, "a penalty of -Inf")
    assert dc.tolist() == [0, 64, 0, 0, 1], dc


@gpu
@pytest.mark.parametrize("origin,span", [(2500, 10 ** 9), (2500, 700), (0, 4000), (9000, 5000), (2 ** 32 - 1, 2 ** 32 - 1)])
def test_the_column_form_equals_the_array_form(origin, span):
    Q = lc.gauss(20000, 64, 64, 1)[1]
    s = _space("gauss", "cosine")
    col = (np.arange(20000) % 5000).astype(np.uint32)
    if s.column_get(1, ["k4999"])[0] != 4999:
        s.column_set(1, ["k%d" % i for i in range(20000)], col)
    p = np.minimum(np.abs(col.astype(np.int64) - origin), span).astype(f32)
    w = 2.0 ** -12 if span > 10 ** 6 else 1e-4
    dc = _run(s, Q, 49, p, w, _deep("gauss", "cosine"), "decay", lambda: s.knn_decay(Q, 49, 1, origin, span, w))
    assert dc[0] + dc[1] == 64, dc
    assert np.array_equal(s.knn_decay(Q, 10, 3, 7, 0)[0], s.knn(Q, 10)[0])   # a column never written: one constant, no error


@gpu
@pytest.mark.parametrize("case", ["16000", "63", "f16", "graph"])
def test_the_exact_route(case):
    X, Q = _data(case)
    kw = {"f16": {"dtype": ehx.DTYPE_F16}, "graph": {"mode": ehx.MODE_GRAPH, "M": 16}}.get(case, {})
    s = _space(case, "l2", **kw)
    p = _penalties("signed", len(X))[0]
    w = np.random.default_rng(4).random(len(Q), dtype=f32) * 3
    e0 = s.stats()["n_exhaustive"]
    for k in (10, 256):
        dc = _run(s, Q, k, p, w, _deep(case, "l2"), "%s k=%d" % (case, k))
        assert dc.tolist() == [0, len(Q), 0, 0, 1], dc
    assert s.stats()["n_exhaustive"] == e0   # as the except route's exact route leaves it


@gpu
@pytest.mark.parametrize("what,code", [("k0", _lib.EINVAL), ("k257", _lib.EUNSUPPORTED), ("negative", _lib.EINVAL),
                                       ("nan", _lib.EINVAL), ("null", _lib.EINVAL), ("sharded", _lib.EUNSUPPORTED)])
def test_errors_leave_the_outputs_unwritten(what, code):
    import torch
    Q = lc.gauss(20000, 64, 64, 1)[1]
    s = ehx.Space.unique("boost-sh", 64, metric=ehx.METRIC_L2SQ, shards=2) if what == "sharded" else _space("gauss", "l2")
    if what == "sharded":
        s.set_batch(["k%d" % i for i in range(256)], lc.gauss(20000, 64, 64, 1)[0][:256])
    k = {"k0": 0, "k257": 257}.get(what, 10)
    dq, dp = torch.from_numpy(Q.copy()).cuda(), torch.zeros(20000, device="cuda")
    dw = torch.ones(64, device="cuda")
    dw[5] = {"negative": -1.0, "nan": float("nan")}.get(what, 1.0)
    ids = torch.full((64, max(k, 1)), 7, dtype=torch.int64, device="cuda")
    sc, cnt = torch.full((64, max(k, 1)), 7.0, device="cuda"), torch.full((64,), 7, dtype=torch.int32, device="cuda")
    calls = [lambda: s.knn_boosted_device(dq, k, dp, 20000, ids, None if what == "null" else sc, cnt, dw),
             lambda: s.knn_decay_device(dq, k, 0, 5, 9, ids, None if what == "null" else sc, cnt, dw)]
    if what != "null":   # (the host forms of the binding allocate their own outputs)
        calls += [lambda: s.knn_boosted(Q, k, np.zeros(20000, dtype=f32), dw.cpu().numpy()),
                  lambda: s.knn_decay(Q, k, 0, 5, 9, dw.cpu().numpy())]
    for call in calls:
        with pytest.raises(ehx.EhxError) as e:
            call()
        assert e.value.code == code, what
    torch.cuda.synchronize()
    assert (ids == 7).all() and (sc == 7).all() and (cnt == 7).all()
    if what == "sharded":
        s.drop()


# ---- without a GPU ----

def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ehx_build.ROOT, "include", "ehx.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS and hasattr(raw, name)
        assert callable(getattr(ehx.Space, name[4:]))
    assert hasattr(raw, "ehx_test_boost_counters") and "ehx_test_boost_counters" not in header
    assert "k_boost.hip" in ehx_build.SOURCES and "ehx_boost.cpp" in ehx_build.SOURCES
    assert re.search(r"#define EHX_ABI_VERSION 5\b", header)   # additive: the version stays


def test_boost_kernels_use_no_scratch_and_spill_no_vector_registers(tmp_path):
    src = os.path.join(ehx_build.CSRC, "k_boost.hip")
    flags = [f for f in ehx_build.FLAGS if f != "-shared"] + ehx_build.EXTRA_FLAGS["k_boost.hip"]
    r = subprocess.run([ehx_build.HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o",
                                                    str(tmp_path / "k_boost.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    for kern, count in (("boost_rerank_kernel", 18), ("boost_floor_kernel", 1)):
        assert sum(kern in n for n in names) == count, names
    for what in ("ScratchSize \\[bytes/lane\\]", "VGPRs Spill"):
        vals = re.findall(what + r": (\d+)", r.stderr)
        assert len(vals) == len(names) and all(v == "0" for v in vals), (what, vals)
