"""GPU tests of the profile search (ehx_combine_rows_device, ehx_knn_profile*; ehx_profile.cpp, k_profile.hip).

The targets' reference is the definition of include/ehx.h restated in numpy float32 (_strands) over the rows read back with
get_batch: the kernel's bytes must equal it.  The search's reference is the CPU oracle alone: pyoracle.exhaustive on the
reference targets at k + the longest list, every query's listed ids dropped, the first k of what remains."""
import ctypes as C
import functools

import numpy as np
import pytest

import largek_cases as lc
from oracle import pyoracle

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402

EM = {"l2": ehx.METRIC_L2SQ, "ip": ehx.METRIC_IP, "cosine": ehx.METRIC_COSINE}
NO_ID = np.uint64(2**64 - 1)
f32 = np.float32
_spaces = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_spaces():
    yield
    for s, _ in _spaces.values():
        s.drop()


def _space(name, X, metric="l2", **kw):
    """a space of rows X under keys k<i>, made once -> (the space, its rows as get_batch returns them)"""
    if name not in _spaces:
        s = ehx.Space.unique("profile-" + name, X.shape[1], metric=EM[metric], initial_capacity=len(X), **kw)
        keys = ["k%d" % i for i in range(len(X))]
        s.set_batch(keys, X)
        _spaces[name] = (s, s.get_batch(keys))
    return _spaces[name]


def _strands(R, ids, w):
    """the definition: eight fp32 strands over the list as given, every multiply and add rounded on its own -> (t, valid)"""
    acc = np.zeros((8, R.shape[1]), dtype=f32)
    for e, (i, we) in enumerate(zip(ids, w)):
        if i < len(R):
            acc[e % 8] = acc[e % 8] + f32(we) * R[int(i)]
    t = acc[0]
    for s in range(1, 8):
        t = t + acc[s]
    return t, int((np.asarray(ids, dtype=np.uint64) < len(R)).any())


def _lists(n, lengths, seed):
    """random ids of the rows — repeats come by themselves — with ids at and beyond the row count in places 2 and 5, and
    signed weights with zeros"""
    rng = np.random.default_rng(seed)
    ids = [rng.integers(0, n, L).astype(np.uint64) for L in lengths]
    for l in ids:
        if len(l) >= 7:
            l[2], l[5] = n, n + 2**40
            l[6] = l[0]
    w = [np.where(rng.random(len(l)) < 0.1, 0, rng.standard_normal(len(l))).astype(f32) for l in ids]
    return ids, w


def _device(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.tensor(a.view(np.int64) if a.dtype == np.uint64 else a, device="cuda")


def _combine(s, ids, w):
    import torch
    off = np.concatenate([[0], np.cumsum([len(l) for l in ids])]).astype(np.uint64)
    out = torch.full((len(ids), s.dims), 7.0, device="cuda")
    valid = torch.full((len(ids),), 5, dtype=torch.int32, device="cuda")
    s.combine_rows_device(_device(np.concatenate(ids)), _device(off), None if w is None else _device(np.concatenate(w)), out, valid)
    torch.cuda.synchronize()
    return out.cpu().numpy(), valid.cpu().numpy()


# ---- 1. the targets: bytes equal to the definition, every row layout, the lengths around the strands and the group of 4 ----

LENGTHS = (0, 1, 7, 8, 9, 67, 4096)
KINDS = {"f32-64": (64, {}), "f32-100": (100, {}), "f16-64": (64, {"dtype": ehx.DTYPE_F16}),
         "graph-40": (40, {"mode": ehx.MODE_GRAPH, "M": 16})}   # (permuted rows; 40: a partial 16-float block)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", list(KINDS))
def test_targets_are_the_definition_to_the_byte(kind, weighted):
    dims, kw = KINDS[kind]
    s, R = _space(kind, lc.gauss(300, dims, 1, 11)[0], **kw)
    ids, w = _lists(300, LENGTHS, 3)
    ids.append(np.array([300, 2**40, 2**63], dtype=np.uint64))   # names no row
    w.append(np.ones(3, dtype=f32))
    got, valid = _combine(s, ids, w if weighted else None)
    ones = [np.ones(len(l), dtype=f32) for l in ids]
    want = [_strands(R, l, x) for l, x in zip(ids, w if weighted else ones)]
    assert valid.tolist() == [v for _, v in want] == [0, 1, 1, 1, 1, 1, 1, 0]
    assert got.tobytes() == np.stack([t for t, _ in want]).tobytes()
    # against float64: (L / 8 + 9) roundings of at most 2^-24 relative on a component's path — not a measurement
    for t, l, x in zip(got, ids, w if weighted else ones):
        ok = l < 300
        terms = x[ok].astype(np.float64)[:, None] * R[l[ok].astype(np.int64)].astype(np.float64)
        assert (np.abs(t - terms.sum(0)) <= (len(l) / 8 + 9) * 2.0**-24 * np.abs(terms).sum(0)).all()


@pytest.mark.parametrize("nq", [1, 256])   # 1: a unit per lane, 4 slabs (2 of binary16); 256: 3 units per lane (2), the last slab short
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_wide_rows_are_cut_into_slabs(dtype, nq):
    s, R = _space(dtype + "-840", lc.gauss(300, 840, 1, 12)[0], **({"dtype": ehx.DTYPE_F16} if dtype == "f16" else {}))
    ids, w = _lists(300, [(67, 9, 33, 8)[i % 4] for i in range(nq)], 4)
    got, valid = _combine(s, ids, w)
    assert got.tobytes() == np.stack([_strands(R, l, x)[0] for l, x in zip(ids, w)]).tobytes() and valid.all()


# ---- 2. the search: the except route's answer for the reference targets, under the lists themselves ----

def _counters(s):
    out = (C.c_uint64 * 5)()
    C.CDLL(_lib.LIB_PATH).ehx_test_except_counters(s._h, out)
    return np.array(list(out), dtype=np.int64)   # scan route, handed to the exact route, of those overflowed, scan passes, calls


@functools.lru_cache(maxsize=None)
def _case(name, metric, L, depth):
    """lists of length L for 64 queries — query 5's empty, query 9's all out of range — their reference targets and the
    oracle's lists for them"""
    s, R = _spaces[name]
    ids, w = _lists(len(R), [L] * 64, 6)
    ids[5], w[5] = ids[5][:0], w[5][:0]
    ids[9], w[9] = np.array([len(R), 2**40], dtype=np.uint64), np.ones(2, dtype=f32)
    T = np.stack([_strands(R, l, x)[0] for l, x in zip(ids, w)])
    return ids, w, pyoracle.exhaustive(np.ascontiguousarray(R), T, min(depth, len(R)), lc.OM[metric])


def _expect(deep, ids, k, n):
    oids, odist, ocnt = deep
    want = np.full((64, k), NO_ID), np.full((64, k), np.inf, dtype=f32), np.zeros(64, dtype=np.uint32)
    for i in range(64):
        if not (ids[i] < n).any():
            continue
        keep = ~np.isin(oids[i, :ocnt[i]], ids[i])
        m = min(k, int(keep.sum()))
        assert m == k or oids.shape[1] == n, "the oracle's depth"
        want[0][i, :m], want[1][i, :m], want[2][i] = oids[i, :ocnt[i]][keep][:m], odist[i, :ocnt[i]][keep][:m], m
    return want


def _assert_exact(got, want, what):
    for g, w, name in zip(got, want, ("ids", "distance bytes", "counts")):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), "%s: %s differ" % (what, name)


@pytest.mark.parametrize("L", [1, 100, 4096])
@pytest.mark.parametrize("k", [10, 256])
@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_the_search_is_the_except_route_on_the_reference_targets(metric, k, L):
    s, R = _space("gauss-" + metric, lc.gauss(20000, 64, 64, 1)[0], metric)
    assert s.scan_engine() == "i8"
    ids, w, deep = _case("gauss-" + metric, metric, L, 256 + L)
    c0 = _counters(s)
    got = s.knn_profile(k, ids, w)
    _assert_exact(got, _expect(deep, ids, k, 20000), "%s k=%d L=%d" % (metric, k, L))
    assert got[2][5] == 0 and got[2][9] == 0 and (got[0][[5, 9]] == NO_ID).all() and np.isinf(got[1][[5, 9]]).all()
    dc = _counters(s) - c0
    assert dc[0] > 0 and dc[0] + dc[1] == 64 and dc[3] == 3 and dc[4] == 1, dc   # the scan route answered, in its 3 passes


@pytest.mark.parametrize("kind", ["f16", "graph"])
def test_binary16_and_graph_spaces_take_the_exact_route(kind):
    X = lc.gauss(20000, 64, 64, 1)[0]
    kw, X = ({"dtype": ehx.DTYPE_F16}, X[:2000]) if kind == "f16" else ({"mode": ehx.MODE_GRAPH, "M": 16}, np.ascontiguousarray(X[:2000, :16]))
    s, R = _space("exact-" + kind, X, **kw)
    ids, w, deep = _case("exact-" + kind, "l2", 100, 110 + 100)
    c0 = _counters(s)
    _assert_exact(s.knn_profile(10, ids, w), _expect(deep, ids, 10, 2000), kind)
    assert (_counters(s) - c0).tolist() == [0, 64, 0, 0, 1]


def test_keys_and_device_forms_equal_the_host_form():
    import torch
    s, R = _space("gauss-l2", lc.gauss(20000, 64, 64, 1)[0], "l2")
    ids, w, _ = _case("gauss-l2", "l2", 100, 256 + 100)
    want = s.knn_profile(10, ids, w)
    keys = [["k%d" % r if r < 20000 else "never-stored-%d" % r for r in l] for l in ids]   # unknown keys keep their places
    _assert_exact(s.knn_profile_keys(10, keys, w), want, "keys")
    off = np.concatenate([[0], np.cumsum([len(l) for l in ids])]).astype(np.uint64)
    o = (torch.full((64, 10), -7, dtype=torch.int64, device="cuda"), torch.full((64, 10), -7.0, device="cuda"),
         torch.full((64,), 77, dtype=torch.int32, device="cuda"))
    st = torch.cuda.Stream()
    s.knn_profile_device(10, _device(np.concatenate(ids)), _device(off), _device(np.concatenate(w)), *o, stream=st.cuda_stream)
    st.synchronize()
    _assert_exact((o[0].cpu().numpy().view(np.uint64), o[1].cpu().numpy(), o[2].cpu().numpy().view(np.uint32)), want, "device")
