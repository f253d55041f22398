"""Nearest-centroid assignment, centroid sums and k-means on the device (ehx_assign_device, ehx_centroid_sums_device,
ehx_kmeans_device) against their definitions in include/ehx.h.

The assignment's reference is the CPU oracle alone: pyoracle.exhaustive(rows, centroids, k = n_rows) scattered into a
[centroids, rows] matrix, argmin per row with ties to the lower centroid, NaN distances no candidates.  The sums' reference
is the eight-strand definition restated in numpy float32 (_strands, as tests/test_knn_profile.py restates it)."""
import ctypes as C

import numpy as np
import pytest

import largek_cases as lc
from oracle import pyoracle

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")
from embeddinghub_amd import _lib  # noqa: E402

EM = {"l2": ehx.METRIC_L2SQ, "ip": ehx.METRIC_IP, "cosine": ehx.METRIC_COSINE}
OM = {"l2": pyoracle.METRIC_L2, "ip": pyoracle.METRIC_IP, "cosine": pyoracle.METRIC_COSINE}
KW = {"f32": {}, "f16": {"dtype": ehx.DTYPE_F16}, "graph": {"mode": ehx.MODE_GRAPH, "M": 16}}
NONE = np.uint32(0xFFFFFFFF)
f32 = np.float32
N = 3001
_spaces = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_spaces():
    yield
    for s, _ in _spaces.values():
        s.drop()


def _space(name, X, metric, kind):
    """a space of rows X, made once -> (the space, its rows as get_batch returns them)"""
    key = (name, metric, kind)
    if key not in _spaces:
        s = ehx.Space.unique("assign-%s-%s-%s" % key, X.shape[1], metric=EM[metric], initial_capacity=len(X), **KW[kind])
        keys = ["k%d" % i for i in range(len(X))]
        s.set_batch(keys, X)
        _spaces[key] = (s, s.get_batch(keys))
    return _spaces[key]


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _counts(s):
    out = (C.c_uint64 * 2)()
    assert C.CDLL(_lib.LIB_PATH).ehx_test_assign_counts(s._h, out) == 0
    return list(out)   # rows certified by the filter, rows answered by the exact kernel


def _assign(s, cent, row0=0, n=None, want_dist=True):
    import torch
    n = len(s) - row0 if n is None else n
    label = torch.full((n,), 5, dtype=torch.int32, device="cuda")
    dist = torch.full((n,), 7.0, device="cuda") if want_dist else None
    s.assign_device(_dev(cent), label, dist, row0=row0, n_rows=n)
    torch.cuda.synchronize()
    return label.cpu().numpy().view(np.uint32), None if dist is None else dist.cpu().numpy()


def _reference(R, cent, metric):
    """the definition: (labels, distances) of every row of R"""
    ids, dists, cnt = pyoracle.exhaustive(R, cent, len(R), OM[metric])
    D = np.full((len(cent), len(R)), np.nan, dtype=f32)
    for c in range(len(cent)):
        D[c, ids[c, :cnt[c]].astype(np.int64)] = dists[c, :cnt[c]]
    none = np.isnan(D).all(axis=0)
    label = np.where(none, 0, np.nanargmin(np.where(none[None, :], f32(0), D), axis=0)).astype(np.uint32)
    dist = D[label, np.arange(len(R))]
    label[none] = NONE
    return label, dist


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), "%s: %d labels differ from the oracle's" % (what, (got[0] != want[0]).sum())
    assert got[1].tobytes() == want[1].tobytes(), "%s: distance bytes differ from the oracle's" % what


def _centroids(R, n_cent, seed):
    """rows of the space, half of them moved a little: some rows sit ON a centroid, near-ties come by themselves"""
    rng = np.random.default_rng(seed)
    cent = R[rng.choice(len(R), n_cent, replace=False)].copy()
    cent[::2] += (0.01 * rng.standard_normal(cent[::2].shape)).astype(f32)
    return cent


# ---- 1. parity: label and distance bytes, every metric, row type, a scalar tail, a partial and several centroid tiles ----

CASES = ([(m, k, 67, 257, 0) for m in EM for k in ("f32", "f16")] + [(m, "f32", 64, 7, 77) for m in EM] +
         [(m, "f32", 64, 1, 0) for m in EM] + [("l2", "f16", 64, 7, 77), ("ip", "f16", 67, 7, 77), ("cosine", "f16", 67, 7, 77),
                                               ("l2", "f32", 768, 257, 0), ("cosine", "f16", 768, 257, 77), ("ip", "f32", 768, 7, 0),
                                               ("l2", "graph", 40, 7, 77)])


@pytest.mark.parametrize("metric,kind,dims,n_cent,row0", CASES)
def test_labels_and_distances_are_the_oracles(metric, kind, dims, n_cent, row0):
    n_all = 300 if kind == "graph" else N   # (a graph space builds its graph as the rows are set)
    s, R = _space("g%d" % dims, lc.gauss(n_all, dims, 1, dims)[0], metric, kind)
    n = n_all - row0 if row0 == 0 else min(2500, n_all - row0 - 1)
    cent = _centroids(R, n_cent, 3)
    before = _counts(s)
    got = _assign(s, cent, row0, n)
    _same(got, _reference(R[row0:row0 + n], cent, metric), "%s %s d=%d C=%d" % (metric, kind, dims, n_cent))
    after = _counts(s)
    assert after[0] - before[0] + after[1] - before[1] == n
    if kind == "graph":
        assert after[0] == before[0]   # block-permuted rows: the exact kernel alone
    assert np.array_equal(_assign(s, cent, row0, n, want_dist=False)[0], got[0])


# ---- 2. the filter is what answers separated data, and gives up where it must ----

def _separated(dims, n_cent, n):
    cent = np.zeros((n_cent, dims), dtype=f32)
    cent[np.arange(n_cent), np.arange(n_cent)] = 3.0   # pairwise sqrt(18) apart
    own = np.arange(n) % n_cent
    X = cent[own] + (1e-4 * np.random.default_rng(5).standard_normal((n, dims))).astype(f32)
    return X, cent, own.astype(np.uint32)


@pytest.mark.parametrize("kind", ["f32", "f16"])
@pytest.mark.parametrize("metric", list(EM))
def test_filter_certifies_every_row_of_separated_data(metric, kind):
    X, cent, own = _separated(64, 16, 1000)
    s, R = _space("sep", X, metric, kind)
    before = _counts(s)
    got = _assign(s, cent)
    after = _counts(s)
    assert (after[0] - before[0], after[1] - before[1]) == (1000, 0)
    assert np.array_equal(got[0], own)
    _same(got, _reference(R, cent, metric), "separated %s %s" % (metric, kind))


@pytest.mark.parametrize("metric", list(EM))
def test_certificate_gives_up_on_ties_and_one_ulp_neighbours(metric):
    X, cent, own = _separated(64, 16, 1000)
    s, R = _space("sep", X, metric, "f32")
    # (i) every centroid twice: nothing can be certified, and the lower index wins
    before = _counts(s)
    got = _assign(s, np.concatenate([cent, cent]))
    after = _counts(s)
    assert (after[0] - before[0], after[1] - before[1]) == (0, 1000)
    assert np.array_equal(got[0], own)
    # (ii) a neighbour one ulp away in one component, in front of and behind the original
    near = cent.copy()
    near[np.arange(16), np.arange(16)] = np.nextafter(f32(3.0), f32(4.0) if metric == "l2" else f32(2.0))
    for both in (np.concatenate([cent, near]), np.concatenate([near, cent])):
        _same(_assign(s, both), _reference(R, both, metric), "one ulp %s" % metric)


# ---- 3. non-finite rows and centroids follow the definition on the exact route ----

@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_non_finite_rows_and_centroids(metric):
    X = lc.gauss(500, 67, 1, 9)[0].copy()
    X[3, 5] = np.nan
    X[100, 66] = np.inf
    X[101, 0] = -np.inf
    X[200] = 0.0
    s, R = _space("nonfinite", X, metric, "f32")
    cent = _centroids(lc.gauss(500, 67, 1, 9)[0], 7, 4)
    # finite centroids: the unsafe rows are handed on one by one
    got = _assign(s, cent)
    want = _reference(R, cent, metric)
    _same(got, want, "non-finite rows %s" % metric)
    assert got[0][3] == NONE and np.isnan(got[1][3])
    # a NaN centroid: the whole call is the exact kernel's, and the centroid is never chosen
    cent[2, 1] = np.nan
    before = _counts(s)
    got = _assign(s, cent)
    assert _counts(s)[0] == before[0]
    _same(got, _reference(R, cent, metric), "NaN centroid %s" % metric)
    assert not (got[0] == 2).any()


# ---- 4. centroid sums: bytes of the strand definition over lists of any length ----

def _strands(R, ids):
    """the definition with every weight 1: eight fp32 strands over the list as given, joined in strand order"""
    acc = np.zeros((8, R.shape[1]), dtype=f32)
    for e, i in enumerate(ids):
        acc[e % 8] = acc[e % 8] + R[int(i)]
    t = acc[0]
    for k in range(1, 8):
        t = t + acc[k]
    return t


SIZES = (0, 1, 4095, 4096, 4097, 8200)


@pytest.mark.parametrize("kind,dims", [("f32", 67), ("f16", 768)])
def test_centroid_sums_are_the_definition_to_the_byte(kind, dims):
    import torch
    labels = np.concatenate([np.full(n, c, dtype=np.uint32) for c, n in enumerate(SIZES)] +
                            [np.full(5, NONE), np.full(5, len(SIZES), dtype=np.uint32), np.full(5, 70000, dtype=np.uint32)])
    labels = labels[np.random.default_rng(2).permutation(len(labels))]
    s, R = _space("sums%d" % dims, lc.gauss(len(labels), dims, 1, 21)[0], "l2", kind)
    sums = torch.full((len(SIZES), dims), 7.0, device="cuda")
    count = torch.full((len(SIZES),), 5, dtype=torch.int32, device="cuda")
    s.centroid_sums_device(_dev(labels), len(SIZES), sums, count)
    torch.cuda.synchronize()
    assert count.cpu().numpy().tolist() == list(SIZES)
    want = np.stack([_strands(R, np.flatnonzero(labels == c)) for c in range(len(SIZES))])
    assert sums.cpu().numpy().tobytes() == want.tobytes()
    # a sub-range: positions are relative to row0, row ids are not
    s.centroid_sums_device(_dev(labels[77:5077]), len(SIZES), sums, count, row0=77, n_rows=5000)
    torch.cuda.synchronize()
    want = np.stack([_strands(R, 77 + np.flatnonzero(labels[77:5077] == c)) for c in range(len(SIZES))])
    assert sums.cpu().numpy().tobytes() == want.tobytes()
    # ... and ehx_combine_rows_device on a list of 4096 still returns the same definition's bytes
    ids = np.random.default_rng(3).integers(0, len(labels), 4096).astype(np.uint64)
    out = torch.full((1, dims), 7.0, device="cuda")
    valid = torch.zeros(1, dtype=torch.int32, device="cuda")
    s.combine_rows_device(torch.from_numpy(ids.view(np.int64)).cuda(), torch.tensor([0, 4096], dtype=torch.int64, device="cuda"), None,
                          out, valid)
    torch.cuda.synchronize()
    assert out.cpu().numpy()[0].tobytes() == _strands(R, ids).tobytes() and valid.item() == 1


# ---- 5. k-means: three Lloyd steps byte for byte a host loop of the references ----

def test_kmeans_is_the_host_loop_of_the_references():
    import torch
    s, R = _space("g67", lc.gauss(N, 67, 1, 67)[0], "l2", "f32")
    start = _centroids(R, 7, 8)
    start[4] = 1000.0   # attracts no row: keeps its bytes
    cent = start.copy()
    for _ in range(3):
        label, _ = _reference(R, cent, "l2")
        for c in range(7):
            ids = np.flatnonzero(label == c)
            if len(ids):
                cent[c] = _strands(R, ids) / f32(len(ids))
    want = _reference(R, cent, "l2")
    assert cent[4].tobytes() == start[4].tobytes()
    d_cent = _dev(start)
    label = torch.full((N,), 5, dtype=torch.int32, device="cuda")
    dist = torch.full((N,), 7.0, device="cuda")
    s.kmeans_device(d_cent, 3, label, dist)
    torch.cuda.synchronize()
    assert d_cent.cpu().numpy().tobytes() == cent.tobytes()
    _same((label.cpu().numpy().view(np.uint32), dist.cpu().numpy()), want, "k-means")
    # iters = 0 from the returned centroids: a plain assignment that moves nothing
    assert s.kmeans_device(d_cent, 0, label, dist) == 0
    _same((label.cpu().numpy().view(np.uint32), dist.cpu().numpy()), want, "k-means, iters = 0")
    assert d_cent.cpu().numpy().tobytes() == cent.tobytes()
    label[:10] = 99
    assert s.kmeans_device(d_cent, 0, label) == 10


# ---- 6. argument rules ----

def test_argument_rules():
    import torch
    s, R = _space("g67", lc.gauss(N, 67, 1, 67)[0], "l2", "f32")
    cent = _dev(R[:7])
    label = torch.full((N,), 5, dtype=torch.int32, device="cuda")
    raw, h = s._L, s._h
    null = C.c_void_p(0)
    cases = [(lambda: raw.ehx_assign_device(h, null, 0, N, cent.data_ptr(), 0, label.data_ptr(), null), _lib.EINVAL),
             (lambda: raw.ehx_assign_device(h, null, 0, N, cent.data_ptr(), 4097, label.data_ptr(), null), _lib.EINVAL),
             (lambda: raw.ehx_assign_device(h, null, 2, N, cent.data_ptr(), 7, label.data_ptr(), null), _lib.EINVAL),
             (lambda: raw.ehx_assign_device(h, null, N + 1, 0, cent.data_ptr(), 7, label.data_ptr(), null), _lib.EINVAL),
             (lambda: raw.ehx_assign_device(h, null, 0, N, null, 7, label.data_ptr(), null), _lib.EINVAL),
             (lambda: raw.ehx_centroid_sums_device(h, null, 0, N + 1, label.data_ptr(), 7, cent.data_ptr(), label.data_ptr()), _lib.EINVAL),
             (lambda: raw.ehx_kmeans_device(h, null, 0, N, 0, 1, cent.data_ptr(), label.data_ptr(), null, None), _lib.EINVAL)]
    for call, code in cases:
        assert call() == code
    s.assign_device(cent, label, None, row0=N, n_rows=0)   # EHX_OK, nothing written
    s.kmeans_device(cent, 2, label, None, row0=5, n_rows=0)
    torch.cuda.synchronize()
    assert (label == 5).all() and cent.cpu().numpy().tobytes() == R[:7].tobytes()
    sh = ehx.Space.unique("assign-sh", 67, metric=ehx.METRIC_L2SQ, shards=2)
    sh.set_batch(["k%d" % i for i in range(100)], R[:100])
    with pytest.raises(ehx.EhxError) as e:
        sh.assign_device(cent, label, None, row0=0, n_rows=100)
    assert e.value.code == _lib.EUNSUPPORTED and "sharded" in str(e.value)
    sh.drop()
