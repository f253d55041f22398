"""CPU: the checks H1-H8 of the fp16 filter scan (tests/f16_checks.py) pass on the numpy model of the device pipeline
(tests/f16_model.py, device layout) and each of them fails on the mutation it exists for; the fp32 scan's list check
likewise.  And the reason the ALIGNED rows exist: with eps halved the soundness check H5 still passes on Gaussian rows and
fails on them."""
import numpy as np
import pytest

import f16_checks as ck
import f16_layout as L
import f16_model as M
from i8_checks import CheckError
from i8_model import _true_distance

f32 = np.float32
N_PUB, CAP = 2200, 2560
KP = 30
PLAN = dict(tile0=0, n_tiles=9, n_chunks=4, tiles_per_chunk=3)      # (chunk 3 has no tiles)


def _data(rng, d, metric, aligned):
    X = rng.standard_normal((N_PUB, d)).astype(f32)
    if metric != "cosine":
        X *= (10.0 ** rng.uniform(-1, 1, (N_PUB, 1))).astype(f32)
    X[7] = 0
    X[40:48] = X[40]                                              # equal scores: ties at the thresholds
    if aligned:
        A = np.concatenate([M.aligned_rows(rng, d, 16), M.aligned_rows(rng, d, 16, above=True)])
        X[100:132] = A
        Q = np.concatenate([A[:8], -A[16:24], rng.standard_normal((8, d)).astype(f32)])
    else:
        Q = np.concatenate([X[:8] + f32(1e-3) * rng.standard_normal((8, d)).astype(f32), X[40:41], np.zeros((1, d), dtype=f32),
                            rng.standard_normal((14, d)).astype(f32)])
    if metric != "cosine":
        Q = Q * f32(3.0)
    return X, np.ascontiguousarray(Q, dtype=f32)


class Model:
    def __init__(self, d, metric, aligned=False, eps_scale=1.0, seed=5, **mut):
        rng = np.random.default_rng(seed)
        self.d, self.metric = d, metric
        self.X, self.Q = _data(rng, d, metric, aligned)
        self.nq = len(self.Q)
        x16, rowp, unsafe = M.make_scan16(self.X, metric, d, CAP, truncate=mut.get("truncate", False),
                                          table=mut.get("x_table", L.SWIZZLE))
        self.snap = ck.Snapshot16(x16, rowp, unsafe, L.ld16_of(d), CAP)
        self.q16, self.gamma, self.quv, self.q_rows = M.prep_queries16(self.Q, metric, d, repeat=mut.get("repeat", True))
        self.eps = M.scan16_eps(d)
        self.S = M.dump_scores(self.snap.X16, self.snap.rowp16, self.q16, self.gamma, self.nq, d, 0, CAP, f32(self.eps * f32(eps_scale)))

    def static_checks(self):
        ck.check_h1(self.snap, self.X, self.d, N_PUB)
        ck.check_h2(self.snap, self.X, self.metric, self.d, N_PUB)
        return ck.check_h3(self.Q, self.d, self.metric, self.q16, self.gamma, self.quv, self.q_rows)

    def lists(self, case, kprime=KP):
        sample = M.sample_select(self.S[:L.SAMPLE_TILES * L.TILE], kprime)
        g = ck.h7_thresholds(self.S, N_PUB, case, kprime, sample)
        part = M.collect_pass(self.S, g, kprime, n_pub=N_PUB, **PLAN)
        return g, part


@pytest.mark.parametrize("metric", ["cosine", "ip", "l2"])
@pytest.mark.parametrize("d", [20, 64, 200])
def test_checks_pass_on_the_model(d, metric):
    m = Model(d, metric, aligned=(d == 64))
    Hq = m.static_checks()
    assert ck.check_h4(m.snap, m.S[:2048], 0, Hq, m.gamma, m.eps) < 1.0
    assert ck.check_h4(m.snap, m.S[512:], 512, Hq, m.gamma, m.eps) < 1.0
    worst = ck.check_h5(m.snap, m.S, m.X, m.Q, metric, m.quv, N_PUB, _true_distance)
    assert worst <= 2e-6
    for kprime in (9, 30, 56):
        ck.check_h6(m.S[:2048], kprime, M.sample_select(m.S[:2048], kprime))
        for case in range(ck.N_THRESHOLD_CASES):
            g, part = m.lists(case, kprime)
            ck.check_h7(m.S, g, part, 0, kprime, PLAN["tile0"], PLAN["n_tiles"], PLAN["tiles_per_chunk"], N_PUB)
            merged, g_out = M.merge(part, g, kprime)
            ck.check_h8(part, merged, g, g_out, kprime)
            if case == 2:
                assert (part == L.KEY_INF).all() and (g_out == g).all()
            if case == 0:
                assert (part[:, :6, kprime - 1] != L.KEY_INF).all()


def test_threshold_cases_exclude_and_keep_what_they_say():
    m = Model(64, "cosine")
    q = 8                                           # the query that equals rows 40..47: eight equal scores
    assert len(np.unique(m.S[40:48, q].view(np.uint32))) == 1
    keys = np.sort(L.make_key(m.S[:N_PUB, q], np.arange(N_PUB)))
    assert list(L.key_id(keys[:8])) == list(range(40, 48))
    g = np.full(m.nq, keys[5], dtype=np.uint64)     # exactly row 45's key
    got = L.key_id(M.collect_pass(m.S, g, KP, n_pub=N_PUB, **PLAN)[q].ravel())
    assert sorted(got[got != 0xFFFFFFFF]) == [40, 41, 42, 43, 44]
    g = np.full(m.nq, keys[5] | np.uint64(0xFFFFFFFF), dtype=np.uint64)
    got = L.key_id(M.collect_pass(m.S, g, KP, n_pub=N_PUB, **PLAN)[q].ravel())
    assert sorted(got[got != 0xFFFFFFFF]) == list(range(40, 48))


def _fails(check, fn):
    with pytest.raises(CheckError) as e:
        fn()
    assert e.value.check == check, str(e.value)


def test_h1_fails_on_truncation_and_on_a_swapped_swizzle():
    m = Model(64, "l2", truncate=True)
    _fails("H1", lambda: ck.check_h1(m.snap, m.X, m.d, N_PUB))
    m = Model(64, "l2", x_table=(0, 2, 3, 1))
    _fails("H1", lambda: ck.check_h1(m.snap, m.X, m.d, N_PUB))
    m = Model(20, "l2")
    m.snap.X16[L.scan16_index(3, 21, m.snap.ld16)] = np.float16(1e-3).view(np.uint16)
    _fails("H1", lambda: ck.check_h1(m.snap, m.X, m.d, N_PUB))


def test_h2_fails_on_wrong_parameters():
    for metric, row, col, val in (("cosine", 5, 0, -1.0000001), ("ip", 5, 1, 0.99999994), ("l2", 5, 1, None), ("l2", N_PUB + 3, 0, -1.0),
                                  ("l2", CAP + 511, 1, 1.0)):
        m = Model(64, metric)
        m.snap.rowp16[row, col] = f32(val) if val is not None else m.snap.rowp16[row, col] * f32(1.00001)
        _fails("H2", lambda: ck.check_h2(m.snap, m.X, metric, 64, N_PUB))
    m = Model(64, "l2")
    m.snap.unsafe[0] = 1
    _fails("H2", lambda: ck.check_h2(m.snap, m.X, "l2", 64, N_PUB))


def test_h3_fails_on_missing_repeated_stages_and_wrong_parameters():
    m = Model(64, "l2", repeat=False)
    _fails("H3", m.static_checks)
    m = Model(64, "l2")
    m.gamma[3] *= f32(1.00001)
    _fails("H3", m.static_checks)
    m = Model(64, "ip")
    m.quv[m.nq + 2, 0] = 2
    _fails("H3", m.static_checks)


def test_h4_fails_when_eps_is_halved():
    m = Model(64, "cosine", eps_scale=0.5)
    Hq = m.static_checks()
    _fails("H4", lambda: ck.check_h4(m.snap, m.S[:2048], 0, Hq, m.gamma, m.eps))


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_h5_with_eps_halved_passes_on_gaussian_rows_and_fails_on_aligned_rows(metric):
    """why the aligned kind exists: an eps of half the size goes unnoticed on Gaussian data"""
    m = Model(64, metric, aligned=False, eps_scale=0.5)
    ck.check_h5(m.snap, m.S, m.X, m.Q, metric, m.quv, N_PUB, _true_distance)
    m = Model(64, metric, aligned=True, eps_scale=0.5)
    _fails("H5", lambda: ck.check_h5(m.snap, m.S, m.X, m.Q, metric, m.quv, N_PUB, _true_distance))


@pytest.mark.parametrize("d,reach", [(64, 0.85), (1024, 0.85), (4096, 0.85)])
def test_aligned_rows_reach_the_worst_case_of_the_rounding_error(d, reach):
    """the float64 model error <q^, x^> - <fp16(q^), fp16(x^)> of the aligned set, rows queried by themselves (below) and by
    their negatives (above), comes within 15 % of 2^-10; Gaussian rows stay far from it"""
    rng = np.random.default_rng(d)
    worst = 0.0
    for above in (False, True):
        A = M.aligned_rows(rng, d, 16, above=above)
        xh = A.astype(np.float64) / np.linalg.norm(A.astype(np.float64), axis=1, keepdims=True)
        h = M.round16(M._unit32(A)[0]).astype(np.float64)
        sign = -1.0 if above else 1.0
        err = sign * (xh * xh).sum(axis=1) - sign * (h * h).sum(axis=1)      # dot - dot16, query = sign * row
        worst = max(worst, float(err.max()))
        assert err.min() > 0
    assert reach * 2.0 ** -10 <= worst <= 2.0 ** -10, worst / 2.0 ** -10
    assert worst + 1e-6 <= float(M.scan16_eps(d))
    G = rng.standard_normal((16, d)).astype(f32)
    gh = G.astype(np.float64) / np.linalg.norm(G.astype(np.float64), axis=1, keepdims=True)
    hg = M.round16(M._unit32(G)[0]).astype(np.float64)
    assert np.abs((gh * gh).sum(axis=1) - (hg * hg).sum(axis=1)).max() < 0.3 * 2.0 ** -10


def test_h6_fails_on_an_off_by_one_rank():
    m = Model(64, "ip")
    _fails("H6", lambda: ck.check_h6(m.S[:2048], KP, M.sample_select(m.S[:2048], KP, off_by_one=True)))


def _h7(m, g, part, err=0):
    ck.check_h7(m.S, g, part, err, KP, PLAN["tile0"], PLAN["n_tiles"], PLAN["tiles_per_chunk"], N_PUB)


def test_h7_fails_on_a_dropped_key_an_unsorted_list_and_foreign_keys():
    m = Model(64, "l2")
    g, part = m.lists(0)
    _fails("H7", lambda: _h7(m, g, part, err=1))
    q = 4
    lst = int(np.argmin(part[q, :, 0]))                  # the list that holds the query's best key ...
    p = part.copy()
    p[q, lst, :-1] = part[q, lst, 1:]                    # ... loses it (a key dropped in a retry round)
    p[q, lst, -1] = L.KEY_INF
    _fails("H7", lambda: _h7(m, g, p))
    p = part.copy()
    p[q, lst, [2, 3]] = part[q, lst, [3, 2]]
    _fails("H7", lambda: _h7(m, g, p))
    p = part.copy()
    p[q, lst, 3] = part[q, lst, 2]
    _fails("H7", lambda: _h7(m, g, p))
    p = part.copy()
    p[q, lst, 0] = part[q, lst ^ 1, 0]                   # a row of the other wave row's list
    _fails("H7", lambda: _h7(m, g, p))
    p = part.copy()
    p[q, lst, 0] = part[q, lst, 0] - np.uint64(1 << 32)  # not the dump's score
    _fails("H7", lambda: _h7(m, g, p))
    p = part.copy()
    p[q, 7, 5] = L.make_key(f32(0), 5)                   # a key behind the first empty slot of an empty list
    _fails("H7", lambda: _h7(m, g, p))
    g3, part3 = m.lists(3)
    g_hi = g3.copy()
    g_hi[q] -= np.uint64(1)                              # the lists hold a key that is not below this threshold
    part_all = M.collect_pass(m.S, m.lists(4)[0], KP, n_pub=N_PUB, **PLAN)
    _fails("H7", lambda: _h7(m, g3, part_all))


def test_h8_fails_on_a_wrong_merge_and_a_wrong_threshold():
    m = Model(64, "cosine")
    g, part = m.lists(1)
    merged, g_out = M.merge(part, g, KP)
    ck.check_h8(part, merged, g, g_out, KP)
    bad = merged.copy()
    bad[2, 1:KP] = merged[2, 2:KP + 1]
    _fails("H8", lambda: ck.check_h8(part, bad, g, g_out, KP))
    bad = g_out.copy()
    bad[2] = merged[2, KP]
    _fails("H8", lambda: ck.check_h8(part, merged, g, bad, KP))
    g, part = m.lists(2)                                 # nothing collected: the threshold stays
    merged, g_out = M.merge(part, g, KP)
    _fails("H8", lambda: ck.check_h8(part, merged, g, np.full_like(g, L.KEY_INF), KP))


def test_f32_list_check_passes_on_a_model_and_fails_on_a_lost_row():
    rng = np.random.default_rng(11)
    d, n_pub = 64, 1100
    for metric in ("cosine", "ip", "l2"):
        X, Q = _data(rng, d, metric, aligned=False)
        X = X[:n_pub]
        S64 = ck.f32_scores(X, Q, metric)
        S32 = S64.astype(f32)
        plan = dict(tile0=0, n_tiles=9, n_chunks=4, tiles_per_chunk=3)
        for g in (np.full(len(Q), L.KEY_INF, dtype=np.uint64), L.make_key(np.sort(S32, axis=0)[2 * KP], 0xFFFFFFFF)):
            part = M.collect_pass(S32, g, KP, n_pub=n_pub, tile_rows=L.TILE_F32, **plan)
            args = (S64, X, Q, metric, d, g, part, 0, KP, 0, 9, 3, n_pub)
            ck.check_f32_lists(*args)
            q = 12
            lst = int(np.argmin(part[q, :, 0]))
            p = part.copy()
            p[q, lst, :-1] = part[q, lst, 1:]
            p[q, lst, -1] = L.KEY_INF
            _fails("F32", lambda: ck.check_f32_lists(S64, X, Q, metric, d, g, p, 0, KP, 0, 9, 3, n_pub))
            p = part.copy()
            p[q, lst, 0] = L.make_key(f32(S32[L.key_id(part[q, lst, :1])[0], q] - f32(0.5) * max(1.0, abs(float(S32[:, q].min())))),
                                      L.key_id(part[q, lst, :1])[0])
            _fails("F32", lambda: ck.check_f32_lists(S64, X, Q, metric, d, g, p, 0, KP, 0, 9, 3, n_pub))
