"""The checker of tests/i8_checks.py can fail (CPU, no library): the numpy model of tests/i8_model.py written in the
DEVICE layout through tests/i8_layout.py — ordered tiles, raised steps, tile and group entries, a dump from i8_score, pools
from the epilogue's integer levels — passes C1-C7; each mutation, applied alone, is caught by the check named for it."""
import numpy as np
import pytest

import i8_checks as ck
import i8_layout as L
from i8_model import (_alarm_k, _datasets, _group_b_margin, _kernel_order, _query_params, _row_params_raised,
                      _true_distance)

f32 = np.float32
D_ = 128
N_PUB = 3 * 256 + 100      # three full (ordered) tiles and a straddling tail
CAP = 5 * 256              # ... and a tile nobody wrote
N_EXACT = 4


def _fma(a, b, c):
    """one rounding (the product of two float32 is exact in float64)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(f32)


def model_snapshot(X, metric, d, n_pub, cap):
    ld8 = (d + 63) // 64 * 64
    T = cap // 256
    codes = np.zeros((cap, ld8), dtype=np.int8)
    rowp = np.tile(ck.PAD_ROW, (cap + 512, 1))
    perm = np.tile(np.arange(256, dtype=np.uint8), T)
    tilep = np.tile(ck.PAD_TILE, (T + 2, 1))
    tileg = np.zeros((T + 2, 16), dtype=f32)
    grp = L.i8_group_of_pos(np.arange(256))
    raise_of = np.zeros(cap)                  # by position: raised step / natural step (the e mutation picks the largest)
    e_nat = np.zeros(cap, dtype=f32)
    for t in range((n_pub + 255) // 256):
        rows = np.arange(t * 256, min((t + 1) * 256, n_pub))
        xi, A, B, C, Dd, e = _row_params_raised(X[rows], metric, d)
        pos = np.arange(len(rows))
        if len(rows) == 256:
            with np.errstate(over="ignore"):
                nat_n = np.sqrt((X[rows].astype(f32) ** 2).sum(axis=1, dtype=f32)) if metric == "l2" else np.zeros(256, dtype=f32)
            order = _kernel_order(A, nat_n)                       # rows in rank order
            pos = np.empty(256, dtype=np.int64)
            pos[order] = L.i8_pos_of_rank(np.arange(256))
            tgt = np.empty(256, dtype=f32)
            tgt[order] = np.repeat(np.abs(A[order]).reshape(8, 32).max(axis=1), 32)
            e_nat[t * 256 + pos] = e
            nat_A = np.abs(A)
            xi, A, B, C, Dd, e = _row_params_raised(X[rows], metric, d, tgt)
            raise_of[t * 256 + pos] = np.abs(A) / np.where(nat_A > 0, nat_A, 1)
            perm[t * 256 + pos] = np.arange(256, dtype=np.uint8)
        codes[t * 256 + pos, :d] = xi
        rowp[t * 256 + pos] = np.stack([A, B, C, Dd], axis=1)
        P = rowp[t * 256:(t + 1) * 256]
        tilep[t] = [np.abs(P[:, 0]).max(), np.abs(P[:, 2]).max(), np.abs(P[:, 3]).max(), P[:, 1].min()]
        for gi in range(8):
            tileg[t, gi] = np.abs(P[grp == gi, 0]).max()
            bmin = np.where(P[grp == gi, 1] >= 0, P[grp == gi, 1], 0).min()
            tileg[t, 8 + gi] = bmin if bmin != 0 else -np.inf
    snap = ck.Snapshot(L.layout_x8(codes, ld8), rowp, tilep, tileg, perm, np.zeros(2, dtype=np.uint64), ld8, cap)
    return snap, raise_of, e_nat


def model_dump(snap, qi, qp, n_pos, table=L.SWIZZLE):
    """i8_score of every (position, query) -> (I, S)"""
    I = (snap.codes(table)[:n_pos].astype(np.float64) @ qi.astype(np.float64).T).astype(np.int64)
    P = snap.rowp8[:n_pos]
    t = (qp[None, :, 0] * I.astype(f32)).astype(f32)
    K = _fma(P[:, 1:2], qp[None, :, 2], _fma(P[:, 2:3], qp[None, :, 1], P[:, 3:4]))
    return I, _fma(P[:, 0:1], t, K)


def model_pass(snap, I, S, qp, thr, n_pub, group_b):
    """the epilogue of flat_scan_i8_kernel: one integer level per (tile, lane group, query) from the tile's extremes, the
    group's max |A| and (group_b) the group's B margin; what reaches its level is judged exactly by the flush"""
    nq = len(thr)
    grp = L.i8_group_of_pos(np.arange(256))
    hit = np.zeros(I.shape, dtype=bool)
    for t in range((n_pub + 255) // 256):
        tp = snap.tilep8[t]
        for q in range(nq):
            sq, eq, g = qp[q, 0], qp[q, 1], qp[q, 2]
            kq = _alarm_k(tp[3], tp[1], tp[2], g, eq, sq, thr[q])
            qinv = f32(f32(1.0 - 1e-5) / sq) if sq > 0 else f32(np.inf)
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                gq = f32(f32(max(g, f32(0)) * qinv) * f32(1.0 - 1e-4))
                for gi in range(8):
                    gm = snap.tileg8[t, gi]
                    rgm = f32(f32(1.0 - 2e-6) * (f32(1.0) / gm if gm != 0 else f32(np.inf)))
                    kg = _fma(_group_b_margin(snap.tileg8[t, 8 + gi], tp[3]), gq, kq) if group_b else kq
                    lvl = f32(kg) * rgm
                    ti = -2.1e9 if np.isnan(lvl) else int(np.clip(np.float64(lvl), -2.1e9, 2.1e9))
                    rows = t * 256 + np.nonzero(grp == gi)[0]
                    hit[rows, q] = I[rows, q] >= ti
    keep = hit & (S <= thr[None, :]) & (np.arange(I.shape[0]) < n_pub)[:, None]
    rows_of = snap.row_of_pos()
    cnt = np.zeros(nq, dtype=np.uint32)
    ovf = np.zeros(nq, dtype=np.uint32)
    ids = np.full((nq, L.POOL_CAP), 0xFFFFFFFF, dtype=np.uint32)
    sc = np.full((nq, L.POOL_CAP), np.inf, dtype=f32)
    for q in range(nq):
        p = np.nonzero(keep[:, q])[0][::-1]                  # (any order: the pool is unsorted)
        cnt[q] = len(p)
        ovf[q] = len(p) > L.POOL_CAP
        m = min(len(p), L.POOL_CAP)
        keys = (L.f32_to_ordered(S[p[:m], q]).astype(np.uint64) << np.uint64(32)) | rows_of[p[:m]].astype(np.uint64)
        ids[q, :m], sc[q, :m] = L.decode_key(keys)
    return cnt, ovf, ids, sc


class Model:
    def __init__(self, metric):
        rng = np.random.default_rng(5)
        self.metric = metric
        pool = np.concatenate([X for _, X in _datasets(rng, D_, n=128)])
        pool = pool[np.abs(pool).sum(axis=1) > 0]               # (zero rows: tests/test_i8_device_bound.py has them)
        self.X = pool[rng.permutation(len(pool))[:N_PUB]].astype(f32)
        self.snap, self.raise_of, self.e_nat = model_snapshot(self.X, metric, D_, N_PUB, CAP)
        rows_of = self.snap.row_of_pos()
        # the exact-row queries: rows stored in lane groups 7, 5, 6, 3 of the ordered tiles
        self.exact_pos = [t * 256 + int(np.nonzero(L.i8_group_of_pos(np.arange(256)) == g)[0][5])
                          for t, g in ((0, 7), (1, 5), (2, 6), (0, 3))]
        self.exact_rows = [int(rows_of[p]) for p in self.exact_pos]
        self.Q = np.concatenate([self.X[self.exact_rows], self.X[:12] + f32(1e-3) * rng.standard_normal((12, D_)).astype(f32),
                                 np.zeros((1, D_), dtype=f32), rng.standard_normal((7, D_)).astype(f32)])
        qi, sq, eq, g, u, v = _query_params(self.Q, metric, D_)
        self.qi = qi
        nq = len(self.Q)
        self.q_rows = 256
        self.qp = np.stack([sq, eq, g, np.full(nq, np.inf, dtype=f32)], axis=1).astype(f32)
        self.quv = np.stack([u, v], axis=1).astype(f32)
        q8 = np.zeros((nq, self.snap.ld8), dtype=np.int8)
        q8[:, :D_] = qi
        self.q8_raw = L.layout_q8(q8, self.q_rows, self.snap.ld8)
        self.n_pos = ((N_PUB + 255) // 256) * 256
        self.group_b = metric == "l2"

    def dump(self, snap, table=L.SWIZZLE):
        return model_dump(snap, self.qi, self.qp, self.n_pos, table)

    def check_all(self, snap):
        m = self.metric
        ck.check_c1(snap, N_PUB, expect_ordered=(0, 1, 2))
        ck.check_c2_rows(snap, self.X, m, D_, N_PUB)
        qi = ck.check_c2_queries(self.Q, D_, self.qp, self.q8_raw, self.q_rows, snap.ld8)
        assert (qi[:, :D_] == self.qi).all()
        ck.check_c3(snap, self.X, N_PUB)
        ck.check_c4(snap, self.X, m, N_PUB)
        I, S = self.dump(snap)
        ck.check_c5(snap, S, 0, qi, self.qp)
        ck.check_c6(snap, S, self.X, self.Q, m, self.quv, N_PUB, _true_distance)
        self.check_c7(snap, I, S)

    def check_c7(self, snap, I, S, cases=range(ck.N_THRESHOLD_CASES)):
        S_row = S[snap.pos_of_row()[:N_PUB]]
        for case in cases:
            thr = ck.thresholds(S_row, case)
            ck.check_c7(snap, S, thr, model_pass(snap, I, S, self.qp, thr, N_PUB, self.group_b), N_PUB)


@pytest.fixture(scope="module", params=["cosine", "l2"])
def model(request):
    return Model(request.param)


@pytest.fixture(scope="module")
def cos():
    return Model("cosine")


def _raises(check, fn):
    with pytest.raises(ck.CheckError) as ei:
        fn()
    assert ei.value.check == check, str(ei.value)
    return str(ei.value)


def test_layout_round_trips():
    rng = np.random.default_rng(0)
    for ld8 in (64, 192, 320):
        codes = rng.integers(-127, 128, size=(512, ld8)).astype(np.int8)
        raw = L.layout_x8(codes, ld8)
        assert (L.delayout_x8(raw, 512, ld8) == codes).all()
        assert sorted(L.scan8_index(np.arange(512)[:, None], np.arange(ld8)[None, :], ld8).ravel()) == list(range(512 * ld8))
        q = L.layout_q8(codes[:300], 512, ld8)
        assert (L.delayout_q8(q, 300, ld8) == codes[:300]).all()
    # element (row 5, col 17) of a 128-byte scan copy: tile 0, stage 0, chunk 1 ^ (0, 2, 3, 1)[1] = 3
    assert int(L.scan8_index(5, 17, 128)) == 5 * 64 + 3 * 16 + 1
    assert int(L.scanq8_index(256 + 5, 2, 17, 128)) == ((1 * 5 + 2) * 256 + 5) * 64 + 3 * 16 + 1
    assert int(L.scan8_dump_index(35, 21, 2048)) == ((2 * 128 + 1) << 8) + (3 << 4) + 5
    assert sorted(L.i8_pos_of_rank(np.arange(256))) == list(range(256))
    assert (L.i8_group_of_pos(L.i8_pos_of_rank(np.arange(256))) == np.arange(256) // 32).all()
    f = np.array([-np.inf, -2.5, -0.0, 0.0, 1e-30, 3.0, np.inf], dtype=f32)
    o = L.f32_to_ordered(f)
    assert (np.diff(o.astype(np.int64)) >= 0).all() and (L.ordered_to_f32(o).view(np.uint32) == f.view(np.uint32)).all()
    ids, sc = L.decode_key(np.array([(int(o[1]) << 32) | 77], dtype=np.uint64))
    assert int(ids[0]) == 77 and sc[0] == f32(-2.5)


def test_dump_layout_round_trip():
    rng = np.random.default_rng(1)
    S = rng.standard_normal((2048, 40)).astype(f32)
    raw = np.zeros(256 * 2048, dtype=f32)
    raw[L.scan8_dump_index(np.arange(40)[None, :], np.arange(2048)[:, None], 2048)] = S
    assert (ck.dump_scores(raw, 256, 40) == S).all()


def test_the_model_in_the_device_layout_passes(model):
    model.check_all(model.snap)
    assert len(ck.ordered_tiles(model.snap, N_PUB)) == 3


def test_error_bound_taken_before_the_step_was_raised_is_caught_by_c2(cos):
    snap = cos.snap.copy()
    cand = np.argsort(cos.raise_of)[::-1][:1]
    p = int(cand[0])
    assert cos.raise_of[p] > 1.02
    a = f32(-1.0)
    snap.rowp8[p, 2] = a * (f32(1.0001) + cos.e_nat[p])
    snap.rowp8[p, 3] = a * (f32(1.0001) * cos.e_nat[p] + f32(4e-6) + f32(1.5e-7) * f32(D_))
    msg = _raises("C2", lambda: ck.check_c2_rows(snap, cos.X, "cosine", D_, N_PUB))
    assert "position %d" % (p & 255) in msg and "tile %d" % (p >> 8) in msg


def _exact_query_threshold_pass(m, snap):
    """C7 under the 1st-smallest thresholds: every exact-row query must collect its own row"""
    I, S = m.dump(snap)
    I0, S0 = m.dump(m.snap)
    assert (S == S0).all()
    m.check_c7(snap, I, S, cases=(1,))


def test_group_maximum_over_the_wrong_positions_is_caught_by_c4_and_c7(cos):
    snap = cos.snap.copy()
    p = cos.exact_pos[0]                      # tile 0, lane group 7
    t, g = p >> 8, int(L.i8_group_of_pos(p & 255))
    assert g == 7 and snap.tileg8[t, 0] < snap.tileg8[t, 7] * f32(0.98)
    snap.tileg8[t, 7] = snap.tileg8[t, 0]     # the maximum over group 0's positions
    _raises("C4", lambda: ck.check_c4(snap, cos.X, "cosine", N_PUB))
    msg = _raises("C7", lambda: _exact_query_threshold_pass(cos, snap))
    assert "missing" in msg and "row %d" % cos.exact_rows[0] in msg


def test_tile_min_b_raised_by_one_per_cent_is_caught_by_c4_and_c7(cos):
    snap = cos.snap.copy()
    snap.tilep8[1, 3] *= f32(1.01)
    _raises("C4", lambda: ck.check_c4(snap, cos.X, "cosine", N_PUB))
    msg = _raises("C7", lambda: _exact_query_threshold_pass(cos, snap))
    assert "missing" in msg and "tile 1" in msg


def test_swapped_perm8_entries_are_caught_by_c1_or_c6(model):
    snap = model.snap.copy()                  # inside an ordered tile: still a permutation — the rows are wrong
    p = model.exact_pos[1]
    o = p ^ 64
    snap.perm8[[p, o]] = snap.perm8[[o, p]]
    ck.check_c1(snap, N_PUB, expect_ordered=(0, 1, 2))
    I, S = model.dump(snap)
    _raises("C6", lambda: ck.check_c6(snap, S, model.X, model.Q, model.metric, model.quv, N_PUB, _true_distance))
    snap = model.snap.copy()                  # inside the straddling tile: no longer the identity
    snap.perm8[[3 * 256 + 7, 3 * 256 + 9]] = snap.perm8[[3 * 256 + 9, 3 * 256 + 7]]
    _raises("C1", lambda: ck.check_c1(snap, N_PUB))
    snap = model.snap.copy()                  # an entry repeated: no permutation
    snap.perm8[256 + 3] = snap.perm8[256 + 4]
    _raises("C1", lambda: ck.check_c1(snap, N_PUB))


def test_the_plain_swizzle_table_is_caught_by_c5(model):
    I, S = model.dump(model.snap)
    qi = ck.check_c2_queries(model.Q, D_, model.qp, model.q8_raw, model.q_rows, model.snap.ld8)
    ck.check_c5(model.snap, S, 0, qi, model.qp)
    _raises("C5", lambda: ck.check_c5(model.snap, S, 0, qi, model.qp, table=(0, 1, 2, 3)))


def test_padding_row_with_finite_parameters_is_caught_by_c3_and_c7(model):
    snap = model.snap.copy()
    snap.rowp8[N_PUB + 3] = snap.rowp8[3 * 256 + 1]
    _raises("C3", lambda: ck.check_c3(snap, model.X, N_PUB))
    I, S = model.dump(snap)
    msg = _raises("C7", lambda: model.check_c7(snap, I, S, cases=(6,)))
    assert "position %d" % ((N_PUB + 3) & 255) in msg
