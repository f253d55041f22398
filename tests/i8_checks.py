"""Checks C1-C7 of the int8 filter scan on RAW arrays — the scan copy as the writers left it (X8, rowp8, tilep8, tileg8,
perm8, the unsafe counters), the sample pass's dump, a collect pass's pools, the prepared queries — against the original
rows and queries in float64.  Pure numpy; tests/test_i8_device_bound.py feeds them what the device wrote,
tests/test_i8_checks_cpu.py what the numpy model writes (and mutations of it: every check must be able to fail).
Every check raises CheckError naming the tile, position, row id and query of the first violation."""
import numpy as np

import i8_layout as L

f32 = np.float32
INF = f32(np.inf)
PAD_ROW = np.array([0.0, np.inf, 0.0, 0.0], dtype=f32)     # rowp8 of a padding row / a row the filter cannot bound
PAD_TILE = np.array([0.0, 0.0, 0.0, np.inf], dtype=f32)    # tilep8 of a tile nobody wrote


class CheckError(AssertionError):
    def __init__(self, check, what, tile=None, pos=None, row=None, query=None):
        self.check = check
        where = ", ".join("%s %s" % (k, v) for k, v in (("tile", tile), ("position", pos), ("row", row), ("query", query))
                          if v is not None)
        super().__init__("%s: %s [%s]" % (check, what, where))


class Snapshot:
    """the int8 scan copy of a space, raw"""

    def __init__(self, X8, rowp8, tilep8, tileg8, perm8, unsafe, ld8, cap):
        self.X8 = np.asarray(X8).view(np.int8).ravel()
        self.rowp8 = np.asarray(rowp8, dtype=f32).reshape(-1, 4)
        self.tilep8 = np.asarray(tilep8, dtype=f32).reshape(-1, 4)
        self.tileg8 = np.asarray(tileg8, dtype=f32).reshape(-1, 16)
        self.perm8 = np.asarray(perm8, dtype=np.uint8).ravel()
        self.unsafe = np.asarray(unsafe, dtype=np.uint64).ravel()
        self.ld8, self.cap = int(ld8), int(cap)
        self._codes = None

    def copy(self):
        return Snapshot(self.X8.copy(), self.rowp8.copy(), self.tilep8.copy(), self.tileg8.copy(), self.perm8.copy(),
                        self.unsafe.copy(), self.ld8, self.cap)

    def codes(self, table=L.SWIZZLE):
        """[cap][ld8] int8 by POSITION"""
        if self._codes is None or self._codes[0] != tuple(table):
            self._codes = (tuple(table), L.delayout_x8(self.X8, self.cap, self.ld8, table))
        return self._codes[1]

    def row_of_pos(self):
        pos = np.arange(self.cap, dtype=np.int64)
        return (pos & ~np.int64(255)) | self.perm8.astype(np.int64)

    def pos_of_row(self):
        out = np.empty(self.cap, dtype=np.int64)
        out[self.row_of_pos()] = np.arange(self.cap, dtype=np.int64)
        return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _first(mask):
    return tuple(int(v) for v in np.argwhere(mask)[0])


def _tiles_written(n_pub):
    return (n_pub + 255) // 256


def ordered_tiles(snap, n_pub):
    """tiles whose perm8 is not the identity"""
    t = _tiles_written(n_pub)
    p = snap.perm8[:t * 256].reshape(t, 256)
    return np.nonzero((p != np.arange(256, dtype=np.uint8)[None, :]).any(axis=1))[0]


# ---- C1 ----------------------------------------------------------------------------------------------------------
def check_c1(snap, n_pub, identity_tiles=(), expect_ordered=()):
    """perm8 of every tile is a permutation of 0..255; the tile that straddles n_pub, every tile behind it and every tile of
    identity_tiles (not full when written) hold the identity; tiles of expect_ordered (written full) do not.  (That position
    p of tile t holds row 256 t + perm8[p] is what C2 and C6 see: they take every row's parameters and codes from there.)"""
    T = snap.cap // 256
    perm = snap.perm8.reshape(T, 256)
    ident = np.arange(256, dtype=np.uint8)
    bad = (np.sort(perm, axis=1) != ident[None, :]).any(axis=1)
    if bad.any():
        t = int(np.nonzero(bad)[0][0])
        p = int(np.nonzero(np.sort(perm[t]) != ident)[0][0])
        raise CheckError("C1", "perm8 is no permutation of 0..255 (sorted entry %d is %d)" % (p, int(np.sort(perm[t])[p])), tile=t)
    must = set(int(t) for t in identity_tiles) | set(range(n_pub // 256 if n_pub % 256 else _tiles_written(n_pub), T))
    for t in sorted(must):
        if (perm[t] != ident).any():
            p = int(np.nonzero(perm[t] != ident)[0][0])
            raise CheckError("C1", "a tile that was not full when written (or padding) is not in row order: perm8 = %d"
                             % int(perm[t, p]), tile=t, pos=p, row=256 * t + int(perm[t, p]))
    for t in expect_ordered:
        if (perm[int(t)] == ident).all():
            raise CheckError("C1", "a tile written full was left in row order", tile=int(t))


# ---- C2 ----------------------------------------------------------------------------------------------------------
def _unit64(V):
    V64 = V.astype(np.float64)
    n = np.linalg.norm(V64, axis=1)
    return V64 / np.where(n > 0, n, 1.0)[:, None], n


def _is_pad(P):
    return (_bits(P) == _bits(PAD_ROW)[None, :]).all(axis=1)


def check_c2_rows(snap, X, metric, d, n_pub, table=L.SWIZZLE):
    """codes in [-127, 127], columns >= d zero; with s_r = |A_r| / |a_r| and e_r = C_r / a_r - 1.0001 recovered from the
    stored parameters (a_r: -1 for cosine, else minus the float64 norm): |x^_r - s_r xi_r|_2 <= e_r in float64"""
    codes = snap.codes(table)
    if (codes == -128).any():
        p, c = _first(codes == -128)
        raise CheckError("C2", "code -128 at column %d" % c, tile=p >> 8, pos=p & 255)
    if (codes[:, d:] != 0).any():
        p, c = _first(codes[:, d:] != 0)
        raise CheckError("C2", "column %d >= d holds code %d" % (d + c, int(codes[p, d + c])), tile=p >> 8, pos=p & 255)
    pos = snap.pos_of_row()[:n_pub]
    P = snap.rowp8[pos].astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        xh, nrm = _unit64(X[:n_pub])
    a_abs = np.ones(n_pub) if metric == "cosine" else nrm
    live = ~_is_pad(snap.rowp8[pos]) & np.isfinite(nrm)
    xi = codes[pos].astype(np.float64)[:, :d]
    zero_a = live & ~(a_abs > 0)           # a zero row under IP / L2^2: a_r = 0, every parameter but B is 0, codes 0
    if zero_a.any() and (xi[zero_a] != 0).any():
        r = int(np.nonzero(zero_a & (xi != 0).any(axis=1))[0][0])
        raise CheckError("C2", "a zero row holds non-zero codes", tile=int(pos[r]) >> 8, pos=int(pos[r]) & 255, row=r)
    ok = live & (a_abs > 0)
    safe_a = np.where(ok, a_abs, 1.0)
    s = np.abs(P[:, 0]) / safe_a
    e = np.abs(P[:, 2]) / safe_a - 1.0001
    with np.errstate(over="ignore", invalid="ignore"):
        res = np.linalg.norm(xh - s[:, None] * xi, axis=1)
    bad = ok & ~(res <= e)
    if bad.any():
        r = int(np.nonzero(bad)[0][0])
        raise CheckError("C2", "|x^ - s xi| = %.9g exceeds the stored bound e = %.9g (s = %.9g) — or perm8 names another row"
                         % (res[r], e[r], s[r]), tile=int(pos[r]) >> 8, pos=int(pos[r]) & 255, row=r)


def check_c2_queries(Q, d, qparams, q8_raw, q_rows, ld8, table=L.SWIZZLE):
    """the same for every query with qparams.x = s_q, qparams.y = e_q and the de-layouted Q8; the three stage blocks behind
    a query tile's last stage equal stages j mod kts"""
    nq = Q.shape[0]
    raw = np.asarray(q8_raw).view(np.int8).ravel()
    if raw.size != L.scanq8_bytes(q_rows, ld8):
        raise CheckError("C2", "Q8 holds %d bytes, the layout %d" % (raw.size, L.scanq8_bytes(q_rows, ld8)))
    kts = ld8 >> 6
    blocks = raw.reshape(q_rows >> 8, kts + 3, 256 * 64)
    for j in range(3):
        if (blocks[:, kts + j] != blocks[:, j % kts]).any():
            t = int(np.nonzero((blocks[:, kts + j] != blocks[:, j % kts]).any(axis=1))[0][0])
            raise CheckError("C2", "repeated stage block %d differs from stage %d" % (kts + j, j % kts), tile=t)
    qi = L.delayout_q8(raw, q_rows, ld8, table)
    if (qi == -128).any() or (qi[:, d:] != 0).any() or (qi[nq:] != 0).any():
        raise CheckError("C2", "query codes outside [-127, 127], beyond column d, or in a padding query")
    qh, nrm = _unit64(Q)
    qp = np.asarray(qparams, dtype=f32).reshape(-1, 4).astype(np.float64)
    res = np.linalg.norm(qh - qp[:nq, 0:1] * qi[:nq, :d].astype(np.float64), axis=1)
    bad = ~(res <= qp[:nq, 1])
    if bad.any():
        q = int(np.nonzero(bad)[0][0])
        raise CheckError("C2", "|q^ - s_q qi| = %.9g exceeds e_q = %.9g" % (res[q], qp[q, 1]), query=q)
    return qi[:nq]


# ---- C3 ----------------------------------------------------------------------------------------------------------
def unbounded_rows(X):
    """rows the filter cannot bound: |x|^2 non-finite or outside (1e-24, 1e30) and not 0 (norm_ok, k_misc.hip).  The kernel
    sums in float32: test rows keep clear of the band's edges."""
    with np.errstate(over="ignore", invalid="ignore"):
        ss = (X.astype(np.float64) ** 2).sum(axis=1)
        ss32 = (X.astype(f32) ** 2).sum(axis=1, dtype=f32)
    return ~(np.isfinite(ss32) & ((ss == 0) | ((ss > 1e-24) & (ss < 1e30))))


def check_c3(snap, X, n_pub, written_once=True):
    """rows outside the band hold (0, +inf, 0, 0) and dUnsafe8[0] counts exactly them (each row written once; else at
    least them); positions in [n_pub, end of rowp8) hold (0, +inf, 0, 0); tiles behind the last written one hold
    tilep8 = (0, 0, 0, +inf)"""
    pos = snap.pos_of_row()[:n_pub]
    unb = unbounded_rows(X[:n_pub])
    pad = _is_pad(snap.rowp8[pos])
    if (unb != pad).any():
        r = int(np.nonzero(unb != pad)[0][0])
        raise CheckError("C3", "row %s the band, parameters %s" % ("outside" if unb[r] else "inside", snap.rowp8[pos[r]]),
                         tile=int(pos[r]) >> 8, pos=int(pos[r]) & 255, row=r)
    n_unb = int(unb.sum())
    if (int(snap.unsafe[0]) != n_unb) if written_once else (int(snap.unsafe[0]) < n_unb):
        raise CheckError("C3", "dUnsafe8[0] = %d, rows the filter cannot bound: %d" % (int(snap.unsafe[0]), n_unb))
    tail = ~_is_pad(snap.rowp8[n_pub:])
    if tail.any():
        p = n_pub + int(np.nonzero(tail)[0][0])
        raise CheckError("C3", "a padding row holds %s" % snap.rowp8[p], tile=p >> 8, pos=p & 255)
    t0 = _tiles_written(n_pub)
    tt = (_bits(snap.tilep8[t0:]) != _bits(PAD_TILE)[None, :]).any(axis=1)
    if tt.any():
        t = t0 + int(np.nonzero(tt)[0][0])
        raise CheckError("C3", "a tile nobody wrote holds tilep8 = %s" % snap.tilep8[t], tile=t)


# ---- C4 ----------------------------------------------------------------------------------------------------------
def group_extremes(P):
    """rowp8 of one tile [256][4] -> (max |A| per lane group [8], the tileg8[8 + g] entries [8]) as ident_tiles8_kernel
    forms them: min over max(B, 0) (anything not >= 0 counts as 0), stored as -inf where that minimum is 0"""
    g = L.i8_group_of_pos(np.arange(256))
    B = np.where(P[:, 1] >= 0, P[:, 1], f32(0)).astype(f32)
    gmax = np.array([np.abs(P[g == i, 0]).max() for i in range(8)], dtype=f32)
    gb = np.array([B[g == i].min() for i in range(8)], dtype=f32)
    gb = np.where(_bits(gb) == 0, f32(-np.inf), gb).astype(f32)
    return gmax, gb


def check_c4(snap, X, metric, n_pub):
    """tile and lane-group extremes, exact to the bit; in an ordered tile every row's |A| is its group's maximum and the
    groups follow the order of rank_tiles8_kernel (step order; L2^2 rows whose norms spread by more than 0.1 %: four norm
    bands, each by step)"""
    T = _tiles_written(n_pub)
    grp = L.i8_group_of_pos(np.arange(256))
    rows_of = snap.row_of_pos()
    with np.errstate(over="ignore", invalid="ignore"):
        nrm_all = np.linalg.norm(X[:n_pub].astype(np.float64), axis=1)
    nrm_all = np.where(unbounded_rows(X[:n_pub]), 0.0, nrm_all)   # (a row the filter cannot bound is ordered as norm 0, step 0)
    ordered = set(int(t) for t in ordered_tiles(snap, n_pub))
    for t in range(T):
        P = snap.rowp8[t * 256:(t + 1) * 256]
        want = np.array([np.abs(P[:, 0]).max(), np.abs(P[:, 2]).max(), np.abs(P[:, 3]).max(), P[:, 1].min()], dtype=f32)
        if (_bits(want) != _bits(snap.tilep8[t])).any():
            raise CheckError("C4", "tilep8 = %s, the stored rows give (max|A|, max|C|, max|D|, min B) = %s"
                             % (snap.tilep8[t], want), tile=t)
        gmax, gb = group_extremes(P)
        for gi in range(8):
            if _bits(gmax[gi]) != _bits(snap.tileg8[t, gi]):
                p = int(np.nonzero(grp == gi)[0][np.abs(P[grp == gi, 0]).argmax()])
                raise CheckError("C4", "tileg8[%d] = %.9g, max |A| of the group's positions = %.9g"
                                 % (gi, snap.tileg8[t, gi], gmax[gi]), tile=t, pos=p, row=int(rows_of[t * 256 + p]))
            if _bits(gb[gi]) != _bits(snap.tileg8[t, 8 + gi]):
                p = int(np.nonzero(grp == gi)[0][P[grp == gi, 1].argmin()])
                raise CheckError("C4", "tileg8[8 + %d] = %.9g, min B of the group's positions = %.9g"
                                 % (gi, snap.tileg8[t, 8 + gi], gb[gi]), tile=t, pos=p, row=int(rows_of[t * 256 + p]))
        if t not in ordered:
            continue
        absA = np.abs(P[:, 0])
        off = (_bits(absA) != _bits(gmax[grp])) & ~_is_pad(P)
        if off.any():
            p = int(np.nonzero(off)[0][0])
            raise CheckError("C4", "ordered tile: |A| = %.9g, its group's maximum %.9g" % (absA[p], gmax[grp[p]]),
                             tile=t, pos=p, row=int(rows_of[t * 256 + p]))
        # the order: ranks 32 g .. 32 g + 31 sit in group g, so the groups' (raised) steps do not decrease along a band
        nrm = nrm_all[rows_of[t * 256:(t + 1) * 256]]
        spread = nrm.max() / nrm.min() if nrm.min() > 0 else np.inf
        if metric == "l2" and abs(spread - 1.001) < 1e-5:
            continue      # (the banding decision is taken on float32 norms: too close to call)
        banded = metric == "l2" and spread > 1.001
        bands = [range(2 * b, 2 * b + 2) for b in range(4)] if banded else [range(8)]
        for band in bands:
            gs = list(band)
            for a, b in zip(gs, gs[1:]):
                if gmax[a] > gmax[b]:
                    raise CheckError("C4", "ordered tile%s: group %d has |A| %.9g above group %d's %.9g"
                                     % (" (norm bands)" if banded else "", a, gmax[a], b, gmax[b]), tile=t)
        if banded:
            bn = [nrm[np.isin(grp, list(band))] for band in bands]
            for b in range(3):
                if bn[b].max() > bn[b + 1].min() * (1 + 1e-6):
                    p = int(np.nonzero(np.isin(grp, list(bands[b])))[0][bn[b].argmax()])
                    raise CheckError("C4", "norm band %d reaches %.9g, band %d starts at %.9g"
                                     % (b, bn[b].max(), b + 1, bn[b + 1].min()), tile=t, pos=p, row=int(rows_of[t * 256 + p]))


# ---- C5 ----------------------------------------------------------------------------------------------------------
def dump_scores(dump, q_rows, nq, n_tiles=L.SAMPLE_TILES):
    """raw dump -> S[position inside the window][query]"""
    n_s = n_tiles * 256
    idx = L.scan8_dump_index(np.arange(nq)[None, :], np.arange(n_s)[:, None], n_s)
    d = np.asarray(dump, dtype=f32).ravel()
    if d.size != q_rows * n_s:
        raise CheckError("C5", "the dump holds %d scores, the layout %d" % (d.size, q_rows * n_s))
    return d[idx]


def check_c5(snap, S, tile0, qi, qparams, table=L.SWIZZLE):
    """S [positions of tiles tile0 ..][nq], the kernel's scores: |S - S64| <= 8 * 2^-24 * (|B g| + |D| + |C e_q| + |A s_q I|)
    with I the exact integer dot product of the de-layouted codes and S64 the expression in float64 on the device's own
    parameters (i8_score: one conversion, one multiply, three fused multiply-adds)"""
    n_pos, nq = S.shape
    p0 = tile0 * 256
    codes = snap.codes(table)[p0:p0 + n_pos].astype(np.float64)
    I = codes @ qi.astype(np.float64).T                           # exact: |I| <= 2048 * 127^2 < 2^53
    P = snap.rowp8[p0:p0 + n_pos].astype(np.float64)
    qp = np.asarray(qparams, dtype=f32).reshape(-1, 4)[:nq].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        t_bg = P[:, 1:2] * qp[None, :, 2]
        t_ce = P[:, 2:3] * qp[None, :, 1]
        t_ai = P[:, 0:1] * (qp[None, :, 0] * I)
        S64 = t_bg + P[:, 3:4] + t_ce + t_ai
        tol = 8.0 * 2.0 ** -24 * (np.abs(t_bg) + np.abs(P[:, 3:4]) + np.abs(t_ce) + np.abs(t_ai))
        fin = np.isfinite(S64)
        bad = np.where(fin, ~(np.abs(S.astype(np.float64) - S64) <= tol), ~(S.astype(np.float64) == S64))
    if bad.any():
        p, q = _first(bad)
        raise CheckError("C5", "score %.9g, the expression gives %.12g (tolerance %.3g, I = %d)" % (S[p, q], S64[p, q], tol[p, q], int(I[p, q])),
                         tile=(p0 + p) >> 8, pos=(p0 + p) & 255, row=int(snap.row_of_pos()[p0 + p]), query=q)


# ---- C6 ----------------------------------------------------------------------------------------------------------
def check_c6(snap, S_pos, X, Q, metric, quv, n_pub, true_distance):
    """S_pos [positions 0 ..][nq]: u S + v <= D_true + 2e-6 scale for every published row and every query, scale as in
    tests/test_i8_model.py (cert_margin's 2e-6 * scale term)"""
    pos = snap.pos_of_row()[:n_pub]
    S = S_pos[pos]
    uv = np.asarray(quv, dtype=f32).reshape(-1, 2)[:Q.shape[0]].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        Dlow = (uv[None, :, 0] * S.astype(np.float64) + uv[None, :, 1]).astype(f32)      # rerank256: fma(u, S, v)
    Dtrue = true_distance(X[:n_pub], Q, metric)
    scale = np.maximum(np.abs(Dtrue), np.maximum((np.linalg.norm(Q.astype(np.float64), axis=1) ** 2)[None, :], 1.0))
    bad = ~(Dlow.astype(np.float64) - Dtrue - 2e-6 * scale <= 0.0)
    if bad.any():
        r, q = _first(bad)
        raise CheckError("C6", "lower bound %.9g above the true distance %.12g (S = %.9g)" % (Dlow[r, q], Dtrue[r, q], S[r, q]),
                         tile=int(pos[r]) >> 8, pos=int(pos[r]) & 255, row=r, query=q)


# ---- C7 ----------------------------------------------------------------------------------------------------------
def thresholds(S_row, case):
    """per query, from the dump of the published rows [n_pub][nq]: case 0 below the minimum, 1 / 2 / 3 / 4 the 1st, 3rd, 40th,
    300th smallest score, 5 the largest finite score, 6 +inf"""
    srt = np.sort(np.where(np.isnan(S_row), INF, S_row), axis=0)
    if case == 0:
        return np.nextafter(srt[0], -INF).astype(f32)
    if case in (1, 2, 3, 4):
        return srt[min((0, 2, 39, 299)[case - 1], srt.shape[0] - 1)].astype(f32)
    if case == 5:
        return np.where(np.isfinite(srt), srt, -INF).max(axis=0).astype(f32)
    return np.full(srt.shape[1], INF, dtype=f32)


N_THRESHOLD_CASES = 7


def check_c7(snap, S_pos, thr, pool, n_pub):
    """pool = (count [nq], overflow [nq], ids [nq][POOL_CAP], scores [nq][POOL_CAP]) of one pass under thr [nq]: per query the
    ids are exactly {row < n_pub : S_dump(row, q) <= thr[q]}, every score the dump's bit for bit, no overflow flag (unless
    the set exceeds the pool: then the flag is up), no id >= n_pub; and the positions behind n_pub score +inf"""
    cnt, ovf, ids, scores = pool
    nq = len(thr)
    if S_pos.shape[0] > n_pub and not np.isposinf(S_pos[n_pub:]).all():
        p, q = _first(~np.isposinf(S_pos[n_pub:]))
        raise CheckError("C7", "a position behind the published rows scores %.9g" % S_pos[n_pub + p, q],
                         tile=(n_pub + p) >> 8, pos=(n_pub + p) & 255, query=q)
    pos = snap.pos_of_row()[:n_pub]
    S = S_pos[pos]                                                # by row id
    for q in range(nq):
        want = np.nonzero(S[:, q] <= thr[q])[0]
        m = min(int(cnt[q]), L.POOL_CAP)
        got = np.asarray(ids[q][:m], dtype=np.int64)
        if (got >= n_pub).any():
            r = int(got[got >= n_pub][0])
            raise CheckError("C7", "the pool holds an id beyond the published rows (threshold %.9g)" % thr[q], row=r, query=q)
        if len(want) > L.POOL_CAP:
            if int(ovf[q]) != 1:
                raise CheckError("C7", "%d rows under the threshold %.9g, overflow flag %d" % (len(want), thr[q], int(ovf[q])), query=q)
            continue
        if int(ovf[q]) != 0:
            raise CheckError("C7", "overflow flag %d with %d rows under the threshold %.9g" % (int(ovf[q]), len(want), thr[q]), query=q)
        order = np.argsort(got, kind="stable")
        gs = got[order]
        if int(cnt[q]) != len(want) or (gs != want).any():
            missing, extra = np.setdiff1d(want, gs), np.setdiff1d(gs, want)
            r = int(missing[0]) if len(missing) else (int(extra[0]) if len(extra) else int(gs[np.nonzero(np.diff(gs) == 0)[0][0]]))
            raise CheckError("C7", "threshold %.9g: %d rows in the pool, %d at or below it; first row %s: %d (S = %.9g)"
                             % (thr[q], int(cnt[q]), len(want), "missing" if len(missing) else ("extra" if len(extra) else "twice"),
                                r, S[r, q]), tile=int(pos[r]) >> 8, pos=int(pos[r]) & 255, row=r, query=q)
        sc = np.asarray(scores[q][:m], dtype=f32)[order]
        if (_bits(sc) != _bits(S[want, q])).any():
            i = int(np.nonzero(_bits(sc) != _bits(S[want, q]))[0][0])
            r = int(want[i])
            raise CheckError("C7", "pool score %.9g, dump score %.9g" % (sc[i], S[r, q]), tile=int(pos[r]) >> 8,
                             pos=int(pos[r]) & 255, row=r, query=q)
