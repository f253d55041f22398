"""Checks H1-H8 of the fp16 filter scan on RAW arrays — the scan copy as the writers left it (X16, rowp16, the unsafe
counter), the prepared queries, the sample pass's dump, sample select's thresholds, a collect pass's published lists and
their merge — against the original rows and queries in float64; and the (weaker) list check of the fp32 scan.  Pure numpy:
tests/test_f16_device_bound.py feeds them what the device wrote, tests/test_f16_checks_cpu.py what the numpy model writes
(and mutations of it: every check must be able to fail).  Every check raises CheckError naming the first violation."""
import numpy as np

import f16_layout as L
from i8_checks import CheckError, _bits, _first, check_c6, unbounded_rows

f32 = np.float32
f16 = np.float16
U = 2.0 ** -24
INF = f32(np.inf)
PAD_ROW = np.array([0.0, np.inf], dtype=f32)     # rowp16 of a padding row / a row the filter cannot bound


def t_of(d):
    """bound of the relative error of the filter's own norm and of a component scaled by it: per-lane sums of d / 64 terms, six
    tree adds, one sqrt, one reciprocal, one multiply"""
    return (d / 128.0 + 8.0) * U


class Snapshot16:
    """the fp16 scan copy of a space, raw"""

    def __init__(self, X16, rowp16, unsafe, ld16, cap):
        self.X16 = np.asarray(X16).view(np.uint16).ravel()
        self.rowp16 = np.asarray(rowp16, dtype=f32).reshape(-1, 2)
        self.unsafe = np.asarray(unsafe, dtype=np.uint64).ravel()
        self.ld16, self.cap = int(ld16), int(cap)
        self._codes = None

    def codes(self, table=L.SWIZZLE):
        """[cap][ld16] binary16"""
        if self._codes is None or self._codes[0] != tuple(table):
            self._codes = (tuple(table), L.delayout_x16(self.X16, self.cap, self.ld16, table))
        return self._codes[1]

    def pos_of_row(self):       # (the int8 checks' view of a copy: here every row sits at its own position)
        return np.arange(self.cap, dtype=np.int64)


def _unit64(V):
    V64 = np.asarray(V, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        n = np.sqrt((V64 * V64).sum(axis=1))
        return V64 / np.where(n > 0, n, 1.0)[:, None], n


def _code_band(V, d):
    """per component the smallest and largest binary16 the filter may store: RN16(x^ (1 -+ t))"""
    t = t_of(d)
    with np.errstate(over="ignore", invalid="ignore"):
        xh, _ = _unit64(V)
        a, b = xh * (1.0 - t), xh * (1.0 + t)
        lo = np.minimum(a, b).astype(f16).astype(np.float64)      # (float64 -> binary16: round to nearest, ties to even)
        hi = np.maximum(a, b).astype(f16).astype(np.float64)
    return lo, hi


# ---- H1 ----------------------------------------------------------------------------------------------------------
def check_h1(snap, X, d, n_pub, table=L.SWIZZLE):
    """every row norm_ok accepts: each stored half inside [RN16(x^ (1 - t)), RN16(x^ (1 + t))], columns [d, ld16) zero, a row of
    zeros stored as zeros; the three blocks of tail padding hold finite halves"""
    assert snap.ld16 == L.ld16_of(d) and snap.cap % L.TILE == 0 and len(snap.X16) == L.x16_halves(snap.cap, snap.ld16)
    H = snap.codes(table)[:n_pub]
    ok = ~unbounded_rows(X[:n_pub])
    if (ok[:, None] & (H[:, d:].view(np.uint16) != 0)).any():
        r, c = _first(ok[:, None] & (H[:, d:].view(np.uint16) != 0))
        raise CheckError("H1", "padding column %d holds %r" % (d + c, H[r, d + c]), tile=r >> 8, row=r)
    lo, hi = _code_band(X[:n_pub], d)
    Hd = H[:, :d].astype(np.float64)
    bad = ok[:, None] & ~((Hd >= lo) & (Hd <= hi))
    if bad.any():
        r, c = _first(bad)
        raise CheckError("H1", "component %d stored as %.9g, allowed [%.9g, %.9g]" % (c, Hd[r, c], lo[r, c], hi[r, c]),
                         tile=r >> 8, row=r)
    zero = ok & ~np.asarray(X[:n_pub], dtype=np.float64).any(axis=1)
    if (H[zero].view(np.uint16) & 0x7FFF).any():
        raise CheckError("H1", "a row of zeros is not stored as zeros", row=int(np.nonzero(zero)[0][0]))
    tail = snap.X16[snap.cap * snap.ld16:].view(f16)
    if len(tail) != L.TAIL_PAD or not np.isfinite(tail.astype(f32)).all():
        raise CheckError("H1", "the tail padding holds a non-finite half")


# ---- H2 ----------------------------------------------------------------------------------------------------------
def check_h2(snap, X, metric, d, n_pub, written_once=True):
    """(a, b) per metric: cosine (-1, 1) to the bit; IP (-n_r, 1); L2^2 (-n_r, ss) with n_r == sqrt_f32(ss) to the bit and
    |ss - |x|^2| <= (d / 64 + 7) u |x|^2 (IP: n_r within half of that plus the square root's rounding); rows outside the band,
    rows from the published count to cap + 512: (0, +inf); the unsafe counter counts the former"""
    P = snap.rowp16
    if len(P) != snap.cap + L.ROWP_PAD:
        raise CheckError("H2", "rowp16 holds %d rows, cap + 512 = %d" % (len(P), snap.cap + L.ROWP_PAD))
    unb = unbounded_rows(X[:n_pub])
    pad = (_bits(P[:n_pub]) == _bits(PAD_ROW)[None, :]).all(axis=1)
    if (unb != pad).any():
        r = int(np.nonzero(unb != pad)[0][0])
        raise CheckError("H2", "row %s the band, parameters %s" % ("outside" if unb[r] else "inside", P[r]), tile=r >> 8, row=r)
    n_unb = int(unb.sum())
    if (int(snap.unsafe[0]) != n_unb) if written_once else (int(snap.unsafe[0]) < n_unb):
        raise CheckError("H2", "the unsafe counter = %d, rows the filter cannot bound: %d" % (int(snap.unsafe[0]), n_unb))
    tail = ~(_bits(P[n_pub:]) == _bits(PAD_ROW)[None, :]).all(axis=1)
    if tail.any():
        r = n_pub + int(np.nonzero(tail)[0][0])
        raise CheckError("H2", "a padding row holds %s" % P[r], tile=r >> 8, row=r)
    ok = ~unb
    Pk = P[:n_pub][ok]
    rows = np.nonzero(ok)[0]
    n2 = (np.asarray(X[:n_pub], dtype=np.float64)[ok] ** 2).sum(axis=1)
    e_ss = (d / 64.0 + 7.0) * U

    def fail(mask, what):
        i = int(np.nonzero(mask)[0][0])
        raise CheckError("H2", "%s: parameters %s, |x|^2 = %.12g" % (what, Pk[i], n2[i]), tile=int(rows[i]) >> 8, row=int(rows[i]))

    if metric == "cosine":
        if (_bits(Pk) != _bits(np.array([-1.0, 1.0], dtype=f32))[None, :]).any():
            fail((_bits(Pk) != _bits(np.array([-1.0, 1.0], dtype=f32))[None, :]).any(axis=1), "cosine wants (-1, 1)")
        return
    a = -Pk[:, 0].astype(np.float64)
    if metric == "ip":
        if (_bits(Pk[:, 1]) != _bits(f32(1.0))).any():
            fail(_bits(Pk[:, 1]) != _bits(f32(1.0)), "IP wants b = 1")
        bad = ~(np.abs(a - np.sqrt(n2)) <= (e_ss / 2 + 2 * U) * np.sqrt(n2))
        if bad.any():
            fail(bad, "a is not -|x|")
        return
    ss = Pk[:, 1]
    if (_bits(-Pk[:, 0]) != _bits(np.sqrt(ss))).any():
        fail(_bits(-Pk[:, 0]) != _bits(np.sqrt(ss)), "a is not -sqrt_f32(b)")
    bad = ~(np.abs(ss.astype(np.float64) - n2) <= e_ss * n2)
    if bad.any():
        fail(bad, "b is not |x|^2 within (d / 64 + 7) u")


# ---- H3 ----------------------------------------------------------------------------------------------------------
def check_h3(Q, d, metric, q16_raw, gamma, quv, q_rows, table=L.SWIZZLE):
    """-> the queries' halves [nq][ld16].  Q16 follows the H1 rule through scanq16_index; blocks kts .. kts + 2 of every
    query tile repeat stages 0 .. 2 byte for byte; padding queries are zero with gamma = 1, (u, v) = (1, 0); gamma, u, v per
    metric within t(d) relative; zero query: (1, 1, 0); query outside the band: u = NaN"""
    nq, ld16 = len(Q), L.ld16_of(d)
    kts = ld16 >> 5
    raw = np.asarray(q16_raw).view(np.uint16)
    assert q_rows == (nq + 255) // 256 * 256 and len(raw) == L.scanq16_halves(q_rows, ld16)
    blocks = raw.reshape(q_rows >> 8, kts + 3, 256 * 32)
    if (blocks[:, kts:kts + 3] != blocks[:, 0:3]).any():
        t, j, _ = _first(blocks[:, kts:kts + 3] != blocks[:, 0:3])
        raise CheckError("H3", "query tile %d: block %d does not repeat stage %d" % (t, kts + j, j))
    Hall = L.delayout_q16(raw, q_rows, ld16, table)
    if (Hall[nq:].view(np.uint16) != 0).any():
        raise CheckError("H3", "a padding query is not zero", query=nq + _first(Hall[nq:].view(np.uint16) != 0)[0])
    H = Hall[:nq]
    g = np.asarray(gamma, dtype=f32)
    uv = np.asarray(quv, dtype=f32).reshape(-1, 2)
    if (_bits(g[nq:q_rows]) != _bits(f32(1))).any() or (_bits(uv[nq:q_rows]) != _bits(np.array([1.0, 0.0], dtype=f32))[None, :]).any():
        raise CheckError("H3", "a padding query's parameters are not gamma = 1, (u, v) = (1, 0)")
    unb = unbounded_rows(Q)
    ok = ~unb
    if (H[ok][:, d:].view(np.uint16) != 0).any():
        raise CheckError("H3", "a padding column of a query is not zero")
    lo, hi = _code_band(Q, d)
    Hd = H[:, :d].astype(np.float64)
    bad = ok[:, None] & ~((Hd >= lo) & (Hd <= hi))
    if bad.any():
        q, c = _first(bad)
        raise CheckError("H3", "component %d stored as %.9g, allowed [%.9g, %.9g]" % (c, Hd[q, c], lo[q, c], hi[q, c]), query=q)
    beta = np.sqrt((np.asarray(Q, dtype=np.float64) ** 2).sum(axis=1))
    zero = beta == 0
    want_g, want_u, want_v = np.ones(nq), np.ones(nq), np.zeros(nq)
    nz = ok & ~zero
    if metric == "ip":
        want_g[nz], want_u[nz] = 1.0 / beta[nz], beta[nz]
    elif metric == "l2":
        want_g[nz], want_u[nz], want_v[nz] = 0.5 / beta[nz], 2.0 * beta[nz], beta[nz] ** 2
    t = t_of(d)
    for name, got, want in (("gamma", g[:nq], want_g), ("u", uv[:nq, 0], want_u), ("v", uv[:nq, 1], want_v)):
        exact = zero | (metric == "cosine") | ((name == "v") & (metric != "l2"))
        bad = ok & np.where(exact, _bits(got) != _bits(want.astype(f32)), ~(np.abs(got.astype(np.float64) - want) <= t * np.abs(want)))
        if bad.any():
            q = int(np.nonzero(bad)[0][0])
            raise CheckError("H3", "%s = %.9g, float64 gives %.12g" % (name, got[q], want[q]), query=q)
    if (unb & ~np.isnan(uv[:nq, 0])).any():
        raise CheckError("H3", "a query the filter cannot bound has a finite u", query=int(np.nonzero(unb & ~np.isnan(uv[:nq, 0]))[0][0]))
    return H


# ---- H4 ----------------------------------------------------------------------------------------------------------
def check_h4(snap, S, row0, Hq, gamma, eps):
    """S [rows][nq], the dump of rows [row0, +rows): |S - (b gamma + a (dot16 + eps))| <= |a| (ld16 + 4) 2^-23 (sum |q16 x16| +
    eps) + 4 2^-23 (|b gamma| + |a| (|dot16| + eps)), dot16 the float64 dot product of the stored halves.  Non-finite values of
    the expression (padding rows: b = +inf) must be met exactly.  -> the largest error / tolerance"""
    n, nq = S.shape
    Xh = snap.codes()[row0:row0 + n].astype(np.float64)
    Qh = Hq.astype(np.float64)
    P = snap.rowp16[row0:row0 + n].astype(np.float64)
    g = np.asarray(gamma, dtype=f32)[:nq].astype(np.float64)
    eps = float(eps)
    with np.errstate(invalid="ignore", over="ignore"):
        dot = Xh @ Qh.T
        mag = np.abs(Xh) @ np.abs(Qh).T
        a, bg = P[:, 0:1], P[:, 1:2] * g[None, :]
        S64 = bg + a * (dot + eps)
        e2 = 2.0 ** -23
        tol = np.abs(a) * (snap.ld16 + 4) * e2 * (mag + eps) + 4 * e2 * (np.abs(bg) + np.abs(a) * (np.abs(dot) + eps))
        fin = np.isfinite(S64)
        S_64 = S.astype(np.float64)
        err = np.abs(S_64 - S64)
        bad = np.where(fin, ~(err <= tol), ~((S_64 == S64) | (np.isnan(S_64) & np.isnan(S64))))
    if bad.any():
        r, q = _first(bad)
        raise CheckError("H4", "score %.9g, the expression gives %.12g (tolerance %.3g)" % (S[r, q], S64[r, q], tol[r, q]),
                         tile=(row0 + r) >> 8, row=row0 + r, query=q)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(fin & (tol > 0), err / tol, 0.0)
    return float(ratio.max()) if ratio.size else 0.0


# ---- H5 ----------------------------------------------------------------------------------------------------------
def check_h5(snap, S_row, X, Q, metric, quv, n_pub, true_distance):
    """u S + v <= D_true + 2e-6 scale for every published row and every query with a finite u (check_c6 of the int8 checks, on
    the same D_true and scale).  -> the largest (u S + v - D_true) / scale"""
    uv = np.asarray(quv, dtype=f32).reshape(-1, 2)[:len(Q)]
    fin = np.isfinite(uv[:, 0])
    qs = np.nonzero(fin)[0]
    if not len(qs):
        return -np.inf
    Qf = np.ascontiguousarray(Q[qs])
    worst = -np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        Dtrue = true_distance(X[:n_pub], Qf, metric)
        Dlow = (uv[qs][None, :, 0].astype(np.float64) * S_row[:n_pub][:, qs].astype(np.float64) + uv[qs][None, :, 1]).astype(f32)
        scale = np.maximum(np.abs(Dtrue), np.maximum((np.linalg.norm(Qf.astype(np.float64), axis=1) ** 2)[None, :], 1.0))
        ex = (Dlow.astype(np.float64) - Dtrue) / scale
        if np.isfinite(ex).any():
            worst = float(ex[np.isfinite(ex)].max())
    try:
        check_c6(snap, S_row[:, qs], X, Qf, metric, uv[qs], n_pub, lambda *_: Dtrue)
    except CheckError as e:
        raise CheckError("H5", str(e) + " [queries renumbered: those with a finite u]")
    return worst


def rounding_loss(snap, Hq, X, Q, n_pub):
    """the largest <q^, x^> - dot16 over the published rows and the queries the filter bounds: what eps has to cover, in the
    direction that matters (a_r <= 0: a dot product that comes out too SMALL raises the score)"""
    okx, okq = ~unbounded_rows(X[:n_pub]), ~unbounded_rows(Q)
    xh, _ = _unit64(np.asarray(X[:n_pub])[okx])
    qh, _ = _unit64(np.asarray(Q)[okq])
    dot16 = snap.codes()[:n_pub][okx].astype(np.float64) @ Hq[okq].astype(np.float64).T
    return float((xh @ qh.T - dot16).max())


# ---- H6 ----------------------------------------------------------------------------------------------------------
def check_h6(S, kprime, gthr):
    """S [2048][nq], the whole dump: gthr[q] == (ordered(k'-th smallest score of query q) << 32) | 0xFFFFFFFF"""
    for q in range(S.shape[1]):
        col = S[:, q]
        col = np.sort(col[~np.isnan(col)])
        want = L.make_key(col[kprime - 1], 0xFFFFFFFF) if len(col) >= kprime else L.KEY_INF
        if np.uint64(gthr[q]) != want:
            raise CheckError("H6", "gthr = %#x, the k'-th smallest dumped score gives %#x (k' = %d)" % (int(gthr[q]), int(want), kprime),
                             query=q)


# ---- H7 ----------------------------------------------------------------------------------------------------------
def _check_lists(check, part, g, kprime, tile0, n_tiles, tiles_per_chunk, n_pub, tile_rows, key_ok):
    """what H7 and the fp32 check share: the shape of every published list.  key_ok(q, ids, scores) -> mask of acceptable
    scores"""
    nq, lists, kp = part.shape
    assert kp == kprime
    lst_of = np.arange(lists, dtype=np.int64)[:, None]
    for q in range(nq):
        keys = part[q]
        valid = keys != L.KEY_INF

        def fail(mask, what):
            lst, i = _first(mask)
            raise CheckError(check, "list %d, slot %d: %s (key %#x, threshold %#x)" % (lst, i, what, int(keys[lst, i]), int(g[q])),
                             row=int(L.key_id(keys[lst, i])), query=q)

        if (valid[:, 1:] & ~valid[:, :-1]).any():
            fail(np.pad(valid[:, 1:] & ~valid[:, :-1], ((0, 0), (1, 0))), "a key behind an empty slot")
        if not valid.any():
            continue
        unsorted = valid[:, 1:] & (keys[:, 1:] <= keys[:, :-1])
        if unsorted.any():
            fail(np.pad(unsorted, ((0, 0), (1, 0))), "the list is not sorted / holds a key twice")
        ids = L.key_id(keys)
        if (valid & (ids >= n_pub)).any():
            fail(valid & (ids >= n_pub), "an id beyond the published rows")
        tile = ids // tile_rows
        foreign = valid & ((tile < tile0) | (tile >= tile0 + n_tiles) | (L.list_of_row(ids, tile0, tiles_per_chunk, tile_rows) != lst_of))
        if foreign.any():
            fail(foreign, "a row of another list")
        if (valid & (keys >= np.uint64(g[q]))).any():
            fail(valid & (keys >= np.uint64(g[q])), "a key not below the threshold")
        okm = np.ones(keys.shape, dtype=bool)
        okm[valid] = key_ok(q, ids[valid], L.key_score(keys[valid]))
        if not okm.all():
            lst, i = _first(~okm)
            fail(~okm, "score %.9g of the key is not the row's" % L.key_score(keys[lst, i:i + 1])[0])


def check_h7(S_row, g, part, err, kprime, tile0, n_tiles, tiles_per_chunk, n_pub):
    """S_row [rows][nq]: the dump by row id (rows from 0).  One collect pass of tiles [tile0, +n_tiles) under thresholds g:
    err == 0; every published key is (ordered(dump bits), id) of a published row of its list, below g[q]; lists sorted, no
    duplicates, the rest kKeyInf; and the k' smallest keys below g[q] among the window's published rows all appear"""
    if int(err) != 0:
        raise CheckError("H7", "the scan's error word = %d" % int(err))
    sbits = _bits(S_row)

    def key_ok(q, ids, sc):
        return _bits(sc) == sbits[ids, q]

    _check_lists("H7", part, g, kprime, tile0, n_tiles, tiles_per_chunk, n_pub, L.TILE, key_ok)
    lo, hi = tile0 * L.TILE, min((tile0 + n_tiles) * L.TILE, n_pub)
    rows = np.arange(lo, hi, dtype=np.int64)
    for q in range(part.shape[0]):
        sc = S_row[lo:hi, q]
        keep = ~np.isnan(sc)
        keys = L.make_key(sc[keep], rows[keep])
        keys = keys[keys < np.uint64(g[q])]
        want = np.partition(keys, kprime - 1)[:kprime] if len(keys) > kprime else keys
        missing = np.sort(want[~np.isin(want, part[q].ravel())])
        if len(missing):
            r = int(L.key_id(missing[:1])[0])
            raise CheckError("H7", "key %#x is among the k' = %d smallest below the threshold %#x and in no list (score %.9g)"
                             % (int(missing[0]), kprime, int(g[q]), S_row[r, q]), tile=r >> 8, row=r, query=q)


N_THRESHOLD_CASES = 5


def h7_thresholds(S_row, n_pub, case, kprime, sample_gthr):
    """keys per query: case 0 all ones (the lists warm from nothing); 1 sample select's value; 2 one key below the query's
    smallest (nothing is collected); 3 exactly the key of the row of rank k' + 3 (that row is excluded, equal scores of lower
    ids are kept); 4 that row's score with the largest id (ties pass)"""
    nq = S_row.shape[1]
    if case == 0:
        return np.full(nq, L.KEY_INF, dtype=np.uint64)
    if case == 1:
        return np.asarray(sample_gthr, dtype=np.uint64).copy()
    out = np.empty(nq, dtype=np.uint64)
    rows = np.arange(n_pub, dtype=np.int64)
    rank = min(kprime + 3, n_pub - 1)
    for q in range(nq):
        sc = S_row[:n_pub, q]
        keys = L.make_key(np.where(np.isnan(sc), INF, sc), rows)
        if case == 2:
            out[q] = keys.min() - np.uint64(1)
        else:
            k = np.partition(keys, rank)[rank]
            out[q] = k if case == 3 else (k | np.uint64(0xFFFFFFFF))
    return out


# ---- H8 ----------------------------------------------------------------------------------------------------------
def check_h8(part, merged, g_in, g_out, kprime):
    """merged[q][:k'] are the k' smallest keys of the union of the query's published lists, sorted; the outgoing threshold is the
    k'-th of them, or the incoming one while fewer are known"""
    for q in range(part.shape[0]):
        want = np.sort(part[q].ravel())[:kprime]
        if (np.asarray(merged[q][:kprime], dtype=np.uint64) != want).any():
            i = int(np.nonzero(np.asarray(merged[q][:kprime], dtype=np.uint64) != want)[0][0])
            raise CheckError("H8", "merged[%d] = %#x, the union's is %#x" % (i, int(merged[q][i]), int(want[i])), query=q)
        exp = want[kprime - 1] if want[kprime - 1] != L.KEY_INF else np.uint64(g_in[q])
        if np.uint64(g_out[q]) != exp:
            raise CheckError("H8", "outgoing threshold %#x, expected %#x" % (int(g_out[q]), int(exp)), query=q)


# ---- the fp32 scan's lists (no dump: a weaker check) --------------------------------------------------------------
def f32_scores(X, Q, metric):
    """float64 value of the fp32 scan's dot * a + b (csrc/k_misc.hip, row_stats_kernel): cosine 1 - <q^, x^>, IP 1 - <q, x>,
    L2^2 |x|^2 - 2 <q, x> (without |q|^2)"""
    X64, Q64 = np.asarray(X, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    if metric == "cosine":
        xh, _ = _unit64(X64)
        qh, _ = _unit64(Q64)
        return 1.0 - xh @ qh.T
    if metric == "ip":
        return 1.0 - X64 @ Q64.T
    return (X64 * X64).sum(axis=1)[:, None] - 2.0 * (X64 @ Q64.T)


def cert_margin(metric, d, qn, max_sumsq, scale):
    """csrc/ehx_kernels.h, in float64"""
    eps_d = 1.3 * (d + 16.0) * 2.0 ** -24
    if metric == "cosine":
        base = eps_d * 1.01
    else:
        qb, mx = np.sqrt(qn), np.sqrt(max_sumsq)
        base = eps_d * 1.01 * qb * mx if metric == "ip" else eps_d * 1.01 * (qb + mx) ** 2
    return base + 2e-6 * np.maximum(scale, np.maximum(qn, 1.0))


def check_f32_lists(S64, X, Q, metric, d, g, part, err, kprime, tile0, n_tiles, tiles_per_chunk, n_pub):
    """S64 = f32_scores of every published row.  With m = cert_margin(|q|^2, max |x|^2, scale = |score|): every published key's
    score within m of the float64 score of its id; every window row whose float64 score lies below the k'-th smallest float64
    score of the window minus 2 m and below the threshold's score minus m is in some list; shape of the lists as in H7"""
    if int(err) != 0:
        raise CheckError("F32", "the scan's error word = %d" % int(err))
    qn = (np.asarray(Q, dtype=np.float64) ** 2).sum(axis=1) if metric != "cosine" else np.ones(len(Q))
    mx = float((np.asarray(X[:n_pub], dtype=np.float64) ** 2).sum(axis=1).max())

    def margin(q, s):
        return cert_margin(metric, d, qn[q], mx, np.abs(s))

    def key_ok(q, ids, sc):
        return np.abs(sc.astype(np.float64) - S64[ids, q]) <= margin(q, S64[ids, q])

    _check_lists("F32", part, g, kprime, tile0, n_tiles, tiles_per_chunk, n_pub, L.TILE_F32, key_ok)
    lo, hi = tile0 * L.TILE_F32, min((tile0 + n_tiles) * L.TILE_F32, n_pub)
    for q in range(part.shape[0]):
        s = S64[lo:hi, q]
        m = margin(q, s)
        kth = np.sort(s)[kprime - 1] if len(s) >= kprime else np.inf
        thr = float(L.key_score(np.array([g[q]], dtype=np.uint64))[0]) if np.uint64(g[q]) != L.KEY_INF else np.inf
        must = np.nonzero((s < kth - 2 * m) & (s < thr - m))[0] + lo
        got = L.key_id(part[q].ravel()[part[q].ravel() != L.KEY_INF])
        missing = must[~np.isin(must, got)]
        if len(missing):
            r = int(missing[0])
            raise CheckError("F32", "row with float64 score %.12g (k'-th smallest %.12g, margin %.3g) is in no list"
                             % (S64[r, q], kth, float(np.max(m))), tile=r // L.TILE_F32, row=r, query=q)
