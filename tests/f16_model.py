"""A numpy model of the fp16 filter scan, in the device's layout: the scan copy (X16, rowp16), the prepared queries (Q16,
gamma, (u, v)), the sample pass's dump, sample select, a collect pass's published lists and their merge — restated from the
comments of csrc/k_flat16.hip, csrc/k_misc.hip and csrc/k_flat.hip.  tests/test_f16_checks_cpu.py runs the checks of
tests/f16_checks.py on it and on mutations of it.  Also the ALIGNED rows: unit vectors whose components sit just below (or
just above) binary16 rounding midpoints, the data on which the filter's rounding error comes within a few per cent of its
2^-10 worst case."""
import numpy as np

import f16_layout as L

f32 = np.float32
f16 = np.float16
INF = f32(np.inf)
DELTA_BELOW = 2.0 ** -11 - 2.0 ** -16     # 2^e (1 + 2^-11 - 2^-16): rounds DOWN to 2^e, losing almost half an ulp
DELTA_ABOVE = 2.0 ** -11 + 2.0 ** -16     # rounds UP to 2^e (1 + 2^-10)


def scan16_eps(d):
    """csrc/ehx_kernels.h, in float32 as the host computes it"""
    return f32(f32(1.0e-3) + f32(f32(2.0e-7) * f32(d)))


def aligned_rows(rng, d, n, above=False):
    """[n][d] float32, unit norm up to float32 rounding: all but max(4, d / 32) components are +-2^e (1 + delta) or
    +-2^(e+1) (1 + delta), carrying ~97 % of the squared norm; the few free components share the rest.  The offset of 2^-16
    from the midpoint is far more than the filter's own normalisation moves a component (t(d) <= 40 * 2^-24 at d = 4096)."""
    delta = DELTA_ABOVE if above else DELTA_BELOW
    e = int(np.floor(np.log2(1.0 / np.sqrt(d))))
    unit = 4.0 ** e * (1.0 + delta) ** 2
    free = max(4, d // 32)
    m = d - free
    budget = int(0.97 / unit)
    n1 = max(0, min(m, (budget - m) // 3))
    if m > budget:                    # (never at the sizes used: 2^e <= 1 / sqrt(d))
        m, n1 = budget, 0
        free = d - m
    base = np.concatenate([np.full(n1, 2.0 ** (e + 1) * (1.0 + delta)), np.full(m - n1, 2.0 ** e * (1.0 + delta))])
    rest = 1.0 - (base ** 2).sum()
    out = np.empty((n, d), dtype=np.float64)
    for i in range(n):
        w = rng.uniform(0.5, 1.5, free)
        fr = np.sqrt(rest * w / w.sum())
        row = np.concatenate([base, fr]) * rng.choice([-1.0, 1.0], d)
        out[i] = row[rng.permutation(d)]
    return out.astype(f32)


def norm_ok(ss):
    return (ss == 0) | ((ss > f32(1e-24)) & (ss < f32(1e30)))


def _unit32(V):
    """the filter's own normalisation, float32: (x * (1 / sqrt(sum x^2)), sum x^2, ok)"""
    V = np.asarray(V, dtype=f32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ss = (V * V).sum(axis=1, dtype=f32)
        ok = norm_ok(ss) & np.isfinite(ss)
        nr = np.where(ok, np.sqrt(ss), f32(0)).astype(f32)
        inv = np.where(nr > 0, f32(1) / np.where(nr > 0, nr, f32(1)), f32(0)).astype(f32)
        return (V * inv[:, None]).astype(f32), ss, nr, ok


def round16(v, truncate=False):
    """float32 -> binary16: round to nearest even, or (the mutation) truncation towards zero"""
    with np.errstate(over="ignore", invalid="ignore"):
        h = np.asarray(v, dtype=f32).astype(f16)
        if truncate:
            over = np.abs(h.astype(f32)) > np.abs(np.asarray(v, dtype=f32))
            h = np.where(over, np.nextafter(h, f16(0)), h).astype(f16)
    return h


def make_scan16(X, metric, d, cap, n_written=None, truncate=False, table=L.SWIZZLE):
    """-> (X16 raw u16 with tail padding, rowp16 [cap + 512][2], unsafe counter)"""
    ld16 = L.ld16_of(d)
    n = len(X) if n_written is None else n_written
    xh, ss, nr, ok = _unit32(X[:n])
    H = np.zeros((n, ld16), dtype=f16)
    H[:, :d] = round16(xh, truncate)
    rowp = np.zeros((cap + L.ROWP_PAD, 2), dtype=f32)
    rowp[:, 1] = INF
    if metric == "cosine":
        rowp[:n] = np.where(ok[:, None], np.array([-1.0, 1.0], dtype=f32)[None, :], rowp[:n])
    elif metric == "ip":
        rowp[:n] = np.where(ok[:, None], np.stack([-nr, np.ones_like(nr)], axis=1), rowp[:n])
    else:
        rowp[:n] = np.where(ok[:, None], np.stack([-nr, ss], axis=1), rowp[:n])
    return L.layout_x16(H, cap, ld16, table), rowp, np.array([int((~ok).sum())], dtype=np.uint64)


def prep_queries16(Q, metric, d, truncate=False, table=L.SWIZZLE, repeat=True):
    """-> (Q16 raw, gamma [q_rows], quv [q_rows][2], q_rows)"""
    nq = len(Q)
    q_rows = (nq + 255) // 256 * 256
    ld16 = L.ld16_of(d)
    qh, ss, beta, ok = _unit32(Q)
    H = np.zeros((nq, ld16), dtype=f16)
    H[:, :d] = round16(qh, truncate)
    g = np.ones(q_rows, dtype=f32)
    uv = np.zeros((q_rows, 2), dtype=f32)
    uv[:, 0] = 1
    pos = beta > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        if metric == "ip":
            g[:nq] = np.where(pos, f32(1) / beta, f32(1))
            uv[:nq, 0] = np.where(pos, beta, f32(1))
        elif metric == "l2":
            g[:nq] = np.where(pos, f32(0.5) / beta, f32(1))
            uv[:nq, 0] = np.where(pos, f32(2) * beta, f32(1))
            uv[:nq, 1] = np.where(pos, ss, f32(0))
    uv[:nq, 0] = np.where(ok, uv[:nq, 0], f32(np.nan))
    return L.layout_q16(H, q_rows, ld16, table, repeat), g, uv, q_rows


def dump_scores(x16_raw, rowp16, q16_raw, gamma, nq, d, row0, n_rows, eps):
    """the kernel's score of rows [row0, +n_rows) against every query: fma(a, dot16 + eps, b * gamma), modelled as the float64
    value rounded once"""
    ld16 = L.ld16_of(d)
    idx = L.scan16_index(np.arange(row0, row0 + n_rows)[:, None], np.arange(ld16)[None, :], ld16)
    Xh = np.asarray(x16_raw).view(np.uint16)[idx].view(f16).astype(np.float64)
    Qh = L.delayout_q16(q16_raw, nq, ld16).astype(np.float64)
    P = rowp16[row0:row0 + n_rows].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        bg = (rowp16[row0:row0 + n_rows, 1:2] * np.asarray(gamma, dtype=f32)[None, :nq]).astype(f32).astype(np.float64)
        return (bg + P[:, 0:1] * (Xh @ Qh.T + float(eps))).astype(f32)


def sample_select(S, kprime, off_by_one=False):
    """S [rows][nq] -> gthr [nq]: the key of the k'-th smallest score with the largest id (NaN scores skipped; fewer: all ones)"""
    out = np.full(S.shape[1], L.KEY_INF, dtype=np.uint64)
    k = kprime + (1 if off_by_one else 0)
    for q in range(S.shape[1]):
        col = S[:, q]
        col = np.sort(col[~np.isnan(col)])
        if len(col) >= k:
            out[q] = L.make_key(col[k - 1], 0xFFFFFFFF)
    return out


def collect_pass(S_win, g, kprime, tile0, n_tiles, n_chunks, tiles_per_chunk, n_pub, tile_rows=L.TILE):
    """S_win [window rows][nq] by row - tile0 * tile_rows -> part [nq][2 n_chunks][k']: every list the k' smallest keys below
    g[q] of its own rows (no threshold shared between the chunks: one of the behaviours the kernel's race allows)"""
    nq = S_win.shape[1]
    part = np.full((nq, 2 * n_chunks, kprime), L.KEY_INF, dtype=np.uint64)
    for lst in range(2 * n_chunks):
        rows = L.list_rows(lst, tile0, n_tiles, tiles_per_chunk, tile_rows)
        rows = rows[rows < n_pub]
        if not len(rows):
            continue
        for q in range(nq):
            sc = S_win[rows - tile0 * tile_rows, q]
            keep = ~np.isnan(sc)
            keys = L.make_key(sc[keep], rows[keep])
            keys = np.sort(keys[keys < g[q]])[:kprime]
            part[q, lst, :len(keys)] = keys
    return part


def merge(part, g, kprime):
    """-> (merged [nq][64], outgoing gthr [nq]): the 64 smallest keys of the union of a query's lists; the k'-th becomes the
    next threshold, which stays what it was while fewer are known"""
    nq = part.shape[0]
    merged = np.full((nq, 64), L.KEY_INF, dtype=np.uint64)
    out = np.array(g, dtype=np.uint64).copy()
    for q in range(nq):
        keys = np.sort(part[q].ravel())[:64]
        merged[q, :len(keys)] = keys
        if merged[q, kprime - 1] != L.KEY_INF:
            out[q] = merged[q, kprime - 1]
    return merged, out
