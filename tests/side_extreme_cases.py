"""Helper of the side searches' extreme-value tests (no test here): the data of every case of
tests/test_side_searches_extreme.py, and the CPU model that says what the int8 radius routes do with each of its queries —
shared by that file and by tests/test_side_extreme_model.py, which checks the model's soundness and the cases' conditions
without a GPU.

The model is range_thr (tests/range_cases.py) over the int8 lower bound of tests/i8_model.py with prep_queries8's query rule
(_query_params(band=True)), driven through the pass plans of tests/masked_cases.py and tests/largek_cases.py.  It follows one
query at a time through the passes, as radius_knn / radius_rerank_kernel do (ehx_call.cpp, k_radius.hip), and — unlike the
cascades of tests/test_masked_model.py and tests/largek_cases.py, which assert that nothing is marked and nothing overflows
— gives every query a verdict:

  served       every pass's pool fill is at most POOL_CAP / 2 = 2048 — or the pass holds at most POOL_CAP (allowed) rows: a
               looser bound lets more of them through, never more than there are, so such a pass cannot overflow
  marked       range_thr marks it in some pass (u NaN or not positive, an infinite radius, a threshold or margin that is not
               finite): the device hands it to an exact path and counts no overflow
  overflowed   more than POOL_CAP = 4096 rows pass the threshold in some pass: handed on, counted as overflowed
  undecided    a fill in (2048, 4096]: the device's bound is a little looser than the model's (steps raised to their lane
               group's), so either may happen; the GPU tests bound the counters of a batch that holds one and do not pin them

A pool fill is what the device's pool counter sees: the rows (the ALLOWED rows, under a bitmap) of the pass's tiles with
S_lower <= thr; for "served" the keys carried between passes are added, as tests/test_masked_model.py does."""
import functools

import numpy as np

import extreme_cases as xc
import grouped_model as gm
import i8_model as m8
import largek_cases as lc
import masked_cases as mc
import masked_multi_cases as mmc
import range_cases as rc
import range_masked_cases as rmc
from oracle import pyoracle

f32 = np.float32
D = 128
N_I8 = 20000            # the int8 routes: above i8_min_rows, three large-k passes
N_EXACT = 4000          # spaces that stay on the exact kernels
N_GRAPH = 3000          # graph-mode spaces
N_PAD = 64              # every batch holds at least largek_cases.MIN_QUERIES queries
METRICS = ("l2", "ip", "cosine")          # the engine's metric numbers 0, 1, 2
RANKS = (1, 10, 100)    # range search: radii at the oracle's j-th distance
MAX_RESULTS = 256
MASKED_KS = (10, 48)
LARGE_K = 100
BYKEYS_K = 48
POOL_CAP = lc.POOL_CAP
SERVED, MARKED, OVERFLOWED, UNDECIDED = "served", "marked", "overflowed", "undecided"
EXACT = "exact"         # under a table of bitmaps: the query's mask takes the exact / list route outright, no verdict
GROUPED_KM = ((10, 1), (100, 3))          # grouped kNN: (k, per_group)
MASK_NAMES = ("half", "few", "block", "no_block", "empty", "ones")


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _pad(rng, Q, n=N_PAD):
    """Q and ordinary queries behind it, `n` in all"""
    return np.concatenate([Q, rng.standard_normal((n - len(Q), Q.shape[1])).astype(f32)]) if len(Q) < n else Q


# ---- the cases: name pieces in, (rows, queries) out ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ladder(kind, metric):
    """a. test_extreme_values' ladder (same seeds) on N_I8 rows for the kinds the filters bound, N_EXACT for the others;
    queries 0-19 ordinary, 20-24 near-copies of block rows 0, 1, 2, 3, 5, 25 zero, 26-63 ordinary"""
    seed = xc.KINDS.index(kind) * 3 + METRICS.index(metric)
    X, Q = xc._ladder(kind, D, seed=seed, n=N_I8 if kind in xc.SAFE else N_EXACT)
    return _frozen(X, _pad(np.random.default_rng(1000 + seed), Q))


@functools.lru_cache(maxsize=None)
def one_kind(kind):
    """b. N_I8 rows of one kind; queries 0-5 ordinary, 6-8 stored rows, 9 zero, 10-31 of the rows' own kind, 32-63 ordinary"""
    rng = np.random.default_rng(7 + xc.KINDS.index(kind))
    X = xc._kind_rows(kind, rng, N_I8, D)
    Q = np.concatenate([rng.standard_normal((6, D)).astype(f32), X[[3, 17, 4000]], np.zeros((1, D), f32),
                        xc._kind_rows(kind, rng, 22, D)])
    return _frozen(X, _pad(rng, Q))


@functools.lru_cache(maxsize=None)
def odd(metric):
    """c. 257 queries, extreme_cases._odd_queries at ODD_AT, over ordinary rows"""
    rng = np.random.default_rng(50 + METRICS.index(metric))
    X = rng.standard_normal((N_I8, D)).astype(f32)
    Q = rng.standard_normal((257, D)).astype(f32)
    for at, q in zip(xc.ODD_AT, xc._odd_queries(rng, D)):
        Q[at] = q
    return _frozen(X, Q)


@functools.lru_cache(maxsize=None)
def cross(rows_huge, metric):
    """d. test_cross_band_rows_and_queries' magnitude pairs: huge rows with tiny queries, or the reverse; queries 0-3 of the
    rows' own scale"""
    rng = np.random.default_rng(70 + METRICS.index(metric) + 2 * rows_huge)
    big, small = (1.25e29, 5e29), (2e-24, 8e-24)
    X = xc._scaled(rng, N_I8, D, *(big if rows_huge else small))
    Q = xc._scaled(rng, N_PAD, D, *(small if rows_huge else big))
    Q[:4] = xc._scaled(rng, 4, D, *(big if rows_huge else small))
    return _frozen(X, Q)


with np.errstate(over="ignore"):
    F16_FINITE = xc.F16_EDGE[np.isfinite(xc.F16_EDGE.astype(np.float16).astype(f32))]


@functools.lru_cache(maxsize=None)
def f16_rows(metric):
    """f. ordinary rows, one binary16 edge value in rows 500 + i and rows 600 + i made of it, ROUNDED to binary16 as the space
    stores them (the caller sets the unrounded rows: second value); queries: ordinary ones and five of those rows"""
    rng = np.random.default_rng(110 + METRICS.index(metric))
    X = rng.standard_normal((N_I8, D)).astype(f32)
    for i, v in enumerate(F16_FINITE):
        X[500 + i, i] = v
        X[600 + i, :] = v
    Xh = X.astype(np.float16).astype(f32)
    assert np.isfinite(Xh).all()
    Q = np.concatenate([rng.standard_normal((12, D)).astype(f32), X[[501, 600, 602, 604, 606]]])
    return _frozen(Xh, X, _pad(rng, Q))


def bitmaps(n, seed):
    """50 % random — on an int8 space masked_cases' "half" with the last tile of its first pass thinned until that pass ends on
    exactly POOL_CAP allowed rows: it cannot overflow whatever the bound lets through, so what the model says of a query there
    does not hang on the few rows by which the device's bound is looser — and a bitmap of at most 1024 allowed rows, a part of
    the block among them, for the exact route"""
    rng = np.random.default_rng(seed)
    if n == N_I8:
        half = mc.masks(n)["half"].copy()
        t0, nt = mc.passes(half)[0]
        last = np.arange((t0 + nt - 1) * mc.TILE, (t0 + nt) * mc.TILE)
        surplus = int(half[:(t0 + nt) * mc.TILE].sum()) - mc.SAMPLE * mc.GROWTH
        half[last[half[last]][:surplus]] = False
        assert mc.passes(half)[0] == (t0, nt) and half[:(t0 + nt) * mc.TILE].sum() == POOL_CAP and len(mc.passes(half)) == 2
        assert half.sum() > mc.exact_cut(n)
    else:
        half = rng.random(n) < 0.5
    few = np.zeros(n, dtype=bool)
    few[rng.choice(n, size=900, replace=False)] = True
    few[xc.BLOCK0:xc.BLOCK0 + 100] = True
    assert few.sum() <= 1024
    return half, few


def lists(n, nq, seed):
    """a shared list of 1500 rows with half of the block in it, and per-query lists of 0 .. 700 rows with some block rows"""
    rng = np.random.default_rng(seed)
    shared = np.unique(np.concatenate([rng.choice(n, size=1400, replace=False),
                                       np.arange(xc.BLOCK0, xc.BLOCK0 + xc.NBLOCK, 2)])).astype(np.uint64)
    lens = [0, 1, 9, 63, 64, 65, 257, 700]
    per = []
    for i in range(nq):   # (unsorted, every id once: a repeated id may come back repeated)
        L = np.unique(np.concatenate([rng.choice(n, size=lens[i % 8], replace=False),
                                      xc.BLOCK0 + rng.choice(xc.NBLOCK, size=min(lens[i % 8], 12), replace=False)]))
        per.append(rng.permutation(L).astype(np.uint64))
    return shared, per


def bykeys_rows(n, seed):
    """64 stored rows as queries: block rows 0-5 among them, the others spread over the ids"""
    rng = np.random.default_rng(seed)
    outside = np.r_[0:xc.BLOCK0, xc.BLOCK0 + xc.NBLOCK:n]
    idx = np.concatenate([xc.BLOCK0 + np.array([0, 1, 2, 3, 4, 5]), rng.choice(outside, size=58, replace=False)])
    return [int(i) for i in idx]


# ---- the model -----------------------------------------------------------------------------------------------------------

class Model:
    """one space (rows X as stored) and one batch of queries under one metric"""

    def __init__(self, X, Q, metric):
        self.metric, self.n, self.nq = metric, X.shape[0], Q.shape[0]
        d = X.shape[1]
        with np.errstate(all="ignore"):
            xi, A, B, C, Dr = m8._row_params(X, metric, d)
            qi, sq, eq, g, u, v = m8._query_params(Q, metric, d, band=True)
            I = xi.astype(np.float64) @ qi.astype(np.float64).T
            t = (sq[None, :] * I.astype(f32)).astype(f32)
            K = (B[:, None] * g[None, :] + (C[:, None] * eq[None, :] + Dr[:, None]).astype(f32)).astype(f32)
            self.S = (A[:, None] * t + K).astype(f32)            # S_lower [rows, queries]
            self.max_sumsq = f32((X.astype(f32) ** 2).sum(axis=1, dtype=f32).max())
        self.u, self.v, self.d = u, v, d
        # the oracle's distance of every pair [rows, queries], NaN where the oracle lists no neighbour
        ids, dist, cnt = pyoracle.exhaustive(np.ascontiguousarray(X), np.ascontiguousarray(Q), self.n, rc.OM[metric])
        self.oracle = (ids, dist, cnt)
        self.Dm = np.full((self.n, self.nq), np.nan, dtype=f32)
        for q in range(self.nq):
            c = int(cnt[q])
            self.Dm[ids[q, :c].astype(np.int64), q] = dist[q, :c]

    def _thr(self, radius):
        return rc.range_thr(radius, self.u, self.v, self.metric, self.d, self.max_sumsq)

    def range(self, radius, allow=None):
        """the range search's ONE pass over every tile -> (verdict [nq], fill [nq]); asserts that the threshold hides no
        member of a query it does not mark.  allow: bool [rows, queries] or [rows] — the rows every query's bitmap allows
        (the range search under row bitmaps: the flush drops the others, so only allowed rows fill the pool and only
        allowed rows are members).  The verdict is the SCAN route's: masked_multi_cases.scans says which queries take the
        list route outright."""
        radius = np.asarray(radius, dtype=f32)
        thr, marked = self._thr(radius)
        with np.errstate(invalid="ignore"):
            through = self.S <= thr[None, :]
            member = self.Dm <= radius[None, :]
        if allow is not None:
            allow = np.asarray(allow, dtype=bool)
            allow = allow[:, None] if allow.ndim == 1 else allow
            through, member = through & allow, member & allow
        hidden = member & ~through & ~marked[None, :]
        assert not hidden.any(), "the threshold hides %d members (queries %s)" % (
            int(hidden.sum()), np.nonzero(hidden.any(axis=0))[0][:8].tolist())
        fill = through.sum(axis=0)
        verdict = np.where(marked, MARKED, np.where(fill > POOL_CAP, OVERFLOWED,
                                                    np.where(fill > POOL_CAP // 2, UNDECIDED, SERVED)))
        return verdict, np.where(marked, -1, fill)

    def knn(self, k, allowed=None):
        """the falling-radius kNN: allowed None: the large-k route (a strided sample seeds the radius), else the bitmap
        search's scan route.  -> (verdict [nq], fills [passes][nq] (-1: not scanned any more), answers: the ids of every served
        query, None for the others).  Asserts, at every pass, that no allowed row within the radius lies above the threshold."""
        n = self.n
        if allowed is None:
            plan, smp, allow = lc.passes(n), lc.sample_ids(n), np.ones(n, dtype=bool)
        else:
            plan, smp, allow = mc.passes(allowed), mc.sample_ids(allowed), allowed
        return self._falling(k, plan, [allow] * self.nq, [smp] * self.nq)

    def knn_table(self, k, tab, mask_of):
        """the bitmap-table scan route (ehx_masked.cpp, masked_answer): ONE pass plan for the batch —
        masked_multi_cases.passes(tab, mask_of), cut by the pointwise maximum of the scanned masks' running counts — every
        scan-route query under its OWN bitmap, its first radius the exact k-th distance over its OWN mask's sample
        (masked_cases.sample_ids of that mask: every ceil(allowed / 256)-th allowed id by rank, +Inf while the sample gives
        fewer than k).  -> knn's triple; a query whose mask takes the exact route outright has the verdict EXACT, fills -1
        and no answer."""
        tab, mask_of = np.asarray(tab, dtype=bool), np.asarray(mask_of)
        scans = mmc.scans(tab)
        smp = [mc.sample_ids(tab[m]) if scans[m] else None for m in range(len(tab))]
        return self._falling(k, mmc.passes(tab, mask_of), [tab[m] if scans[m] else None for m in mask_of],
                             [smp[m] for m in mask_of])

    def _falling(self, k, plan, allow_of, sample_of):
        """the falling-radius cascade of knn / knn_table: query q under the rows allow_of[q] (None: not on the route), its
        first radius from the rows sample_of[q]"""
        n, nq, Dm = self.n, self.nq, self.Dm
        live = np.array([a is not None for a in allow_of])
        radius = np.full(nq, np.inf, dtype=f32)
        for q in np.nonzero(live)[0]:
            dq = Dm[sample_of[q], q]
            dq = np.sort(dq[~np.isnan(dq)])
            if len(dq) >= k:                # fewer than k: +Inf, the query is marked
                radius[q] = dq[k - 1]
        verdict = np.where(live, SERVED, EXACT).astype(object)
        carried = [np.zeros(0, dtype=np.int64) for _ in range(nq)]
        fills = []
        for t0, nt in plan:
            lo, hi = t0 * lc.TILE, min((t0 + nt) * lc.TILE, n)
            thr, marked = self._thr(radius)
            fill = np.full(nq, -1, dtype=np.int64)
            for q in np.nonzero(live)[0]:
                if marked[q]:
                    verdict[q], live[q] = MARKED, False
                    continue
                allow = allow_of[q]
                in_pass = int(allow[lo:hi].sum())   # (a pass of at most POOL_CAP rows cannot overflow, however loose the bound)
                with np.errstate(invalid="ignore"):
                    through = (self.S[lo:hi, q] <= thr[q]) & allow[lo:hi]
                    member = allow[lo:hi] & (Dm[lo:hi, q] <= radius[q])
                assert not (member & ~through).any(), "query %d: the threshold hides %d rows within the radius" % (
                    q, int((member & ~through).sum()))
                fill[q] = int(through.sum())
                if fill[q] > POOL_CAP:
                    verdict[q], live[q] = OVERFLOWED, False
                elif fill[q] + len(carried[q]) > POOL_CAP // 2 and in_pass > POOL_CAP:
                    verdict[q], live[q] = UNDECIDED, False
                else:                                                 # radius_rerank_kernel
                    pool = np.concatenate([carried[q], lo + np.nonzero(member)[0]])
                    pool = pool[np.lexsort((pool, Dm[pool, q]))][:k]
                    if len(pool) == k:
                        assert Dm[pool[-1], q] <= radius[q]           # the radius only falls
                        radius[q] = Dm[pool[-1], q]
                    carried[q] = pool
            fills.append(fill)
        answers = [carried[q] if verdict[q] == SERVED else None for q in range(nq)]
        return verdict, fills, answers

    def top(self, q, k, allowed=None):
        """the oracle's first k (allowed) rows of query q in (distance, id) order"""
        ids, dist, cnt = self.oracle
        L = ids[q, :int(cnt[q])].astype(np.int64)
        return (L if allowed is None else L[allowed[L]])[:k]

    def knn_grouped(self, k, m, labels):
        """the grouped kNN's scan route (ehx_grouped.cpp): grouped_model.passes_model — the large-k route's strided sample
        capped and cut at k for the first radius, then per pass: hits capped, merged with the carried keys, capped again, the
        radius falling — over largek_cases' passes, the rows let through being S_lower <= range_thr(radius).
        -> (verdict [nq], fills [passes][nq], answers, short: bool [nq], the capped sample holds fewer than k rows — the radius
        stays +Inf and the query is marked through the seed).  Verdicts as knn's; asserts that no row within a radius is hidden
        (passes_model does) and that a served query's answer is the capped greedy over the oracle's order."""
        n, nq, Dm = self.n, self.nq, self.Dm
        ranges, smp = gm.scan_ranges(n), lc.sample_ids(n)
        verdict = np.full(nq, SERVED, dtype=object)
        fills = [np.full(nq, -1, dtype=np.int64) for _ in ranges]
        answers, short = [None] * nq, np.zeros(nq, dtype=bool)
        for q in range(nq):
            dist = Dm[:, q]
            ok = smp[~np.isnan(dist[smp])]
            capped = gm._cap(ok[np.lexsort((ok, dist[ok]))].tolist(), labels, m)
            short[q] = len(capped) < k
            carried_at = []

            def through(j, lo, hi, radius, q=q, carried_at=carried_at):
                thr, marked = rc.range_thr(np.array([radius], dtype=f32), self.u[q:q + 1], self.v[q:q + 1], self.metric,
                                           self.d, self.max_sumsq)
                if marked[0]:
                    raise _Handed(MARKED)
                with np.errstate(invalid="ignore"):
                    t = self.S[lo:hi, q] <= thr[0]
                fills[j][q] = int(t.sum())
                if fills[j][q] > POOL_CAP:
                    raise _Handed(OVERFLOWED)
                if fills[j][q] + carried_at[j] > POOL_CAP // 2 and hi - lo > POOL_CAP:
                    raise _Handed(UNDECIDED)
                return t
            try:
                ans, _, _ = gm.passes_model(dist, labels, k, m, ranges, sample=smp, through=through, carried_at=carried_at)
            except _Handed as e:
                verdict[q] = e.args[0]
                continue
            order = self.oracle[0][q, :int(self.oracle[2][q])].astype(np.int64)
            assert ans == gm.capped_greedy(order.tolist(), labels, k, m), "query %d: not the capped greedy" % q
            answers[q] = np.asarray(ans, dtype=np.int64)
        assert not (short & (verdict == SERVED)).any()   # (+Inf is never served)
        return verdict, fills, answers, short


class _Handed(Exception):
    pass


def tally(verdict):
    """-> (served, marked, overflowed, undecided) of a batch"""
    v = np.asarray(verdict)
    return tuple(int((v == w).sum()) for w in (SERVED, MARKED, OVERFLOWED, UNDECIDED))


def worst(fills):
    """the worst fill of every pass (-1: no query scanned)"""
    return [int(f.max()) for f in fills]


def rank_radii(oracle, rank, other=1.0):
    """the oracle's rank-th distance of every query; `other` for a query with fewer neighbours than that"""
    ids, dist, cnt = oracle
    return np.array([dist[q, rank - 1] if cnt[q] >= rank else other for q in range(len(cnt))], dtype=f32)


def route_verdicts(X, Q, metric, half, key_rows=None, radii=None):
    """what every int8 route of the GPU tests does with the batch Q on the space X: {route: (verdict, fills, answers)} and the
    model under "model".  Routes: ("range", rank) (radii: {rank: radius per query} in place of the oracle's rank-th distances),
    ("masked", k) under the bitmap `half`, "largek", and "bykeys" (the queries are the stored rows `key_rows`, k + 1)."""
    m = Model(X, Q, metric)
    out = {"model": m}
    for rank in RANKS:
        r = rank_radii(m.oracle, rank) if radii is None else radii[rank]
        out["range", rank] = m.range(r) + (None,)
    for k in MASKED_KS:
        out["masked", k] = m.knn(k, half)
    out["largek"] = m.knn(LARGE_K)
    if key_rows is not None:
        out["bykeys"] = Model(X, np.ascontiguousarray(X[key_rows]), metric).knn(BYKEYS_K + 1)
    return out


def expect_counters(verdict, route, handed, overflowed, what):
    """the counters of one call against the model's verdicts: a served query is counted on its route, a marked one as handed on
    and not as overflowed, an overflowed one as both; with undecided queries in the batch only the sums are pinned"""
    sv, mk, ov, un = tally(verdict)
    assert route + handed == len(verdict), (what, route, handed)
    assert overflowed == handed - mk, (what, "handed", handed, "marked", mk, "overflowed", overflowed)
    if un == 0:
        assert (route, handed, overflowed) == (sv, mk + ov, ov), (what, (route, handed, overflowed), (sv, mk, ov))
    else:
        assert sv <= route <= sv + un, (what, route, sv, un)


# ---- the int8 cases by name: what both test files walk -------------------------------------------------------------------

def odd_radii(oracle, rank):
    """c. the ordinary queries' rank-th distance; every odd query gets the median of those, a finite radius"""
    r = rank_radii(oracle, rank)
    keep = np.setdiff1d(np.arange(len(r)), xc.ODD_AT)
    r[xc.ODD_AT] = np.median(r[keep])
    return r


def int8_case_names():
    return (["ladder-%s-%s" % (k, m) for k in xc.KINDS if k in xc.SAFE for m in METRICS]
            + ["one-%s-%s" % (k, m) for k in ("a_lo", "a_hi", "f") for m in METRICS]
            + ["odd-%s" % m for m in METRICS]
            + ["cross-%s-%s" % (w, m) for w in ("rows_huge", "queries_huge") for m in ("l2", "ip")]
            + ["f16-%s" % m for m in METRICS])


def int8_case(name):
    """-> dict: X (the rows as stored), X_set (the rows the caller sets), Q, metric, key_rows (or None), ordinary (the indices
    of the queries that are ordinary ones)"""
    parts = name.split("-")
    fam, metric = parts[0], parts[-1]
    out = {"metric": metric, "key_rows": None}
    if fam == "ladder":
        X, Q = ladder(parts[1], metric)
        out.update(X=X, X_set=X, Q=Q, key_rows=bykeys_rows(len(X), 5), ordinary=np.r_[0:20, 26:N_PAD])
    elif fam == "one":
        X, Q = one_kind(parts[1])
        out.update(X=X, X_set=X, Q=Q, key_rows=bykeys_rows(len(X), 6), ordinary=np.r_[0:6, 32:N_PAD])
    elif fam == "odd":
        X, Q = odd(metric)
        out.update(X=X, X_set=X, Q=Q, ordinary=np.setdiff1d(np.arange(len(Q)), xc.ODD_AT))
    elif fam == "cross":
        X, Q = cross(parts[1] == "rows_huge", metric)
        out.update(X=X, X_set=X, Q=Q, ordinary=np.zeros(0, dtype=np.int64))
    elif fam == "f16":
        Xh, X, Q = f16_rows(metric)
        out.update(X=Xh, X_set=X, Q=Q, key_rows=bykeys_rows(len(X), 7)[6:] + [501, 600, 601, 602, 604, 606],
                   ordinary=np.r_[0:12, 17:N_PAD])
    else:
        raise ValueError(name)
    return out


def case_verdicts(name):
    c = int8_case(name)
    half, _ = bitmaps(len(c["X"]), 1)
    radii = None
    if name.startswith("odd"):
        oracle = pyoracle.exhaustive(np.ascontiguousarray(c["X"]), np.ascontiguousarray(c["Q"]), max(RANKS),
                                     rc.OM[c["metric"]])
        radii = {rank: odd_radii(oracle, rank) for rank in RANKS}
    v = route_verdicts(c["X"], c["Q"], c["metric"], half, c["key_rows"], radii)
    v["radii"] = radii
    return c, half, v


# ---- the filtered searches: range under a table of bitmaps, kNN under it, grouped kNN ---------------------------------------

def mask_table(n, seed=1):
    """bool [6, n], MASK_NAMES: bitmaps(n, seed)'s half (on an int8 space: a first pass that cannot overflow) and few (<= 1024
    rows, 100 of the block: the list / exact route in the same batch as scan-route queries); only the block's 256 rows (a
    list made wholly of the extreme kind); every row but the block; none; all"""
    half, few = bitmaps(n, seed)
    block = np.zeros(n, dtype=bool)
    block[xc.BLOCK0:xc.BLOCK0 + xc.NBLOCK] = True
    tab = np.stack([half, few, block, ~block, np.zeros(n, dtype=bool), np.ones(n, dtype=bool)])
    tab.setflags(write=False)
    return tab


BIG_LABEL = 0xFFFFFFFE   # the largest real label: beside NONE, and beside the padding key of the cap's sort
BIG_LABEL_ROWS = (3, 4003, 8003, 12003, 16003)


def group_labels(n, few_in_sample=False):
    """uint32 [n]: row % 97, every 11th row a group of its own; the block's rows {5, 6, 7, NONE} in turn, so that extreme rows
    compete with ordinary rows of the same label for a quota; BIG_LABEL on BIG_LABEL_ROWS (those below n).
    few_in_sample (the spaces of one kind): row % 100 and every 13th row NONE instead — the large-k sample of 20 000 rows, the
    ids 0, 20, 40, ..., then carries six labels and 76 NONE rows: 82 capped rows at per_group 1, 94 at per_group 3.  At
    (k, per_group) = (100, 3) the cap leaves the seed fewer than k rows, the radius stays +Inf and EVERY query is marked
    through the seed; at (10, 1) the seed is whole.  (Whether the capped sample reaches k does not depend on the query, NaN
    distances aside: no one labeling gives a batch both.)"""
    g = (np.arange(n, dtype=np.int64) % (100 if few_in_sample else 97)).astype(np.uint32)
    g[::13 if few_in_sample else 11] = gm.NONE
    g[xc.BLOCK0:xc.BLOCK0 + xc.NBLOCK] = np.array([5, 6, 7, gm.NONE], dtype=np.uint32)[np.arange(xc.NBLOCK) % 4]
    for r in BIG_LABEL_ROWS:
        if r < n:
            g[r] = BIG_LABEL
    g.setflags(write=False)
    return g


def for_counters(verdict):
    """a table's verdicts as expect_counters reads them: a query whose mask takes the exact / list route outright is handed on
    and is no overflow, as a marked one is"""
    v = np.asarray(verdict).copy()
    v[v == EXACT] = MARKED
    return v


FILTERED_ROUTES = ([("rangem", rank) for rank in RANKS] + [("table", k) for k in MASKED_KS]
                   + [("grouped", k, per) for k, per in GROUPED_KM])


class _Routes(dict):
    """filtered_routes' result: a route's verdicts are worked out when they are first asked for"""

    def __missing__(self, key):
        m, tab, mask_of, scans = self["model"], self["tab"], self["mask_of"], self["scans"]
        if key[0] == "radii":
            value = rmc.radii_at(self["lists"], m.nq, key[1])
        elif key[0] == "rangem":
            verdict, fill = m.range(self["radii", key[1]], tab[mask_of].T)
            value = (np.where(scans, verdict, EXACT), np.where(scans, fill, -1))
        elif key[0] == "table":
            value = m.knn_table(key[1], tab, mask_of)
        elif key[0] == "grouped":
            value = m.knn_grouped(key[1], key[2], self["labels"])
        else:
            raise KeyError(key)
        self[key] = value
        return value


def filtered_routes(X, Q, metric, few_in_sample=False):
    """what the three filtered searches' int8 routes do with the batch Q on the space X under mask_table / group_labels:
    {"model", "tab", "mask_of", "labels", "lists" (range_masked_cases.lists_under: the oracle under every mask), "scans" (bool
    [nq]: the query's mask is on the scan route), and per route of FILTERED_ROUTES, worked out at its first use: ("radii",
    rank): the rank-th allowed distance of every query, ("rangem", rank): (verdict, fill), ("table", k): knn's triple,
    ("grouped", k, m): knn_grouped's four}.  few_in_sample: group_labels'."""
    n, nq = len(X), len(Q)
    tab, mask_of = mask_table(n), mmc.interleaved(nq, len(MASK_NAMES))
    return _Routes(model=Model(X, Q, metric), tab=tab, mask_of=mask_of, labels=group_labels(n, few_in_sample),
                   lists=rmc.lists_under(X, Q, rc.OM[metric], tab, mask_of), scans=mmc.scans(tab)[mask_of])


@functools.lru_cache(maxsize=2)
def filtered_verdicts(name):
    """-> (case, filtered_routes of it); the spaces of one kind under group_labels' few_in_sample"""
    c = int8_case(name)
    return c, filtered_routes(c["X"], c["Q"], c["metric"], few_in_sample=name.startswith("one-"))


@functools.lru_cache(maxsize=None)
def sharded():
    """h. 40 000 rows just inside the band's high edge for two row shards (shard i holds rows i, i + 2, ...); one_kind's mix
    of queries"""
    rng = np.random.default_rng(91)
    X = xc._kind_rows("a_hi", rng, 2 * N_I8, D)
    Q = np.concatenate([rng.standard_normal((6, D)).astype(f32), X[[3, 17, 4000]], np.zeros((1, D), f32),
                        xc._kind_rows("a_hi", rng, 22, D)])
    return _frozen(X, _pad(rng, Q))


FLT_MAX = np.finfo(f32).max
RADIUS_KINDS = ("+FLT_MAX", "-FLT_MAX", "+0", "-0", "smallest subnormal", "a distance near 1e-24", "one ulp below it",
                "a distance near 1e30", "one ulp below it")


@functools.lru_cache(maxsize=None)
def extreme_radii(space, metric):
    """e. (rows, 64 queries, one radius per query: RADIUS_KINDS[i % 9]).  space "a_hi": one_kind("a_hi"), whose L2 distances
    reach 1e30; "ordinary": Gaussian rows, and every query that gets a radius near 1e-24 is a stored row moved by 1e-12 in a
    component that is zero there — its L2 distance to that row is 1e-24.  "A distance near t" is the query's oracle distance
    closest to t in magnitude (by ratio), zero and non-finite ones aside."""
    if space == "a_hi":
        X, Q = one_kind("a_hi")
    else:
        rng = np.random.default_rng(130 + METRICS.index(metric))
        X = rng.standard_normal((N_I8, D)).astype(f32)
        Q = rng.standard_normal((N_PAD, D)).astype(f32)
        for i in range(N_PAD):
            if i % 9 in (5, 6):
                X[100 + i, 0] = 0
                Q[i] = X[100 + i]
                Q[i, 0] = 1e-12
    ids, dist, cnt = pyoracle.exhaustive(np.ascontiguousarray(X), np.ascontiguousarray(Q), len(X), rc.OM[metric])
    radius = np.zeros(len(Q), dtype=f32)
    for i in range(len(Q)):
        kind = i % 9
        dq = dist[i, :int(cnt[i])]
        dq = dq[np.isfinite(dq) & (dq != 0)]
        logs = np.log(np.abs(dq.astype(np.float64)))
        near = lambda t: dq[np.argmin(np.abs(logs - np.log(t)))] if len(dq) else f32(t)  # noqa: E731
        if kind < 5:
            radius[i] = (FLT_MAX, -FLT_MAX, f32(0.0), f32(-0.0), np.nextafter(f32(0), f32(1)))[kind]
        elif kind < 7:
            radius[i] = near(1e-24) if kind == 5 else np.nextafter(near(1e-24), f32(-np.inf))
        else:
            radius[i] = near(1e30) if kind == 7 else np.nextafter(near(1e30), f32(-np.inf))
    return _frozen(X, Q, radius)
