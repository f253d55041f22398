"""CPU model of the side searches at extreme values (host logic, no GPU): what the int8 radius routes — the range search's
one pass, the bitmap search's scan route, the large-k route and the by-key lookup that rides on it — do with every query
of the int8 cases of tests/test_side_searches_extreme.py (data and model: tests/side_extreme_cases.py, on range_thr of
tests/range_cases.py and the int8 bound of tests/i8_model.py with prep_queries8's query rule).

  (a) soundness, at every radius a route meets: no row within the radius has S_lower above the threshold unless the query
      is marked, and the answer the model's cascade reaches for a served query is the oracle's;
  (b) the verdict of every (case, route, query) — served, marked, overflowed, undecided — which the GPU tests assert on the
      device's counters;
  (c) every row-ladder case of a kind the filters bound serves its 20 ordinary queries on every route, so that no GPU case
      passes because everything fell through to an exact path — with ONE exception that no data can remove, pinned below;
  (d) no case leaves more than a quarter of a batch undecided.

The exception to (c): a block of rows just inside the band's high edge under L2, on every route.  cert_margin carries
eps_d (|q| + max|x|)^2 with max|x| the largest norm in the SPACE, 7e14 here: the margin, 5.6e24, dwarfs every distance
between ordinary vectors (at most 375), every ordinary row passes the threshold of an ordinary query, and any pass of
more than 4096 rows overflows (test_the_margin_of_the_exception_exceeds_every_ordinary_distance).  No choice of ordinary
rows changes that, so the condition cannot be met there; the model pins "overflowed" for those queries instead and the
GPU test asserts the overflow counters.  That is the bound working as designed — a loose threshold costs time, never
correctness.  Under inner product the margin, eps_d |q| max|x| = 1e11, is as hopeless among ordinary rows, but the radii
the routes meet lie among the huge rows themselves (distances near -1e14), where it is small again: the range search
serves the ordinary queries outright, and the kNN routes do once their first pass — exactly 4096 allowed rows under the
bitmap of side_extreme_cases.bitmaps, the first 4096 rows on the large-k route: neither can overflow — has pulled the
radius down there.

Figures of one run (served / marked / overflowed of a batch of 64, of 257 for the odd queries; worst pool fill per pass
over the SERVED queries), as ranges over the metrics named:
  ladder a_lo, f    L2: 64 / 0 / 0.  range 256 (the block), bitmap k 10: 416-442, k 48: 1164-1202, large k 766-790, by key
                    493-521.  inner product, cosine: 58 / 0 / 6 or 63 / 0 / 1 (the zero query and the near-copies of tiny
                    rows overflow: 20 000 rows through).  range 5-182, bitmap 320-408 | 38-49 and 1134-1240 | 125-148, large k
                    589-635 | 541-625 | 48-55, by key 329-356 | 276-312 | 26-30
  ladder a_hi       cosine: 63 / 0 / 1, fills as above.  inner product: 63 / 0 / 1, range 5-126, bitmap 4053 | 0 and large k
                    4012 | 0 | 0 in a first pass that cannot overflow.  L2: 0 / 0 / 64 on every route (range@1: 5 / 0 / 59)
  one kind a_hi     64 / 0 / 0 (L2) or 63 / 0 / 1: range 3-205, bitmap 272-400 | 43-48 and 993-1261 | 119-135, large k
                    593-628 | 450-543 | 39-49
  one kind a_lo     cosine 63 / 0 / 1; L2 and inner product 0 / 0 / 64: every row passes every threshold
  one kind f        0 / 0 / 64 under every metric
  odd queries       range 248 / 7 / 2 (cosine 250 / 7 / 0), kNN routes 246-249 / 7 / 1-4: the seven marked are the two NaN, the
                    two Inf, the two out-of-band and the subnormal query; fills 6-190, 399-419 | 45-48, 1223-1284 | 144-157,
                    624-667 | 503-590 | 47-58
  cross-band        huge rows, tiny queries: L2 4 / 60 / 0 (the quotient overflows), inner product 64 / 0 / 0;
                    tiny rows, huge queries: 0 / 0 / 64
  binary16          cosine 63 / 0 / 1; L2 and inner product 0 / 0 / 64 (a row of 65504s: max|x|^2 = 5.5e11) except range@1:
                    2 / 0 / 62 and 49 / 0 / 15
  two shards        64 / 0 / 0 each, 550-567 | 478-516 | 45-47
No case leaves a query undecided.  The test prints every figure before it asserts.

The filtered searches (side_extreme_cases.filtered_routes; tests/test_filtered_searches_extreme.py asserts the counters): the
range search and the kNN under the table of six bitmaps half, few, block, no_block, empty, ones with the queries' masks
interleaved — half, no_block and ones take the scan route: 32 queries of a batch of 64, 128 of 257 — and the grouped kNN at
(k, per_group) = (10, 1) and (100, 3) under side_extreme_cases.group_labels, every query on the scan route.  The same
conditions (a) .. (d) hold for the scan-route queries, with these pinned exceptions to (c), all the margin's again:
  ladder a_hi, L2             every route, as above;
  ladder a_hi, inner product  where the bitmap or the cap takes the huge rows away the radius lies among ordinary distances
                              again and the margin (it carries the largest norm of the SPACE, allowed or not) lets every row
                              through: under no_block on both routes, under half at the 100th allowed distance (about 64 of
                              its 128 block rows lie on a query's side), and the grouped search at (100, 3), where the cap
                              leaves about 41 of the block's rows eligible on a query's side.  Pinned as overflowed.
Figures of one run (of the queries on the route: served / marked / overflowed; worst fill per pass over the served):
  ladder a_lo, f    L2: range 32 / 0 / 0, fill 256 (the block); table k 10: 442-505 | 94-120, k 48: 1095-1220 | 349-372; grouped
                    64 / 0 / 0, 348-364 | 0 | 0 and 818-838 | 198-201 | 19-20.  inner product (and f cosine): 29 / 0 / 3, grouped
                    58 / 0 / 6; a_lo cosine 32 / 0 / 0, grouped 63 / 0 / 1: range 4-179, table 277-353 | 86-125 and 1029-1220 |
                    334-387, grouped 93-136 | 96-103 | 11-12 and 590-636 | 541-627 | 50-55
  ladder a_hi       cosine 32 / 0 / 0 and 63 / 0 / 1, fills as above.  inner product: range 21 / 0 / 11 (rank 100: 10 / 0 / 22),
                    table 21 / 0 / 11 with 4012 | 0 in a first pass that cannot overflow, grouped (10, 1) 63 / 0 / 1 with
                    4012 | 0 | 0, grouped (100, 3) 0 / 0 / 64.  L2: 0 / 0 / 32 and 0 / 0 / 64 (range@1: 2 / 0 / 30)
  one kind a_hi     range and table 32 / 0 / 0 (L2) or 31 / 0 / 1: range 3-172, table 260-287 | 75-111 and 983-1105 | 324-375;
                    grouped (10, 1) 64 / 0 / 0 or 63 / 0 / 1: 484-735 | 71-85 | 9-11
  one kind a_lo     cosine 31 / 0 / 1, grouped (10, 1) 63 / 0 / 1; L2 and inner product 0 / 0 / 32 and 0 / 0 / 64
  one kind f        0 / 0 / 32 and 0 / 0 / 64 under every metric
  one kind, (100, 3) every space of one kind: 0 / 64 / 0 — all 64 queries MARKED THROUGH THE SEED: under group_labels'
                    few_in_sample the capped sample holds 94 rows
  odd queries       range and table 124-126 / 1 / 1-3 of 128 (of the eleven odd queries four are on the scan route); grouped
                    246-249 / 7 / 1-4 of 257, two of the seven marked (cosine: four) through the seed — queries without any
                    neighbour, whose sample is empty whatever the labels;
                    fills 6-187, 346-381 | 116-139, 1122-1247 | 368-418, 132-143 | 100-105 | 10-11, 624-672 | 527-622 | 47-58
  cross-band        huge rows, tiny queries: L2 2 / 30 / 0 and 4 / 60 / 0, inner product 32 / 0 / 0 and 64 / 0 / 0;
                    tiny rows, huge queries: 0 / 0 / 32 and 0 / 0 / 64
  binary16          cosine 32 / 0 / 0 and 63 / 0 / 1; L2 and inner product 0 / 0 / 32 and 0 / 0 / 64 except range@1: 1 / 0 / 31
                    and 27 / 0 / 5
A served grouped answer holds a block row in most cases (all 64 queries of ladder a_lo and f under L2).  No case leaves a query undecided on any of the three routes."""
import numpy as np
import pytest

import extreme_cases as xc
import grouped_model as gm
import i8_model as m8
import largek_cases as lc
import masked_multi_cases as mmc
import range_cases as rc
import side_extreme_cases as sx
import test_masked_model as tmm

f32 = np.float32
CANNOT_SERVE = {("ladder-a_hi-l2", "range"), ("ladder-a_hi-l2", "masked"), ("ladder-a_hi-l2", "largek"),
                ("ladder-a_hi-l2", "bykeys"), ("ladder-a_hi-l2", "rangem"), ("ladder-a_hi-l2", "table"),
                ("ladder-a_hi-l2", "grouped")}
# The same margin under a bitmap that takes the huge rows away: under inner product the unfiltered routes serve the a_hi ladder
# because their radii lie among the huge rows' distances (the docstring above); "no_block" allows none of them, the radii lie
# among ordinary distances again, and the margin — it carries the largest norm of the SPACE, allowed or not — lets every row
# through.  "half" allows 128 of the block's rows, about 64 of them on the query's side (a negative product): the 10th and
# the 48th allowed distance lie among them, the 100th among the ordinary rows again.  Pinned as overflowed, as the L2 case is.
CANNOT_SERVE_UNDER = ({("ladder-a_hi-ip", ("rangem", rank), "no_block") for rank in sx.RANKS}
                      | {("ladder-a_hi-ip", ("table", k), "no_block") for k in sx.MASKED_KS}
                      | {("ladder-a_hi-ip", ("rangem", 100), "half")}
                      # the cap leaves about 41 of the block's rows eligible on a query's side at per_group 3 (32 NONE, 3 x 3)
                      | {("ladder-a_hi-ip", ("grouped", 100, 3), None)})


def _routes(v):
    return [r for r in v if r not in ("model", "radii")]


def _family(route):
    return route if isinstance(route, str) else route[0]


@pytest.mark.parametrize("name", sx.int8_case_names())
def test_routes_are_sound_and_the_cases_meet_their_conditions(name):
    c, half, v = sx.case_verdicts(name)    # asserts (a)'s first half at every pass of every route
    m = v["model"]
    for route in _routes(v):
        verdict, fills, answers = v[route]
        sv, mk, ov, un = sx.tally(verdict)
        worst = [int(fills.max())] if answers is None else sx.worst(fills)
        served = np.nonzero(np.asarray(verdict) == sx.SERVED)[0]
        fills_served = []
        if len(served):
            fills_served = [int(fills[served].max())] if answers is None else [int(f[served].max()) for f in fills]
        print("%s %s: served %d marked %d overflowed %d undecided %d; worst fill per pass %s, of the served %s"
              % (name, route, sv, mk, ov, un, worst, fills_served))
        if answers is not None:              # (a) the cascade's answer is the oracle's
            mm = m if route != "bykeys" else sx.Model(c["X"], np.ascontiguousarray(c["X"][c["key_rows"]]), c["metric"])
            k = sx.LARGE_K if route == "largek" else (sx.BYKEYS_K + 1 if route == "bykeys" else route[1])
            allowed = half if _family(route) == "masked" else None
            for q in served:
                assert np.array_equal(answers[q], mm.top(q, k, allowed)), (name, route, q)
        assert un * 4 <= len(verdict), "(d) %s %s: %d undecided" % (name, route, un)
        if name.startswith("ladder") and route != "bykeys":
            ordinary = np.asarray(verdict)[:20]
            if (name, _family(route)) in CANNOT_SERVE:
                assert (ordinary == sx.OVERFLOWED).all(), (name, route, ordinary)
            else:
                assert (ordinary == sx.SERVED).all(), "(c) %s %s: %s" % (name, route, ordinary)
        if name.startswith("ladder") and route == "bykeys":   # (the queries are stored rows: 6 of the block, 58 ordinary)
            ordinary = np.asarray(verdict)[6:]
            want = sx.OVERFLOWED if (name, "bykeys") in CANNOT_SERVE else sx.SERVED
            assert (ordinary == want).all(), "(c) %s %s: %s" % (name, route, ordinary)


@pytest.mark.parametrize("name", sx.int8_case_names())
def test_filtered_routes_are_sound_and_the_cases_meet_their_conditions(name):
    """the range search and the kNN under the table of six, and the grouped kNN (side_extreme_cases.filtered_routes):
    (a), (c) and (d) above, for the queries whose mask is on the scan route"""
    c, v = sx.filtered_verdicts(name)      # asserts (a)'s first half at every pass of every route, and the grouped greedy
    m, tab, mask_of, labels, scans = v["model"], v["tab"], v["mask_of"], v["labels"], v["scans"]
    assert mmc.scans(tab).tolist() == [True, False, False, True, False, True] and scans.sum() * 2 >= len(scans) - 1
    assert len(mmc.passes(tab, mask_of)) == 2 and len(gm.scan_ranges(len(c["X"]))) == 3
    block = np.arange(xc.BLOCK0, xc.BLOCK0 + xc.NBLOCK)
    for route in sx.FILTERED_ROUTES:
        verdict, fills = v[route][0], v[route][1]
        verdict = np.asarray(verdict)
        sv, mk, ov, un = sx.tally(verdict)
        on = scans if route[0] != "grouped" else np.ones(len(verdict), dtype=bool)
        assert ((verdict == sx.EXACT) == ~on).all()
        fills = fills if isinstance(fills, list) else [fills]
        served = np.nonzero(verdict == sx.SERVED)[0]
        print("%s %s: of %d on the route served %d marked %d overflowed %d undecided %d; worst fill per pass %s, of the served %s"
              % (name, route, on.sum(), sv, mk, ov, un, sx.worst(fills), [int(f[served].max()) for f in fills] if len(served) else []))
        if route[0] == "table":            # (a) the cascade's answer is the oracle's under the query's own mask
            for q in served:
                assert np.array_equal(v[route][2][q], m.top(q, route[1], tab[mask_of[q]])), (name, route, q)
        if route[0] == "grouped":          # (knn_grouped has asserted the capped greedy)
            k, per = route[1:]
            answers, short = v[route][2], v[route][3]
            for q in served:
                assert len(answers[q]) == len(gm.capped_greedy(gm.ordered_rows(m.Dm[:, q]), labels, k, per))
            assert (verdict[short] == sx.MARKED).all()
            real = short & ~np.isnan(m.Dm).all(axis=0)       # (a query without any neighbour is marked whatever the seed)
            with_block = [int(q) for q in served if np.isin(answers[q], block).any()]
            print("   marked through the seed: %d (%d of them queries with neighbours); served with a block row: %d"
                  % (short.sum(), real.sum(), len(with_block)))
        assert un * 4 <= len(verdict), "(d) %s %s: %d undecided" % (name, route, un)
        if name.startswith("ladder"):
            at = np.nonzero(on[:20])[0]
            assert len(at) >= 10
            want = [sx.OVERFLOWED if (name, route[0]) in CANNOT_SERVE or (name, route, sx.MASK_NAMES[mask_of[q]] if
                    route[0] != "grouped" else None) in CANNOT_SERVE_UNDER else sx.SERVED for q in at]
            assert verdict[at].tolist() == want, "(c) %s %s: %s" % (name, route, verdict[at])


def test_the_grouped_cases_hold_a_seed_that_falls_short_and_a_block_row_that_is_served():
    """some int8 case has queries WITH neighbours whose capped sample holds fewer than k rows (marked through the seed: the
    spaces of one kind at (100, 3), side_extreme_cases.group_labels), and some case serves a query whose answer holds a row
    of the block; the test above prints both figures for every case"""
    block = np.arange(xc.BLOCK0, xc.BLOCK0 + xc.NBLOCK)
    seed, with_block = [], []
    for name in ("one-a_hi-l2", "ladder-a_lo-l2"):
        c, v = sx.filtered_verdicts(name)
        for k, per in sx.GROUPED_KM:
            verdict, _, answers, short = v["grouped", k, per]
            real = short & ~np.isnan(v["model"].Dm).all(axis=0)
            if real.any():
                assert (np.asarray(verdict)[real] == sx.MARKED).all()
                seed.append((name, k, per, int(real.sum())))
            n = sum(1 for a in answers if a is not None and np.isin(a, block).any())
            if n:
                with_block.append((name, k, per, n))
    print("marked through the seed (case, k, per_group, queries):", seed)
    print("served with a block row in the answer:", with_block)
    assert seed and with_block


def test_the_labelings_put_the_edges_where_the_cap_meets_them():
    g = sx.group_labels(sx.N_I8)
    assert (g[list(sx.BIG_LABEL_ROWS)] == sx.BIG_LABEL).all() and sx.BIG_LABEL == gm.NONE - 1
    assert g[xc.BLOCK0:xc.BLOCK0 + 8].tolist() == [5, 6, 7, gm.NONE] * 2 and g[11] == gm.NONE and g[12] == 12
    assert (g[np.arange(sx.N_I8) % 97 == 5] == 5).sum() > 100          # ordinary rows share the block's labels
    for few, counts in ((False, (10, 100)), (True, (10, 94))):          # the capped sample at (10, 1) and (100, 3)
        g = sx.group_labels(sx.N_I8, few)
        smp = [int(r) for r in lc.sample_ids(sx.N_I8)]
        assert tuple(min(len(gm._cap(smp, g, per)), k) for k, per in sx.GROUPED_KM) == counts
    tab = sx.mask_table(sx.N_I8)
    assert tab.sum(axis=1).tolist()[2:] == [xc.NBLOCK, sx.N_I8 - xc.NBLOCK, 0, sx.N_I8] and tab[1].sum() <= 1024
    assert tab[1, xc.BLOCK0:xc.BLOCK0 + 100].all()


def test_the_margin_of_the_exception_exceeds_every_ordinary_distance():
    """the exception to (c) is the margin's, not the data's: 1.001 m of an ordinary query on the a_hi ladder lies far above
    its distance to every ordinary row, whatever those rows are"""
    for metric in ("l2", "ip"):   # (ip: what "no_block" leaves of CANNOT_SERVE_UNDER's case)
        X, Q = sx.ladder("a_hi", metric)
        qn = (Q[:20] ** 2).sum(axis=1, dtype=f32)
        mx = f32((X ** 2).sum(axis=1, dtype=f32).max())
        m = rc.cert_margin(metric, sx.D, qn, mx, np.zeros(20, dtype=f32))
        ordinary = np.r_[0:xc.BLOCK0, xc.BLOCK0 + xc.NBLOCK:len(X)]
        far = np.abs(m8._true_distance(X[ordinary][::50], Q[:20], metric)).max()
        print("%s: margin %.3g .. %.3g, the farthest ordinary pair %.3g" % (metric, m.min(), m.max(), far))
        assert m.min() > 1e3 * far


def test_the_query_rule_of_prep_queries8():
    rng = np.random.default_rng(3)
    Q = np.stack(xc._odd_queries(rng, 16) + [rng.standard_normal(16).astype(f32)])
    for metric in sx.METRICS:
        qi, s, e, g, u, v = m8._query_params(Q, metric, 16, band=True)
        # zero | +NaN -NaN +Inf -Inf | 2e-24 in, 5e-25 out, 5e29 in, 2e30 out | one component 1e15: sumsq 9.9999994e29, in |
        # subnormal products: sumsq 9e-42, out | ordinary
        assert np.isnan(u).tolist() == [False, True, True, True, True, False, True, False, True, False, True, False], metric
        assert (g[0], u[0], v[0]) == (1, 1, 0) and not qi[0].any()
        assert not qi[np.isnan(u)].any() and (v[np.isnan(u)] == 0).all()
        q0 = m8._query_params(Q, metric, 16)
        ok = ~np.isnan(u)
        for a, b in zip((qi, s, e, g, u, v), q0):                 # in-band queries: the plain model's values, untouched
            assert np.array_equal(a[ok], b[ok])
        thr, marked = rc.range_thr(np.full(len(Q), 0.5, dtype=f32), u, v, metric, 16, f32(20.0))
        assert marked[~ok].all() and np.isneginf(thr[~ok]).all()


def test_the_verdicts_agree_with_the_masked_model_where_it_applies():
    """one case with every query served and nothing marked: tests/test_masked_model.py's cascade (which asserts both) reaches
    the same answers and the same fills"""
    c, half, v = sx.case_verdicts("one-a_hi-l2")
    m = v["model"]
    case = (m.S, m.u, m.v, m.max_sumsq, np.where(np.isnan(m.Dm), f32(np.inf), m.Dm), np.full(m.nq, np.inf, dtype=f32))
    for k in sx.MASKED_KS:
        verdict, fills, answers = v["masked", k]
        assert sx.tally(verdict) == (m.nq, 0, 0, 0)
        carried, tfills, _ = tmm._cascade(case, "l2", sx.D, half, k)
        for q in range(m.nq):
            assert np.array_equal(carried[q], answers[q])
        # (that model's fill counts the carried keys too)
        assert all(w <= t <= w + k for w, t in zip(sx.worst(fills), tfills)), (sx.worst(fills), tfills)


def test_the_shards_of_the_sharded_case_serve_every_query():
    X, Q = sx.sharded()
    plan = lc.passes(len(X) // 2)
    assert len(plan) == 3
    for i in range(2):
        verdict, fills, answers = sx.Model(np.ascontiguousarray(X[i::2]), Q, "l2").knn(sx.LARGE_K)
        print("shard %d: worst fill per pass %s" % (i, sx.worst(fills)))
        assert sx.tally(verdict) == (len(Q), 0, 0, 0) and max(sx.worst(fills)) <= sx.POOL_CAP // 2


@pytest.mark.parametrize("space", ["a_hi", "ordinary"])
@pytest.mark.parametrize("metric", sx.METRICS)
def test_extreme_radii_are_sound(metric, space):
    X, Q, radius = sx.extreme_radii(space, metric)
    verdict, fill = sx.Model(X, Q, metric).range(radius)    # asserts that no member is hidden
    print("%s %s: served %d marked %d overflowed %d undecided %d" % ((space, metric) + sx.tally(verdict)))
    for j, r in enumerate(radius):
        print("   query %2d radius %-14.8g %s fill %d" % (j, r, verdict[j], fill[j]))
    assert sx.tally(verdict)[3] * 4 <= len(Q)
