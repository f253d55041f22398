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
No case leaves a query undecided.  The test prints every figure before it asserts."""
import numpy as np
import pytest

import extreme_cases as xc
import i8_model as m8
import largek_cases as lc
import range_cases as rc
import side_extreme_cases as sx
import test_masked_model as tmm

f32 = np.float32
CANNOT_SERVE = {("ladder-a_hi-l2", "range"), ("ladder-a_hi-l2", "masked"), ("ladder-a_hi-l2", "largek"),
                ("ladder-a_hi-l2", "bykeys")}


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


def test_the_margin_of_the_exception_exceeds_every_ordinary_distance():
    """the exception to (c) is the margin's, not the data's: 1.001 m of an ordinary query on the a_hi ladder lies far above
    its distance to every ordinary row, whatever those rows are"""
    for metric in ("l2",):
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
