"""The filtered range search (ehx_range_masked*), the kNN under a table of bitmaps (ehx_knn_masked_multi*) and the grouped kNN
(ehx_knn_grouped*) against the oracle at extreme and non-finite values: what tests/test_side_searches_extreme.py does for the
range, one-bitmap, list, large-k and by-key searches, at its shapes and to its bar.

Every expected answer comes from pyoracle.exhaustive alone: run over the rows each mask allows and mapped back
(range_masked_cases.lists_under), cut at the radius (range_masked_cases.want) or at k; or run over every row and capped by the
plain-Python greedy (grouped_model.oracle_all, grouped_model.expected).  Bar everywhere: ids equal, distance BYTES equal,
counts (and the range search's totals) equal, NO_ID / +Inf behind the count, no query uncertified, the device form byte for
byte the host form.  On the spaces that keep the int8 engine the routes' counters must move as the CPU model says
(side_extreme_cases.filtered_routes, checked without a GPU by tests/test_side_extreme_model.py).  Fixed inputs: the table of
six bitmaps side_extreme_cases.mask_table (half, few, block, no_block, empty, ones), the queries' masks interleaved, and the
labels side_extreme_cases.group_labels.

Deliberate damage these cases catch (each tried once on a scratch build; none of it is in the tree; every failure an ordinary
assertion, none a fault; of the 69 tests the file had then, the odd queries' four parts still one test per metric):
  range_list_kernel: `d <= r` -> `d < r`       64 fail — every test that calls the range search: "totals differ", the member at
                                               exactly the rank-th allowed distance is lost on the list route (few, block,
                                               every flagged query, every space off the int8 engine); kind f's radius-0
                                               totals under the block mask become 0
  cap_sorted without `label == kGroupNone ||`  60 fail — NONE rows capped at per_group: "ids differ" in every family with the
                                               grouped search (one row in eleven is NONE), test_label_edges_in_a_full_slab at
                                               both sizes; on the spaces of one kind the counters too (64 handed on, 0 marked)
  grouped_rerank_kernel's seed writing the     9 fail — test_spaces_made_entirely_of_one_kind alone, at (100, 3), where the
  k-th UNCAPPED sample key as the radius       cap leaves the seed 94 rows (side_extreme_cases.group_labels): the model marks
                                               all 64 queries, the damaged build serves or overflows them ("handed 0, marked
                                               64", "overflowed 64").  Under the other families' labels the seed reaches k
                                               capped rows, and the smaller radius still holds k eligible rows: nothing shows
  the int8 range stage's flush testing the     23 fail — the int8 spaces of families a (8 of 9: not a_hi-l2, where every
  batch's first bitmap for every query         scan-route query overflows), b (4), c (3), d (rows_huge), e (4) and f (2):
                                               "totals differ" for the scan-route queries under no_block and ones, judged
                                               by half"""

import numpy as np
import pytest

import extreme_cases as xc
import grouped_model as gm
import masked_multi_cases as mmc
import range_cases as rc
import range_masked_cases as rmc
import side_extreme_cases as sx
import test_knn_grouped as t_grouped
import test_knn_masked_multi as t_table
import test_range_masked as t_rangem
import test_side_searches_extreme as t_side

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")

NO_ID = np.uint64(2**64 - 1)
f32 = np.float32
D, MR = sx.D, sx.MAX_RESULTS
NM = len(sx.MASK_NAMES)
_assert_rows, _assert_range, _space, _hook = t_side._assert_rows, t_side._assert_range, t_side._space, t_side._hook


def _rangem_ctr(s):
    return _hook(s, "ehx_test_range_masked_counters", 5)   # scan route, list route, pool overflows, truncated, calls


def _table_ctr(s):
    return _hook(s, "ehx_test_masked_counters", 5)         # scan route, exact route, overflowed, scan passes, calls


def _grouped_ctr(s):
    return _hook(s, "ehx_test_grouped_counters", 5)        # scan route, exact route, of those overflowed, passes, calls


def _same_bytes(a, b):
    return all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes() for x, y in zip(a, b))


def _cut_at_k(lists, nq, k):
    """[(ids, dist)] per query: the oracle over the rows its mask allows, mapped back, the first k"""
    out = [None] * nq
    for at, ids, dist, cnt in lists.values():
        for j, i in enumerate(at):
            c = min(int(cnt[j]), k)
            out[i] = (ids[j, :c], dist[j, :c])
    return out


# ---- one routine per search, one for every search of a case ------------------------------------------------------------

def _rangem(s, Q, radius, tab, mask_of, lists, verdict, what, device=False):
    """One range_masked call: exact, and the counters as the model's verdicts say (verdict None: no int8 scan, every query
    on the list route).  The counting rules, read from ehx_rangem.cpp (rangem_locked, rangem_list_stage):
      scan route [0]  the scan-route queries the int8 stage answers; a scan-route query it FLAGS (its pool overflowed, or the
                      bound does not serve its radius) is counted on the
      list route [1]  with every query whose mask has at most masked_exact_cut rows;
      overflows  [2]  once per query, by whichever stage saw it first: the int8 stage for a pool that overflowed there
                      (counted[j] keeps the list stage from counting it again), the list stage for a query that came to it
                      uncounted — a MARKED query (or a list-route one) with more than POOL_CAP allowed members;
      truncated  [3]  where the page is written: by the int8 stage for the queries it answers, by the list stage for all others
                      (total > max_results either way);
      calls      [4]."""
    nq = len(Q)
    want = rmc.want(lists, nq, radius, MR)
    c0 = _rangem_ctr(s)
    got = s.range_masked(Q, radius, MR, tab, mask_of)
    dc = _rangem_ctr(s) - c0
    _assert_range(got, want, what)
    totals = np.array([w[2] for w in want])
    assert dc[3] == (totals > MR).sum() and dc[4] == 1, (what, dc)
    if verdict is None:
        assert dc[:3].tolist() == [0, nq, int((totals > sx.POOL_CAP).sum())], (what, dc)
    else:
        v = sx.for_counters(verdict)
        list_over = int(((v == sx.MARKED) & (totals > sx.POOL_CAP)).sum())
        sx.expect_counters(v, dc[0], dc[1], dc[2] - list_over, what)
    if device:
        assert _same_bytes(got, t_rangem._device_form(s, Q, radius, MR, tab, mask_of)), what + ": host and device forms differ"
    return got


def _table(s, Q, k, tab, mask_of, lists, verdict, what, device=False):
    """one knn_masked_multi call; verdict None: the exact route for every query"""
    nq = len(Q)
    c0 = _table_ctr(s)
    got = s.knn_masked_multi(Q, k, tab, mask_of)
    dc = _table_ctr(s) - c0
    _assert_rows(got, _cut_at_k(lists, nq, k), what)
    if verdict is None:
        assert dc.tolist() == [0, nq, 0, 0, 1], (what, dc)
    else:
        sx.expect_counters(sx.for_counters(verdict), dc[0], dc[1], dc[2], what)
        assert dc[3] == len(mmc.passes(tab, mask_of)) and dc[4] == 1, (what, dc)
    if device:
        assert _same_bytes(got, t_table._device_form(s, Q, k, tab, mask_of)), what + ": host and device forms differ"
    return got


def _grouped(s, Q, k, per, labels, full, verdict, what, device=False):
    """one knn_grouped call; verdict None: the exact route for every query"""
    nq = len(Q)
    c0 = _grouped_ctr(s)
    got = s.knn_grouped(Q, k, labels, per_group=per)
    dc = _grouped_ctr(s) - c0
    _assert_rows(got, gm.expected(full, labels, k, per), what)
    assert got[0].shape == (nq, k)
    if verdict is None:
        assert dc.tolist() == [0, nq, 0, 0, 1], (what, dc)
    else:
        sx.expect_counters(verdict, dc[0], dc[1], dc[2], what)
        assert dc[3] == len(gm.scan_ranges(len(labels))) and dc[4] == 1, (what, dc)
    if device:
        assert _same_bytes(got, t_grouped._device_form(s, Q, k, labels, per)), what + ": host and device forms differ"
    return got


def _inputs(X, Q, metric):
    """the fixed inputs of a space the model does not cover: filtered_routes' entries without the verdicts"""
    n, nq = len(X), len(Q)
    tab, mask_of = sx.mask_table(n), mmc.interleaved(nq, NM)
    return {"tab": tab, "mask_of": mask_of, "labels": sx.group_labels(n), "full": gm.oracle_all(X, Q, metric),
            "lists": rmc.lists_under(X, Q, rc.OM[metric], tab, mask_of)}


def _tally(what, route, verdict):
    print("%s %s: served %d marked %d overflowed %d undecided %d" % ((what, route) + sx.tally(verdict)))
    return verdict


def _every_filtered_search(s, X, Q, metric, v, what, i8=True, families=("rangem", "table", "grouped")):
    """range_masked at the 1st, 10th and 100th ALLOWED distance under the table of six, knn_masked_multi at k 10 and 48,
    knn_grouped at (k, per_group) (10, 1) and (100, 3); the rank-10 / k = 10 / (10, 1) calls once more in their device form,
    byte for byte.  v: side_extreme_cases.filtered_routes' result on an int8 space (i8), _inputs' on a space that stays on
    the exact kernels.  families: the searches to run (a case too long for one test runs them in several)."""
    tab, mask_of, labels, lists = v["tab"], v["mask_of"], v["labels"], v["lists"]
    full = v["model"].oracle if i8 else v["full"]
    nq = len(Q)
    out = {}
    for rank in sx.RANKS if "rangem" in families else ():
        r = v["radii", rank] if i8 else rmc.radii_at(lists, nq, rank)
        out["rangem", rank] = _rangem(s, Q, r, tab, mask_of, lists, _tally(what, rank, v["rangem", rank][0]) if i8 else None,
                                      "%s range@%d under the table" % (what, rank), device=rank == 10)
    for k in sx.MASKED_KS if "table" in families else ():
        out["table", k] = _table(s, Q, k, tab, mask_of, lists, _tally(what, k, v["table", k][0]) if i8 else None,
                                 "%s table k=%d" % (what, k), device=k == 10)
    for k, per in sx.GROUPED_KM if "grouped" in families else ():
        verdict = _tally(what, (k, per), v["grouped", k, per][0]) if i8 else None
        out["grouped", k, per] = _grouped(s, Q, k, per, labels, full, verdict, "%s grouped k=%d m=%d" % (what, k, per),
                                          device=(k, per) == (10, 1))
    assert s.stats()["n_uncertified"] == 0, what
    return out


# ---- a. the row-magnitude ladder, and h. the grouped exact route across slabs on the same spaces -----------------------

@pytest.mark.parametrize("metric", sx.METRICS)
@pytest.mark.parametrize("kind", xc.KINDS)
def test_row_magnitude_ladder(kind, metric):
    """ordinary rows plus a block of 256 rows of one kind.  A kind the filters bound keeps the int8 engine and the counters
    follow the model; any other kind sends every range query to the list route (range_list_kernel over fp32 rows), every
    grouped query to the exact route and the whole table to the exact route."""
    name = "ladder-%s-%s" % (kind, metric)
    safe = kind in xc.SAFE
    if safe:
        c, v = sx.filtered_verdicts(name)
        X, Q = c["X"], c["Q"]
    else:
        X, Q = sx.ladder(kind, metric)
        v = _inputs(X, Q, metric)
    s = _space("fx-ladder", X, metric)
    assert s.scan_engine() == ("i8" if safe else "f32"), (kind, s.scan_engine())
    out = _every_filtered_search(s, X, Q, metric, v, name, i8=safe)
    if safe:   # h. 63 queries: below the gate of 64, the exact route over five slabs, the block in slab 0
        for k, per in sx.GROUPED_KM:
            c0 = _grouped_ctr(s)
            got = s.knn_grouped(Q[:63], k, v["labels"], per_group=per)
            assert (_grouped_ctr(s) - c0).tolist() == [0, 63, 0, 0, 1]
            assert _same_bytes(got, [a[:63] for a in out["grouped", k, per]]), (name, "63 queries", k, per)
    if kind == "g":   # queries 20, 21 and 24 copy rows that hold a NaN: no neighbour, no member, under any mask
        nan_q = np.repeat(Q[[20, 21, 24]], NM, axis=0)
        of = np.tile(np.arange(NM, dtype=np.uint32), 3)
        ids, dist, cnt, total = s.range_masked(nan_q, np.full(len(nan_q), np.inf, dtype=f32), MR, v["tab"], of)
        assert (cnt == 0).all() and (total == 0).all() and (ids == NO_ID).all()
        assert (s.knn_masked_multi(nan_q, 10, v["tab"], of)[2] == 0).all()
        nan_rows = np.nonzero(np.isnan(X).any(axis=1))[0]
        assert len(nan_rows) == xc.NBLOCK // 2
        for route, got in out.items():
            assert (got[2][[20, 21, 24]] == 0).all(), (name, route)
            assert not np.isin(got[0], nan_rows.astype(np.uint64)).any(), (name, route, "a NaN row in an answer")
    s.drop()


# ---- b. spaces made entirely of one kind -------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", sx.METRICS)
@pytest.mark.parametrize("kind", ["a_lo", "a_hi", "f"])
def test_spaces_made_entirely_of_one_kind(kind, metric):
    name = "one-%s-%s" % (kind, metric)
    c, v = sx.filtered_verdicts(name)
    X, Q = c["X"], c["Q"]
    s = _space("fx-one", X, metric)
    assert s.scan_engine() == "i8"
    out = _every_filtered_search(s, X, Q, metric, v, name)
    if kind == "f":
        block = np.arange(xc.BLOCK0, xc.BLOCK0 + xc.NBLOCK, dtype=np.uint64)
        if metric == "l2":   # every distance of a query ties: the capped greedy over ascending ids, under the block mask its rows
            for k, per in sx.GROUPED_KM:
                ids, dist, cnt = out["grouped", k, per]
                greedy = np.array(gm.capped_greedy(range(len(X)), v["labels"], k, per), dtype=np.uint64)
                assert len(greedy) == k and (cnt == k).all() and (ids == greedy[None, :]).all(), (name, k, per)
            for k in sx.MASKED_KS:
                ids = out["table", k][0]
                assert (ids[v["mask_of"] == 2] == block[None, :k]).all() and (ids[v["mask_of"] == 5] == np.arange(k)[None, :]).all()
        # radius 0 under the block mask alone: under L2 a zero row is at distance |q|^2 — a zero query (9, and 6 .. 31: stored
        # rows and rows of the kind) has all 256 rows as members (0 <= 0), in id order, any other query none; inner product
        # and cosine: whatever the oracle says of a zero row
        zero = np.zeros(len(Q), dtype=f32)
        of = np.zeros(len(Q), dtype=np.uint32)
        lists = rmc.lists_under(X, Q, rc.OM[metric], v["tab"][2:3], of)
        got = _rangem(s, Q, zero, v["tab"][2:3], of, lists, np.full(len(Q), sx.EXACT, dtype=object), name + " radius 0, block",
                      device=True)
        if metric == "l2":
            zq = ~Q.any(axis=1)
            assert zq[9] and zq.sum() == 26 and (got[3][zq] == xc.NBLOCK).all() and (got[0][zq] == block[None, :]).all(), name
            assert (got[3][~zq] == 0).all(), name
    s.drop()


# ---- c. odd queries inside ordinary batches ----------------------------------------------------------------------------

@pytest.mark.parametrize("part", ["rangem", "table", "grouped", "inf"])
@pytest.mark.parametrize("metric", sx.METRICS)
def test_odd_queries_inside_ordinary_batches(metric, part):
    """257 queries, eleven odd ones among them; one search per test, and the range search under +Inf radii in a fourth: all
    of them in one test took 1.5 s, three times the slowest test of tests/test_side_searches_extreme.py"""
    name = "odd-" + metric
    c, v = sx.filtered_verdicts(name)
    X, Q, keep = c["X"], c["Q"], c["ordinary"]
    tab, mask_of, labels = v["tab"], v["mask_of"], v["labels"]
    s = _space("fx-odd", X, metric)
    assert s.scan_engine() == "i8"
    out = _every_filtered_search(s, X, Q, metric, v, name, families=(part,))
    for route, got in out.items():
        assert (got[2][[1, 2]] == 0).all(), (route, "NaN queries")
        if route[0] == "rangem":
            assert (got[3][[1, 2]] == 0).all(), (route, "NaN queries")
            again = s.range_masked(Q[keep], v["radii", route[1]][keep], MR, tab, mask_of[keep])
        elif route[0] == "table":
            again = s.knn_masked_multi(Q[keep], route[1], tab, mask_of[keep])
        else:
            again = s.knn_grouped(Q[keep], route[1], labels, per_group=route[2])
        assert _same_bytes(again, [g[keep] for g in got]), (name, route, "the ordinary queries depend on the odd ones beside them")
    if part != "inf":
        s.drop()
        return
    # the range search once more, the masks shifted by four — the NaN queries 1 and 2 now under ones and half — and the odd
    # queries under +Inf: on the scan route marked whatever they are.  Scan-route queries with a NaN QUERY, flagged queries,
    # and list-route queries riding along under a NaN RADIUS in one device batch
    of2 = ((np.arange(len(Q)) + 4) % NM).astype(np.uint32)
    scans2 = mmc.scans(tab)[of2]
    assert scans2[[1, 2]].all()
    lists2 = rmc.lists_under(X, Q, rc.OM[metric], tab, of2)
    r = rmc.radii_at(lists2, len(Q), 10)
    r[xc.ODD_AT] = np.inf
    verdict, _ = v["model"].range(r, tab[of2].T)
    odd_scan = np.array(xc.ODD_AT)[scans2[xc.ODD_AT]]
    assert len(odd_scan) >= 5 and (np.asarray(verdict)[odd_scan] == sx.MARKED).all()
    got = _rangem(s, Q, r, tab, of2, lists2, np.where(scans2, verdict, sx.EXACT), name + " range, +Inf for the odd queries",
                  device=True)
    assert (got[3][[1, 2]] == 0).all() and int(got[3][0]) == int(tab[of2[0]].sum())   # (the zero query: every allowed row)
    assert s.stats()["n_uncertified"] == 0
    s.drop()


# ---- d. cross-band: rows and queries of opposite extremes --------------------------------------------------------------

@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("which", ["rows_huge", "queries_huge"])
def test_cross_band_rows_and_queries(which, metric):
    name = "cross-%s-%s" % (which, metric)
    c, v = sx.filtered_verdicts(name)
    s = _space("fx-cross", c["X"], metric)
    assert s.scan_engine() == "i8"
    _every_filtered_search(s, c["X"], c["Q"], metric, v, name)
    s.drop()


# ---- e. extreme radii under masks --------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", sx.METRICS)
@pytest.mark.parametrize("space", ["a_hi", "ordinary"])
def test_extreme_radii_under_masks(space, metric):
    """side_extreme_cases.extreme_radii's rows, queries and radii (+-FLT_MAX, +-0, the smallest subnormal, a distance near
    1e-24 and near 1e30 and one ulp below each — of the UNFILTERED space, so under a mask some fall between allowed distances)
    under the table of six"""
    X, Q, radius = sx.extreme_radii(space, metric)
    tab, mask_of = sx.mask_table(len(X)), mmc.interleaved(len(Q), NM)
    lists = rmc.lists_under(X, Q, rc.OM[metric], tab, mask_of)
    scans = mmc.scans(tab)[mask_of]
    verdict, fill = sx.Model(X, Q, metric).range(radius, tab[mask_of].T)
    verdict = np.where(scans, verdict, sx.EXACT)
    print("radii %s %s: served %d marked %d overflowed %d undecided %d" % ((space, metric) + sx.tally(verdict)))
    s = _space("fx-radii", X, metric)
    assert s.scan_engine() == "i8"
    got = _rangem(s, Q, radius, tab, mask_of, lists, verdict, "radii %s %s" % (space, metric), device=True)
    assert (got[3][1::9] == 0).all()              # -FLT_MAX: below every distance
    assert s.stats()["n_uncertified"] == 0
    s.drop()


@pytest.mark.parametrize("metric", sx.METRICS)
def test_infinite_distances_under_masks(metric):
    """a space off the band: finite rows whose L2 distances overflow to +Inf (kind d), radii +Inf and +FLT_MAX — a row at
    distance +Inf is a member under the first and not under the second, a NaN distance under neither"""
    X, Q = sx.ladder("d", metric)
    v = _inputs(X, Q, metric)
    tab, mask_of, lists = v["tab"], v["mask_of"], v["lists"]
    s = _space("fx-inf", X, metric)
    assert s.scan_engine() == "f32"
    nq = len(Q)
    inf = _rangem(s, Q, np.full(nq, np.inf, dtype=f32), tab, mask_of, lists, None, "kind d %s, +Inf" % metric, device=True)
    big = _rangem(s, Q, np.full(nq, sx.FLT_MAX, dtype=f32), tab, mask_of, lists, None, "kind d %s, +FLT_MAX" % metric)
    listed = np.zeros(nq, dtype=np.int64)        # rows the oracle lists under the query's mask: every non-NaN distance
    at_inf = np.zeros(nq, dtype=np.int64)        # ... of them at +Inf
    for at, ids, dist, cnt in lists.values():
        for j, i in enumerate(at):
            listed[i], at_inf[i] = int(cnt[j]), int(np.isposinf(dist[j, :int(cnt[j])]).sum())
    assert (inf[3].astype(np.int64) == listed).all() and (big[3].astype(np.int64) == listed - at_inf).all()
    if metric == "l2":
        assert at_inf[mask_of == 5].min() >= xc.NBLOCK - 1   # (a near-copy of a block row: that row alone is near)
    assert s.stats()["n_uncertified"] == 0
    s.drop()


# ---- f. binary16 storage -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", sx.METRICS)
def test_binary16_rows_at_their_limits(metric):
    name = "f16-" + metric
    c, v = sx.filtered_verdicts(name)
    s = _space("fx-f16", c["X_set"], metric, dtype=ehx.DTYPE_F16)
    assert s.scan_engine() == "i8"
    _every_filtered_search(s, c["X"], c["Q"], metric, v, name)
    s.drop()


@pytest.mark.parametrize("metric", sx.METRICS)
def test_binary16_edge_rows_off_the_int8_engine(metric):
    """N_EXACT binary16 rows: every extreme_cases.F16_EDGE value (those that round to +-Inf included) in rows 500 + i and rows
    600 + i made of it, and a block just outside the band's high edge, which binary16 stores as +-Inf: the space stays off
    the int8 engine, and range_list_kernel and grouped_rerank_kernel walk whole lists and slabs of binary16 rows"""
    X0, Q = sx.ladder("b_hi", metric)
    X = X0.copy()
    for i, e in enumerate(xc.F16_EDGE):
        X[500 + i, i] = e
        X[600 + i, :] = e
    Q = Q.copy()
    Q[26:31] = X[[500, 600, 603, 604, 608]]
    with np.errstate(over="ignore"):
        Xh = X.astype(np.float16).astype(f32)
    assert np.isinf(Xh[602]).all() and np.isinf(Xh[xc.BLOCK0]).all()
    s = _space("fx-f16-edge", X, metric, dtype=ehx.DTYPE_F16)
    assert s.scan_engine() != "i8"
    assert s.get("k606").tobytes() == Xh[606].tobytes() and s.get("k602").tobytes() == Xh[602].tobytes()
    _every_filtered_search(s, Xh, Q, metric, _inputs(Xh, Q, metric), "f16 edge rows " + metric, i8=False)
    s.drop()


# ---- g. the block-permuted layout --------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", sx.METRICS)
@pytest.mark.parametrize("kind", ["c", "d", "g"])
def test_graph_space_rows_of_one_kind(kind, metric):
    """a graph-mode space stores its fp32 rows once, block-permuted (the graph itself is not built, as in
    tests/test_side_searches_extreme.py): the range search under the table takes the list route throughout, the grouped
    search the exact route in one slab, the table the exact route"""
    X, Q = xc._ladder(kind, D, seed=300 + xc.KINDS.index(kind) * 3 + sx.METRICS.index(metric), n=sx.N_GRAPH)
    s = _space("fx-graph", X, metric, mode=ehx.MODE_GRAPH, M=16, build_batch=0xFFFFFFFF)
    _every_filtered_search(s, X, Q, metric, _inputs(X, Q, metric), "graph %s %s" % (kind, metric), i8=False)
    s.drop()


# ---- i. label edges in a full slab -------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [4096, 4095])
def test_label_edges_in_a_full_slab(n):
    """exactly one slab of 4096 rows (and one row fewer): cap_sorted sorts a full, unpadded image in which NONE and the
    largest real label sit side by side; ties planted across rows of both"""
    d, nq = 16, 5
    rng = np.random.default_rng(4096)
    X = rng.standard_normal((4096, d)).astype(f32)
    Q = rng.standard_normal((nq, d)).astype(f32)
    order = rng.permutation(4096)
    labels = (np.arange(4096) % 50 + 1).astype(np.uint32)
    labels[order[:300]] = sx.BIG_LABEL
    labels[order[300:600]] = 0
    labels[order[600:800]] = gm.NONE
    tied = np.sort(np.concatenate([order[:8], order[600:608]]))     # eight rows of the largest label, eight of NONE: one vector
    X[tied] = Q[0] + f32(0.125)
    X[order[300:304]] = Q[0] + f32(0.125)                            # ... and four of label 0
    X, labels = np.ascontiguousarray(X[:n]), labels[:n]
    planted = sorted(int(r) for r in np.concatenate([tied, order[300:304]]) if r < n)
    if len(planted) < 20:                                            # (n = 4095: row 4095 is not one of them)
        pytest.fail("the seed puts the last row among the planted ones: choose another")
    assert (labels == sx.BIG_LABEL).sum() >= 299 and (labels == gm.NONE).sum() >= 199
    s = _space("fx-labels", X, "l2")
    full = gm.oracle_all(X, Q, "l2")
    for k, per in ((256, 1), (256, 255), (100, 2)):
        got = _grouped(s, Q, k, per, labels, full, None, "labels n=%d k=%d m=%d" % (n, k, per), device=k == 100)
        eligible = int((labels == gm.NONE).sum()) + sum(min(per, int(c)) for c in np.unique(labels[labels != gm.NONE],
                                                                                            return_counts=True)[1])
        assert (got[2] == min(k, eligible)).all() and (eligible < k) == (per == 1)   # (256, 1): 200 NONE rows and 52 labels
        seen, nearest = {}, []                                       # query 0: the planted rows tie, nearest of all
        for r in planted:
            g = int(labels[r])
            if g == gm.NONE or seen.get(g, 0) < per:
                nearest.append(r)
                seen[g] = seen.get(g, 0) + 1
        assert [int(r) for r in got[0][0, :len(nearest)]] == nearest and len(nearest) == min(8 + 2 * per, len(planted))
    s.drop()
