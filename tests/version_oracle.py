"""The oracle's answer for every version of a space that is REWRITTEN while searches run, and the seeded inputs of the
cases of test_rewrite_under_search.py (no GPU needed; tests/test_version_oracle.py checks both on the CPU).

One writer thread sends batches 1..T; version v is the state after batches 1..v (flat: the rows; graph: the rows and
the HNSW graph hnswlib builds when it is fed the same rows in call order — a fresh label is addPoint, a known label is
updatePoint).  A batch that is not a pure append of fresh keys holds the space's lock exclusively from start to finish,
a host search holds it shared, a device search that returned early is fenced, so:

  a search that started after `lo` batches had returned and finished when `hi` had returned answers exactly — ids,
  distance bytes, counts — as the oracle does on version v, for ONE v with lo <= v <= min(hi + 1, T)

(+1: a batch is visible when it commits, just before the writer's counter moves).  The versions are counted by the
writer, not read from len(space): a marker row per batch would give an exact version number, but it would make every
batch an append as well — the row count, the tile that straddles it and the graph's array sizes would move with every
rewrite, and the in-place path (same count, same tiles, re-made) is the one under test.  The window costs one version
of slack, which the input design pays for: between ANY two versions every query's answer differs in at least two ids
(`min_id_difference`), so an answer that mixes two versions, or is stale by one batch outside the window, is no
version's.

Flat versions are full scans (pyoracle.exhaustive over the whole matrix of each version); DTYPE_F16 spaces are fed
rows rounded through numpy's float16, as the engine rounds them (round-to-nearest-even)."""
import numpy as np

from oracle import pyoracle
from prefix_oracle import PrefixOracle

SEED_CORPUS = 20250211      # embeddinghub_amd.SEED_CORPUS (the GPU test asserts they are equal)
TILE = 256                  # rows per int8 tile (k_misc.hip)
OM = {"cos": pyoracle.METRIC_COSINE, "l2": pyoracle.METRIC_L2}


def f16(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def apply_batch(X, ids, rows):
    """the rows after one batch written in call order (the last write of an id wins; ids from len(X) on append, dense)"""
    top = int(max(ids)) + 1
    if top > len(X):
        X = np.concatenate([X, np.zeros((top - len(X), X.shape[1]), dtype=np.float32)])
    else:
        X = X.copy()
    for i, row in zip(ids, rows):
        X[int(i)] = row
    return X


answers_equal = PrefixOracle._equal     # (got, want) triples (ids, dist, count): ids and distance bytes up to the counts, and the counts


class VersionOracle:
    """answers[v] = the oracle's (ids [nq, k] u64, dist [nq, k] f32, count [nq] u32) on version v, v = 0..T"""

    def __init__(self, answers, k):
        self.answers = [(np.asarray(i).astype(np.uint64), np.asarray(d, dtype=np.float32), np.asarray(c).astype(np.uint32))
                        for i, d, c in answers]
        self.k, self.T = k, len(answers) - 1

    def answer(self, v):
        return self.answers[v]

    def window(self, lo, hi):
        return range(int(lo), min(int(hi) + 1, self.T) + 1)

    def assert_is_some_version(self, ids, dist, cnt, lo, hi):
        """-> the version in [lo, min(hi + 1, T)] whose answer (ids, dist, cnt) is, ids and distance bytes and counts"""
        assert 0 <= lo <= hi <= self.T, "bad window [%d, %d] (T = %d)" % (lo, hi, self.T)
        got = (np.asarray(ids), np.asarray(dist, dtype=np.float32), np.asarray(cnt))
        for v in self.window(lo, hi):
            if answers_equal(got, self.answers[v]):
                return v
        best = None     # how far the closest version is off (over ALL versions: a stale answer names the one it is)
        for v in range(self.T + 1):
            oids, odist, ocnt = self.answers[v]
            bad_i = int(sum(not np.array_equal(got[0][q, :ocnt[q]].astype(np.uint64), oids[q, :ocnt[q]])
                            for q in range(len(ocnt))))
            bad_d = int(sum(got[1][q, :ocnt[q]].tobytes() != odist[q, :ocnt[q]].tobytes() for q in range(len(ocnt))))
            bad_c = int((got[2].astype(np.int64) != ocnt.astype(np.int64)).sum())
            cand = (bad_i + bad_d + bad_c, bad_i, bad_d, bad_c, v)
            best = cand if best is None or cand < best else best
        raise AssertionError("the answer is the oracle's top-%d of no version in [%d, %d]: closest is version %d, where %d of "
                             "%d queries differ in ids, %d in distance bytes, %d in counts"
                             % (self.k, lo, min(hi + 1, self.T), best[4], best[1], len(self.answers[0][2]), best[2], best[3]))

    def min_id_difference(self):
        """over every pair of versions and every query: the fewest ids of one answer that the other does not hold"""
        worst = None
        for v in range(self.T + 1):
            iv, _, cv = self.answers[v]
            for w in range(v + 1, self.T + 1):
                iw, _, cw = self.answers[w]
                in_v = np.arange(iv.shape[1])[None, :] < cv[:, None]
                in_w = np.arange(iw.shape[1])[None, :] < cw[:, None]
                hit = ((iv[:, :, None] == iw[:, None, :]) & in_w[:, None, :]).any(axis=2)
                gone = (in_v & ~hit).sum(axis=1)
                hit2 = ((iw[:, :, None] == iv[:, None, :]) & in_v[:, None, :]).any(axis=2)
                new = (in_w & ~hit2).sum(axis=1)
                m = int(np.maximum(gone, new).min())
                worst = m if worst is None else min(worst, m)
        return worst


def flat_versions(X0, batches, queries, metric):
    """X0: version 0 (as the space holds it: rounded for an F16 space); batches: [(ids, rows as the space holds them)];
    queries: {tag: (Q, k)} -> ({tag: VersionOracle}, the last version's rows)"""
    ans = {t: [] for t in queries}
    X = np.ascontiguousarray(X0, dtype=np.float32)
    for v in range(len(batches) + 1):
        if v:
            X = apply_batch(X, *batches[v - 1])
        for t, (Q, k) in queries.items():
            ans[t].append(pyoracle.exhaustive(X, Q, k, metric))
    return {t: VersionOracle(ans[t], queries[t][1]) for t in queries}, X


def graph_versions(X0, batches, queries, metric, ef, M=16, ef_construction=200, seed=100):
    """the same for a graph space: one pyoracle.Hnsw fed in call order, searched at `ef` after every batch
    -> ({tag: VersionOracle}, the last version's rows, the Hnsw after the last batch)"""
    total = max(len(X0), max(int(max(ids)) + 1 for ids, _ in batches))
    h = pyoracle.Hnsw(X0.shape[1], metric, total, M=M, ef_construction=ef_construction, seed=seed)
    h.add_rows(np.ascontiguousarray(X0, dtype=np.float32))
    h.set_ef(ef)
    ans = {t: [] for t in queries}
    X = np.ascontiguousarray(X0, dtype=np.float32)
    for v in range(len(batches) + 1):
        if v:
            ids, rows = batches[v - 1]
            for i, row in zip(ids, rows):
                h.add(row, int(i))
            X = apply_batch(X, ids, rows)
        for t, (Q, k) in queries.items():
            labels, dists, counts, _, _ = h.search_batch(Q, k, threads=1)
            ans[t].append((labels, dists, counts))
    return {t: VersionOracle(ans[t], queries[t][1]) for t in queries}, X, h


# ---- the inputs of the cases -------------------------------------------------------------------------------------------
# Every rewriting batch, for every centre the queries sit near: the four rows nearest to the centre (at least two inside every
# query's top-k) are overwritten with far-away vectors, and far rows are overwritten with vectors at distances spread
# below and above the current k-th distance, so they land inside the top-k.  A rewritten id is never reused for the
# opposite purpose, so two versions always differ by the rows evicted between them.

def _unit(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def centres(seed, c, d):
    return _unit(np.random.default_rng(seed).standard_normal((c, d)).astype(np.float32))


def queries_near(cen, per, seed, spread=0.05):
    r = np.random.default_rng(seed)
    c, d = cen.shape
    scale = np.linalg.norm(cen, axis=1).mean()
    q = np.repeat(cen, per, axis=0) + np.float32(spread * scale) * r.standard_normal((c * per, d)).astype(np.float32) / np.sqrt(d)
    return q.astype(np.float32)


def _near(r, p, t, metric):
    """a vector at distance ~t from the probe p (cosine: 1 - cos = t exactly, any length; L2: |x - p|^2 = t)"""
    d = p.shape[0]
    u = r.standard_normal(d).astype(np.float64)
    if metric == "cos":
        t = min(float(t), 0.95)
        c = p.astype(np.float64) / np.linalg.norm(p)
        u -= c * (u @ c)
        u /= np.linalg.norm(u)
        x = (c + np.sqrt(1.0 / (1.0 - t) ** 2 - 1.0) * u) * r.uniform(0.8, 1.25)
    else:
        x = p.astype(np.float64) + np.sqrt(float(t)) * u / np.linalg.norm(u)
    return x.astype(np.float32)


def _far(r, d, metric, far_norm):
    x = r.standard_normal(d)
    if far_norm is not None:
        x = x / np.linalg.norm(x) * r.uniform(*far_norm)
    return x.astype(np.float32)


def _scatter(j, n, G, count, avoid):
    """`count` ids to overwrite in batch j, none in `avoid`, scattered over the 256-row tiles of the (per-shard: row g
    of a space of G shards is local row g // G of shard g % G) matrix: eight in ONE tile, its first and its last row
    among them; one in the tile that straddles the row count; the others one per tile"""
    n_loc = n // G
    full = n_loc // TILE
    assert full >= 4 and n_loc % TILE >= 2, "the case needs a straddling tile"
    gid = lambda loc, i: loc * G + i % G      # noqa: E731
    out = []

    def take(loc, i):
        g = gid(loc, i)
        if g in avoid or g in out or g >= n:
            return False
        out.append(g)
        return True

    free = [t for t in range(full) if gid(t * TILE, 0) not in avoid and gid(t * TILE + TILE - 1, 1) not in avoid]
    assert free, "every tile's first or last row was rewritten before: fewer batches, or more rows"
    a = free[(7 * j + 3) % len(free)]
    take(a * TILE, 0)
    take(a * TILE + TILE - 1, 1)
    off = 0
    while len(out) < min(8, count):
        off += 29
        take(a * TILE + 1 + off % (TILE - 2), len(out))
    loc = n_loc - 1 - j % (n_loc % TILE)      # the straddling tile
    while not take(loc, len(out)):
        loc -= 1
        assert loc >= full * TILE
    i = 0
    while len(out) < count:
        i += 1
        t = (a + 1 + 5 * i) % full
        if t == a:
            continue
        take(t * TILE + (37 * i + 11 * j) % TILE, len(out))
    return out[:count]


def make_rewrite_batches(X0, cen, ks, metric, T, seed, probe, top, G=1, round16=False, far_norm=None,
                         appends=None, extra_ids=None, on_batch=None, tiles=True):
    """-> [(ids, rows)] (rows as the caller Sets them: NOT rounded).  `top(X, P, kk)` is the oracle's (ids, dist) of the
    probes P on state X; `probe` the point the queries of each centre sit around.  appends: {batch number: n fresh rows}
    makes those batches pure appends (near rows at spread radii among background rows); extra_ids(j) -> ids every
    rewriting batch j also overwrites with far vectors (the graph's entry point); on_batch(ids, rows as held) is called
    with every batch once it is made."""
    r = np.random.default_rng(seed)
    rnd = f16 if round16 else (lambda a: np.asarray(a, dtype=np.float32))
    X = rnd(X0).copy()
    d = X.shape[1]
    ks = sorted(set(ks))
    kmax = ks[-1]
    spread = [(ks[0], f) for f in (0.4, 0.7, 0.95, 1.2)] + [(kk, f) for kk in ks[1:] for f in (0.9, 1.1)]
    used, batches = set(), []
    for j in range(1, T + 1):
        n = len(X)
        pid, pdist = top(X, probe, kmax + 64)
        writes = []      # (id, row) in call order
        if appends and j in appends:
            m = appends[j]
            rows = [_near(r, probe[ci], f * pdist[ci, kk - 1], metric) for ci in range(len(cen)) for kk, f in spread]
            rows += [_far(r, d, metric, far_norm) for _ in range(m - len(rows))]
            order = r.permutation(m)
            writes = [(n + i, rows[order[i]]) for i in range(m)]
        else:
            busy = set(int(i) for i in pid.ravel())
            if tiles:
                tg = _scatter(j, n, G, len(cen) * len(spread), busy | used)
            else:       # (graph spaces have no tiles: any rows not rewritten before)
                tg = [int(i) for i in r.permutation(n) if int(i) not in busy and int(i) not in used][:len(cen) * len(spread)]
            evicted = []
            for ci in range(len(cen)):
                ev = [int(i) for i in pid[ci] if int(i) not in evicted][:4]
                evicted += ev
                writes += [(e, _far(r, d, metric, far_norm)) for e in ev]
                writes += [(tg[ci * len(spread) + s], _near(r, probe[ci], f * pdist[ci, kk - 1], metric))
                           for s, (kk, f) in enumerate(spread)]
            for e in (extra_ids(j) if extra_ids else []):
                if e not in evicted and e not in tg:
                    writes.append((int(e), _far(r, d, metric, far_norm)))
            writes = [writes[i] for i in r.permutation(len(writes))]
            # one key twice, the last wins — both ways: an evicted row first set right on its centre, and a row that lands
            # in the top-k first set far away
            writes.insert(0, (evicted[0], (probe[0] * np.float32(1.0)).astype(np.float32)))
            writes.insert(1, (tg[1], _far(r, d, metric, far_norm)))
        ids = np.array([w[0] for w in writes], dtype=np.int64)
        rows = np.stack([w[1] for w in writes]).astype(np.float32)
        used |= set(int(i) for i in ids)
        X = apply_batch(X, ids, rnd(rows))
        batches.append((ids, rows))
        if on_batch:
            on_batch(ids, rnd(rows))
    return batches


def _flat_top(om):
    def top(X, P, kk):
        ids, dist, _ = pyoracle.exhaustive(X, P, kk, om)
        return ids, dist
    return top


class CaseInput:
    """what a case writes and asks: X0 (raw base rows, or None: `synthetic` rows of the generator), batches of raw rows,
    queries {tag: (Q, k)}; held() rounds as the space does"""

    def __init__(self, **kw):
        self.G, self.round16, self.graph, self.ef, self.appends = 1, False, False, 0, {}
        self.__dict__.update(kw)

    def held(self, a):
        return f16(a) if self.round16 else np.asarray(a, dtype=np.float32)

    def versions(self):
        """-> {tag: VersionOracle}, the last version's rows, (graph cases) the oracle's Hnsw after the last batch"""
        held = [(ids, self.held(rows)) for ids, rows in self.batches]
        if self.graph:
            return graph_versions(self.held(self.X0), held, self.queries, OM[self.metric], self.ef)
        return flat_versions(self.held(self.X0), held, self.queries, OM[self.metric]) + (None,)


def _query_sets(probe, qsets, seed):
    """qsets: {tag: (queries per centre, k)} or {tag: (queries, k, the one centre they sit near)}"""
    out = {}
    for i, (t, q) in enumerate(qsets.items()):
        p = probe if len(q) == 2 else probe[q[2]:q[2] + 1]
        out[t] = (queries_near(p, q[0], seed * 100 + i), q[1])
    return out


def _flat_case(name, d, n, metric, c, T, seed, qsets, base, G=1, round16=False, qscale=1.0, far_norm=None):
    cen = centres(seed, c, d)
    probe = (cen * np.float32(qscale)).astype(np.float32)
    queries = _query_sets(probe, qsets, seed)
    X0 = base(n, d)
    batches = make_rewrite_batches(X0, cen, [q[1] for q in qsets.values()], metric, T, seed, probe, _flat_top(OM[metric]),
                                   G=G, round16=round16, far_norm=far_norm)
    return CaseInput(name=name, d=d, n=n, metric=metric, cen=cen, queries=queries, X0=X0, batches=batches, G=G,
                     round16=round16)


def _synthetic(n, d):
    return pyoracle.gen_rows(SEED_CORPUS, 0, n, d, normalize=True)


def _l2_base(n, d):
    r = np.random.default_rng(5)        # norms spread +-1 % inside every tile
    return _unit(r.standard_normal((n, d)).astype(np.float32)) * (2.0 * r.uniform(0.99, 1.01, (n, 1))).astype(np.float32)


def _normal_base(n, d):
    return np.random.default_rng(6).standard_normal((n, d)).astype(np.float32)


def _graph_case(name, d, n, metric, c, T, seed, qsets, ef, n_app, round16=False):
    """batches alternate: updates of known keys (the entry point among them), appends of fresh keys, updates, ..."""
    cen = np.random.default_rng(seed).standard_normal((c, d)).astype(np.float32)
    queries = _query_sets(cen, qsets, seed)
    X0 = _normal_base(n, d)
    appends = {j: n_app for j in range(2, T + 1, 2)}
    total = n + n_app * len(appends)
    rnd = f16 if round16 else (lambda a: a)
    # the generator's own index follows the batches it makes: it names the rows the walk finds and the entry point
    h = pyoracle.Hnsw(d, OM[metric], total)
    h.add_rows(np.ascontiguousarray(rnd(X0)))
    h.set_ef(ef)

    def top(X, P, kk):
        labels, dists, counts, _, _ = h.search_batch(P, kk, threads=1)
        assert (counts == kk).all()
        return labels, dists

    def follow(ids, rows):
        for i, row in zip(ids, rows):
            h.add(row, int(i))

    batches = make_rewrite_batches(X0, cen, [q[1] for q in qsets.values()], metric, T, seed, cen, top, round16=round16,
                                   appends=appends, extra_ids=lambda j: [int(h.enterpoint)], on_batch=follow, tiles=False)
    return CaseInput(name=name, d=d, n=n, metric=metric, cen=cen, queries=queries, X0=X0, batches=batches,
                     round16=round16, graph=True, ef=ef, appends=appends, total=total)


CASE_INPUTS = {
    "r_i8": lambda: _flat_case("r_i8", 256, 65536 + 91, "cos", 16, 12, 11, {"h10": (4, 10), "h48": (4, 48), "dev": (16, 10)},
                               _synthetic),
    "r_i8_l2": lambda: _flat_case("r_i8_l2", 128, 32768 + 57, "l2", 16, 12, 21, {"h10": (4, 10), "dev": (8, 10)}, _l2_base,
                                  qscale=2.0, far_norm=(1.7, 2.6)),
    "r_f16rows": lambda: _flat_case("r_f16rows", 512, 32768 + 130, "cos", 16, 12, 31, {"h10": (4, 10), "dev": (8, 10)},
                                    _synthetic, round16=True),
    "r_f16flt": lambda: _flat_case("r_f16flt", 256, 8000 + 45, "cos", 16, 12, 41, {"h10": (4, 10), "dev": (8, 10)}, _synthetic),
    "r_f32": lambda: _flat_case("r_f32", 128, 20000 + 33, "cos", 8, 12, 51, {"h10": (4, 10)}, _synthetic),
    "r_paged": lambda: _flat_case("r_paged", 128, 20000 + 33, "cos", 8, 12, 52, {"k65": (2, 65), "k200": (2, 200), "dev": (8, 100)}, _synthetic),
    "r_one": lambda: _flat_case("r_one", 128, 4000 + 21, "cos", 8, 12, 61, {"q%d" % t: (1, 10, t) for t in range(4)}, _synthetic),
    "r_shards": lambda: _flat_case("r_shards", 96, 9000, "l2", 8, 10, 71, {"h10": (4, 10), "dev": (8, 10)}, _l2_base, G=3,
                                   qscale=2.0, far_norm=(1.7, 2.6)),
    "g_strict": lambda: _graph_case("g_strict", 64, 6500, "l2", 8, 10, 83, {"h10": (4, 10), "one": (1, 10, 0), "dev": (8, 10)},
                                    64, 300),
    "g_cos16": lambda: _graph_case("g_cos16", 100, 3000, "cos", 8, 10, 91, {"h10": (4, 10), "dev": (8, 10)}, 64, 200,
                                   round16=True),
}
