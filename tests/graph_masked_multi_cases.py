"""Helper of the tests of the graph walk under a table of bitmaps, one per query (ehx_graph_knn_masked_multi*; no test
here): the bitmap kinds of tests/test_graph_knn_masked.py as a table, the queries' masks, the model of a batch — one
filtered_search per query under ITS OWN allowed set — and a restatement, once, of what ehx_masked.cpp derives from a table:
the route EHX_WALK_AUTO gives every mask and the word offset of every walked query's bitmap.  Shared by the CPU tests
(tests/test_graph_knn_masked_multi_host.py) and the GPU tests (tests/test_graph_knn_masked_multi.py)."""
import numpy as np

from filtered_walk_model import WALK_LIST_FACTOR, filtered_search, walk_cap

KINDS = ("ones", "half", "tenth", "first_half", "entry_cleared", "one_row", "none")
SPARSE_SEED = 5      # tests/test_graph_knn_masked.py's: at 3000 x 64, share 1 / 50, ef 50 the model's list reaches cap
MAX_MASKS = 64


def bitmap(name, n, entry, seed=1):
    """bool [n]: the bitmap kinds of tests/test_graph_knn_masked.py, drawn as it draws them"""
    rng = np.random.default_rng(seed)
    a = np.zeros(n, dtype=bool)
    if name == "ones":
        a[:] = True
    elif name == "half":
        a = rng.random(n) < 0.5
    elif name == "tenth":
        a = rng.random(n) < 0.1
    elif name == "fiftieth":
        a = rng.random(n) < 0.02
    elif name == "first_half":
        a[:n // 2] = True
    elif name == "entry_cleared":
        a = rng.random(n) < 0.5
        a[entry] = False
    elif name == "one_row":
        a[(entry + n // 3) % n] = True
    else:
        assert name == "none", name
    return a


def table(names, n, entry):
    """bool [len(names), n]; a name is a kind or (kind, seed)"""
    return np.stack([bitmap(*((nm, n, entry) if isinstance(nm, str) else (nm[0], n, entry, nm[1]))) for nm in names])


def counted_table(n, n_bits, counts, seed=3):
    """bool [len(counts), n]: mask m allows exactly counts[m] rows below n_bits, drawn at random, and EVERY row at or above
    n_bits (not allowed, not counted: the call never looks at those bits)"""
    rng = np.random.default_rng(seed)
    t = np.zeros((len(counts), n), dtype=bool)
    for m, c in enumerate(counts):
        t[m, rng.choice(n_bits, c, replace=False)] = True
    t[:, n_bits:] = True
    return t


def pack(tab):
    """bool [n_masks, n] -> packed uint32 words [n_masks, ceil(n / 32)] (bit r & 31 of word r >> 5), written out here so
    that the offsets below are checked against something that is not the binding's own marshalling"""
    n_masks, n = tab.shape
    words = np.zeros((n_masks, (n + 31) // 32), dtype=np.uint32)
    for m in range(n_masks):
        r = np.flatnonzero(tab[m]).astype(np.uint32)
        np.bitwise_or.at(words[m], r >> 5, np.uint32(1) << (r & 31))
    return words


def short_bits(tab, n_bits):
    """the packed table with the call's n_bits below the rows: the spare bits of the last word, and every word behind it,
    SET in every bitmap — nothing at or above n_bits may be looked at.  -> words [n_masks, ceil(n / 32)]"""
    words = pack(tab)
    words[:, n_bits >> 5] |= np.uint32((0xFFFFFFFF << (n_bits & 31)) & 0xFFFFFFFF)
    words[:, (n_bits >> 5) + 1:] = 0xFFFFFFFF
    return words


def interleaved(nq, n_masks):
    """mask_of: neighbouring queries carry different masks"""
    return (np.arange(nq) % n_masks).astype(np.uint32)


def shuffled(nq, n_masks, seed=17):
    """mask_of: drawn at random (runs of one mask, masks out of order, possibly a mask no query uses)"""
    return np.random.default_rng(seed).integers(0, n_masks, nq).astype(np.uint32)


# ---- what the engine derives from a table, restated ----
def covered(n_bits, n_rows):
    """the rows the bitmaps cover: below n_bits and below the call's snapshot of the row count"""
    return min(int(n_bits), int(n_rows))


def allow_of(mask_of, n_bits, n_rows):
    """GraphArgs::allow_of: query i's bitmap begins mask_of[i] * words into the staged table, words = those of the covered
    rows (the table is staged dense at that stride, whatever the caller's)"""
    words = (covered(n_bits, n_rows) + 31) // 32
    return np.asarray(mask_of, dtype=np.int64) * words


def auto_walks(tab, n_bits, n_rows):
    """per mask: EHX_WALK_AUTO walks iff its allowed rows * EHX_WALK_LIST_FACTOR >= the rows covered"""
    c = covered(n_bits, n_rows)
    return np.asarray(tab)[:, :c].sum(axis=1) * WALK_LIST_FACTOR >= c


def split(mask_of, walks):
    """-> (the walked queries, the others), each ascending: the two parts of a batch"""
    w = np.asarray(walks)[np.asarray(mask_of)]
    return np.flatnonzero(w), np.flatnonzero(~w)


# ---- the model of a batch ----
_memo = {}


def model_rows(key, graph, D, tab, mask_of, ef, k, rows=None):
    """One filtered_search per query under its own allowed set.  graph: (level0, upper, entry point, max level); D[i]: the
    oracle's distances of query i to every row; tab: bool [n_masks, n], already cut at the rows covered.  key names
    (graph, D); answers are kept per (key, bitmap, query, ef, k) — a reference computed once and shared.
    -> ([(ids, dists)] per query of `rows` (default: all), the counters summed)"""
    l0, upper, ep, maxlevel = graph
    e = max(ef, k)
    out, tot = [], {"n_dist": 0, "n_hops0": 0, "n_hops_up": 0, "hit_cap": 0}
    for i in (range(D.shape[0]) if rows is None else rows):
        a = tab[mask_of[i]]
        mk = (key, a.tobytes(), int(i), ef, k)
        if mk not in _memo:
            _memo[mk] = filtered_search(l0, upper, ep, maxlevel, D[i], a, ef, walk_cap(e), k)
        ids, dist, c = _memo[mk]
        out.append((ids, dist))
        for f in tot:
            tot[f] += int(c[f])
    return out, tot
