"""The oracle's answer for every published prefix of a space that grew by appends (used by test_append_under_search.py;
no GPU needed).

A search that runs beside streamed Sets must answer exactly as the oracle would on the rows of SOME prefix X[:b_j] that
was published while it ran: ids identical, distance bytes identical.  The prefix answers are merged from per-part top-k
lists — the oracle's top-k of the base and of every appended part, ids shifted to the part's first row, merged in the
oracle's (distance, id) order — instead of re-scanning every prefix: a row's distance bytes do not depend on the other
rows, so the merge is exact."""
import numpy as np

from oracle import pyoracle


def merge_topk(a, b, k):
    """two (ids [nq, ka], dist [nq, ka], count [nq]) answers over DISJOINT rows -> the top-k of their union, in the
    oracle's (distance, id) order"""
    ia, da, ca = a
    ib, db, cb = b
    ids = np.concatenate([ia, ib], axis=1)
    dist = np.concatenate([da, db], axis=1)
    valid = np.concatenate([np.arange(ia.shape[1])[None, :] < ca[:, None],
                            np.arange(ib.shape[1])[None, :] < cb[:, None]], axis=1)
    key_d = np.where(valid, dist, np.float32(np.inf))
    key_i = np.where(valid, ids, np.uint64(np.iinfo(np.uint64).max))
    order = np.lexsort((key_i, key_d), axis=-1)[:, :k]
    out_i = np.take_along_axis(ids, order, axis=1)
    out_d = np.take_along_axis(dist, order, axis=1)
    cnt = np.minimum(ca.astype(np.int64) + cb, k).astype(np.uint32)
    keep = np.arange(k)[None, :] < cnt[:, None]
    return (np.where(keep, out_i, np.uint64(0)).astype(np.uint64), np.where(keep, out_d, np.float32(0)).astype(np.float32),
            cnt)


class PrefixOracle:
    """X: every row in id order; bounds: the published row counts b_0 < b_1 < ... (b_0: the base)."""

    def __init__(self, X, Q, k, metric, bounds):
        X = np.ascontiguousarray(X, dtype=np.float32)
        self.Q = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1, X.shape[1])
        self.k, self.bounds = k, [int(b) for b in bounds]
        assert all(b0 < b1 for b0, b1 in zip(self.bounds, self.bounds[1:])), "bounds must grow"
        assert self.bounds[-1] <= X.shape[0]
        self.answers = []
        acc, r0 = None, 0
        for b in self.bounds:
            ids, dist, cnt = pyoracle.exhaustive(X[r0:b], self.Q, k, metric)
            part = (ids.astype(np.uint64) + np.uint64(r0), dist, cnt.astype(np.uint32))
            acc = part if acc is None else merge_topk(acc, part, k)
            self.answers.append(acc)
            r0 = b

    def answer(self, b):
        return self.answers[self.bounds.index(int(b))]

    @staticmethod
    def _equal(got, want):
        ids, dist, cnt = got
        oids, odist, ocnt = want
        if not np.array_equal(np.asarray(cnt, dtype=np.int64), ocnt.astype(np.int64)):
            return False
        keep = np.arange(ids.shape[1])[None, :] < ocnt[:, None]
        gi = np.where(keep, np.asarray(ids).astype(np.uint64), np.uint64(0))
        gd = np.where(keep, np.asarray(dist, dtype=np.float32), np.float32(0))
        wi = np.where(keep, oids, np.uint64(0))
        wd = np.where(keep, odist, np.float32(0))
        return np.array_equal(gi, wi) and gd.tobytes() == wd.tobytes()

    def assert_is_some_prefix(self, ids, dist, cnt, lo, hi):
        """the answer (ids, dist, cnt) of a search that started after `lo` rows were published and returned before more
        than `hi` were must be the oracle's answer over X[:b_j] for some boundary lo <= b_j <= hi — ids and distance
        bytes"""
        cands = [b for b in self.bounds if lo <= b <= hi]
        assert cands, "no publish boundary within [%d, %d] (bounds %r)" % (lo, hi, self.bounds)
        got = (np.asarray(ids), np.asarray(dist, dtype=np.float32), np.asarray(cnt))
        for b in cands:
            if self._equal(got, self.answer(b)):
                return b
        # report how far the closest prefix is off
        best = None
        for b in cands:
            oids, _, ocnt = self.answer(b)
            bad = int(sum(not np.array_equal(np.asarray(ids)[q, :ocnt[q]].astype(np.uint64), oids[q, :ocnt[q]])
                          for q in range(len(ocnt))))
            best = (bad, b) if best is None or bad < best[0] else best
        raise AssertionError("the answer is the oracle's top-%d of no published prefix in [%d, %d]: closest X[:%d], "
                             "%d of %d queries differ in ids (or distance bytes elsewhere)"
                             % (self.k, lo, hi, best[1], best[0], len(self.Q)))
