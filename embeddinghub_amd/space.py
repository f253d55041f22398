"""Thin numpy-facing wrapper of one engine space (all arithmetic happens in libehx.so on the GPU).

Mirrors the embeddingstore service surface for one space
(embeddinghub/embeddingstore/embedding_store.proto:9-19): Set / MultiSet / Get / NearestNeighbor /
FreezeSpace, and the Go VectorStoreTable surface (provider/online.go:50-64): Set / Get / Nearest.
"""
import ctypes as C
import itertools

import numpy as np

from . import _lib
from ._lib import EhxError, Params, Stats, check

_counter = itertools.count()


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def _ptr(t):
    """a device pointer for the C call: a torch CUDA tensor, an address (int), or None (NULL)"""
    return C.c_void_p(0 if t is None else (t.data_ptr() if hasattr(t, "data_ptr") else int(t)))


def _results(nq, k, with_total=False):
    """The result arrays of a batched call, filled as "nothing written": ids [nq, max(k, 1)] u64 (2**64 - 1), dist (same
    shape) f32 (inf), count [nq] u32 and, with_total, total [nq] u64 -> (the arrays, their C pointers in the same order)"""
    out = [np.full((nq, max(k, 1)), np.uint64(2**64 - 1), dtype=np.uint64),
           np.full((nq, max(k, 1)), np.inf, dtype=np.float32), np.zeros(nq, dtype=np.uint32)]
    if with_total:
        out.append(np.zeros(nq, dtype=np.uint64))
    return out, [a.ctypes.data_as(C.POINTER(t)) for a, t in zip(out, (C.c_uint64, C.c_float, C.c_uint32, C.c_uint64))]


def _with_arena(call, n_off, cap=1 << 16, grow=4):
    """rc = call(arena, cap, key_off) with a key arena of `cap` bytes, made `grow` times larger for as long as the call
    answers ERANGE -> (rc, the arena's bytes, the n_off offsets as a list)"""
    off = np.zeros(n_off, dtype=np.uint64)
    while True:
        arena = C.create_string_buffer(cap)
        rc = call(arena, cap, off.ctypes.data_as(C.POINTER(C.c_uint64)))
        if rc != _lib.ERANGE:
            return rc, arena.raw, off.tolist()
        cap *= grow


def _key_lists(raw, off, cnt, k):
    """the keys of result lists [n][k] packed in an arena -> list per query of key lists, nearest first"""
    return [[raw[off[i * k + j]:off[i * k + j + 1]].decode() for j in range(c)] for i, c in enumerate(cnt.tolist())]


class Space:
    def __init__(self, name, dims, metric=_lib.METRIC_L2SQ, mode=_lib.MODE_FLAT, M=0, ef_construction=0,
                 ef=0, seed=0, initial_capacity=0, build_batch=0, dtype=_lib.DTYPE_F32, scan=_lib.SCAN_AUTO, shards=0,
                 search_width=0, _handle=None):
        self._L = _lib.load()
        self.name, self.dims, self.metric = name, int(dims), metric
        self._M = M or 16
        if _handle is not None:
            self._h = _handle
            return
        p = Params(mode=mode, M=M, ef_construction=ef_construction, ef=ef, seed=seed,
                   initial_capacity=initial_capacity, build_batch=build_batch, scan=scan, shards=shards,
                   search_width=search_width)
        h = C.c_void_p()
        nm = name.encode()
        check(self._L.ehx_space_create(nm, len(nm), self.dims, metric, dtype, C.byref(p), C.byref(h)))
        self._h = h

    @classmethod
    def unique(cls, prefix, dims, **kw):
        return cls("%s-%d" % (prefix, next(_counter)), dims, **kw)

    @classmethod
    def open(cls, name):
        L = _lib.load()
        h = C.c_void_p()
        nm = name.encode()
        check(L.ehx_space_open(nm, len(nm), C.byref(h)))
        d = C.c_uint32()
        check(L.ehx_space_dims(h, C.byref(d)))
        return cls(name, d.value, _handle=h)

    def drop(self):
        if self._h:
            check(self._L.ehx_space_drop(self._h))
            self._h = None

    def freeze(self):
        check(self._L.ehx_space_freeze(self._h))

    def reserve(self, rows):
        check(self._L.ehx_space_reserve(self._h, rows))

    def __len__(self):
        n = C.c_uint64()
        check(self._L.ehx_space_size(self._h, C.byref(n)))
        return n.value

    # ---- writes ----
    def set(self, key, vec):
        v, pv = _f32(vec)
        if v.size != self.dims:
            raise ValueError("expected %d dims, got %d" % (self.dims, v.size))
        k = key.encode() if isinstance(key, str) else bytes(key)
        check(self._L.ehx_set(self._h, k, len(k), pv))

    def set_batch(self, keys, vecs):
        v, pv = _f32(vecs)
        v = v.reshape(-1, self.dims)
        n, arr, lens, keep = marshal_keys(keys)
        if n != v.shape[0]:
            raise ValueError("keys/vecs length mismatch")
        check(self._L.ehx_set_batch(self._h, n, arr, lens, pv))
        del keep

    def prepare_batch(self, keys, vecs):
        """Marshal a batch once (key arrays, contiguous fp32 rows) so that set_prepared() is ONE C call with no Python
        work in front of it — what a cgo / C++ caller's BatchSet looks like; used by the concurrency measurements,
        where a Python writer thread would otherwise hold the GIL for milliseconds per chunk."""
        v, pv = _f32(vecs)
        v = v.reshape(-1, self.dims)
        n, arr, lens, keep = marshal_keys(keys)
        if n != v.shape[0]:
            raise ValueError("keys/vecs length mismatch")
        return (n, arr, lens, pv, v, keep)

    def set_prepared(self, prep):
        check(self._L.ehx_set_batch(self._h, prep[0], prep[1], prep[2], prep[3]))

    def set_batch_device(self, keys, d_vecs, stream=None):
        """set_batch with the rows read from device memory (ehx_set_batch_device): d_vecs is a contiguous torch CUDA tensor
        [n, dims] of float32 or float16 — what a model on the same GPU produced; nothing is copied to the host.  stream:
        the stream (its address) whose work produced the tensor, None = the default stream.  Returns after the rows are
        published, as set_batch does."""
        n, dtype = _device_rows(d_vecs, self.dims)
        nk, arr, lens, keep = marshal_keys(keys)
        if nk != n:
            raise ValueError("keys/vecs length mismatch")
        check(self._L.ehx_set_batch_device(self._h, C.c_void_p(stream or 0), n, arr, lens, _ptr(d_vecs), dtype))
        del keep

    def graph_import(self, level0, levels, upper, entry_point, max_level):
        """Attach an HNSW graph over the rows already Set (graph mode).

        level0: [n, 1+2M] u32 rows = (count, ids...); levels: [n] i32; upper: {(node, level>=1): ids}.
        """
        l0 = np.ascontiguousarray(level0, dtype=np.uint32)
        lv = np.ascontiguousarray(levels, dtype=np.int32)
        items = sorted(upper.items())
        un = np.array([key[0] for key, _ in items], dtype=np.uint32)
        ul = np.array([key[1] for key, _ in items], dtype=np.int32)
        off = np.zeros(len(items) + 1, dtype=np.uint64)
        if items:
            off[1:] = np.cumsum([len(v) for _, v in items])
            ids = np.concatenate([np.asarray(v, dtype=np.uint32) for _, v in items]).astype(np.uint32)
        else:
            ids = np.zeros(1, dtype=np.uint32)
        P = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
        check(self._L.ehx_graph_import(self._h, l0.shape[0], P(l0, C.c_uint32), P(lv, C.c_int32), len(items),
                                       P(un, C.c_uint32), P(ul, C.c_int32), P(off, C.c_uint64),
                                       P(ids, C.c_uint32), int(entry_point), int(max_level)))

    def graph_export(self):
        """-> level0 [n, 1+2M] u32, levels [n] i32, upper {(node, level): ids}, entry_point, max_level."""
        n = len(self)
        nl, ep, ml = C.c_uint64(), C.c_uint32(), C.c_int32()
        check(self._L.ehx_graph_export(self._h, None, None, None, None, 0, C.byref(nl), C.byref(ep), C.byref(ml)))
        M = self._M
        l0 = np.zeros((n, 1 + 2 * M), dtype=np.uint32)
        lv = np.zeros(n, dtype=np.int32)
        us = np.zeros(n, dtype=np.uint32)
        ul = np.zeros((max(nl.value, 1), M), dtype=np.uint32)
        P = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
        check(self._L.ehx_graph_export(self._h, P(l0, C.c_uint32), P(lv, C.c_int32), P(us, C.c_uint32),
                                       P(ul, C.c_uint32), ul.shape[0], C.byref(nl), C.byref(ep), C.byref(ml)))
        upper = {}
        for i in np.nonzero(lv > 0)[0]:
            for level in range(1, int(lv[i]) + 1):
                row = ul[int(us[i]) + level - 1]
                upper[(int(i), level)] = row[row != 0xFFFFFFFF].copy()
        return l0, lv, upper, ep.value, ml.value

    def set_ef(self, ef):
        check(self._L.ehx_space_set_ef(self._h, ef))

    def set_search_width(self, width):
        """graph spaces: level-0 expansions per search step (1 = the strict, hnswlib-order walk; 2 / 4 = the wide walk)"""
        check(self._L.ehx_space_set_search_width(self._h, width))

    def set_scan(self, scan):
        check(self._L.ehx_space_set_scan(self._h, scan))

    def scan_engine(self):
        """the engine that answers first right now: "f32" | "f16" | "i8" """
        e = C.c_uint32()
        check(self._L.ehx_space_scan_engine(self._h, C.byref(e)))
        return ("f32", "f16", "i8")[e.value]

    def fill_synthetic(self, seed, row0, n_rows, normalize):
        check(self._L.ehx_fill_synthetic(self._h, seed, row0, n_rows, int(bool(normalize))))

    def fill_manifold(self, seed, row0, n_rows, latent_dims, normalize):
        """EHX-MANIFOLD-1 rows (include/ehx_datagen.h) generated on the device: a latent_dims-dimensional linear subspace
        + 5 % noise"""
        check(self._L.ehx_fill_manifold(self._h, seed, row0, n_rows, latent_dims, int(bool(normalize))))

    # ---- reads ----
    def get(self, key):
        k = key.encode() if isinstance(key, str) else bytes(key)
        out = np.empty(self.dims, dtype=np.float32)
        check(self._L.ehx_get(self._h, k, len(k), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def get_by_id(self, i):
        out = np.empty(self.dims, dtype=np.float32)
        check(self._L.ehx_get_by_id(self._h, int(i), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def get_batch(self, keys):
        """get for a batch of stored keys in ONE engine call (one gather on the device, one copy back) -> f32 [n, dims],
        row i what get(keys[i]) returns.  An unknown key raises EhxError (ENOTFOUND) whose `bad_index` is its position."""
        n, arr, lens, keep = marshal_keys(keys)
        out = np.empty((n, self.dims), dtype=np.float32)
        bad = C.c_size_t(0)
        rc = self._L.ehx_get_batch(self._h, n, arr, lens, out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(bad))
        del keep
        _check_bad(rc, bad)
        return out

    def get_by_ids_device(self, d_row_ids, d_out, d_valid, stream=None):
        """The stored rows by row id without leaving the device (torch CUDA tensors): d_row_ids [n] u64 (int64 storage),
        d_out [n, dims] f32, d_valid [n] u32 (int32 storage); an id >= len(self) gives a zero row and valid 0."""
        n = d_row_ids.shape[0] if hasattr(d_row_ids, "shape") else None
        if n is None:
            raise ValueError("pass torch tensors (row ids [n])")
        check(self._L.ehx_get_by_ids_device(self._h, C.c_void_p(stream or 0), n, _ptr(d_row_ids), _ptr(d_out), _ptr(d_valid)))

    def key_of(self, i):
        n = C.c_size_t()
        buf = C.create_string_buffer(4096)
        check(self._L.ehx_key_of(self._h, int(i), buf, 4096, C.byref(n)))
        return buf.raw[:n.value].decode()

    # ---- kNN ----
    def knn(self, queries, k):
        """-> ids [nq,k] u64, dist [nq,k] f32, count [nq] u32 (nearest first)."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.dims)
        nq = q.shape[0]
        (ids, dist, cnt), out = _results(nq, k)
        check(self._L.ehx_knn(self._h, nq, pq, k, *out))
        return ids[:, :k], dist[:, :k], cnt

    def knn_into(self, queries, k, ids, dist, cnt):
        """ehx_knn into the caller's arrays (C-contiguous: queries [nq, dims] f32, ids [nq, k] u64, dist [nq, k] f32,
        cnt [nq] u32) — nothing is allocated or converted on the way; callable from several threads at once."""
        nq = queries.shape[0]
        if (queries.dtype != np.float32 or ids.dtype != np.uint64 or dist.dtype != np.float32 or cnt.dtype != np.uint32
                or not (queries.flags.c_contiguous and ids.flags.c_contiguous and dist.flags.c_contiguous
                        and cnt.flags.c_contiguous)
                or queries.shape[1] != self.dims or ids.shape != (nq, k) or dist.shape != (nq, k) or cnt.shape != (nq,)):
            raise ValueError("knn_into: arrays of the wrong dtype / shape / layout")
        check(self._L.ehx_knn(self._h, nq, queries.ctypes.data_as(C.POINTER(C.c_float)), k,
                              ids.ctypes.data_as(C.POINTER(C.c_uint64)), dist.ctypes.data_as(C.POINTER(C.c_float)),
                              cnt.ctypes.data_as(C.POINTER(C.c_uint32))))

    def knn_keys(self, queries, k):
        """-> list (per query) of key lists, nearest first."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.dims)
        nq = q.shape[0]
        (_, _, cnt), out = _results(nq, k)
        rc, raw, off = _with_arena(lambda *arena: self._L.ehx_knn_keys(self._h, nq, pq, k, *out, *arena), nq * k + 1)
        check(rc)
        return _key_lists(raw, off, cnt, k)

    def knn_by_key(self, key, k):
        kb = key.encode() if isinstance(key, str) else bytes(key)
        ids = np.zeros(max(k, 1), dtype=np.uint64)
        dist = np.zeros(max(k, 1), dtype=np.float32)
        cnt = C.c_uint32()
        check(self._L.ehx_knn_by_key(self._h, kb, len(kb), k, ids.ctypes.data_as(C.POINTER(C.c_uint64)),
                                     dist.ctypes.data_as(C.POINTER(C.c_float)), C.byref(cnt)))
        return ids[:cnt.value], dist[:cnt.value]

    def knn_by_key_keys(self, key, k):
        """the NearestNeighbor RPC by key in ONE engine call -> list of neighbour keys, nearest first"""
        kb = key.encode() if isinstance(key, str) else bytes(key)
        cnt = C.c_uint32()
        rc, raw, o = _with_arena(lambda *arena: self._L.ehx_knn_by_key_keys(self._h, kb, len(kb), k, None, None,
                                                                            C.byref(cnt), *arena),
                                 k + 1, cap=1 << 12, grow=8)
        check(rc)
        return [raw[o[j]:o[j + 1]].decode() for j in range(cnt.value)]

    def knn_by_keys(self, keys, k):
        """knn_by_key for a batch of stored keys in ONE engine call: the rows are gathered into the query batch on the
        device, searched with k + 1, and every key is dropped from its own list there.
        -> ids [n,k] u64, dist [n,k] f32, count [n] u32.  An unknown key raises EhxError (ENOTFOUND) whose
        `bad_index` is the position of the first one."""
        n, arr, lens, keep = marshal_keys(keys)
        (ids, dist, cnt), out = _results(n, k)
        bad = C.c_size_t(0)
        rc = self._L.ehx_knn_by_keys(self._h, n, arr, lens, k, *out, C.byref(bad))
        del keep
        _check_bad(rc, bad)
        return ids[:, :k], dist[:, :k], cnt

    def knn_by_keys_keys(self, keys, k):
        """-> list (per key) of neighbour key lists, nearest first (the NearestNeighbor RPC by key, batched)."""
        n, arr, lens, keep = marshal_keys(keys)
        (_, _, cnt), out = _results(n, k)
        bad = C.c_size_t(0)
        rc, raw, off = _with_arena(lambda *arena: self._L.ehx_knn_by_keys_keys(self._h, n, arr, lens, k, *out, C.byref(bad),
                                                                               *arena), n * k + 1)
        del keep
        _check_bad(rc, bad)
        return _key_lists(raw, off, cnt, k)

    # ---- device-resident (torch tensors on the GPU) ----
    def knn_device(self, d_queries, k, d_ids, d_dist, d_count, stream=None):
        """All arguments are device pointers (ints) or torch CUDA tensors; enqueues on `stream`."""
        nq = d_queries.shape[0] if hasattr(d_queries, "shape") else None
        if nq is None:
            raise ValueError("pass torch tensors (queries [nq, dims])")
        check(self._L.ehx_knn_device(self._h, C.c_void_p(stream or 0), nq, _ptr(d_queries), k, _ptr(d_ids),
                                     _ptr(d_dist), _ptr(d_count)))

    def knn_by_ids_device(self, d_row_ids, k, d_ids, d_dist, d_count, stream=None):
        """The neighbours of stored rows, by row id, without the rows leaving the device: d_row_ids [n] u64, outputs as
        knn_device's (torch CUDA tensors); row i's own id is dropped from its list; an id >= len(self) gives count 0."""
        n = d_row_ids.shape[0] if hasattr(d_row_ids, "shape") else None
        if n is None:
            raise ValueError("pass torch tensors (row ids [n])")
        check(self._L.ehx_knn_by_ids_device(self._h, C.c_void_p(stream or 0), n, _ptr(d_row_ids), k, _ptr(d_ids),
                                            _ptr(d_dist), _ptr(d_count)))

    # ---- kNN among lists of row ids (filtered search) ----
    def knn_among(self, queries, k, cand_ids, cand_off=None):
        """The k nearest rows of every query among a list of row ids, exact (ehx_knn_among).  cand_ids: ONE id sequence
        shared by every query; or, with cand_off [nq + 1], the concatenated per-query lists; or a list of per-query id
        sequences (the offsets are built here).  -> ids [nq,k] u64, dist [nq,k] f32, count [nq] u32."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.dims)
        nq = q.shape[0]
        ids_in, off_in = marshal_id_lists(cand_ids, cand_off)
        if off_in is not None and off_in.shape[0] != nq + 1:
            raise ValueError("expected %d per-query lists, got %d" % (nq, off_in.shape[0] - 1))
        (ids, dist, cnt), out = _results(nq, k)
        u64p = C.POINTER(C.c_uint64)
        check(self._L.ehx_knn_among(self._h, nq, pq, k, ids_in.ctypes.data_as(u64p),
                                    off_in.ctypes.data_as(u64p) if off_in is not None else None, ids_in.shape[0], *out))
        return ids[:, :k], dist[:, :k], cnt

    def knn_among_keys(self, queries, k, keys):
        """knn_among with the shared list given as stored keys, looked up under the same state of the space the search
        sees.  An unknown key raises EhxError (ENOTFOUND) whose `bad_index` is the position of the first one."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.dims)
        nq = q.shape[0]
        n, arr, lens, keep = marshal_keys(keys)
        (ids, dist, cnt), out = _results(nq, k)
        bad = C.c_size_t(0)
        rc = self._L.ehx_knn_among_keys(self._h, nq, pq, k, n, arr, lens, *out, C.byref(bad))
        del keep
        _check_bad(rc, bad)
        return ids[:, :k], dist[:, :k], cnt

    def knn_among_device(self, d_queries, k, d_cand_ids, d_cand_off, d_ids, d_dist, d_count, max_list_hint=0, stream=None):
        """knn_among without anything leaving the device: torch CUDA tensors — d_queries [nq, dims] f32, d_cand_ids
        [n_cand] u64 (int64 storage), d_cand_off [nq + 1] or None (one shared list), outputs as knn_device's.
        max_list_hint: an upper bound of one list's length (0 = unknown); it sizes the launch only."""
        nq = d_queries.shape[0] if hasattr(d_queries, "shape") else None
        n_cand = d_cand_ids.shape[0] if hasattr(d_cand_ids, "shape") else None
        if nq is None or n_cand is None:
            raise ValueError("pass torch tensors (queries [nq, dims], candidate ids [n_cand])")
        check(self._L.ehx_knn_among_device(self._h, C.c_void_p(stream or 0), nq, _ptr(d_queries), k, _ptr(d_cand_ids),
                                           _ptr(d_cand_off), n_cand, int(max_list_hint), _ptr(d_ids), _ptr(d_dist),
                                           _ptr(d_count)))

    # ---- kNN under a row bitmap (filtered search at ordinary selectivity) ----
    def knn_masked(self, queries, k, allow, n_bits=None):
        """The k nearest ALLOWED rows of every query, exact (ehx_knn_masked): the answer of knn_among on the ascending list
        of allowed rows.  allow: a bool array, entry r allows row r; or packed uint32 words (bit r & 31 of word r >> 5) with
        n_bits.  Rows at or above n_bits or len(self) are not allowed.  -> ids [nq,k] u64, dist [nq,k] f32, count [nq] u32."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.dims)
        nq = q.shape[0]
        words, n_bits = marshal_mask(allow, n_bits)
        (ids, dist, cnt), out = _results(nq, k)
        check(self._L.ehx_knn_masked(self._h, nq, pq, k, words.ctypes.data_as(C.POINTER(C.c_uint32)) if n_bits else None,
                                     n_bits, *out))
        return ids[:, :k], dist[:, :k], cnt

    def knn_masked_device(self, d_queries, k, d_mask, n_bits, d_ids, d_dist, d_count, stream=None):
        """knn_masked without anything leaving the device: torch CUDA tensors — d_queries [nq, dims] f32, d_mask
        [ceil(n_bits / 32)] packed u32 words (int32 storage), outputs as knn_device's."""
        nq = d_queries.shape[0] if hasattr(d_queries, "shape") else None
        if nq is None:
            raise ValueError("pass torch tensors (queries [nq, dims], mask words)")
        if hasattr(d_mask, "numel") and d_mask.numel() * 32 < n_bits:
            raise ValueError("%d mask words hold fewer than n_bits = %d bits" % (d_mask.numel(), n_bits))
        check(self._L.ehx_knn_masked_device(self._h, C.c_void_p(stream or 0), nq, _ptr(d_queries), k, _ptr(d_mask), int(n_bits),
                                            _ptr(d_ids), _ptr(d_dist), _ptr(d_count)))

    # ---- kNN under a table of row bitmaps, one per query (a micro-batch of requests with different filters) ----
    def knn_masked_multi(self, queries, k, allows, mask_of, n_bits=None):
        """knn_masked with a bitmap per query (ehx_knn_masked_multi): query i is searched under allows[mask_of[i]], and row i
        of the answer is knn_masked's for that query and bitmap.  allows: a 2-d bool array [n_masks, rows], or packed uint32
        words [n_masks, words] with n_bits; at most 64 bitmaps.  mask_of: [nq] indices into allows.
        -> ids [nq,k] u64, dist [nq,k] f32, count [nq] u32."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.dims)
        nq = q.shape[0]
        words, n_masks, n_bits = marshal_mask_table(allows, n_bits)
        of = np.ascontiguousarray(np.asarray(mask_of).reshape(-1), dtype=np.uint32)
        if of.shape[0] != nq:
            raise ValueError("expected %d mask_of entries, got %d" % (nq, of.shape[0]))
        (ids, dist, cnt), out = _results(nq, k)
        check(self._L.ehx_knn_masked_multi(self._h, nq, pq, k, words.ctypes.data_as(C.POINTER(C.c_uint32)) if n_bits else None,
                                           n_masks, n_bits, of.ctypes.data_as(C.POINTER(C.c_uint32)), *out))
        return ids[:, :k], dist[:, :k], cnt

    def knn_masked_multi_device(self, d_queries, k, d_masks, n_masks, n_bits, d_mask_of, d_ids, d_dist, d_count, stream=None):
        """knn_masked_multi without anything leaving the device: torch CUDA tensors — d_queries [nq, dims] f32, d_masks
        [n_masks, ceil(n_bits / 32)] packed u32 words (int32 storage), d_mask_of [nq] u32 (int32 storage), outputs as
        knn_device's."""
        nq = d_queries.shape[0] if hasattr(d_queries, "shape") else None
        if nq is None:
            raise ValueError("pass torch tensors (queries [nq, dims], mask words, mask_of)")
        if hasattr(d_masks, "numel") and d_masks.numel() < int(n_masks) * ((int(n_bits) + 31) // 32):
            raise ValueError("%d mask words hold fewer than %d bitmaps of n_bits = %d bits" % (d_masks.numel(), n_masks, n_bits))
        if hasattr(d_mask_of, "numel") and d_mask_of.numel() < nq:
            raise ValueError("%d mask_of entries for %d queries" % (d_mask_of.numel(), nq))
        check(self._L.ehx_knn_masked_multi_device(self._h, C.c_void_p(stream or 0), nq, _ptr(d_queries), k, _ptr(d_masks),
                                                  int(n_masks), int(n_bits), _ptr(d_mask_of), _ptr(d_ids), _ptr(d_dist),
                                                  _ptr(d_count)))

    # ---- grouped kNN: at most per_group rows per group label ----
    def knn_grouped(self, queries, k, group_of, per_group=1):
        """The k nearest ELIGIBLE rows of every query, exact (ehx_knn_grouped): rows in (distance, id) order, a row eligible
        iff its label is GROUP_NONE or fewer than per_group rows of its label precede it.  group_of: one integer label per
        row (marshal_groups: -1 is GROUP_NONE); rows at or above len(group_of) or len(self) are not searched.  per_group = 1
        is "collapse".  k <= 256.  -> ids [nq,k] u64, dist [nq,k] f32, count [nq] u32."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.dims)
        nq = q.shape[0]
        labels, n_labels = marshal_groups(group_of)
        (ids, dist, cnt), out = _results(nq, k)
        check(self._L.ehx_knn_grouped(self._h, nq, pq, k, int(per_group),
                                      labels.ctypes.data_as(C.POINTER(C.c_uint32)) if n_labels else None, n_labels, *out))
        return ids[:, :k], dist[:, :k], cnt

    def knn_grouped_device(self, d_queries, k, d_group_of, n_labels, d_ids, d_dist, d_count, per_group=1, stream=None):
        """knn_grouped without anything leaving the device (the serving path: the labels stay resident): torch CUDA tensors —
        d_queries [nq, dims] f32, d_group_of [n_labels] u32 (int32 storage), outputs as knn_device's."""
        nq = d_queries.shape[0] if hasattr(d_queries, "shape") else None
        if nq is None:
            raise ValueError("pass torch tensors (queries [nq, dims], group labels)")
        if hasattr(d_group_of, "numel") and d_group_of.numel() < int(n_labels):
            raise ValueError("%d group labels are fewer than n_labels = %d" % (d_group_of.numel(), n_labels))
        check(self._L.ehx_knn_grouped_device(self._h, C.c_void_p(stream or 0), nq, _ptr(d_queries), k, int(per_group),
                                             _ptr(d_group_of), int(n_labels), _ptr(d_ids), _ptr(d_dist), _ptr(d_count)))

    # ---- grouped kNN under row bitmaps: filter first, then at most per_group rows per group label ----
    def knn_grouped_masked(self, queries, k, group_of, allows, mask_of=None, per_group=1, n_bits=None):
        """knn_grouped over the allowed rows alone (ehx_knn_grouped_masked): query i is answered under allows[mask_of[i]];
        rows that are not allowed neither appear nor count toward a group's cap.  group_of as knn_grouped's.  allows: a 2-d
        bool array [n_masks, rows] or packed uint32 words [n_masks, words] with n_bits, at most 64 bitmaps; or ONE 1-d bitmap
        (a table of one), under which every query is answered when mask_of is None.  Rows at or above len(group_of), n_bits
        or len(self) are not searched.  k <= 256.  -> ids [nq,k] u64, dist [nq,k] f32, count [nq] u32."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.dims)
        nq = q.shape[0]
        labels, n_labels = marshal_groups(group_of)
        a = np.asarray(allows)
        if a.ndim == 1:
            words, n_bits = marshal_mask(a, n_bits)
            words, n_masks = words[None], 1
        else:
            words, n_masks, n_bits = marshal_mask_table(a, n_bits)
        of = None
        if mask_of is not None:
            of = np.ascontiguousarray(np.asarray(mask_of).reshape(-1), dtype=np.uint32)
            if of.shape[0] != nq:
                raise ValueError("expected %d mask_of entries, got %d" % (nq, of.shape[0]))
        elif n_masks != 1:
            raise ValueError("a table of %d bitmaps needs mask_of" % n_masks)
        (ids, dist, cnt), out = _results(nq, k)
        check(self._L.ehx_knn_grouped_masked(self._h, nq, pq, k, int(per_group),
                                             labels.ctypes.data_as(C.POINTER(C.c_uint32)) if n_labels else None, n_labels,
                                             words.ctypes.data_as(C.POINTER(C.c_uint32)) if n_bits else None, n_masks, n_bits,
                                             of.ctypes.data_as(C.POINTER(C.c_uint32)) if of is not None else None, *out))
        return ids[:, :k], dist[:, :k], cnt

    def knn_grouped_masked_device(self, d_queries, k, d_group_of, n_labels, d_masks, n_masks, n_bits, d_mask_of, d_ids, d_dist,
                                  d_count, per_group=1, stream=None):
        """knn_grouped_masked without anything leaving the device (the serving path: labels and bitmaps stay resident): torch
        CUDA tensors — d_queries [nq, dims] f32, d_group_of [n_labels] u32 (int32 storage), d_masks [n_masks,
        ceil(n_bits / 32)] packed u32 words (int32 storage), d_mask_of [nq] u32 (int32 storage) or None with n_masks == 1,
        outputs as knn_device's."""
        nq = d_queries.shape[0] if hasattr(d_queries, "shape") else None
        if nq is None:
            raise ValueError("pass torch tensors (queries [nq, dims], group labels, mask words, mask_of)")
        if hasattr(d_group_of, "numel") and d_group_of.numel() < int(n_labels):
            raise ValueError("%d group labels are fewer than n_labels = %d" % (d_group_of.numel(), n_labels))
        if hasattr(d_masks, "numel") and d_masks.numel() < int(n_masks) * ((int(n_bits) + 31) // 32):
            raise ValueError("%d mask words hold fewer than %d bitmaps of n_bits = %d bits" % (d_masks.numel(), n_masks, n_bits))
        if hasattr(d_mask_of, "numel") and d_mask_of.numel() < nq:
            raise ValueError("%d mask_of entries for %d queries" % (d_mask_of.numel(), nq))
        check(self._L.ehx_knn_grouped_masked_device(self._h, C.c_void_p(stream or 0), nq, _ptr(d_queries), k, int(per_group),
                                                    _ptr(d_group_of), int(n_labels), _ptr(d_masks), int(n_masks), int(n_bits),
                                                    _ptr(d_mask_of), _ptr(d_ids), _ptr(d_dist), _ptr(d_count)))

    # ---- partitioned kNN: a label per row, a wanted label per query (tenants, namespaces, collections) ----
    def knn_labeled(self, queries, k, label_of, want, n_labels=None):
        """The k nearest rows of every query among the rows that carry ITS wanted label, exact (ehx_knn_labeled): query i sees
        row r iff label_of[r] == want[i].  label_of: one unsigned 32-bit label per row, no value special (0xFFFFFFFF is an
        ordinary label); rows at or above n_labels (default len(label_of)) or len(self) are not searched.  want: [nq] labels;
        any number of distinct ones.  Row i of the answer is knn_masked's under the bitmap label_of == want[i].
        -> ids [nq,k] u64, dist [nq,k] f32, count [nq] u32."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.dims)
        nq = q.shape[0]
        labels = np.ascontiguousarray(np.asarray(label_of).reshape(-1), dtype=np.uint32)
        n_labels = labels.shape[0] if n_labels is None else int(n_labels)
        if n_labels < 0 or n_labels > labels.shape[0]:
            raise ValueError("n_labels = %d with %d labels" % (n_labels, labels.shape[0]))
        w = np.ascontiguousarray(np.asarray(want).reshape(-1), dtype=np.uint32)
        if w.shape[0] != nq:
            raise ValueError("expected %d wanted labels, got %d" % (nq, w.shape[0]))
        (ids, dist, cnt), out = _results(nq, k)
        check(self._L.ehx_knn_labeled(self._h, nq, pq, k, labels.ctypes.data_as(C.POINTER(C.c_uint32)) if n_labels else None,
                                      n_labels, w.ctypes.data_as(C.POINTER(C.c_uint32)), *out))
        return ids[:, :k], dist[:, :k], cnt

    def knn_labeled_device(self, d_queries, k, d_label_of, n_labels, d_want, d_ids, d_dist, d_count, stream=None):
        """knn_labeled without anything leaving the device (the serving path: the label column stays resident): torch CUDA
        tensors — d_queries [nq, dims] f32, d_label_of [n_labels] u32 (int32 storage), d_want [nq] u32 (int32 storage),
        outputs as knn_device's."""
        nq = d_queries.shape[0] if hasattr(d_queries, "shape") else None
        if nq is None:
            raise ValueError("pass torch tensors (queries [nq, dims], row labels, wanted labels)")
        if hasattr(d_label_of, "numel") and d_label_of.numel() < int(n_labels):
            raise ValueError("%d row labels are fewer than n_labels = %d" % (d_label_of.numel(), n_labels))
        if hasattr(d_want, "numel") and d_want.numel() < nq:
            raise ValueError("%d wanted labels for %d queries" % (d_want.numel(), nq))
        check(self._L.ehx_knn_labeled_device(self._h, C.c_void_p(stream or 0), nq, _ptr(d_queries), k, _ptr(d_label_of),
                                             int(n_labels), _ptr(d_want), _ptr(d_ids), _ptr(d_dist), _ptr(d_count)))

    # ---- partitioned grouped kNN: a tenant label per row, a wanted tenant per query, a cap per group ----
    def knn_grouped_labeled(self, queries, k, group_of, label_of, want, per_group=1, n_labels=None):
        """knn_grouped over the rows of every query's own tenant alone (ehx_knn_grouped_labeled): query i sees row r iff
        label_of[r] == want[i]; rows of other tenants neither appear nor count toward a group's cap.  group_of as
        knn_grouped's (marshal_groups: -1 is GROUP_NONE), label_of and want as knn_labeled's (no value special); the two
        columns have one length, n_labels (default: that length) may cut both.  Rows at or above n_labels or len(self) are
        not searched.  Any number of distinct wanted labels.  k <= 256.
        -> ids [nq,k] u64, dist [nq,k] f32, count [nq] u32."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.dims)
        nq = q.shape[0]
        groups, n_groups = marshal_groups(group_of)
        labels = np.ascontiguousarray(np.asarray(label_of).reshape(-1), dtype=np.uint32)
        if n_labels is None:
            if n_groups != labels.shape[0]:
                raise ValueError("%d group labels but %d row labels" % (n_groups, labels.shape[0]))
            n_labels = n_groups
        n_labels = int(n_labels)
        if n_labels < 0 or n_labels > labels.shape[0] or n_labels > n_groups:
            raise ValueError("n_labels = %d with %d group labels and %d row labels" % (n_labels, n_groups, labels.shape[0]))
        w = np.ascontiguousarray(np.asarray(want).reshape(-1), dtype=np.uint32)
        if w.shape[0] != nq:
            raise ValueError("expected %d wanted labels, got %d" % (nq, w.shape[0]))
        (ids, dist, cnt), out = _results(nq, k)
        u32p = C.POINTER(C.c_uint32)
        check(self._L.ehx_knn_grouped_labeled(self._h, nq, pq, k, int(per_group),
                                              groups.ctypes.data_as(u32p) if n_labels else None,
                                              labels.ctypes.data_as(u32p) if n_labels else None, n_labels,
                                              w.ctypes.data_as(u32p), *out))
        return ids[:, :k], dist[:, :k], cnt

    def knn_grouped_labeled_device(self, d_queries, k, d_group_of, d_label_of, n_labels, d_want, d_ids, d_dist, d_count,
                                   per_group=1, stream=None):
        """knn_grouped_labeled without anything leaving the device (the serving path: both columns stay resident): torch CUDA
        tensors — d_queries [nq, dims] f32, d_group_of and d_label_of [n_labels] u32 (int32 storage), d_want [nq] u32 (int32
        storage), outputs as knn_device's."""
        nq = d_queries.shape[0] if hasattr(d_queries, "shape") else None
        if nq is None:
            raise ValueError("pass torch tensors (queries [nq, dims], group labels, row labels, wanted labels)")
        if hasattr(d_group_of, "numel") and d_group_of.numel() < int(n_labels):
            raise ValueError("%d group labels are fewer than n_labels = %d" % (d_group_of.numel(), n_labels))
        if hasattr(d_label_of, "numel") and d_label_of.numel() < int(n_labels):
            raise ValueError("%d row labels are fewer than n_labels = %d" % (d_label_of.numel(), n_labels))
        if hasattr(d_want, "numel") and d_want.numel() < nq:
            raise ValueError("%d wanted labels for %d queries" % (d_want.numel(), nq))
        check(self._L.ehx_knn_grouped_labeled_device(self._h, C.c_void_p(stream or 0), nq, _ptr(d_queries), k, int(per_group),
                                                     _ptr(d_group_of), _ptr(d_label_of), int(n_labels), _ptr(d_want),
                                                     _ptr(d_ids), _ptr(d_dist), _ptr(d_count)))

    # ---- stored label columns: labels written with the rows, searched by column number ----
    def set_batch_cols(self, keys, vecs, columns):
        """set_batch plus labels (ehx_set_batch_cols): columns maps a column number (< MAX_COLUMNS) to one u32 value per
        key.  The labels land before the rows are published; a key given twice keeps its last value; an empty mapping is
        set_batch."""
        v, pv = _f32(vecs)
        v = v.reshape(-1, self.dims)
        n, arr, lens, keep = marshal_keys(keys)
        if n != v.shape[0]:
            raise ValueError("keys/vecs length mismatch")
        cols, vals = marshal_columns(columns, n)
        u32p = C.POINTER(C.c_uint32)
        ptrs = (u32p * max(len(vals), 1))(*[a.ctypes.data_as(u32p) for a in vals])
        check(self._L.ehx_set_batch_cols(self._h, n, arr, lens, pv, len(vals), cols.ctypes.data_as(u32p), ptrs))
        del keep

    def column_set(self, col, keys, values):
        """Relabel existing rows by key (ehx_column_set).  An unknown key raises EhxError (ENOTFOUND) whose `bad_index` is its
        position, and nothing is written."""
        n, arr, lens, keep = marshal_keys(keys)
        vals = np.ascontiguousarray(np.asarray(values).reshape(-1), dtype=np.uint32)
        if vals.shape[0] != n:
            raise ValueError("expected %d values, got %d" % (n, vals.shape[0]))
        bad = C.c_size_t(0)
        rc = self._L.ehx_column_set(self._h, int(col), n, arr, lens, vals.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(bad))
        del keep
        _check_bad(rc, bad)

    def column_get(self, col, keys):
        """The column's values of stored keys (ehx_column_get) -> u32 [n]; GROUP_NONE where none was ever given.  An unknown
        key raises EhxError (ENOTFOUND) with `bad_index`."""
        n, arr, lens, keep = marshal_keys(keys)
        out = np.zeros(n, dtype=np.uint32)
        bad = C.c_size_t(0)
        rc = self._L.ehx_column_get(self._h, int(col), n, arr, lens, out.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(bad))
        del keep
        _check_bad(rc, bad)
        return out

    def column_load_device(self, col, row0, d_values, n=None, stream=None):
        """Rows [row0, row0 + n) of a column from a torch CUDA tensor of u32 (int32 storage) (ehx_column_load_device); n
        defaults to the tensor's length.  The range must lie below len(self)."""
        if n is None:
            if not hasattr(d_values, "numel"):
                raise ValueError("pass a torch tensor, or n")
            n = d_values.numel()
        if hasattr(d_values, "numel") and d_values.numel() < int(n):
            raise ValueError("%d values are fewer than n = %d" % (d_values.numel(), n))
        check(self._L.ehx_column_load_device(self._h, C.c_void_p(stream or 0), int(col), int(row0), int(n), _ptr(d_values)))

    def column_read_device(self, col, row0, d_out, n=None, stream=None):
        """Rows [row0, row0 + n) of a column into a torch CUDA tensor of u32 (int32 storage) (ehx_column_read_device)."""
        if n is None:
            if not hasattr(d_out, "numel"):
                raise ValueError("pass a torch tensor, or n")
            n = d_out.numel()
        if hasattr(d_out, "numel") and d_out.numel() < int(n):
            raise ValueError("%d entries are fewer than n = %d" % (d_out.numel(), n))
        check(self._L.ehx_column_read_device(self._h, C.c_void_p(stream or 0), int(col), int(row0), int(n), _ptr(d_out)))

    def knn_by_label(self, queries, k, label_col, want):
        """knn_labeled on the STORED column label_col (ehx_knn_by_label): query i sees the rows whose stored label is
        want[i]; rows never labelled carry 0xFFFFFFFF.  No column travels: the space indexes it once and reuses the index
        until the column or the row count changes.  -> ids [nq,k] u64, dist [nq,k] f32, count [nq] u32."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.dims)
        nq = q.shape[0]
        w = np.ascontiguousarray(np.asarray(want).reshape(-1), dtype=np.uint32)
        if w.shape[0] != nq:
            raise ValueError("expected %d wanted labels, got %d" % (nq, w.shape[0]))
        (ids, dist, cnt), out = _results(nq, k)
        check(self._L.ehx_knn_by_label(self._h, nq, pq, k, int(label_col), w.ctypes.data_as(C.POINTER(C.c_uint32)), *out))
        return ids[:, :k], dist[:, :k], cnt

    def knn_by_label_device(self, d_queries, k, label_col, d_want, d_ids, d_dist, d_count, stream=None):
        """knn_by_label without anything leaving the device: torch CUDA tensors — d_queries [nq, dims] f32, d_want [nq] u32
        (int32 storage), outputs as knn_device's."""
        nq = d_queries.shape[0] if hasattr(d_queries, "shape") else None
        if nq is None:
            raise ValueError("pass torch tensors (queries [nq, dims], wanted labels)")
        if hasattr(d_want, "numel") and d_want.numel() < nq:
            raise ValueError("%d wanted labels for %d queries" % (d_want.numel(), nq))
        check(self._L.ehx_knn_by_label_device(self._h, C.c_void_p(stream or 0), nq, _ptr(d_queries), k, int(label_col),
                                              _ptr(d_want), _ptr(d_ids), _ptr(d_dist), _ptr(d_count)))

    def knn_grouped_by_label(self, queries, k, group_col, label_col, want, per_group=1):
        """knn_grouped_labeled on STORED columns (ehx_knn_grouped_by_label): group_col holds every row's group (GROUP_NONE: a
        group of its own, also every row never given one), label_col its tenant.
        -> ids [nq,k] u64, dist [nq,k] f32, count [nq] u32."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.dims)
        nq = q.shape[0]
        w = np.ascontiguousarray(np.asarray(want).reshape(-1), dtype=np.uint32)
        if w.shape[0] != nq:
            raise ValueError("expected %d wanted labels, got %d" % (nq, w.shape[0]))
        (ids, dist, cnt), out = _results(nq, k)
        check(self._L.ehx_knn_grouped_by_label(self._h, nq, pq, k, int(per_group), int(group_col), int(label_col),
                                               w.ctypes.data_as(C.POINTER(C.c_uint32)), *out))
        return ids[:, :k], dist[:, :k], cnt

    def knn_grouped_by_label_device(self, d_queries, k, group_col, label_col, d_want, d_ids, d_dist, d_count, per_group=1,
                                    stream=None):
        """knn_grouped_by_label without anything leaving the device: tensors as knn_by_label_device's."""
        nq = d_queries.shape[0] if hasattr(d_queries, "shape") else None
        if nq is None:
            raise ValueError("pass torch tensors (queries [nq, dims], wanted labels)")
        if hasattr(d_want, "numel") and d_want.numel() < nq:
            raise ValueError("%d wanted labels for %d queries" % (d_want.numel(), nq))
        check(self._L.ehx_knn_grouped_by_label_device(self._h, C.c_void_p(stream or 0), nq, _ptr(d_queries), k, int(per_group),
                                                      int(group_col), int(label_col), _ptr(d_want), _ptr(d_ids), _ptr(d_dist),
                                                      _ptr(d_count)))

    # ---- predicate filters on stored columns: the bitmap searches' answers, the bitmaps built on the device ----
    def _where_args(self, preds, pred_of, nq):
        table, n_preds = marshal_preds(preds)
        if pred_of is None:
            if n_preds != 1:
                raise ValueError("a table of %d predicates needs pred_of" % n_preds)
            of = np.zeros(nq, dtype=np.uint32)
        else:
            of = np.ascontiguousarray(np.asarray(pred_of).reshape(-1), dtype=np.uint32)
            if of.shape[0] != nq:
                raise ValueError("expected %d pred_of entries, got %d" % (nq, of.shape[0]))
        return table, n_preds, of

    @staticmethod
    def _where_device_args(d_queries, preds, d_pred_of):
        nq = d_queries.shape[0] if hasattr(d_queries, "shape") else None
        if nq is None:
            raise ValueError("pass torch tensors (queries [nq, dims], pred_of)")
        table, n_preds = marshal_preds(preds)
        if hasattr(d_pred_of, "numel") and d_pred_of.numel() < nq:
            raise ValueError("%d pred_of entries for %d queries" % (d_pred_of.numel(), nq))
        return nq, table, n_preds

    def knn_where(self, queries, k, preds, pred_of=None):
        """knn_masked_multi under the bitmaps the predicates describe (ehx_knn_where): query i sees row r iff every term of
        preds[pred_of[i]] holds for r's stored column values.  preds: a list of predicates (marshal_preds), at most 64, each a
        list of (col, lo, hi) or (col, lo, hi, True) for NOT — lo <= value <= hi, unsigned; pred_of: [nq] indices, or None with
        one predicate (every query under it).  -> ids [nq,k] u64, dist [nq,k] f32, count [nq] u32."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.dims)
        nq = q.shape[0]
        table, n_preds, of = self._where_args(preds, pred_of, nq)
        (ids, dist, cnt), out = _results(nq, k)
        check(self._L.ehx_knn_where(self._h, nq, pq, k, table, n_preds, of.ctypes.data_as(C.POINTER(C.c_uint32)), *out))
        return ids[:, :k], dist[:, :k], cnt

    def knn_where_device(self, d_queries, k, preds, d_pred_of, d_ids, d_dist, d_count, stream=None):
        """knn_where with queries, pred_of ([nq] u32, int32 storage) and results on the device (torch CUDA tensors, as
        knn_masked_multi_device's); the predicates stay a host list."""
        nq, table, n_preds = self._where_device_args(d_queries, preds, d_pred_of)
        check(self._L.ehx_knn_where_device(self._h, C.c_void_p(stream or 0), nq, _ptr(d_queries), k, table, n_preds,
                                           _ptr(d_pred_of), _ptr(d_ids), _ptr(d_dist), _ptr(d_count)))

    def knn_grouped_where(self, queries, k, group_col, preds, pred_of=None, per_group=1):
        """knn_grouped_masked under the predicates' bitmaps, the groups read from the stored column group_col
        (ehx_knn_grouped_where).  -> ids [nq,k] u64, dist [nq,k] f32, count [nq] u32."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.dims)
        nq = q.shape[0]
        table, n_preds, of = self._where_args(preds, pred_of, nq)
        (ids, dist, cnt), out = _results(nq, k)
        check(self._L.ehx_knn_grouped_where(self._h, nq, pq, k, int(per_group), int(group_col), table, n_preds,
                                            of.ctypes.data_as(C.POINTER(C.c_uint32)), *out))
        return ids[:, :k], dist[:, :k], cnt

    def knn_grouped_where_device(self, d_queries, k, group_col, preds, d_pred_of, d_ids, d_dist, d_count, per_group=1, stream=None):
        """knn_grouped_where without queries or results leaving the device: tensors as knn_where_device's."""
        nq, table, n_preds = self._where_device_args(d_queries, preds, d_pred_of)
        check(self._L.ehx_knn_grouped_where_device(self._h, C.c_void_p(stream or 0), nq, _ptr(d_queries), k, int(per_group),
                                                   int(group_col), table, n_preds, _ptr(d_pred_of), _ptr(d_ids), _ptr(d_dist),
                                                   _ptr(d_count)))

    def range_where(self, queries, radius, max_results, preds, pred_of=None):
        """range_masked under the predicates' bitmaps (ehx_range_where).
        -> ids [nq, max_results] u64, dist [nq, max_results] f32, count [nq] u32, total [nq] u64."""
        nq, pq, r, (ids, dist, cnt, total), out, keep = self._range_args(queries, radius, max_results)
        table, n_preds, of = self._where_args(preds, pred_of, nq)
        check(self._L.ehx_range_where(self._h, nq, pq, r.ctypes.data_as(C.POINTER(C.c_float)), max_results, table, n_preds,
                                      of.ctypes.data_as(C.POINTER(C.c_uint32)), *out))
        del keep
        return ids[:, :max_results], dist[:, :max_results], cnt, total

    def range_where_device(self, d_queries, d_radius, max_results, preds, d_pred_of, d_ids, d_dist, d_count, d_total=None,
                           stream=None):
        """range_where without queries, radii or results leaving the device: tensors as range_masked_device's."""
        nq, table, n_preds = self._where_device_args(d_queries, preds, d_pred_of)
        if hasattr(d_radius, "shape") and tuple(d_radius.shape) != (nq,):
            raise ValueError("expected %d radii, got shape %s" % (nq, tuple(d_radius.shape)))
        check(self._L.ehx_range_where_device(self._h, C.c_void_p(stream or 0), nq, _ptr(d_queries), _ptr(d_radius), max_results,
                                             table, n_preds, _ptr(d_pred_of), _ptr(d_ids), _ptr(d_dist), _ptr(d_count),
                                             _ptr(d_total)))

    # ---- Boolean filters on stored columns: OR of clauses, IN-lists; the bitmap searches' answers, the graph walk included ----
    @staticmethod
    def _filter_args(filters, filter_of, nq):
        ft = filters if isinstance(filters, FilterTable) else marshal_filters(filters)
        if filter_of is None:
            if ft.n_filters != 1:
                raise ValueError("a table of %d filters needs filter_of" % ft.n_filters)
            of = np.zeros(nq, dtype=np.uint32)
        else:
            of = np.ascontiguousarray(np.asarray(filter_of).reshape(-1), dtype=np.uint32)
            if of.shape[0] != nq:
                raise ValueError("expected %d filter_of entries, got %d" % (nq, of.shape[0]))
        return ft, of

    @staticmethod
    def _filter_device_args(d_queries, filters, d_filter_of):
        nq = d_queries.shape[0] if hasattr(d_queries, "shape") else None
        if nq is None:
            raise ValueError("pass torch tensors (queries [nq, dims], filter_of)")
        ft = filters if isinstance(filters, FilterTable) else marshal_filters(filters)
        if hasattr(d_filter_of, "numel") and d_filter_of.numel() < nq:
            raise ValueError("%d filter_of entries for %d queries" % (d_filter_of.numel(), nq))
        return nq, ft

    def knn_filter(self, queries, k, filters, filter_of=None):
        """knn_masked_multi under the bitmaps the filters describe (ehx_knn_filter): query i sees row r iff SOME clause of
        filters[filter_of[i]] holds for r's stored column values — a row several clauses allow is returned once.  filters: a
        list of filters (marshal_filters) or a FilterTable, at most 64; filter_of: [nq] indices, or None with one filter.
        -> ids [nq,k] u64, dist [nq,k] f32, count [nq] u32."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.dims)
        nq = q.shape[0]
        ft, of = self._filter_args(filters, filter_of, nq)
        (ids, dist, cnt), out = _results(nq, k)
        check(self._L.ehx_knn_filter(self._h, nq, pq, k, C.byref(ft.struct), of.ctypes.data_as(C.POINTER(C.c_uint32)), *out))
        return ids[:, :k], dist[:, :k], cnt

    def knn_filter_device(self, d_queries, k, filters, d_filter_of, d_ids, d_dist, d_count, stream=None):
        """knn_filter with queries, filter_of ([nq] u32, int32 storage) and results on the device (torch CUDA tensors, as
        knn_masked_multi_device's); the filters stay on the host."""
        nq, ft = self._filter_device_args(d_queries, filters, d_filter_of)
        check(self._L.ehx_knn_filter_device(self._h, C.c_void_p(stream or 0), nq, _ptr(d_queries), k, C.byref(ft.struct),
                                            _ptr(d_filter_of), _ptr(d_ids), _ptr(d_dist), _ptr(d_count)))

    def knn_grouped_filter(self, queries, k, group_col, filters, filter_of=None, per_group=1):
        """knn_grouped_masked under the filters' bitmaps, the groups read from the stored column group_col
        (ehx_knn_grouped_filter).  -> ids [nq,k] u64, dist [nq,k] f32, count [nq] u32."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.dims)
        nq = q.shape[0]
        ft, of = self._filter_args(filters, filter_of, nq)
        (ids, dist, cnt), out = _results(nq, k)
        check(self._L.ehx_knn_grouped_filter(self._h, nq, pq, k, int(per_group), int(group_col), C.byref(ft.struct),
                                             of.ctypes.data_as(C.POINTER(C.c_uint32)), *out))
        return ids[:, :k], dist[:, :k], cnt

    def knn_grouped_filter_device(self, d_queries, k, group_col, filters, d_filter_of, d_ids, d_dist, d_count, per_group=1,
                                  stream=None):
        """knn_grouped_filter without queries or results leaving the device: tensors as knn_filter_device's."""
        nq, ft = self._filter_device_args(d_queries, filters, d_filter_of)
        check(self._L.ehx_knn_grouped_filter_device(self._h, C.c_void_p(stream or 0), nq, _ptr(d_queries), k, int(per_group),
                                                    int(group_col), C.byref(ft.struct), _ptr(d_filter_of), _ptr(d_ids),
                                                    _ptr(d_dist), _ptr(d_count)))

    def range_filter(self, queries, radius, max_results, filters, filter_of=None):
        """range_masked under the filters' bitmaps (ehx_range_filter).
        -> ids [nq, max_results] u64, dist [nq, max_results] f32, count [nq] u32, total [nq] u64."""
        nq, pq, r, (ids, dist, cnt, total), out, keep = self._range_args(queries, radius, max_results)
        ft, of = self._filter_args(filters, filter_of, nq)
        check(self._L.ehx_range_filter(self._h, nq, pq, r.ctypes.data_as(C.POINTER(C.c_float)), max_results, C.byref(ft.struct),
                                       of.ctypes.data_as(C.POINTER(C.c_uint32)), *out))
        del keep
        return ids[:, :max_results], dist[:, :max_results], cnt, total

    def range_filter_device(self, d_queries, d_radius, max_results, filters, d_filter_of, d_ids, d_dist, d_count, d_total=None,
                            stream=None):
        """range_filter without queries, radii or results leaving the device: tensors as range_masked_device's."""
        nq, ft = self._filter_device_args(d_queries, filters, d_filter_of)
        if hasattr(d_radius, "shape") and tuple(d_radius.shape) != (nq,):
            raise ValueError("expected %d radii, got shape %s" % (nq, tuple(d_radius.shape)))
        check(self._L.ehx_range_filter_device(self._h, C.c_void_p(stream or 0), nq, _ptr(d_queries), _ptr(d_radius), max_results,
                                              C.byref(ft.struct), _ptr(d_filter_of), _ptr(d_ids), _ptr(d_dist), _ptr(d_count),
                                              _ptr(d_total)))

    def graph_knn_filter(self, queries, k, filters, filter_of=None, route=_lib.WALK_AUTO):
        """graph_knn_masked_multi under the filters' bitmaps (ehx_graph_knn_filter): the graph WALK under Boolean filters,
        the exact answer, or both by filter — route as graph_knn_masked_multi's.
        -> ids [nq,k] u64, dist [nq,k] f32, count [nq] u32."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.dims)
        nq = q.shape[0]
        ft, of = self._filter_args(filters, filter_of, nq)
        (ids, dist, cnt), out = _results(nq, k)
        check(self._L.ehx_graph_knn_filter(self._h, nq, pq, k, C.byref(ft.struct), of.ctypes.data_as(C.POINTER(C.c_uint32)),
                                           int(route), *out))
        return ids[:, :k], dist[:, :k], cnt

    def graph_knn_filter_device(self, d_queries, k, filters, d_filter_of, d_ids, d_dist, d_count, route=_lib.WALK_AUTO,
                                stream=None):
        """graph_knn_filter without queries or results leaving the device: tensors as knn_filter_device's."""
        nq, ft = self._filter_device_args(d_queries, filters, d_filter_of)
        check(self._L.ehx_graph_knn_filter_device(self._h, C.c_void_p(stream or 0), nq, _ptr(d_queries), k, C.byref(ft.struct),
                                                  _ptr(d_filter_of), int(route), _ptr(d_ids), _ptr(d_dist), _ptr(d_count)))

    # ---- kNN under a row bitmap on the graph path ----
    def graph_knn_masked(self, queries, k, allow, n_bits=None, route=_lib.WALK_AUTO):
        """The k nearest ALLOWED rows the graph walk finds (ehx_graph_knn_masked): approximate when walked, possibly fewer
        than k entries; route WALK_EXACT (and WALK_AUTO below an allowed share of 1 / WALK_LIST_FACTOR, and every flat
        space) gives knn_masked's answer.  allow / n_bits as knn_masked.  -> ids [nq,k] u64, dist [nq,k] f32, count [nq] u32."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.dims)
        nq = q.shape[0]
        words, n_bits = marshal_mask(allow, n_bits)
        (ids, dist, cnt), out = _results(nq, k)
        check(self._L.ehx_graph_knn_masked(self._h, nq, pq, k, words.ctypes.data_as(C.POINTER(C.c_uint32)) if n_bits else None,
                                           n_bits, int(route), *out))
        return ids[:, :k], dist[:, :k], cnt

    def graph_knn_masked_device(self, d_queries, k, d_mask, n_bits, d_ids, d_dist, d_count, route=_lib.WALK_AUTO, stream=None):
        """graph_knn_masked without anything leaving the device: tensors as knn_masked_device's."""
        nq = d_queries.shape[0] if hasattr(d_queries, "shape") else None
        if nq is None:
            raise ValueError("pass torch tensors (queries [nq, dims], mask words)")
        if hasattr(d_mask, "numel") and d_mask.numel() * 32 < n_bits:
            raise ValueError("%d mask words hold fewer than n_bits = %d bits" % (d_mask.numel(), n_bits))
        check(self._L.ehx_graph_knn_masked_device(self._h, C.c_void_p(stream or 0), nq, _ptr(d_queries), k, _ptr(d_mask),
                                                  int(n_bits), int(route), _ptr(d_ids), _ptr(d_dist), _ptr(d_count)))

    # ---- ... under a table of row bitmaps, one per query ----
    def graph_knn_masked_multi(self, queries, k, allows, mask_of, n_bits=None, route=_lib.WALK_AUTO):
        """graph_knn_masked with a bitmap per query (ehx_graph_knn_masked_multi): query i is searched under
        allows[mask_of[i]] in one walk launch, and row i of the answer is graph_knn_masked's for that query, bitmap and route.
        WALK_AUTO decides per bitmap, so one batch may hold walked (approximate) and exact rows.  allows / mask_of / n_bits as
        knn_masked_multi.  -> ids [nq,k] u64, dist [nq,k] f32, count [nq] u32."""
        q, pq = _f32(queries)
        q = q.reshape(-1, self.dims)
        nq = q.shape[0]
        words, n_masks, n_bits = marshal_mask_table(allows, n_bits)
        of = np.ascontiguousarray(np.asarray(mask_of).reshape(-1), dtype=np.uint32)
        if of.shape[0] != nq:
            raise ValueError("expected %d mask_of entries, got %d" % (nq, of.shape[0]))
        (ids, dist, cnt), out = _results(nq, k)
        check(self._L.ehx_graph_knn_masked_multi(self._h, nq, pq, k,
                                                 words.ctypes.data_as(C.POINTER(C.c_uint32)) if n_bits else None, n_masks,
                                                 n_bits, of.ctypes.data_as(C.POINTER(C.c_uint32)), int(route), *out))
        return ids[:, :k], dist[:, :k], cnt

    def graph_knn_masked_multi_device(self, d_queries, k, d_masks, n_masks, n_bits, d_mask_of, d_ids, d_dist, d_count,
                                      route=_lib.WALK_AUTO, stream=None):
        """graph_knn_masked_multi without anything leaving the device: tensors as knn_masked_multi_device's."""
        nq = d_queries.shape[0] if hasattr(d_queries, "shape") else None
        if nq is None:
            raise ValueError("pass torch tensors (queries [nq, dims], mask words, mask_of)")
        if hasattr(d_masks, "numel") and d_masks.numel() < int(n_masks) * ((int(n_bits) + 31) // 32):
            raise ValueError("%d mask words hold fewer than %d bitmaps of n_bits = %d bits" % (d_masks.numel(), n_masks, n_bits))
        if hasattr(d_mask_of, "numel") and d_mask_of.numel() < nq:
            raise ValueError("%d mask_of entries for %d queries" % (d_mask_of.numel(), nq))
        check(self._L.ehx_graph_knn_masked_multi_device(self._h, C.c_void_p(stream or 0), nq, _ptr(d_queries), k, _ptr(d_masks),
                                                        int(n_masks), int(n_bits), _ptr(d_mask_of), int(route), _ptr(d_ids),
                                                        _ptr(d_dist), _ptr(d_count)))

    # ---- range search (every row within a radius) ----
    def _range_args(self, queries, radius, max_results):
        q, pq = _f32(queries)
        q = q.reshape(-1, self.dims)
        nq = q.shape[0]
        r = marshal_radius(radius, nq)
        arrays, out = _results(nq, int(max_results), with_total=True)
        return nq, pq, r, arrays, out, (q,)

    def range_search(self, queries, radius, max_results):
        """Every row whose distance to the query is <= radius, exact (ehx_range), nearest first: radius is one number for
        every query or one per query.  -> ids [nq, max_results] u64, dist [nq, max_results] f32, count [nq] u32 (entries
        written per query), total [nq] u64 (rows inside the radius: total > count means the answer was cut)."""
        nq, pq, r, (ids, dist, cnt, total), out, keep = self._range_args(queries, radius, max_results)
        check(self._L.ehx_range(self._h, nq, pq, r.ctypes.data_as(C.POINTER(C.c_float)), max_results, *out))
        del keep
        return ids[:, :max_results], dist[:, :max_results], cnt, total

    def range_search_keys(self, queries, radius, max_results):
        """range_search with the members' keys -> (list per query of key lists, nearest first; dist; count; total)."""
        nq, pq, r, (_, dist, cnt, total), out, keep = self._range_args(queries, radius, max_results)
        k = max_results
        rc, raw, off = _with_arena(lambda *arena: self._L.ehx_range_keys(self._h, nq, pq, r.ctypes.data_as(C.POINTER(C.c_float)),
                                                                        k, *out, *arena), nq * max(k, 1) + 1)
        del keep
        check(rc)
        return _key_lists(raw, off, cnt, k), dist[:, :k], cnt, total

    def range_device(self, d_queries, d_radius, max_results, d_ids, d_dist, d_count, d_total=None, stream=None):
        """range_search without anything leaving the device: torch CUDA tensors — d_queries [nq, dims] f32, d_radius [nq]
        f32, d_ids [nq, max_results] u64 (int64 storage), d_dist [nq, max_results] f32, d_count [nq] u32 (int32 storage),
        d_total [nq] u64 (int64 storage) or None."""
        nq = d_queries.shape[0] if hasattr(d_queries, "shape") else None
        if nq is None:
            raise ValueError("pass torch tensors (queries [nq, dims], radius [nq])")
        if hasattr(d_radius, "shape") and tuple(d_radius.shape) != (nq,):
            raise ValueError("expected %d radii, got shape %s" % (nq, tuple(d_radius.shape)))
        check(self._L.ehx_range_device(self._h, C.c_void_p(stream or 0), nq, _ptr(d_queries), _ptr(d_radius), max_results,
                                       _ptr(d_ids), _ptr(d_dist), _ptr(d_count), _ptr(d_total)))

    # ---- range search under row bitmaps (every ALLOWED row within a radius) ----
    def range_masked(self, queries, radius, max_results, allows, mask_of=None, n_bits=None):
        """range_search over the allowed rows alone (ehx_range_masked): query i is answered under allows[mask_of[i]], and
        total counts allowed rows only.  allows: a 2-d bool array [n_masks, rows] or packed uint32 words [n_masks, words] with
        n_bits, at most 64 bitmaps; or ONE 1-d bitmap (a table of one), under which every query is answered when mask_of is
        None.  -> ids [nq, max_results] u64, dist [nq, max_results] f32, count [nq] u32, total [nq] u64."""
        nq, pq, r, (ids, dist, cnt, total), out, keep = self._range_args(queries, radius, max_results)
        a = np.asarray(allows)
        words, n_masks, n_bits = marshal_mask_table(a[None] if a.ndim == 1 else a, n_bits)
        of = None
        if mask_of is not None:
            of = np.ascontiguousarray(np.asarray(mask_of).reshape(-1), dtype=np.uint32)
            if of.shape[0] != nq:
                raise ValueError("expected %d mask_of entries, got %d" % (nq, of.shape[0]))
        elif n_masks != 1:
            raise ValueError("a table of %d bitmaps needs mask_of" % n_masks)
        check(self._L.ehx_range_masked(self._h, nq, pq, r.ctypes.data_as(C.POINTER(C.c_float)), max_results,
                                       words.ctypes.data_as(C.POINTER(C.c_uint32)) if n_bits else None, n_masks, n_bits,
                                       of.ctypes.data_as(C.POINTER(C.c_uint32)) if of is not None else None, *out))
        del keep
        return ids[:, :max_results], dist[:, :max_results], cnt, total

    def range_masked_device(self, d_queries, d_radius, max_results, d_masks, n_masks, n_bits, d_mask_of, d_ids, d_dist, d_count,
                            d_total=None, stream=None):
        """range_masked without anything leaving the device: torch CUDA tensors — d_queries, d_radius and the outputs as
        range_device's, d_masks [n_masks, ceil(n_bits / 32)] packed u32 words (int32 storage), d_mask_of [nq] u32 (int32
        storage) or None with n_masks == 1."""
        nq = d_queries.shape[0] if hasattr(d_queries, "shape") else None
        if nq is None:
            raise ValueError("pass torch tensors (queries [nq, dims], radius [nq], mask words, mask_of)")
        if hasattr(d_radius, "shape") and tuple(d_radius.shape) != (nq,):
            raise ValueError("expected %d radii, got shape %s" % (nq, tuple(d_radius.shape)))
        if hasattr(d_masks, "numel") and d_masks.numel() < int(n_masks) * ((int(n_bits) + 31) // 32):
            raise ValueError("%d mask words hold fewer than %d bitmaps of n_bits = %d bits" % (d_masks.numel(), n_masks, n_bits))
        if hasattr(d_mask_of, "numel") and d_mask_of.numel() < nq:
            raise ValueError("%d mask_of entries for %d queries" % (d_mask_of.numel(), nq))
        check(self._L.ehx_range_masked_device(self._h, C.c_void_p(stream or 0), nq, _ptr(d_queries), _ptr(d_radius), max_results,
                                              _ptr(d_masks), int(n_masks), int(n_bits), _ptr(d_mask_of), _ptr(d_ids),
                                              _ptr(d_dist), _ptr(d_count), _ptr(d_total)))

    def stats(self):
        st = Stats()
        check(self._L.ehx_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in Stats._fields_}

    def stats_reset(self):
        check(self._L.ehx_stats_reset(self._h))

    def graph_counters(self):
        """(rows fetched, level-0 expansions, upper-level expansions, prefetch hits, ...) since the last reset"""
        out = (C.c_uint64 * 12)()
        check(self._L.ehx_graph_counters(self._h, out, 12))
        return tuple(int(v) for v in out)  # [4:] phase timers of -DEHX_GRAPH_PROFILE builds, else zeros


def _device_rows(t, dims):
    """The checks of set_batch_device, in front of the C call: a contiguous CUDA tensor [n, dims] of float32 or float16
    -> (n, EHX_DTYPE_* of the source)"""
    if isinstance(t, np.ndarray) or not (hasattr(t, "data_ptr") and hasattr(t, "dtype") and hasattr(t, "shape")):
        raise ValueError("pass a torch CUDA tensor [n, dims]; rows in host memory go through set_batch")
    dtype = {"torch.float32": _lib.DTYPE_F32, "torch.float16": _lib.DTYPE_F16}.get(str(t.dtype))
    if dtype is None:
        raise ValueError("rows must be float32 or float16, got %s" % (t.dtype,))
    if len(t.shape) != 2 or int(t.shape[1]) != dims:
        raise ValueError("expected rows of shape [n, %d], got %s" % (dims, tuple(t.shape)))
    if not getattr(t, "is_cuda", True):
        raise ValueError("the rows are not on a GPU; rows in host memory go through set_batch")
    if not t.is_contiguous():
        raise ValueError("the rows must be contiguous (dense, row-major)")
    return int(t.shape[0]), dtype


def _check_bad(rc, bad):
    """check(rc) of a batched by-key call: an ENOTFOUND error carries the index of the first unknown key"""
    try:
        check(rc)
    except EhxError as e:
        e.bad_index = bad.value if e.code == _lib.ENOTFOUND else None
        raise


def marshal_radius(radius, nq):
    """The radii of range_search -> f32 [nq], C-contiguous: a scalar (or a 0-d / one-element array) is broadcast to every
    query; otherwise one radius per query."""
    r = np.asarray(radius, dtype=np.float32)
    if r.ndim == 0 or r.size == 1:
        return np.full(nq, r.reshape(-1)[0], dtype=np.float32)
    r = np.ascontiguousarray(r.reshape(-1), dtype=np.float32)
    if r.shape[0] != nq:
        raise ValueError("expected %d radii, got %d" % (nq, r.shape[0]))
    return r


def marshal_mask(allow, n_bits=None):
    """The row bitmap of knn_masked -> (packed u32 words [ceil(n_bits / 32)], C-contiguous; n_bits).  allow is a 1-d bool
    array (entry r allows row r: packed here, bit r & 31 of word r >> 5, n_bits = its length unless a smaller one is given),
    or 1-d uint32 words already packed, passed through, with n_bits (at most 32 bits per word given)."""
    a = np.asarray(allow)
    if a.ndim != 1:
        raise ValueError("expected a 1-d mask, got shape %s" % (a.shape,))
    if a.dtype == np.bool_:
        n = a.shape[0] if n_bits is None else int(n_bits)
        if n < 0 or n > a.shape[0]:
            raise ValueError("n_bits = %d outside a bool mask of %d entries" % (n, a.shape[0]))
        bits = np.zeros((n + 31) // 32 * 32, dtype=np.uint8)
        bits[:n] = a[:n]
        words = np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view("<u4")
        return np.ascontiguousarray(words, dtype=np.uint32), n
    if a.dtype != np.uint32:
        raise ValueError("a mask is a bool array or packed uint32 words, got dtype %s" % a.dtype)
    if n_bits is None:
        raise ValueError("packed mask words need n_bits")
    n = int(n_bits)
    if n < 0 or n > a.shape[0] * 32:
        raise ValueError("n_bits = %d outside %d mask words" % (n, a.shape[0]))
    return np.ascontiguousarray(a), n


def marshal_columns(columns, n):
    """The labels of set_batch_cols -> (u32 column numbers [n_cols]; the u32 value arrays, [n] each, C-contiguous).  columns:
    a mapping column number -> n integer values (0 .. 0xFFFFFFFF)."""
    cols, vals = [], []
    for c, v in dict(columns).items():
        a = np.asarray(v).reshape(-1)
        if a.dtype.kind not in "ui" and a.size:
            raise ValueError("column values must be integers, got dtype %s" % a.dtype)
        if a.shape[0] != n:
            raise ValueError("column %d: expected %d values, got %d" % (c, n, a.shape[0]))
        if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
            raise ValueError("column values must fit 32 bits")
        cols.append(int(c))
        vals.append(np.ascontiguousarray(a, dtype=np.uint32))
    return np.asarray(cols, dtype=np.uint32).reshape(-1), vals


def marshal_preds(preds):
    """The predicates of the *_where searches -> (a ctypes array of ehx_pred, n_preds).  preds: a list of predicates, each a
    list of terms (col, lo, hi) or (col, lo, hi, negate): the term holds iff lo <= value <= hi as unsigned 32-bit numbers,
    inverted when negate is true; a predicate is the conjunction of its terms, and one without terms allows every row.
    ValueError where the C side would say EHX_EINVAL: no predicate, more than PRED_MAX_TERMS terms, a column at or above
    MAX_COLUMNS, a bound outside 32 bits.  (More than 64 predicates are the C side's EHX_EUNSUPPORTED.)"""
    preds = list(preds)
    if not preds:
        raise ValueError("no predicate")
    table = (_lib.Pred * len(preds))()
    for p, terms in enumerate(preds):
        terms = list(terms)
        if len(terms) > _lib.PRED_MAX_TERMS:
            raise ValueError("predicate %d has %d terms: at most %d" % (p, len(terms), _lib.PRED_MAX_TERMS))
        table[p].n_terms = len(terms)
        for t, term in enumerate(terms):
            if len(term) not in (3, 4):
                raise ValueError("predicate %d, term %d: expected (col, lo, hi) or (col, lo, hi, negate)" % (p, t))
            col, lo, hi = (int(x) for x in term[:3])
            if not 0 <= col < _lib.MAX_COLUMNS:
                raise ValueError("predicate %d, term %d: column %d: a space has %d columns" % (p, t, col, _lib.MAX_COLUMNS))
            if not (0 <= lo <= 0xFFFFFFFF and 0 <= hi <= 0xFFFFFFFF):
                raise ValueError("predicate %d, term %d: bounds must fit 32 bits (unsigned)" % (p, t))
            table[p].terms[t] = _lib.Term(col, lo, hi, _lib.TERM_NOT if len(term) == 4 and term[3] else 0)
    return table, len(preds)


class FilterTable:
    """A marshalled table of Boolean filters (marshal_filter_table): .struct is the ehx_filters the *_filter calls take; the
    arrays it points into live as long as this object."""

    def __init__(self, clauses, values, runs):
        self.clauses, self.values, self.runs = clauses, values, runs
        self.n_clauses, self.n_values, self.n_filters = len(clauses), len(values), len(runs)
        self.struct = _lib.Filters(clauses if len(clauses) else None, len(clauses),
                                   values.ctypes.data_as(C.POINTER(C.c_uint32)) if len(values) else None, len(values),
                                   runs if len(runs) else None, len(runs))


def marshal_filter_table(clauses, runs, pack=True):
    """Clauses and the filters' runs over them -> FilterTable.  clauses: a list of clauses, each a list of terms
    (col, lo, hi[, negate]) — marshal_preds' range term — or (col, "in", values[, negate]): the term holds iff the stored value
    is one of `values` (none: never; under negate: always).  runs: a list of (first_clause, n_clauses), filter f the OR of that
    run; runs may overlap, and n_clauses == 0 is the empty disjunction, which allows no row.  pack: every IN term's set is
    sorted and de-duplicated here, as the library would do with its private copy; False passes the values as given.
    ValueError where the C side would say EHX_EINVAL: no filter, a run past the clauses, more than PRED_MAX_TERMS terms, a
    column at or above MAX_COLUMNS, a bound or value outside 32 bits, a malformed term.  (More than 64 filters,
    FILTER_MAX_CLAUSES clauses or FILTER_MAX_VALUES values are the C side's EHX_EUNSUPPORTED.)"""
    clauses, runs = list(clauses), list(runs)
    if not runs:
        raise ValueError("no filter")
    table = (_lib.Pred * len(clauses))()
    values = []
    for c, terms in enumerate(clauses):
        terms = list(terms)
        if len(terms) > _lib.PRED_MAX_TERMS:
            raise ValueError("clause %d has %d terms: at most %d" % (c, len(terms), _lib.PRED_MAX_TERMS))
        table[c].n_terms = len(terms)
        for t, term in enumerate(terms):
            if len(term) not in (3, 4):
                raise ValueError("clause %d, term %d: expected (col, lo, hi[, negate]) or (col, 'in', values[, negate])" % (c, t))
            col = int(term[0])
            if not 0 <= col < _lib.MAX_COLUMNS:
                raise ValueError("clause %d, term %d: column %d: a space has %d columns" % (c, t, col, _lib.MAX_COLUMNS))
            flags = _lib.TERM_NOT if len(term) == 4 and term[3] else 0
            if isinstance(term[1], str):
                if term[1].lower() != "in":
                    raise ValueError("clause %d, term %d: %r is not 'in'" % (c, t, term[1]))
                vals = [int(v) for v in term[2]]
                if any(not 0 <= v <= 0xFFFFFFFF for v in vals):
                    raise ValueError("clause %d, term %d: values must fit 32 bits (unsigned)" % (c, t))
                if pack:
                    vals = sorted(set(vals))
                table[c].terms[t] = _lib.Term(col, len(values), len(vals), flags | _lib.TERM_IN)
                values.extend(vals)
            else:
                lo, hi = int(term[1]), int(term[2])
                if not (0 <= lo <= 0xFFFFFFFF and 0 <= hi <= 0xFFFFFFFF):
                    raise ValueError("clause %d, term %d: bounds must fit 32 bits (unsigned)" % (c, t))
                table[c].terms[t] = _lib.Term(col, lo, hi, flags)
    if len(values) > 0xFFFFFFFF:
        raise ValueError("too many values")
    fl = (_lib.Filter * len(runs))()
    for f, (first, n) in enumerate(runs):
        first, n = int(first), int(n)
        if first < 0 or n < 0 or first + n > len(clauses):
            raise ValueError("filter %d: clauses [%d, %d + %d) of %d" % (f, first, first, n, len(clauses)))
        fl[f] = _lib.Filter(first, n)
    return FilterTable(table, np.asarray(values, dtype=np.uint32), fl)


def marshal_filters(filters, pack=True):
    """The filters of the *_filter searches -> FilterTable.  filters: a list of filters, each a list of clauses (ORed), each
    clause a list of terms (ANDed) as marshal_filter_table takes them; a filter without clauses allows no row, a clause
    without terms every row.  Every filter gets a run of its own (marshal_filter_table shares clauses between filters).
    ValueError as marshal_filter_table."""
    clauses, runs = [], []
    for f in list(filters):
        f = list(f)
        runs.append((len(clauses), len(f)))
        clauses.extend(f)
    return marshal_filter_table(clauses, runs, pack)


def marshal_groups(group_of):
    """The group labels of knn_grouped -> (u32 labels [n_labels], C-contiguous; n_labels).  group_of is a 1-d integer
    sequence, one label per row; -1 (signed dtypes) and 0xFFFFFFFF both mean GROUP_NONE, a row that is a group of its own.
    Other negative labels, labels above 0xFFFFFFFF and non-integral dtypes are refused."""
    a = np.asarray(group_of)
    if a.size == 0:
        return np.zeros(0, dtype=np.uint32), 0
    if a.ndim != 1:
        raise ValueError("expected 1-d group labels, got shape %s" % (a.shape,))
    if a.dtype.kind not in "ui":
        raise ValueError("group labels must be integers, got dtype %s" % a.dtype)
    if a.dtype != np.uint32:
        if a.dtype.kind == "i":
            if (a < -1).any():
                raise ValueError("group labels must not be negative (-1 alone means GROUP_NONE)")
            a = np.where(a == -1, _lib.GROUP_NONE, a.astype(np.int64) if a.dtype.itemsize < 8 else a)
        if a.max() > _lib.GROUP_NONE:
            raise ValueError("group labels must fit 32 bits")
    return np.ascontiguousarray(a, dtype=np.uint32), int(a.shape[0])


def marshal_mask_table(allows, n_bits=None):
    """The bitmaps of knn_masked_multi -> (packed u32 words [n_masks, ceil(n_bits / 32)], C-contiguous; n_masks; n_bits).
    allows is a 2-d bool array [n_masks, rows] (every row packed as marshal_mask packs it, n_bits = rows unless a smaller
    one is given), or 2-d uint32 words [n_masks, words] already packed, passed through, with n_bits."""
    a = np.asarray(allows)
    if a.ndim != 2:
        raise ValueError("expected a 2-d table of masks, got shape %s" % (a.shape,))
    if a.dtype == np.bool_:
        n = a.shape[1] if n_bits is None else int(n_bits)
        if n < 0 or n > a.shape[1]:
            raise ValueError("n_bits = %d outside bool masks of %d entries" % (n, a.shape[1]))
        n_words = (n + 31) // 32
        bits = np.zeros((a.shape[0], n_words * 32), dtype=np.uint8)
        bits[:, :n] = a[:, :n]
        packed = np.packbits(bits.reshape(a.shape[0], n_words * 4, 8), axis=2, bitorder="little")
        words = np.ascontiguousarray(packed.reshape(a.shape[0], n_words * 4)).view("<u4").reshape(a.shape[0], n_words)
        return np.ascontiguousarray(words, dtype=np.uint32), a.shape[0], n
    if a.dtype != np.uint32:
        raise ValueError("a mask is a bool array or packed uint32 words, got dtype %s" % a.dtype)
    if n_bits is None:
        raise ValueError("packed mask words need n_bits")
    n = int(n_bits)
    if n < 0 or n > a.shape[1] * 32:
        raise ValueError("n_bits = %d outside %d mask words" % (n, a.shape[1]))
    # (the table is dense at ceil(n_bits / 32) words per bitmap: words beyond them are cut)
    return np.ascontiguousarray(a[:, :(n + 31) // 32]), a.shape[0], n


def marshal_id_lists(cand_ids, cand_off=None):
    """The candidate lists of knn_among -> (ids u64 [n_cand], offsets u64 [nq + 1] or None).  cand_ids is a flat id
    sequence (shared by every query when cand_off is None, else cut by cand_off), or a list / tuple of per-query id
    sequences, from which the offsets are built (empty lists allowed).  Ids are coerced to uint64; negative ids and
    non-integral values are refused."""
    def as_u64(a):
        a = np.asarray(a)
        if a.size == 0:
            return np.zeros(0, dtype=np.uint64)
        if a.dtype.kind not in "ui":
            raise ValueError("row ids must be integers, got dtype %s" % a.dtype)
        if a.dtype.kind == "i" and (a < 0).any():
            raise ValueError("row ids must not be negative")
        return np.ascontiguousarray(a.reshape(-1), dtype=np.uint64)
    nested = (cand_off is None and isinstance(cand_ids, (list, tuple))
              and (len(cand_ids) == 0 or any(not np.isscalar(c) for c in cand_ids)))
    if nested:
        parts = [as_u64(c) for c in cand_ids]
        off = np.zeros(len(parts) + 1, dtype=np.uint64)
        if parts:
            np.cumsum([p.shape[0] for p in parts], out=off[1:])
        ids = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)
        return np.ascontiguousarray(ids, dtype=np.uint64), off
    ids = as_u64(cand_ids)
    if cand_off is None:
        return ids, None
    return ids, as_u64(cand_off)


def marshal_keys(keys):
    """keys (str or bytes) -> (n, `const char* const*`, `const size_t*`, keep-alive) for ehx_set_batch: ONE joined
    byte buffer and two numpy arrays (pointers = buffer address + running offsets, lengths) instead of a ctypes object
    per key — 1.1 ms instead of 4.2 ms per 8192 keys, which is as long as the engine itself takes for such a chunk.
    The returned keep-alive tuple owns the memory the pointers refer to: hold it until the call has returned."""
    ks = [k.encode() if isinstance(k, str) else bytes(k) for k in keys]
    n = len(ks)
    lens = np.fromiter(map(len, ks), dtype=np.uint64, count=n)
    blob = b"".join(ks)
    buf = C.create_string_buffer(blob, len(blob) + 1)
    ptrs = np.zeros(n, dtype=np.uint64)
    if n:
        np.cumsum(lens[:-1], out=ptrs[1:])
        ptrs += np.uint64(C.addressof(buf))
    return (n, ptrs.ctypes.data_as(C.POINTER(C.c_char_p)), lens.ctypes.data_as(C.POINTER(C.c_size_t)),
            (buf, ptrs, lens))


def nearest_neighbor_rpc(space, num, key="", embedding=None):
    """NearestNeighbor RPC semantics of embeddinghub/embeddingstore/server.cc:172-210 over a Space.

    Returns (grpc_status_code, keys): 0 OK, 3 INVALID_ARGUMENT, 5 NOT_FOUND.
    """
    has_key = key != ""
    has_vec = embedding is not None and len(embedding) != 0
    if has_key and has_vec:
        return 3, []
    if not has_key and not has_vec:
        return 3, []
    try:
        if has_key:
            return 0, space.knn_by_key_keys(key, num)   # (one engine call: lookup, search k + 1, drop the key, keys back)
        return 0, space.knn_keys(np.asarray(embedding, dtype=np.float32), num)[0]
    except EhxError as e:
        if e.code == _lib.ENOTFOUND:
            return 5, []
        raise
