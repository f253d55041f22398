// The write path (ANNIndex::set, index.cc:20-37; Go BatchSet; the generator): three ways to land rows, one finish, one publish,
// one graph join — and the write combiner of concurrent single-row Sets.
#include "ehx_internal.h"

#include <unordered_set>

extern "C" int ehx_set_batch(ehx_space* s, size_t n, const char* const* keys, const size_t* klens, const float* vecs) {
  if (!valid_space(s)) return fail(EHX_EINVAL, "space is NULL");
  if (n == 0) return EHX_OK;
  if (!keys || !klens || !vecs) return fail(EHX_EINVAL, "NULL argument");
  RowSource src;
  src.host = vecs;
  return set_batch_from(s, n, keys, klens, src);
}

namespace ehx_impl {

bool is_dense_run(const uint64_t* ids, size_t n) {
  for (size_t i = 1; i < n; ++i)
    if (ids[i] != ids[0] + i) return false;
  return true;
}

WriteBatch write_batch(const uint64_t* ids, size_t n, uint64_t old_n) {
  WriteBatch b{ids, n};
  for (size_t i = 0; ids && i < n; ++i) {
    b.lo = std::min(b.lo, ids[i]);
    b.hi = std::max(b.hi, ids[i]);
  }
  if (!ids && n) b = {nullptr, n, old_n, old_n + n - 1};   // (the generator's rows)
  b.dense_run = !ids || is_dense_run(ids, n);
  b.touches_committed = b.lo < old_n;
  b.all_appended = b.dense_run && (n == 0 || b.lo == old_n);   // (every id fresh and distinct: `next` is old_n + n)
  return b;
}

// rows -> pinned staging (fp16 spaces: rounded to binary16, round-to-nearest-even, on the way); large slabs are split
// over four threads
static void stage_rows(char* dst, const float* src, size_t elems, bool half) {
  auto work = [=](size_t e0, size_t e1) {
    if (half) {
      _Float16* h = (_Float16*)dst;
      for (size_t e = e0; e < e1; ++e) h[e] = (_Float16)src[e];
    } else {
      memcpy(dst + e0 * sizeof(float), src + e0, (e1 - e0) * sizeof(float));
    }
  };
  constexpr size_t kThreads = 4;
  if (elems * sizeof(float) < (2u << 20)) {
    work(0, elems);
    return;
  }
  const size_t per = ((elems + kThreads - 1) / kThreads + 63) & ~(size_t)63;
  std::thread th[kThreads - 1];
  size_t started = 0, done_to = std::min(elems, per);  // [0, per) is this thread's share
  for (size_t t = 1; t < kThreads && t * per < elems; ++t) {
    try {
      th[t - 1] = std::thread(work, t * per, std::min(elems, (t + 1) * per));
      ++started;
      done_to = std::min(elems, (t + 1) * per);
    } catch (const std::system_error&) {
      break;  // no thread to be had (a process at its thread limit): the caller's thread copies the rest
    }
  }
  work(0, std::min(elems, per));
  for (size_t t = 0; t < started; ++t) th[t].join();
  if (done_to < elems) work(done_to, elems);
}

// wait for a stream of the space: the writers' stream through the blocking event, any other by hipStreamSynchronize
int sync_stream(ehx_space* s, hipStream_t st) {
  if (st == s->wr.wstream && s->wr.wev) {
    HIP_TRY(hipEventRecord(s->wr.wev, st));
    HIP_TRY(hipEventSynchronize(s->wr.wev));
  } else {
    HIP_TRY(hipStreamSynchronize(st));
  }
  return EHX_OK;
}

// (re)build the derived copies of rows [row0, row0+n) after they were written; must follow row_stats:
// graph mode: the search copy; flat fp32 spaces: the fp16 scan copy and the int8 scan copy, with their unsafe-row and margin
// flags
// exclusive: no search can be reading the space (the caller holds s->mu exclusively and the writer's stream has waited
// for the searches in flight) — rows below the published count may then move inside their tiles; otherwise every row
// of [row0, row0 + n) lies beyond the published row count.  n_after: the row count once this write is published.
int refresh_derived_copies(ehx_space* s, uint64_t row0, uint64_t n, hipStream_t st, bool exclusive, uint64_t n_after) {
  if (s->xs() && !s->x_perm && n)
    HIP_TRY(launch_make_search_copy(s->rows.dX.p, s->x_half, s->rows.dInv.p, row0, n, s->ld, s->metric, s->xs(), st));
  if ((!s->has16 && !s->has8) || n == 0) return EHX_OK;  // (kept current whatever engine is selected right now)
  unsigned long long u = 0, u8[2] = {0, 0};
  if (s->has16) {
    HIP_TRY(launch_make_scan16(s->rows.dX.p, s->x_half, row0, n, s->dims, s->ld, s->ld16, s->metric, s->f16.dX16.p, s->f16.dRowp16.p,
                               s->f16.dUnsafe.p, st));
    HIP_TRY(hipMemcpyAsync(&u, s->f16.dUnsafe.p, sizeof(u), hipMemcpyDeviceToHost, st));
  }
  if (s->has8) {
    // Full tiles are stored ordered by quantisation step (k_misc.hip).  Re-ordering moves rows inside a tile, so it
    // happens only where no scan can look: the fresh rows of an append (a tile that straddles the published row count
    // keeps the row order, for good), or anywhere under an exclusive writer — which re-makes whole tiles, because a
    // rewritten row of an ordered tile no longer sits where its id says.
    uint64_t r8 = row0, e8 = row0 + n;
    const bool sort_tiles = env().i8_sort;
    if (exclusive) {
      if (int rcw = wait_searches_in_flight(s, st)) return rcw;   // searches still in flight on other streams
      r8 = row0 & ~(uint64_t)255;
      e8 = std::min<uint64_t>(round_up(row0 + n, 256), std::max<uint64_t>(n_after, row0 + n));
    }
    const uint64_t slo = sort_tiles ? r8 : 0, shi = sort_tiles ? e8 : 0;
    if (int rc8 = s->i8.dTileList.ensure((make_scan8_scratch_bytes(r8, e8 - r8, slo, shi) + 7) / 8)) return rc8;
    HIP_TRY(launch_make_scan8(s->rows.dX.p, s->x_half, r8, e8 - r8, s->dims, s->ld, s->ld8, s->metric, s->i8.dX8.p, s->i8.dRowp8.p,
                              s->i8.dTilep8.p, s->i8.dPerm8.p, s->i8.dTileg8.p, slo, shi, s->i8.dTileList.p, s->i8.dUnsafe8.p, st));
    if (s->i8.dTileList.n > (64u << 20) / 8) {  // (a bulk load's scratch — 9 bytes per row — is not kept)
      HIP_TRY(hipStreamSynchronize(st));
      s->i8.dTileList.release();
    }
    HIP_TRY(hipMemcpyAsync(u8, s->i8.dUnsafe8.p, sizeof(u8), hipMemcpyDeviceToHost, st));
  }
  if (int rcs = sync_stream(s, st)) return rcs;
  // (before the caller's release store of the row count: a search that sees these rows sees these counts)
  s->h_unsafe.store(u, std::memory_order_relaxed);
  s->h_unsafe8.store(u8[0], std::memory_order_relaxed);
  if (s->has8) s->h_margin8.store(u8[1], std::memory_order_relaxed);   // (cumulative: only ever grows — using the margins is sound either way)
  return EHX_OK;
}

// ---- the three landers: each puts rows into dX on stream `st` and does nothing else.  The prepare half of each (and
// prepare_permutation) does every allocation and every fallible step that does not depend on the rows; a caller runs all
// prepare halves before the first row lands. ----

// Host rows go up through pinned staging in slabs (fp16 spaces: rounded to binary16 while they are staged).  Two staging
// halves, ping-pong: slab i is copied into its half (by up to four host threads — one core moves ~8 GB/s, a 25-MB chunk
// of copy.go's 8192 x 768 rows would spend 3 ms there) while slab i-1 is on the wire.
static size_t host_slab_rows(const ehx_space* s, size_t n) { return std::max<size_t>(1, std::min<size_t>(n, (8u << 20) / ((size_t)s->dims * s->esz))); }
static size_t host_half_bytes(const ehx_space* s, size_t n) { return (host_slab_rows(s, n) * s->dims * s->esz + 255) & ~(size_t)255; }

static int land_host(ehx_space* s, hipStream_t st, const WriteBatch& b, const float* rows) {
  const size_t row_bytes = (size_t)s->dims * s->esz, slab_rows = host_slab_rows(s, b.n), half_bytes = host_half_bytes(s, b.n);
  size_t slab = 0;
  for (size_t i0 = 0; i0 < b.n; i0 += slab_rows, ++slab) {
    const size_t m = std::min(slab_rows, b.n - i0);
    const uint64_t* ids = b.ids + i0;
    char* stage = (char*)s->wr.hStage.p + (slab & 1) * half_bytes;
    if (slab >= 2) HIP_TRY(hipEventSynchronize(s->wr.sev[slab & 1]));  // the upload that last used this half
    stage_rows(stage, rows + i0 * s->dims, m * s->dims, s->x_half);
    // a slab that is one run of ids (it can be, inside a batch that is not) -> one 2D copy; otherwise row by row
    if (is_dense_run(ids, m)) {
      HIP_TRY(hipMemcpy2DAsync(s->xrow(ids[0]), (size_t)s->ld * s->esz, stage, row_bytes, row_bytes, m, hipMemcpyHostToDevice, st));
    } else {
      for (size_t i = 0; i < m; ++i)
        HIP_TRY(hipMemcpyAsync(s->xrow(ids[i]), stage + i * row_bytes, row_bytes, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipEventRecord(s->wr.sev[slab & 1], st));
  }
  return EHX_OK;   // (the caller waits for the stream before it returns: both halves are free again then)
}

// Device rows are scattered by one kernel.  A batch that is not a run needs the duplicate rule (last_writers) in a list
// on the device; `dst_rows` lives in the caller's frame until the stream is drained (DrainUnlessOk).
static int prepare_device(ehx_space* s, const WriteBatch& b, const RowSource& src, std::vector<uint64_t>* dst_rows) {
  if (b.n > 0xFFFFFFFFull) return fail(EHX_EINVAL, "too many rows in one call: %zu", b.n);
  if (!b.dense_run) {
    dst_rows->resize(b.n);
    last_writers(b.ids, b.n, dst_rows->data());
    if (int rc = s->wr.dDstRows.ensure(b.n)) return rc;
  }
  return src.idx ? s->wr.dSrcIdx.ensure(b.n) : EHX_OK;
}

static int land_device(ehx_space* s, hipStream_t st, const WriteBatch& b, const RowSource& src, const std::vector<uint64_t>& dst_rows) {
  // the rows are complete when `ready` is: the writers' stream waits for the event, the producer's is not drained
  HIP_TRY(hipStreamWaitEvent(st, src.ready, 0));
  // (pageable host memory: the runtime stages it before the call returns)
  if (!b.dense_run) HIP_TRY(hipMemcpyAsync(s->wr.dDstRows.p, dst_rows.data(), b.n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  if (src.idx) HIP_TRY(hipMemcpyAsync(s->wr.dSrcIdx.p, src.idx, b.n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  ScatterRowsArgs a = {};
  a.src = src.dev;
  a.src_half = src.dtype == EHX_DTYPE_F16;
  a.src_idx = src.idx ? s->wr.dSrcIdx.p : nullptr;
  a.dst_row = b.dense_run ? nullptr : s->wr.dDstRows.p;
  a.row0 = b.ids[0];
  a.X = s->rows.dX.p;
  a.ld = s->ld;
  a.dims = s->dims;
  a.x_half = (uint32_t)s->x_half;
  a.n = (uint32_t)b.n;
  HIP_TRY(launch_scatter_rows(a, st));
  return EHX_OK;
}

// Rows row0, row0 + stride, ... of dataset `seed` into rows [old_n, old_n + n) of a space grown for them.  Order: the one
// allocation first (binary16 spaces generate fp32 slabs of 65 536 rows and round them into the rows), then the launches.
static int land_generated(ehx_space* s, hipStream_t st, uint64_t old_n, uint64_t n, uint64_t seed, uint64_t row0, int normalize,
                          uint64_t stride, uint32_t latent) {
  if (!s->x_half) {
    HIP_TRY(launch_gen_rows(seed, row0, n, s->dims, s->ld, normalize, (float*)s->xrow(old_n), st, stride, latent));
    return EHX_OK;
  }
  const uint64_t slab = 1u << 16;
  DevBuf<float> tmp;
  if (int rc = tmp.ensure(std::min<uint64_t>(slab, n) * s->ld)) return rc;
  for (uint64_t r0 = 0; r0 < n; r0 += slab) {
    const uint64_t m = std::min<uint64_t>(slab, n - r0);
    HIP_TRY(launch_gen_rows(seed, row0 + r0 * stride, m, s->dims, s->ld, normalize, tmp.p, st, stride, latent));
    HIP_TRY(launch_store_rows_f16(tmp.p, s->ld, nullptr, old_n + r0, m, s->dims, s->ld, (__half*)s->rows.dX.p, st));
  }
  HIP_TRY(hipStreamSynchronize(st));   // (the slab is released with this frame)
  return EHX_OK;
}

// ---- the one tail behind the landers ----

// A single-copy graph space (x_perm) keeps its rows in the search copy's block order: rows land raw and are permuted in
// place.  While committed rows sit there raw the space must not be left to searches: a failure inside this guard's life —
// from "the first row may land" to "permutation complete" — poisons the space.
struct RawRowsGuard {
  ehx_space* s;
  bool armed;
  RawRowsGuard(ehx_space* s_, const WriteBatch& b) : s(s_), armed(s_->x_perm && b.touches_committed) {}
  ~RawRowsGuard() { if (armed) s->poisoned.store(true); }
};

// the id list of the permutation of a batch that is not a run: sorted, unique (the permutation is its own inverse: a row
// written twice in a batch is permuted once), and its device buffer
static int prepare_permutation(ehx_space* s, const WriteBatch& b, std::vector<uint64_t>* perm_ids) {
  if (!s->x_perm || b.dense_run) return EHX_OK;
  perm_ids->assign(b.ids, b.ids + b.n);
  std::sort(perm_ids->begin(), perm_ids->end());
  perm_ids->erase(std::unique(perm_ids->begin(), perm_ids->end()), perm_ids->end());
  return s->rows.dPermIds.ensure(perm_ids->size());
}

// The rows of `b` have been enqueued on `st`: block order (single-copy graph spaces), row statistics over [lo, hi]
// (idempotent for untouched rows in between), the derived copies with their flags, and the stream wait.  `copies_made`
// (optional) is recorded between the last two.
static int finish_rows(ehx_space* s, hipStream_t st, const WriteBatch& b, const std::vector<uint64_t>& perm_ids, RawRowsGuard& raw,
                       bool exclusive, uint64_t next, hipEvent_t copies_made) {
  if (s->x_perm) {
    if (b.dense_run) {
      HIP_TRY(launch_permute_blocks((float*)s->rows.dX.p, s->ld, b.lo, b.n, nullptr, st));
    } else {
      HIP_TRY(hipMemcpyAsync(s->rows.dPermIds.p, perm_ids.data(), perm_ids.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
      HIP_TRY(launch_permute_blocks((float*)s->rows.dX.p, s->ld, 0, perm_ids.size(), s->rows.dPermIds.p, st));
    }
    HIP_TRY(hipStreamSynchronize(st));  // (the list lives on the caller's frame; the rows are in block order from here on)
    raw.armed = false;
  }
  HIP_TRY(launch_row_stats(s->rows.dX.p, s->x_half, b.lo, b.hi - b.lo + 1, s->dims, s->ld, s->metric, s->rows.dInv.p, s->rows.dRowp.p,
                           s->rows.dMaxSumsq.p, st, s->x_perm ? 1 : 0));
  if (int rc = refresh_derived_copies(s, b.lo, b.hi - b.lo + 1, st, exclusive, next)) return rc;
  if (copies_made) HIP_TRY(hipEventRecord(copies_made, st));
  return sync_stream(s, st);
}

void publish_keys(ehx_space* s, uint64_t old_n, std::vector<std::string>& new_keys) {
  std::unique_lock<std::shared_mutex> kl(s->kmu);
  for (size_t i = 0; i < new_keys.size(); ++i) s->key_to_id.emplace(new_keys[i], old_n + i);
  for (auto& k : new_keys) s->id_to_key.push_back(std::move(k));
}

// the new row count, one release store.  An append-only writer holds no lock on the space: s->mu shared keeps a drop and a
// re-allocation out, not the searches — the count is atomic, see ehx_internal.h (the exclusive lock this used to take starved
// behind two pipelined search callers: 63 ms per chunk at 12.5 M x 1536 under search).  Else s->mu is held exclusively.
static int publish_rows(ehx_space* s, uint64_t next, bool append_only) {
  std::shared_lock<std::shared_mutex> pl(s->mu, std::defer_lock);
  if (append_only) pl.lock();
  if (append_only && s->dropped) return fail(EHX_ENOTFOUND, "Not found");
  s->n.store(next, std::memory_order_release);
  return EHX_OK;
}

// The published rows of `b` join the graph in call order (ANNIndex::set -> addPoint, index.cc:36): a fresh id is an
// insertion, a known id hnswlib's update-in-place (graph_update: updatePoint's repair of the row's links).  Rows that are
// all appended join in graph_insert's concurrent rounds instead — hnswlib's multi-threaded add_items (SURVEY A.7;
// offlinehub.py:89): the generator's always, a Set's when ehx_params.build_batch > 1 was given explicitly.
static int join_graph(ehx_space* s, const WriteBatch& b, uint64_t old_n, uint64_t next) {
  if (s->params.mode != EHX_MODE_GRAPH) return EHX_OK;
  if (s->g_n != old_n || s->params.build_batch == 0xFFFFFFFFu) {
    s->g_stale_updates += b.n - (next - old_n);
    return EHX_OK;
  }
  if (int rc = graph_ensure_arrays(s)) return rc;
  if (b.all_appended && (!b.ids || s->params.build_batch > 1)) return graph_insert(s, old_n, b.n, s->params.build_batch);
  for (size_t i = 0; i < b.n; ++i)
    if (int rc = b.ids[i] >= s->g_n ? graph_insert(s, b.ids[i], 1, 1) : graph_update(s, (uint32_t)b.ids[i])) return rc;
  return EHX_OK;
}

// ---- the callers ----

// rows `src[i]` -> row b.ids[i] of the space (ids < next; ids >= s->n are appended, dense), then the tail; finally publishes
// the keys (new_keys, in id order from s->n; nullptr: a shard, whose parent keeps them) and the new row count `next`.
//   append_only = false: the caller holds s->mu exclusively (rows may be rewritten in place, graphs change).
//   append_only = true : flat spaces, b.all_appended.  The caller holds s->wmu only: searches keep running while the rows
//     are landed, described and copied BEYOND the published row count (every kernel masks rows >= n), on the writers' stream.
// What holds on this path, each in one place:
//   1. A batch that rewrites in place first makes the writers' stream wait for the searches in flight and for the gathers of
//      ehx_get_by_ids_device (by_ev); an append-only batch and the generator wait for neither.  refresh_derived_copies
//      (exclusive) keeps its own wait before it re-makes straddling int8 tiles.
//   2. An append-only batch takes s->mu exclusively only to grow, re-checking `dropped`; it publishes keys under kmu with
//      s->mu shared, then the row count by a release store under s->mu shared after a `dropped` check.  Keys before count.
//   3. Nothing fallible that is independent of the rows happens after the first row may have landed: every prepare half
//      runs first.  (A failure after committed rows landed raw in a permuted store poisons the space: RawRowsGuard.)
//   4. The unsafe-row and margin flags are stored (refresh_derived_copies) before the release store of the row count.
//   5. DrainUnlessOk on the writers' stream covers a device source from the first enqueue to the final stream wait (its
//      lists are uploaded from this frame).
//   6. tev[0..2] are recorded before the rows, behind the rows, and behind the derived copies; the generator records none.
//   7. Graph rows join in call order (join_graph), after the row count is published.
//   8. Stored columns (ehx_columns.cpp) are written on the writers' stream in front of the rows: EHX_GROUP_NONE for every
//      appended row of every live column, then the batch's own values — both before the stream wait of finish_rows, so before
//      the keys and the row count are published.  A search that sees a row sees its labels.
int write_rows(ehx_space* s, const WriteBatch& b, uint64_t next, const RowSource& src, std::vector<std::string>* new_keys,
               bool append_only, const ColumnWrite* cw) {
  if (s->frozen) return fail(EHX_EIMMUTABLE, "Cannot write to immutable space");
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t ws = s->wr.wstream ? s->wr.wstream : s->stream;
  int rc;
  if (!append_only) {
    if ((rc = wait_searches_in_flight(s, ws))) return rc;
    if (s->by.by_ev) HIP_TRY(hipStreamWaitEvent(ws, s->by.by_ev, 0));
  }
  const uint64_t old_n = s->n;
  {
    std::unique_lock<std::shared_mutex> gl(s->mu, std::defer_lock);
    if (append_only && next >= s->cap) gl.lock();  // the arrays move: no search may be running
    if (gl && s->dropped) return fail(EHX_ENOTFOUND, "Not found");
    if ((rc = ensure_rows(s, next))) return rc;
  }
  std::vector<uint64_t> perm_ids, dst_rows;
  if (src.host && (rc = ensure_stage(s, 2 * host_half_bytes(s, b.n)))) return rc;
  if ((rc = prepare_permutation(s, b, &perm_ids))) return rc;
  if (s->wr.timed) HIP_TRY(hipEventRecord(s->wr.tev[0], ws));
  DrainUnlessOk drain{ws, src.host != nullptr};
  if (src.dev && (rc = prepare_device(s, b, src, &dst_rows))) return rc;
  if ((rc = columns_land(s, ws, b, old_n, next, cw))) return rc;
  {
    RawRowsGuard raw(s, b);
    if ((rc = src.host ? land_host(s, ws, b, src.host) : land_device(s, ws, b, src, dst_rows))) return rc;
    if (s->wr.timed) HIP_TRY(hipEventRecord(s->wr.tev[1], ws));
    if ((rc = finish_rows(s, ws, b, perm_ids, raw, !append_only, next, s->wr.timed ? s->wr.tev[2] : nullptr))) return rc;
  }
  drain.ok = true;   // (nothing of this call is in flight any more)
  // commit: the rows are resident and described — the keys first, under their own lock, then the row count
  if (new_keys) {
    std::shared_lock<std::shared_mutex> rl(s->mu, std::defer_lock);
    if (append_only) rl.lock();  // (shared: keeps a drop out, not the searches)
    if (append_only && s->dropped) return fail(EHX_ENOTFOUND, "Not found");
    publish_keys(s, old_n, *new_keys);
  }
  if ((rc = publish_rows(s, next, append_only))) return rc;
  return join_graph(s, b, old_n, next);
}

static int set_batch_locked(ehx_space* s, size_t n, const char* const* keys, const size_t* klens, const RowSource& src,
                            const ColumnWrite* cw) {
  if (is_parent(s)) return sharded_set_batch(s, n, keys, klens, src);
  if (s->frozen) return fail(EHX_EIMMUTABLE, "Cannot write to immutable space");
  std::vector<uint64_t> ids;
  std::vector<std::string> new_keys;
  uint64_t next = 0;
  resolve_keys(s, n, keys, klens, &ids, &next, &new_keys);
  return write_rows(s, write_batch(ids.data(), n, s->n), next, src, &new_keys, false, cw);
}

int set_batch_from(ehx_space* s, size_t n, const char* const* keys, const size_t* klens, const RowSource& src,
                   const ColumnWrite* cw) {
  std::lock_guard<std::mutex> wg(s->wmu);
  if (cw)   // (a column's first write takes the exclusive path once; a dropped, row-sharded or frozen space is refused there)
    if (int rc = columns_create(s, *cw)) return rc;
  std::vector<uint64_t> ids;
  std::vector<std::string> new_keys;
  uint64_t next = 0;
  if (!is_parent(s) && s->params.mode == EHX_MODE_FLAT) {
    // Streaming fast path (copy.go's BatchSet chunks, MultiSet): a batch made only of fresh keys is a pure append.
    // The key lookup needs the lock shared only, and the upload runs with no lock on the space at all.
    WriteBatch b;
    {
      std::shared_lock<std::shared_mutex> rl(s->mu);
      if (s->dropped) return fail(EHX_ENOTFOUND, "Not found");
      if (s->keyless) return fail(EHX_EINVAL, "a shard is written through its parent space");
      if (!s->frozen) {
        resolve_keys(s, n, keys, klens, &ids, &next, &new_keys);
        b = write_batch(ids.data(), n, s->n);
      }
    }
    if (b.all_appended) return write_rows(s, b, next, src, &new_keys, true, cw);
  }
  s->excl_waiting.fetch_add(1, std::memory_order_release);   // (searches that arrive from here on wait for this batch's turn)
  std::unique_lock<std::shared_mutex> wl(s->mu);
  s->excl_waiting.fetch_sub(1, std::memory_order_release);
  if (s->dropped) return fail(EHX_ENOTFOUND, "Not found");
  if (s->keyless) return fail(EHX_EINVAL, "a shard is written through its parent space");
  if (s->params.mode == EHX_MODE_GRAPH && n > 1 && s->params.build_batch != 0xFFFFFFFFu) {
    // graph mode replays a batch in call order; when it re-writes keys (known ones, or the same key
    // twice) every row must be in HBM exactly when its turn comes, so such batches go row by row
    resolve_keys(s, n, keys, klens, &ids, &next, &new_keys);
    if (!write_batch(ids.data(), n, s->n).all_appended) {
      for (size_t i = 0; i < n; ++i) {
        const ColumnWrite one = cw ? cw->from(i) : ColumnWrite{};
        if (int rc = set_batch_locked(s, 1, keys + i, klens + i, src.from(i, s->dims), cw ? &one : nullptr)) return rc;
      }
      return EHX_OK;
    }
  }
  return set_batch_locked(s, n, keys, klens, src, cw);
}

// rows row0, row0 + stride, ... of dataset `seed` appended to the space (locked exclusively by the caller) by the tail of
// write_rows; the reservation is exact (grow), not ensure_rows' doubling
int fill_synthetic_locked(ehx_space* s, uint64_t seed, uint64_t row0, uint64_t n_rows, int normalize, uint64_t stride,
                          uint32_t latent) {
  if (s->frozen) return fail(EHX_EIMMUTABLE, "Cannot write to immutable space");
  if (s->implicit_n != s->n)   // (generated rows form the head of a space: their keys are their decimal row ids)
    return fail(EHX_EINVAL, "space '%s' already holds keyed rows", s->name.c_str());
  HIP_TRY(hipSetDevice(s->device));
  const uint64_t old_n = s->n, next = old_n + n_rows;
  if (next >= (1ull << 32)) return fail(EHX_EUNSUPPORTED, "a shard holds at most 2^32-1 rows");
  int rc = grow(s, next);
  if (rc) return rc;
  s->implicit_keys = true;
  const WriteBatch b = write_batch(nullptr, n_rows, old_n);
  RawRowsGuard raw(s, b);   // (never armed: nothing committed is touched)
  if ((rc = columns_land(s, s->stream, b, old_n, next, nullptr))) return rc;
  if ((rc = land_generated(s, s->stream, old_n, n_rows, seed, row0, normalize, stride, latent))) return rc;
  if ((rc = finish_rows(s, s->stream, b, {}, raw, true, next, nullptr))) return rc;
  if ((rc = publish_rows(s, next, false))) return rc;
  {
    std::unique_lock<std::shared_mutex> kl(s->kmu);
    s->implicit_n = next;
  }
  return join_graph(s, b, old_n, next);
}

void last_writers(const uint64_t* ids, size_t n, uint64_t* out) {
  std::unordered_set<uint64_t> seen;
  seen.reserve(n);
  for (size_t i = n; i-- > 0;) out[i] = seen.insert(ids[i]).second ? ids[i] : ~0ull;
}

}  // namespace ehx_impl

// Single-row Sets (the reference's usage: one Set per RPC / per goroutine, runner/copy.go:146-161 runs 500 at a time) are
// combined like the single-query searches are, by the space's request combiner (ehx_combine.h): the leader takes every
// request that queued up meanwhile (up to 4096) and writes them as ONE batch; under load the batch size grows by itself.  A
// call returns after its row is published, so a following ehx_knn from the same thread sees it (index_test.cc:39-49).
constexpr size_t kCombineMaxBatch = 4096;
typedef Combiner<ehx_space::SetReq>::Group SetGroup;

static SetGroup set_take(SetGroup& queue) {
  const size_t m = std::min(queue.size(), kCombineMaxBatch);
  SetGroup group(queue.begin(), queue.begin() + m);
  queue.erase(queue.begin(), queue.begin() + m);
  return group;
}

static int set_serve(ehx_space* s, const SetGroup& group) {   // (a group of one: straight through, no copy)
  const size_t m = group.size();
  if (m == 1) return ehx_set_batch(s, 1, &group[0]->key, &group[0]->klen, group[0]->vec);
  std::vector<const char*> ks(m);
  std::vector<size_t> kl(m);
  std::vector<float> rows(m * s->dims);
  for (size_t i = 0; i < m; ++i) {
    ks[i] = group[i]->key;
    kl[i] = group[i]->klen;
    memcpy(rows.data() + i * s->dims, group[i]->vec, s->dims * sizeof(float));
  }
  const int rc = ehx_set_batch(s, m, ks.data(), kl.data(), rows.data());
  s->n_combined_batches += 1;
  s->n_combined_sets += m;
  return rc;
}

extern "C" int ehx_set(ehx_space* s, const char* key, size_t klen, const float* vec) {
  if (!valid_space(s)) return fail(EHX_EINVAL, "space is NULL");
  if (!key || !vec) return fail(EHX_EINVAL, "key / vector is NULL");
  ehx_space::SetReq me{{}, key, klen, vec};
  return s->set_combiner.submit(me, set_take, [s](const SetGroup& g) { return set_serve(s, g); }, g_err, sizeof(g_err));
}
