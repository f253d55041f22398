// Stored label columns: up to EHX_MAX_COLUMNS 32-bit columns that the space owns (ehx_space::cols), written through the write
// path by key, and the index over each of them that the label searches on stored columns read (ehx_knn_by_label*,
// ehx_knn_grouped_by_label*: ehx_labeled.cpp, ehx_groupedl.cpp).
//   columns     dCol[c]: one uint32_t per row, sized to the capacity, moved by grow with the rows.  A column exists from its
//               first write (columns_create: the exclusive path, once); until then it reads as EHX_GROUP_NONE everywhere.
//               Every appended row holds EHX_GROUP_NONE until a value is given (columns_land fills [old_n, next) of every live
//               column in front of the batch's own values, all on the writers' stream before the row count is published).
//   index       ColIndex (k_colindex.hip): perm (row ids by (label, row id)), labels, start; the column's prefix behind a head
//               of kLabelHead words — the block of the int8 scan's flush, so a search copies no column; and for the labels
//               with more than masked_exact_cut(n) rows (at most 127: ehx_labeled.cpp's argument) the rows before every
//               256-row tile and the by-rank sample.  The host keeps a MIRROR of labels, start and those prefixes: planning a
//               search (colindex_plan) is host arithmetic alone, no launch and no wait.  The mirror costs 8 bytes per distinct
//               label read back at build time.
//   freshness   valid for a search's snapshot n_pub iff gen == col_gen[c] and n == n_pub.  Writes to entries below the
//               published row count bump col_gen (they hold mu exclusively); appends change the row count.  A stale index is
//               rebuilt whole, under scratch_mu, on the search's stream, by the search that finds it stale: one copy of the
//               prefix, one histogram pass, one sort pass per digit that has more than one occupied bucket, the boundary
//               passes, and four waits (histograms, L, the mirror, the heavy labels' prefixes).
#include "ehx_internal.h"

namespace {

constexpr const char* kColumnsWhy = "stored columns over shards are not built yet";

int check_col(uint32_t col) {
  return col < EHX_MAX_COLUMNS ? (int)EHX_OK : fail(EHX_EINVAL, "column %u: a space has %u columns", col, (unsigned)EHX_MAX_COLUMNS);
}

// (mu held exclusively, the space's device current) column c exists from here on: EHX_GROUP_NONE for every row
int column_make_live(ehx_space* s, uint32_t c) {
  if (s->col_live[c]) return EHX_OK;
  DevBuf<uint32_t> nc;
  if (s->cap) {
    if (int rc = nc.fresh(s->cap)) return rc;
    // (the fill runs on the NULL stream; the spaces' streams are not ordered with it: wait)
    HIP_TRY(hipMemset(nc.p, 0xFF, s->cap * sizeof(uint32_t)));
    HIP_TRY(hipStreamSynchronize(nullptr));
  }
  s->cols.dCol[c].swap(nc);
  s->col_live[c] = true;
  return EHX_OK;
}

// what every writer of committed entries checks under mu held exclusively, in this order
int check_column_writable(const ehx_space* s, const char* what) {
  if (int rc = check_unsharded(s, what, kColumnsWhy)) return rc;
  if (s->keyless) return fail(EHX_EINVAL, "a shard is written through its parent space");
  if (s->frozen) return fail(EHX_EIMMUTABLE, "Cannot write to immutable space");
  return EHX_OK;
}

struct ExclusiveWriter {   // wmu, then mu exclusively, searches that arrive meanwhile yielding (set_batch_from's way)
  std::lock_guard<std::mutex> wg;
  std::unique_lock<std::shared_mutex> wl;
  explicit ExclusiveWriter(ehx_space* s) : wg(s->wmu), wl(s->mu, std::defer_lock) {
    s->excl_waiting.fetch_add(1, std::memory_order_release);
    wl.lock();
    s->excl_waiting.fetch_sub(1, std::memory_order_release);
  }
};

}  // namespace

namespace ehx_impl {

int columns_create(ehx_space* s, const ColumnWrite& cw) {
  {
    std::shared_lock<std::shared_mutex> rl(s->mu);
    if (int rc = check_column_writable(s, "ehx_set_batch_cols")) return rc;
    bool all = true;   // (col_live only changes under wmu, which the caller holds)
    for (uint32_t c = 0; c < cw.n_cols; ++c) all = all && s->col_live[cw.cols[c]];
    if (all) return EHX_OK;
  }
  s->excl_waiting.fetch_add(1, std::memory_order_release);
  std::unique_lock<std::shared_mutex> wl(s->mu);
  s->excl_waiting.fetch_sub(1, std::memory_order_release);
  if (int rc = check_column_writable(s, "ehx_set_batch_cols")) return rc;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipDeviceSynchronize());   // (as grow does before it swaps arrays in)
  for (uint32_t c = 0; c < cw.n_cols; ++c)
    if (int rc = column_make_live(s, cw.cols[c])) return rc;
  return EHX_OK;
}

int grow_columns(ehx_space* s, uint64_t want, uint64_t keep, hipStream_t st) {
  for (uint32_t c = 0; c < EHX_MAX_COLUMNS; ++c) {
    if (!s->col_live[c]) continue;
    DevBuf<uint32_t> nc;
    if (nc.fresh(want))
      return fail(EHX_ENOMEM, "hipMalloc failed growing column %u of space '%s' to %llu rows", c, s->name.c_str(),
                  (unsigned long long)want);
    if (keep) HIP_TRY(hipMemcpyAsync(nc.p, s->cols.dCol[c].p, keep * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemsetAsync(nc.p + keep, 0xFF, (want - keep) * sizeof(uint32_t), st));
    HIP_TRY(hipStreamSynchronize(st));
    s->cols.dCol[c].swap(nc);
  }
  return EHX_OK;
}

int columns_land(ehx_space* s, hipStream_t ws, const WriteBatch& b, uint64_t old_n, uint64_t next, const ColumnWrite* cw) {
  if (next > s->cap && next > old_n) return fail(EHX_EINTERNAL, "columns: %llu rows beyond the capacity", (unsigned long long)next);
  for (uint32_t c = 0; c < EHX_MAX_COLUMNS; ++c)
    if (s->col_live[c] && next > old_n)
      HIP_TRY(hipMemsetAsync(s->cols.dCol[c].p + old_n, 0xFF, (next - old_n) * sizeof(uint32_t), ws));
  if (!cw || !cw->n_cols || !b.n || !b.ids) return EHX_OK;
  for (uint32_t c = 0; c < cw->n_cols; ++c)
    if (!s->col_live[cw->cols[c]]) return fail(EHX_EINTERNAL, "column %u was not created", cw->cols[c]);
  // (pageable host memory, here and below: the runtime stages it before the call returns)
  if (b.all_appended) {   // fresh, distinct keys: rows old_n, old_n + 1, ...
    for (uint32_t c = 0; c < cw->n_cols; ++c)
      HIP_TRY(hipMemcpyAsync(s->cols.dCol[cw->cols[c]].p + b.lo, cw->vals[c], b.n * sizeof(uint32_t), hipMemcpyHostToDevice, ws));
    return EHX_OK;
  }
  std::vector<uint64_t> dst(b.n);
  last_writers(b.ids, b.n, dst.data());   // the rows' duplicate rule: a key given twice keeps its last value
  int rc;
  if ((rc = s->cols.dDst.ensure(b.n)) || (rc = s->cols.dVals.ensure(b.n * cw->n_cols))) return rc;
  HIP_TRY(hipMemcpyAsync(s->cols.dDst.p, dst.data(), b.n * sizeof(uint64_t), hipMemcpyHostToDevice, ws));
  for (uint32_t c = 0; c < cw->n_cols; ++c) {
    uint32_t* d_vals = s->cols.dVals.p + (size_t)c * b.n;
    HIP_TRY(hipMemcpyAsync(d_vals, cw->vals[c], b.n * sizeof(uint32_t), hipMemcpyHostToDevice, ws));
    HIP_TRY(launch_column_scatter(s->cols.dCol[cw->cols[c]].p, s->cap, s->cols.dDst.p, d_vals, b.n, ws));
    if (b.touches_committed) s->col_gen[cw->cols[c]].fetch_add(1, std::memory_order_relaxed);   // (mu is held exclusively)
  }
  return EHX_OK;
}

int colindex_ensure(ehx_space* s, hipStream_t st, uint32_t col, uint64_t n_pub, const ehx_space::ColIndex** out) {
  ehx_space::ColIndex& ix = s->colidx[col];
  const uint64_t gen = s->col_gen[col].load(std::memory_order_relaxed);   // (stable: its writers hold mu exclusively)
  *out = &ix;
  if (ix.valid && ix.gen == gen && ix.n == n_pub) {
    ix.served_fresh += 1;
    return EHX_OK;
  }
  ix.valid = false;
  test_pause();   // (appends land labels beyond n_pub meanwhile: the build reads the prefix alone)
  if (n_pub > 0xFFFFFFFFull) return fail(EHX_EINTERNAL, "column index: %llu rows", (unsigned long long)n_pub);
  const uint64_t n = n_pub, n1 = std::max<uint64_t>(n, 1);
  const uint32_t n_tiles = (uint32_t)((n + kTileRows16 - 1) / kTileRows16), blocks = colindex_blocks(n);
  // (sized for the space's capacity, not for n: a rebuild behind every append must not allocate — and free, which waits
  // for the device — ten arrays again)
  const uint64_t c1 = std::max<uint64_t>(s->cap, n1);
  int rc;
  if ((rc = ix.dBlock.ensure(kLabelHead + c1)) || (rc = ix.dKey[0].ensure(c1)) || (rc = ix.dKey[1].ensure(c1)) ||
      (rc = ix.dVal[0].ensure(c1)) || (rc = ix.dVal[1].ensure(c1)) ||
      (rc = ix.dHist.ensure(256 * (size_t)colindex_blocks(c1) + 1024)) || (rc = ix.dBounds.ensure(c1 / kTileRows16 + 3)) ||
      (rc = ix.dLabels.ensure(c1)) || (rc = ix.dStart.ensure(c1 + 1)) || (rc = ix.dPerm.ensure(c1)))
    return rc;
  // the prefix as the index describes it: the sort's input, and the flush's copy of the column for as long as the index lives
  uint32_t* keys0 = ix.dBlock.p + kLabelHead;
  if (n && s->col_live[col])
    HIP_TRY(hipMemcpyAsync(keys0, s->cols.dCol[col].p, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  else if (n)
    HIP_TRY(hipMemsetAsync(keys0, 0xFF, n * sizeof(uint32_t), st));
  uint32_t* d_ghist = ix.dHist.p + 256 * (size_t)blocks;
  uint32_t ghist[4][256];
  HIP_TRY(launch_colindex_digits(keys0, n, d_ghist, st));
  HIP_TRY(hipMemcpyAsync(ghist, d_ghist, sizeof(ghist), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const uint32_t* keys = keys0;
  const uint32_t* vals = nullptr;
  uint32_t passes = 0;
  for (uint32_t d = 0; d < 4 && n; ++d) {
    uint32_t occupied = 0;
    for (uint32_t i = 0; i < 256; ++i) occupied += ghist[d][i] != 0;
    if (occupied <= 1) continue;   // every key has this digit: the pass would be the identity
    uint32_t *ko = ix.dKey[passes & 1].p, *vo = ix.dVal[passes & 1].p;
    HIP_TRY(launch_colindex_pass(keys, vals, ko, vo, n, d, d_ghist, ix.dHist.p, st));
    keys = ko;
    vals = vo;
    passes += 1;
  }
  HIP_TRY(launch_colindex_bounds(keys, vals, n, ix.dBounds.p, ix.dLabels.p, ix.dStart.p, ix.dPerm.p, st));
  uint32_t L = 0;
  HIP_TRY(hipMemcpyAsync(&L, ix.dBounds.p + n_tiles, sizeof(L), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (L > n) return fail(EHX_EINTERNAL, "column index: %u labels of %llu rows", L, (unsigned long long)n);
  ix.labels.assign(L, 0u);
  ix.start.assign((size_t)L + 1, 0u);
  if (L) {
    HIP_TRY(hipMemcpyAsync(ix.labels.data(), ix.dLabels.p, L * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(ix.start.data(), ix.dStart.p, ((size_t)L + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  // what the scan route needs of every label that may take it
  const uint64_t cut = masked_exact_cut(n);
  ix.heavy.clear();
  std::vector<uint64_t> run;
  for (uint32_t i = 0; i < L; ++i)
    if ((uint64_t)ix.start[i + 1] - ix.start[i] > cut) ix.heavy.push_back(i);
  const uint32_t H = (uint32_t)ix.heavy.size();
  if (H > kLabeledMaxScan) return fail(EHX_EINTERNAL, "column index: %u labels above the cut", H);
  ix.cum.assign((size_t)H * (n_tiles + 1), 0u);
  if (H) {
    run.resize(2 * (size_t)H);
    for (uint32_t h = 0; h < H; ++h) {
      run[h] = ix.start[ix.heavy[h]];
      run[H + h] = ix.start[ix.heavy[h] + 1];
    }
    if ((rc = ix.dRun.ensure(2 * (size_t)kLabeledMaxScan)) || (rc = ix.dCum.ensure((size_t)H * (c1 / kTileRows16 + 2))) ||
        (rc = ix.dSample.ensure((size_t)kLabeledMaxScan * 256)))
      return rc;
    HIP_TRY(hipMemcpyAsync(ix.dRun.p, run.data(), run.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(launch_colindex_heavy(ix.dPerm.p, ix.dRun.p, H, n_tiles, ix.dCum.p, ix.dSample.p, st));
    HIP_TRY(hipMemcpyAsync(ix.cum.data(), ix.dCum.p, ix.cum.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  ix.gen = gen;
  ix.n = n;
  ix.n_tiles = n_tiles;
  ix.builds += 1;
  ix.last_passes = passes;
  ix.valid = true;
  return EHX_OK;
}

void colindex_plan(const ehx_space::ColIndex& ix, size_t m, const uint32_t* want, bool scan_serves, uint64_t cut,
                   size_t min_scan_queries, LabeledPlan* p) {
  labeled_slots(want, m, p);
  const uint32_t n_slots = p->n_slots;
  p->n_tiles = ix.n_tiles;
  p->total = ix.n;   // (the lists are runs of the whole permutation)
  p->n_allowed.assign(n_slots, 0);
  p->off.assign(n_slots, 0);
  p->scans.assign(n_slots, 0);
  p->scan_of.assign(n_slots, kLabeledNoScan);
  p->cum.clear();
  p->n_scan = 0;
  std::vector<uint32_t> label_at(n_slots, kLabeledNoScan);   // the slot's position in ix.labels
  for (uint32_t f = 0; f < n_slots; ++f) {
    const auto it = std::lower_bound(ix.labels.begin(), ix.labels.end(), p->table[f]);
    if (it == ix.labels.end() || *it != p->table[f]) continue;   // no row carries the label
    const uint32_t i = label_at[f] = (uint32_t)(it - ix.labels.begin());
    p->off[f] = ix.start[i];
    p->n_allowed[f] = (uint64_t)ix.start[i + 1] - ix.start[i];
  }
  // the route: the cut; of those only the labels the index prepared prefixes for (above masked_exact_cut(n): a cut forced
  // below it leaves the others on lists); the gate; then the scanning slots' rows of ix.cum
  filter_routes_cut(scan_serves, cut, p->n_allowed.data(), n_slots, p->scans.data());
  for (uint32_t f = 0; f < n_slots; ++f)
    p->scans[f] = p->scans[f] && std::binary_search(ix.heavy.begin(), ix.heavy.end(), label_at[f]);
  filter_routes_gate(p->slot_of.data(), m, min_scan_queries, n_slots, p->scans.data());
  for (uint32_t f = 0; f < n_slots; ++f) {
    if (!p->scans[f]) continue;
    p->scan_of[f] = (uint32_t)(std::lower_bound(ix.heavy.begin(), ix.heavy.end(), label_at[f]) - ix.heavy.begin());
    p->n_scan += 1;
  }
}

int column_as_groups(ehx_space* s, hipStream_t st, uint32_t col, uint64_t n_pub, const uint32_t** out) {
  if (s->col_live[col]) {
    *out = s->cols.dCol[col].p;
    return EHX_OK;
  }
  // filled ONCE per allocation, sized for the capacity: nothing else writes it, so a call makes no pass that grows with the
  // row count (the fill is enqueued in front of this search's launches; later searches are ordered behind its fence)
  if (s->cols.dNone.n < std::max<uint64_t>(n_pub, 1)) {
    if (int rc = s->cols.dNone.fresh(std::max<uint64_t>(s->cap, std::max<uint64_t>(n_pub, 1)))) return rc;
    HIP_TRY(hipMemsetAsync(s->cols.dNone.p, 0xFF, s->cols.dNone.n * sizeof(uint32_t), st));
  }
  *out = s->cols.dNone.p;
  return EHX_OK;
}

}  // namespace ehx_impl

extern "C" {

int ehx_set_batch_cols(ehx_space* s, size_t n, const char* const* keys, const size_t* klens, const float* vecs, uint32_t n_cols,
                       const uint32_t* cols, const uint32_t* const* values) {
  if (!valid_space(s)) return fail(EHX_EINVAL, "space is NULL");
  if (n_cols == 0) return ehx_set_batch(s, n, keys, klens, vecs);
  if (n_cols > EHX_MAX_COLUMNS || !cols || !values) return fail(EHX_EINVAL, "n_cols = %u with %s", n_cols, cols && values ? "at most 4 columns" : "a NULL argument");
  ColumnWrite cw;
  cw.n_cols = n_cols;
  for (uint32_t c = 0; c < n_cols; ++c) {
    if (int rc = check_col(cols[c])) return rc;
    for (uint32_t e = 0; e < c; ++e)
      if (cols[e] == cols[c]) return fail(EHX_EINVAL, "column %u is named twice", cols[c]);
    if (n && !values[c]) return fail(EHX_EINVAL, "NULL values of column %u", cols[c]);
    cw.cols[c] = cols[c];
    cw.vals[c] = values[c];
  }
  if (n == 0) return EHX_OK;
  if (!keys || !klens || !vecs) return fail(EHX_EINVAL, "NULL argument");
  RowSource src;
  src.host = vecs;
  return set_batch_from(s, n, keys, klens, src, &cw);
}

int ehx_column_set(ehx_space* s, uint32_t col, size_t n, const char* const* keys, const size_t* klens, const uint32_t* values,
                   size_t* bad_index) {
  if (!valid_space(s)) return fail(EHX_EINVAL, "space is NULL");
  if (int rc = check_col(col)) return rc;
  if (n == 0) return EHX_OK;
  if (!keys || !klens || !values) return fail(EHX_EINVAL, "NULL argument");
  ExclusiveWriter w(s);
  int rc;
  if ((rc = check_column_writable(s, "ehx_column_set"))) return rc;
  std::vector<uint64_t> ids;
  if ((rc = lookup_keys(s, n, keys, klens, &ids, bad_index))) return rc;   // (nothing is written)
  HIP_TRY(hipSetDevice(s->device));
  if (!s->col_live[col]) {
    HIP_TRY(hipDeviceSynchronize());
    if ((rc = column_make_live(s, col))) return rc;
  }
  const hipStream_t ws = s->wr.wstream ? (hipStream_t)s->wr.wstream : (hipStream_t)s->stream;
  // a rewrite in place: the searches in flight have read the column, or an index's copy of it that the next search replaces
  if ((rc = wait_searches_in_flight(s, ws))) return rc;
  std::vector<uint64_t> dst(n);
  last_writers(ids.data(), n, dst.data());
  if ((rc = s->cols.dDst.ensure(n)) || (rc = s->cols.dVals.ensure(n))) return rc;
  DrainUnlessOk drain{ws};
  HIP_TRY(hipMemcpyAsync(s->cols.dDst.p, dst.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, ws));
  HIP_TRY(hipMemcpyAsync(s->cols.dVals.p, values, n * sizeof(uint32_t), hipMemcpyHostToDevice, ws));
  HIP_TRY(launch_column_scatter(s->cols.dCol[col].p, std::min<uint64_t>(s->cap, s->n.load(std::memory_order_relaxed)), s->cols.dDst.p,
                                s->cols.dVals.p, n, ws));
  s->col_gen[col].fetch_add(1, std::memory_order_relaxed);
  return drain.done(sync_stream(s, ws));
}

int ehx_column_get(ehx_space* s, uint32_t col, size_t n, const char* const* keys, const size_t* klens, uint32_t* out_values,
                   size_t* bad_index) {
  if (!valid_space(s)) return fail(EHX_EINVAL, "space is NULL");
  if (int rc = check_col(col)) return rc;
  if (n == 0) return EHX_OK;
  if (!keys || !klens || !out_values) return fail(EHX_EINVAL, "NULL argument");
  return search_shared(s, "ehx_column_get", kColumnsWhy, [&]() -> int {
    std::vector<uint64_t> ids;
    int rc;
    if ((rc = lookup_keys(s, n, keys, klens, &ids, bad_index))) return rc;
    if (!s->col_live[col]) {
      std::fill(out_values, out_values + n, EHX_GROUP_NONE);
      return EHX_OK;
    }
    return on_device(s, n, s->stream, [&]() -> int {
      if ((rc = s->cols.dGetIds.ensure(n)) || (rc = s->cols.dGetVals.ensure(n))) return rc;
      const hipStream_t st = s->stream;
      HIP_TRY(hipMemcpyAsync(s->cols.dGetIds.p, ids.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
      HIP_TRY(launch_column_gather(s->cols.dCol[col].p, s->cap, s->cols.dGetIds.p, s->cols.dGetVals.p, n, st));
      HIP_TRY(hipMemcpyAsync(out_values, s->cols.dGetVals.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      return EHX_OK;
    });
  });
}

int ehx_column_load_device(ehx_space* s, void* stream, uint32_t col, uint64_t row0, uint64_t n, const uint32_t* d_values) {
  if (!valid_space(s)) return fail(EHX_EINVAL, "space is NULL");
  if (int rc = check_col(col)) return rc;
  if (n && !d_values) return fail(EHX_EINVAL, "NULL argument");
  const hipStream_t st = (hipStream_t)stream;
  ExclusiveWriter w(s);
  int rc;
  if ((rc = check_column_writable(s, "ehx_column_load_device"))) return rc;
  const uint64_t rows = s->n.load(std::memory_order_relaxed);
  if (row0 > rows || n > rows - row0)
    return fail(EHX_EINVAL, "rows [%llu, %llu + %llu) do not lie below the row count %llu", (unsigned long long)row0,
                (unsigned long long)row0, (unsigned long long)n, (unsigned long long)rows);
  if (n == 0) return EHX_OK;
  HIP_TRY(hipSetDevice(s->device));
  if (!s->col_live[col]) {
    HIP_TRY(hipDeviceSynchronize());
    if ((rc = column_make_live(s, col))) return rc;
  }
  if ((rc = wait_searches_in_flight(s, st))) return rc;
  DrainUnlessOk drain{st};
  HIP_TRY(hipMemcpyAsync(s->cols.dCol[col].p + row0, d_values, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  s->col_gen[col].fetch_add(1, std::memory_order_relaxed);
  HIP_TRY(hipStreamSynchronize(st));   // (the call returns with the values in place: the lock is released behind them)
  return drain.done(EHX_OK);
}

int ehx_column_read_device(ehx_space* s, void* stream, uint32_t col, uint64_t row0, uint64_t n, uint32_t* d_out) {
  if (!valid_space(s)) return fail(EHX_EINVAL, "space is NULL");
  if (int rc = check_col(col)) return rc;
  if (n && !d_out) return fail(EHX_EINVAL, "NULL argument");
  const hipStream_t st = (hipStream_t)stream;
  return search_shared(s, "ehx_column_read_device", kColumnsWhy, [&]() -> int {
    const uint64_t rows = s->n.load(std::memory_order_acquire);
    if (row0 > rows || n > rows - row0)
      return fail(EHX_EINVAL, "rows [%llu, %llu + %llu) do not lie below the row count %llu", (unsigned long long)row0,
                  (unsigned long long)row0, (unsigned long long)n, (unsigned long long)rows);
    if (n == 0) return EHX_OK;
    HIP_TRY(hipSetDevice(s->device));
    DrainUnlessOk drain{st};
    if (s->col_live[col])
      HIP_TRY(hipMemcpyAsync(d_out, s->cols.dCol[col].p + row0, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    else
      HIP_TRY(hipMemsetAsync(d_out, 0xFF, n * sizeof(uint32_t), st));
    HIP_TRY(hipStreamSynchronize(st));   // (a writer that follows rewrites the column in place)
    return drain.done(EHX_OK);
  });
}

// test hook, not part of the ABI: index builds of the column, searches served from a fresh index, digit passes of the last build
void ehx_test_column_counters(ehx_space* s, uint32_t col, uint64_t out[3]) {
  out[0] = out[1] = out[2] = 0;
  if (!s || col >= EHX_MAX_COLUMNS) return;
  std::lock_guard<std::mutex> sl(s->scratch_mu);
  out[0] = s->colidx[col].builds;
  out[1] = s->colidx[col].served_fresh;
  out[2] = s->colidx[col].last_passes;
}

// test hook, not part of the ABI: the column's index as the device holds it — perm[*n], labels[*L], start[*L + 1] (the caller's
// arrays hold at least the row count, and one more for start); EHX_ENOTFOUND while no index has been built
int ehx_test_column_index(ehx_space* s, uint32_t col, uint64_t* perm, uint32_t* labels, uint32_t* start, uint64_t* n, uint32_t* L) {
  if (!s || col >= EHX_MAX_COLUMNS || !perm || !labels || !start || !n || !L) return fail(EHX_EINVAL, "NULL argument");
  std::shared_lock<std::shared_mutex> rl(s->mu);
  std::lock_guard<std::mutex> sl(s->scratch_mu);
  const ehx_space::ColIndex& ix = s->colidx[col];
  if (s->dropped || !ix.valid) return fail(EHX_ENOTFOUND, "column %u has no index", col);
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipDeviceSynchronize());
  *n = ix.n;
  *L = (uint32_t)ix.labels.size();
  start[0] = 0;
  if (!ix.n) return EHX_OK;
  HIP_TRY(hipMemcpy(perm, ix.dPerm.p, ix.n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(labels, ix.dLabels.p, *L * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(start, ix.dStart.p, ((size_t)*L + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return EHX_OK;
}

}  // extern "C"
