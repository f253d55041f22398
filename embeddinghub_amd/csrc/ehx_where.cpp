// Predicate filters on stored columns: ehx_knn_where*, ehx_knn_grouped_where*, ehx_range_where* (include/ehx.h has the
// contract).  A call carries up to 64 predicates — conjunctions of at most EHX_PRED_MAX_TERMS unsigned range terms over the
// space's stored columns (ehx_columns.cpp) — and query i is searched under predicate pred_of[i].  The answers are the bitmap
// forms' under the bitmaps the predicates describe, byte for byte, because they ARE the bitmap forms: each entry point enters
// the locked body of its bitmap form (masked_locked, groupedm_locked, rangem_locked) with a MaskTable whose bitmaps are BUILT
// on the device instead of copied.  masked_plan reads the row count once and calls the builder (where_build) with that
// snapshot where it would copy the caller's table into masked.dBlock: one launch of where_bitmaps_kernel (k_where.hip) writes
// the same dense table, and the compaction, the cut between the routes, the engines, the counters and the waits are the
// bitmap forms', untouched.  n_bits is all ones: the snapshot alone bounds the rows.
// Why the columns are read where they lie, without an index and without a copy:
//   - a write to an entry below the published row count (ehx_column_set, ehx_column_load_device, a Set with columns on known
//     keys) holds `mu` exclusively and waits for the searches in flight; a search holds `mu` shared from before its snapshot
//     until its launches are ordered behind its fence: the prefix cannot change under the kernel;
//   - an append lands its labels at rows >= the row count it publishes afterwards, i.e. at or above every snapshot taken
//     before: the kernel never reads them (it loads nothing at or above its n_rows), and what it reads below was landed on
//     the writers' stream before the count it saw was published;
//   - col_live and the arrays that grow swaps in change only under `mu` held exclusively: the pointers the kernel is given stay
//     valid, and a column that is not live is not read at all — it is the constant EHX_GROUP_NONE.
// The predicates travel as a small device buffer (masked.dPreds: 64 x 132 bytes do not fit a kernel argument), uploaded behind
// wait_searches_in_flight like the table itself, so an earlier call's kernel has read its own predicates by then.
// Disjunctions, IN-lists and the graph walk under them are ehx_filter.cpp's, which enters the same bodies and
// shares the pieces below that ehx_internal.h names.  Not built: shards, the per-tile counts fused into the
// build kernel, the column index for very selective equality terms.
// Entry scaffold and host staging are ehx_call.cpp's (search_on_device, HostStage).
#include "ehx_internal.h"

namespace {

static_assert(sizeof(ehx_pred) == sizeof(WherePred) && sizeof(ehx_pred) == 132 && sizeof(ehx_term) == sizeof(WhereTerm) &&
                  offsetof(ehx_pred, terms) == offsetof(WherePred, terms) && offsetof(ehx_term, flags) == offsetof(WhereTerm, flags),
              "the kernel reads the ABI's predicates as they are");
static_assert(EHX_MAX_COLUMNS == kWhereMaxCols && EHX_PRED_MAX_TERMS == kWhereMaxTerms && EHX_TERM_NOT == 1u,
              "k_where.hip's constants are the header's");

// the additions to the bitmap form's checks, behind them (n_preds == 0 and n_preds > 64 are the bitmap form's n_masks checks)
int where_check(const ehx_pred* preds, uint32_t n_preds) {
  if (!preds) return fail(EHX_EINVAL, "NULL preds");
  if (n_preds == 0) return fail(EHX_EINVAL, "n_preds is 0");
  if (n_preds > kMaskedMaxMasks) return fail(EHX_EUNSUPPORTED, "n_preds=%u exceeds %u", n_preds, kMaskedMaxMasks);
  for (uint32_t p = 0; p < n_preds; ++p) {
    if (preds[p].n_terms > EHX_PRED_MAX_TERMS)
      return fail(EHX_EINVAL, "predicate %u has %u terms: at most %u", p, preds[p].n_terms, (unsigned)EHX_PRED_MAX_TERMS);
    for (uint32_t t = 0; t < preds[p].n_terms; ++t) {
      const ehx_term& tm = preds[p].terms[t];
      if (tm.col >= EHX_MAX_COLUMNS)
        return fail(EHX_EINVAL, "predicate %u, term %u: column %u: a space has %u columns", p, t, tm.col, (unsigned)EHX_MAX_COLUMNS);
      if (tm.flags & ~EHX_TERM_NOT) return fail(EHX_EINVAL, "predicate %u, term %u: flags %#x", p, t, tm.flags);
    }
  }
  return EHX_OK;
}

}  // namespace

namespace ehx_impl {

WhereCols where_cols(const ehx_space* s, const ehx_pred* preds, uint32_t n_preds) {
  WhereCols cols = {};
  for (uint32_t p = 0; p < n_preds; ++p)
    for (uint32_t t = 0; t < preds[p].n_terms; ++t) cols.named |= 1u << preds[p].terms[t].col;
  for (uint32_t c = 0; c < EHX_MAX_COLUMNS; ++c) {
    if (!s->col_live[c]) cols.named &= ~(1u << c);   // (never written: EHX_GROUP_NONE for every row, nothing to read)
    cols.p[c] = (cols.named >> c) & 1u ? s->cols.dCol[c].p : nullptr;
  }
  return cols;
}

int check_group_col(uint32_t col) {
  return col < EHX_MAX_COLUMNS ? (int)EHX_OK
                               : fail(EHX_EINVAL, "group_col = %u: a space has %u columns", col, (unsigned)EHX_MAX_COLUMNS);
}

// the stored column as the labels of the whole prefix, read where it lies
int grouped_built_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, uint32_t per_group,
                         uint32_t group_col, const MaskTable& tab, const uint32_t* mask_of, const uint32_t* d_mask_of,
                         const ResultBlock& out) {
  int rc;
  const uint32_t* d_group_of = nullptr;
  // A column never written is cols.dNone, which column_as_groups allocates again where it holds fewer entries than it is
  // asked for — behind the searches in flight that read it, as ehx_knn_grouped_by_label* does.  It is asked for the CAPACITY,
  // not for a row count read here: the plan takes the call's snapshot later, an append may publish rows in between, and an
  // array an earlier call sized for a smaller capacity would be read past its end.  The capacity changes only under `mu`
  // held exclusively, so it bounds every row count this shared hold can see.
  if ((rc = wait_searches_in_flight(s, st)) || (rc = column_as_groups(s, st, group_col, s->cap, &d_group_of))) return rc;
  return groupedm_locked(s, st, nq, d_queries, k, per_group, d_group_of, false, kAllRows, tab, kAllRows, mask_of, d_mask_of, out);
}

int built_table_hook(ehx_space* s, const char* what, const MaskTable& tab, uint64_t* out_n,
                     const std::function<int(uint64_t, uint64_t, uint32_t*, hipStream_t)>& then) {
  return search_on_device(s, what, kWhereWhy, 1, nullptr, [&]() -> int {
    int rc;
    const hipStream_t st = s->stream;
    const uint64_t n_pub = s->n.load(std::memory_order_acquire), words = (n_pub + 31) / 32;
    *out_n = n_pub;
    if ((rc = s->masked.dBlock.ensure(kTabWords + std::max<size_t>((size_t)tab.n_masks * words, 1)))) return rc;
    if ((rc = wait_searches_in_flight(s, st))) return rc;
    if (!words) return EHX_OK;
    uint32_t* dst = s->masked.dBlock.p + kTabWords;
    if ((rc = tab.build(n_pub, words, dst, st))) return rc;
    return then(n_pub, words, dst, st);
  });
}

}  // namespace ehx_impl

namespace {

// MaskTable::build of a predicate search: the space locked shared, scratch_mu held, masked.dBlock ensured, `st` ordered behind
// the searches in flight; n_eff is the plan's snapshot of the row count
int where_build(ehx_space* s, const ehx_pred* preds, uint32_t n_preds, uint64_t n_eff, uint64_t words, uint32_t* dst,
                hipStream_t st) {
  if (int rc = s->masked.dPreds.ensure(kMaskedMaxMasks)) return rc;
  const WhereCols cols = where_cols(s, preds, n_preds);
  // (pageable host memory: the runtime stages it before the call returns)
  HIP_TRY(hipMemcpyAsync(s->masked.dPreds.p, preds, n_preds * sizeof(ehx_pred), hipMemcpyHostToDevice, st));
  HIP_TRY(launch_where_bitmaps(cols, s->masked.dPreds.p, n_preds, n_eff, words, dst, st));
  return EHX_OK;
}

MaskTable where_table(ehx_space* s, const ehx_pred* preds, uint32_t n_preds) {
  MaskTable tab = {nullptr, 0, n_preds, false};
  tab.build = [s, preds, n_preds](uint64_t n_eff, uint64_t words, uint32_t* dst, hipStream_t st) {
    return where_build(s, preds, n_preds, n_eff, words, dst, st);
  };
  return tab;
}

int knn_where_check(const ehx_space* s, size_t nq, uint32_t k, const void* q, const ehx_pred* preds, uint32_t n_preds,
                    const void* pred_of, const void* o_ids, const void* o_dist, const void* o_cnt) {
  if (int rc = masked_table_check(s, nq, k, q, nullptr, n_preds, 0, pred_of, o_ids, o_dist, o_cnt)) return rc;
  return nq ? where_check(preds, n_preds) : (int)EHX_OK;
}

int grouped_where_check(const ehx_space* s, size_t nq, uint32_t k, uint32_t per_group, uint32_t group_col, const void* q,
                        const ehx_pred* preds, uint32_t n_preds, const void* pred_of, const void* o_ids, const void* o_dist,
                        const void* o_cnt) {
  if (int rc = groupedm_check(s, nq, k, per_group, q, nullptr, 0, nullptr, n_preds, 0, pred_of, o_ids, o_dist, o_cnt)) return rc;
  if (int rc = check_group_col(group_col)) return rc;
  return nq ? where_check(preds, n_preds) : (int)EHX_OK;
}

int range_where_check(const ehx_space* s, size_t nq, uint32_t max_results, const void* q, const void* radius,
                      const ehx_pred* preds, uint32_t n_preds, const void* pred_of, const void* o_ids, const void* o_dist,
                      const void* o_cnt) {
  if (!s) return fail(EHX_EINVAL, "space is NULL");   // (before the device is looked for)
  if (int rc = rangem_check(s, nq, max_results, q, radius, nullptr, n_preds, 0, pred_of, o_ids, o_dist, o_cnt)) return rc;
  return nq ? where_check(preds, n_preds) : (int)EHX_OK;
}

// what the two test hooks below share: built_table_hook behind the hooks' own checks
template <class Then>
int where_hook(ehx_space* s, const char* what, const ehx_pred* preds, uint32_t n_preds, uint64_t* out_n, Then&& then) {
  if (!s || !out_n) return fail(EHX_EINVAL, "NULL argument");
  if (int rc = ehx_init(nullptr, 0)) return rc;
  if (int rc = where_check(preds, n_preds)) return rc;
  return built_table_hook(s, what, where_table(s, preds, n_preds), out_n, then);
}

}  // namespace

extern "C" {

int ehx_knn_where_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k, const ehx_pred* preds,
                         uint32_t n_preds, const uint32_t* d_pred_of, uint64_t* d_out_ids, float* d_out_dist,
                         uint32_t* d_out_count) {
  if (int rc = knn_where_check(s, n_queries, k, d_queries, preds, n_preds, d_pred_of, d_out_ids, d_out_dist, d_out_count)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_knn_where_device", kWhereWhy, n_queries, &st, [&] {
    return masked_locked(s, st, n_queries, d_queries, k, where_table(s, preds, n_preds), kAllRows, nullptr, d_pred_of,
                         ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_knn_where(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const ehx_pred* preds, uint32_t n_preds,
                  const uint32_t* pred_of, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (int rc = knn_where_check(s, n_queries, k, queries, preds, n_preds, pred_of, out_ids, out_dist, out_count)) return rc;
  if (int rc = check_mask_of(pred_of, n_queries, n_preds)) return rc;   // (before anything is enqueued)
  return search_on_device(s, "ehx_knn_where", kWhereWhy, n_queries, nullptr, [&]() -> int {
    int rc;
    HostStage& h = s->masked.host;
    if ((rc = h.up(s->stream, queries, n_queries, s->dims, k, false))) return rc;
    if ((rc = masked_locked(s, s->stream, n_queries, h.q, k, where_table(s, preds, n_preds), kAllRows, pred_of, nullptr, h.out)))
      return rc;
    return h.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
  });
}

int ehx_knn_grouped_where_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                 uint32_t per_group, uint32_t group_col, const ehx_pred* preds, uint32_t n_preds,
                                 const uint32_t* d_pred_of, uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count) {
  if (int rc = grouped_where_check(s, n_queries, k, per_group, group_col, d_queries, preds, n_preds, d_pred_of, d_out_ids,
                                   d_out_dist, d_out_count))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_knn_grouped_where_device", kWhereWhy, n_queries, &st, [&] {
    return grouped_built_locked(s, st, n_queries, d_queries, k, per_group, group_col, where_table(s, preds, n_preds), nullptr, d_pred_of,
                                ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_knn_grouped_where(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint32_t per_group,
                          uint32_t group_col, const ehx_pred* preds, uint32_t n_preds, const uint32_t* pred_of,
                          uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (int rc = grouped_where_check(s, n_queries, k, per_group, group_col, queries, preds, n_preds, pred_of, out_ids, out_dist,
                                   out_count))
    return rc;
  if (pred_of)
    if (int rc = check_mask_of(pred_of, n_queries, n_preds)) return rc;   // (before anything is enqueued)
  return search_on_device(s, "ehx_knn_grouped_where", kWhereWhy, n_queries, nullptr, [&]() -> int {
    int rc;
    HostStage& h = s->grouped.host;
    if ((rc = h.up(s->stream, queries, n_queries, s->dims, k, false))) return rc;
    if ((rc = grouped_built_locked(s, s->stream, n_queries, h.q, k, per_group, group_col, where_table(s, preds, n_preds), pred_of,
                                   nullptr, h.out)))
      return rc;
    return h.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
  });
}

int ehx_range_where_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, const float* d_radius,
                           uint32_t max_results, const ehx_pred* preds, uint32_t n_preds, const uint32_t* d_pred_of,
                           uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count, uint64_t* d_out_total) {
  if (int rc = range_where_check(s, n_queries, max_results, d_queries, d_radius, preds, n_preds, d_pred_of, d_out_ids, d_out_dist,
                                 d_out_count))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_range_where_device", kWhereWhy, n_queries, &st, [&] {
    return rangem_locked(s, st, n_queries, d_queries, d_radius, max_results, where_table(s, preds, n_preds), kAllRows, nullptr,
                         d_pred_of, ResultBlock{d_out_ids, d_out_dist, d_out_count, d_out_total, n_queries, max_results});
  });
}

int ehx_range_where(ehx_space* s, size_t n_queries, const float* queries, const float* radius, uint32_t max_results,
                    const ehx_pred* preds, uint32_t n_preds, const uint32_t* pred_of, uint64_t* out_ids, float* out_dist,
                    uint32_t* out_count, uint64_t* out_total) {
  if (int rc = range_where_check(s, n_queries, max_results, queries, radius, preds, n_preds, pred_of, out_ids, out_dist, out_count))
    return rc;
  if (pred_of)
    if (int rc = check_mask_of(pred_of, n_queries, n_preds)) return rc;   // (before anything is enqueued)
  return search_on_device(s, "ehx_range_where", kWhereWhy, n_queries, nullptr, [&]() -> int {
    int rc;
    HostStage& h = s->rangem.host;
    if ((rc = h.up(s->stream, queries, n_queries, s->dims, max_results, true, n_queries))) return rc;
    float* d_r = h.q + n_queries * s->dims;
    HIP_TRY(hipMemcpyAsync(d_r, radius, n_queries * sizeof(float), hipMemcpyHostToDevice, s->stream));
    if ((rc = rangem_locked(s, s->stream, n_queries, h.q, d_r, max_results, where_table(s, preds, n_preds), kAllRows, pred_of,
                            nullptr, h.out)))
      return rc;
    return h.out.copy_out(s->stream, out_ids, out_dist, out_count, out_total);
  });
}

// test hook, not part of the ABI: the validation's code for a table of predicates, without touching a device
int ehx_test_where_check(const ehx_pred* preds, uint32_t n_preds) { return where_check(preds, n_preds); }

// test hook, not part of the ABI: the builder alone, under the search's locks — *out_n = the snapshot of the row count,
// out_words[p * ceil(*out_n / 32) + w] = word w of predicate p's bitmap.  The caller's array holds n_preds bitmaps of the
// space's rows, and nothing appends meanwhile.
int ehx_test_where_bitmaps(ehx_space* s, const ehx_pred* preds, uint32_t n_preds, uint32_t* out_words, uint64_t* out_n) {
  if (!out_words) return fail(EHX_EINVAL, "NULL argument");
  return where_hook(s, "ehx_test_where_bitmaps", preds, n_preds, out_n, [&](uint64_t, uint64_t words, uint32_t* dst, hipStream_t st) -> int {
    HIP_TRY(hipMemcpyAsync(out_words, dst, (size_t)n_preds * words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return EHX_OK;
  });
}

// test hook, not part of the ABI (scripts/bench_where.py): the build kernel alone — `reps` launches back to back over the
// prefix, between two events on the space's stream, behind the upload of the predicates and one warm launch; *out_ms = the
// mean of one launch (0 for an empty space), *out_n the snapshot
int ehx_test_where_build_ms(ehx_space* s, const ehx_pred* preds, uint32_t n_preds, uint32_t reps, float* out_ms, uint64_t* out_n) {
  if (!out_ms || !reps) return fail(EHX_EINVAL, "NULL argument");
  *out_ms = 0.f;
  return where_hook(s, "ehx_test_where_build_ms", preds, n_preds, out_n, [&](uint64_t n_pub, uint64_t words, uint32_t* dst, hipStream_t st) -> int {
    const WhereCols cols = where_cols(s, preds, n_preds);
    Event e0, e1;   // (the hook's own, gone with it)
    if (int rc = e0.ensure()) return rc;
    if (int rc = e1.ensure()) return rc;
    HIP_TRY(hipEventRecord(e0, st));
    for (uint32_t i = 0; i < reps; ++i) HIP_TRY(launch_where_bitmaps(cols, s->masked.dPreds.p, n_preds, n_pub, words, dst, st));
    HIP_TRY(hipEventRecord(e1, st));
    HIP_TRY(hipEventSynchronize(e1));
    HIP_TRY(hipEventElapsedTime(out_ms, e0, e1));
    *out_ms /= (float)reps;
    return EHX_OK;
  });
}

}  // extern "C"
