// Boolean filters on stored columns: ehx_knn_filter*, ehx_knn_grouped_filter*, ehx_range_filter*, ehx_graph_knn_filter*
// (include/ehx.h has the contract).  A call carries up to 64 filters — each the OR of a run of the call's clauses, a clause an
// ehx_pred whose terms may also be set-membership tests (EHX_TERM_IN) — and query i is searched under filter filter_of[i].
// The answers are the bitmap forms' under the bitmaps the filters describe, byte for byte, because they ARE the bitmap forms:
// each entry point enters the locked body of its bitmap form (masked_locked, groupedm_locked through grouped_built_locked,
// rangem_locked, graphm_locked) with a MaskTable whose `build` has ONE launch of filter_bitmaps_kernel (k_filter.hip) write
// the table, exactly as ehx_where.cpp does it for plain conjunctions.  A row that several clauses of a filter allow is one
// bit of one bitmap: it cannot come back twice, which the merge of several ehx_knn_where answers could not promise.
// Why the columns are read where they lie, without an index and without a copy, is ehx_where.cpp's argument
// and carries over unchanged: searches hold `mu` shared from before their snapshot, writes below the row count hold it
// exclusively, appends land at or above every earlier snapshot.
// The expression is validated and PACKED on the host before anything is enqueued (pack_filters): the clauses as they are,
// but every IN term's (first index, count) into the caller's values replaced by (first index, count) into a private copy in
// which each term's set is sorted and de-duplicated — what the kernel's binary search needs; then the packed values, then
// the filters' runs.  It travels as ONE upload into masked.dFilter (sized once for the limits: 128 clauses, 4096 values, 64
// runs), behind wait_searches_in_flight like masked.dPreds, so an earlier call's kernel has read its own copy by then.
// Not built: nesting beyond OR-of-AND, sets beyond 4096 values (the column index), shards, the gRPC shim, the
// per-tile counts fused into the build kernel.
// Entry scaffold and host staging are ehx_call.cpp's (search_on_device, HostStage).
#include "ehx_internal.h"

namespace {

static_assert(EHX_TERM_IN == kFilterTermIn && EHX_FILTER_MAX_CLAUSES == kFilterMaxClauses &&
                  EHX_FILTER_MAX_VALUES == kFilterMaxValues && sizeof(ehx_filter) == 2 * sizeof(uint32_t),
              "k_filter.hip's constants and layouts are the header's");
constexpr uint32_t kClauseWords = sizeof(ehx_pred) / sizeof(uint32_t);

// the additions to the bitmap form's checks, behind them
int filter_check(const ehx_filters* f) {
  if (!f) return fail(EHX_EINVAL, "NULL filters");
  if ((f->n_clauses && !f->clauses) || (f->n_filters && !f->filters) || (f->n_values && !f->values))
    return fail(EHX_EINVAL, "NULL clauses, filters or values with a count above 0");
  if (f->n_filters == 0) return fail(EHX_EINVAL, "n_filters is 0");
  if (f->n_filters > kMaskedMaxMasks) return fail(EHX_EUNSUPPORTED, "n_filters=%u exceeds %u", f->n_filters, kMaskedMaxMasks);
  if (f->n_clauses > EHX_FILTER_MAX_CLAUSES)
    return fail(EHX_EUNSUPPORTED, "n_clauses=%u exceeds %u", f->n_clauses, (unsigned)EHX_FILTER_MAX_CLAUSES);
  for (uint32_t i = 0; i < f->n_filters; ++i)
    if ((uint64_t)f->filters[i].first_clause + f->filters[i].n_clauses > f->n_clauses)
      return fail(EHX_EINVAL, "filter %u: clauses [%u, %u + %u) of %u", i, f->filters[i].first_clause, f->filters[i].first_clause,
                  f->filters[i].n_clauses, f->n_clauses);
  uint64_t in_values = 0;
  for (uint32_t c = 0; c < f->n_clauses; ++c) {
    const ehx_pred& cl = f->clauses[c];
    if (cl.n_terms > EHX_PRED_MAX_TERMS)
      return fail(EHX_EINVAL, "clause %u has %u terms: at most %u", c, cl.n_terms, (unsigned)EHX_PRED_MAX_TERMS);
    for (uint32_t t = 0; t < cl.n_terms; ++t) {
      const ehx_term& tm = cl.terms[t];
      if (tm.col >= EHX_MAX_COLUMNS)
        return fail(EHX_EINVAL, "clause %u, term %u: column %u: a space has %u columns", c, t, tm.col, (unsigned)EHX_MAX_COLUMNS);
      if (tm.flags & ~(EHX_TERM_NOT | EHX_TERM_IN)) return fail(EHX_EINVAL, "clause %u, term %u: flags %#x", c, t, tm.flags);
      if (!(tm.flags & EHX_TERM_IN)) continue;
      if ((uint64_t)tm.lo + tm.hi > f->n_values)
        return fail(EHX_EINVAL, "clause %u, term %u: values [%u, %u + %u) of %u", c, t, tm.lo, tm.lo, tm.hi, f->n_values);
      in_values += tm.hi;
    }
  }
  if (in_values > EHX_FILTER_MAX_VALUES)
    return fail(EHX_EUNSUPPORTED, "the IN terms hold %llu values: at most %u", (unsigned long long)in_values,
                (unsigned)EHX_FILTER_MAX_VALUES);
  return EHX_OK;
}

// a checked table as the kernel reads it
struct PackedFilters {
  std::vector<uint32_t> words;   // n_clauses x 33 | n_values | n_filters x 2
  std::vector<ehx_pred> clauses;   // the caller's, for where_cols
  uint32_t n_clauses = 0, n_values = 0, n_filters = 0;
};

std::shared_ptr<const PackedFilters> pack_filters(const ehx_filters* f) {
  auto pk = std::make_shared<PackedFilters>();
  pk->n_clauses = f->n_clauses;
  pk->n_filters = f->n_filters;
  pk->clauses.assign(f->clauses, f->clauses + f->n_clauses);
  std::vector<ehx_pred> cl = pk->clauses;
  std::vector<uint32_t> vals;
  for (ehx_pred& c : cl)
    for (uint32_t t = 0; t < c.n_terms; ++t) {
      ehx_term& tm = c.terms[t];
      if (!(tm.flags & EHX_TERM_IN)) continue;
      std::vector<uint32_t> set(f->values + tm.lo, f->values + tm.lo + tm.hi);
      std::sort(set.begin(), set.end());   // (unsigned)
      set.erase(std::unique(set.begin(), set.end()), set.end());
      tm.lo = (uint32_t)vals.size();
      tm.hi = (uint32_t)set.size();
      vals.insert(vals.end(), set.begin(), set.end());
    }
  pk->n_values = (uint32_t)vals.size();   // (at most the sum filter_check bounded)
  pk->words.resize((size_t)cl.size() * kClauseWords);
  if (!cl.empty()) memcpy(pk->words.data(), cl.data(), cl.size() * sizeof(ehx_pred));
  pk->words.insert(pk->words.end(), vals.begin(), vals.end());
  for (uint32_t i = 0; i < f->n_filters; ++i) {
    pk->words.push_back(f->filters[i].first_clause);
    pk->words.push_back(f->filters[i].n_clauses);
  }
  return pk;
}

// MaskTable::build of a filter search: the space locked shared, scratch_mu held, masked.dBlock ensured, `st` ordered behind
// the searches in flight; n_eff is the plan's snapshot of the row count
int filter_build(ehx_space* s, const PackedFilters& pk, uint64_t n_eff, uint64_t words, uint32_t* dst, hipStream_t st) {
  if (int rc = s->masked.dFilter.ensure(kFilterExprWords)) return rc;
  const WhereCols cols = where_cols(s, pk.clauses.data(), pk.n_clauses);
  // (pageable host memory: the runtime stages it before the call returns)
  HIP_TRY(hipMemcpyAsync(s->masked.dFilter.p, pk.words.data(), pk.words.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HIP_TRY(launch_filter_bitmaps(cols, s->masked.dFilter.p, pk.n_clauses, pk.n_values, pk.n_filters, n_eff, words, dst, st));
  return EHX_OK;
}

// the table of a CHECKED expression (no queries: nothing was checked, and nothing will ask for the table)
MaskTable filter_table(ehx_space* s, const ehx_filters* f, size_t nq = 1) {
  if (!nq) return MaskTable{nullptr, 0, 0, false};
  const std::shared_ptr<const PackedFilters> pk = pack_filters(f);
  MaskTable tab = {nullptr, 0, f->n_filters, false};
  tab.build = [s, pk](uint64_t n_eff, uint64_t words, uint32_t* dst, hipStream_t st) {
    return filter_build(s, *pk, n_eff, words, dst, st);
  };
  return tab;
}

uint32_t n_filters_of(const ehx_filters* f) { return f ? f->n_filters : 0u; }   // (NULL: the bitmap form's "n_masks is 0")

int knn_filter_check(const ehx_space* s, size_t nq, uint32_t k, const void* q, const ehx_filters* f, const void* filter_of,
                     const void* o_ids, const void* o_dist, const void* o_cnt) {
  if (int rc = masked_table_check(s, nq, k, q, nullptr, n_filters_of(f), 0, filter_of, o_ids, o_dist, o_cnt)) return rc;
  return nq ? filter_check(f) : (int)EHX_OK;
}

int grouped_filter_check(const ehx_space* s, size_t nq, uint32_t k, uint32_t per_group, uint32_t group_col, const void* q,
                         const ehx_filters* f, const void* filter_of, const void* o_ids, const void* o_dist, const void* o_cnt) {
  if (int rc = groupedm_check(s, nq, k, per_group, q, nullptr, 0, nullptr, n_filters_of(f), 0, filter_of, o_ids, o_dist, o_cnt))
    return rc;
  if (int rc = check_group_col(group_col)) return rc;
  return nq ? filter_check(f) : (int)EHX_OK;
}

int range_filter_check(const ehx_space* s, size_t nq, uint32_t max_results, const void* q, const void* radius,
                       const ehx_filters* f, const void* filter_of, const void* o_ids, const void* o_dist, const void* o_cnt) {
  if (!s) return fail(EHX_EINVAL, "space is NULL");   // (before the device is looked for)
  if (int rc = rangem_check(s, nq, max_results, q, radius, nullptr, n_filters_of(f), 0, filter_of, o_ids, o_dist, o_cnt)) return rc;
  return nq ? filter_check(f) : (int)EHX_OK;
}

int graph_filter_check(const ehx_space* s, size_t nq, uint32_t k, const void* q, const ehx_filters* f, const void* filter_of,
                       uint32_t route, const void* o_ids, const void* o_dist, const void* o_cnt) {
  if (int rc = graphm_table_check(s, nq, k, q, nullptr, n_filters_of(f), 0, filter_of, route, o_ids, o_dist, o_cnt)) return rc;
  return nq ? filter_check(f) : (int)EHX_OK;
}

// the hooks' checks and table
int filter_hook(ehx_space* s, const char* what, const ehx_filters* f, uint64_t* out_n,
                const std::function<int(uint64_t, uint64_t, uint32_t*, hipStream_t)>& then) {
  if (!s || !out_n) return fail(EHX_EINVAL, "NULL argument");
  if (int rc = ehx_init(nullptr, 0)) return rc;
  if (int rc = filter_check(f)) return rc;
  return built_table_hook(s, what, filter_table(s, f), out_n, then);
}

}  // namespace

extern "C" {

int ehx_knn_filter_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                          const ehx_filters* filters, const uint32_t* d_filter_of, uint64_t* d_out_ids, float* d_out_dist,
                          uint32_t* d_out_count) {
  if (int rc = knn_filter_check(s, n_queries, k, d_queries, filters, d_filter_of, d_out_ids, d_out_dist, d_out_count)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const MaskTable tab = filter_table(s, filters, n_queries);
  return search_on_device(s, "ehx_knn_filter_device", kWhereWhy, n_queries, &st, [&] {
    return masked_locked(s, st, n_queries, d_queries, k, tab, kAllRows, nullptr, d_filter_of,
                         ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_knn_filter(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const ehx_filters* filters,
                   const uint32_t* filter_of, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (int rc = knn_filter_check(s, n_queries, k, queries, filters, filter_of, out_ids, out_dist, out_count)) return rc;
  if (n_queries)
    if (int rc = check_mask_of(filter_of, n_queries, filters->n_filters)) return rc;   // (before anything is enqueued)
  const MaskTable tab = filter_table(s, filters, n_queries);
  return search_on_device(s, "ehx_knn_filter", kWhereWhy, n_queries, nullptr, [&]() -> int {
    int rc;
    HostStage& h = s->masked.host;
    if ((rc = h.up(s->stream, queries, n_queries, s->dims, k, false))) return rc;
    if ((rc = masked_locked(s, s->stream, n_queries, h.q, k, tab, kAllRows, filter_of, nullptr, h.out))) return rc;
    return h.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
  });
}

int ehx_knn_grouped_filter_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                  uint32_t per_group, uint32_t group_col, const ehx_filters* filters,
                                  const uint32_t* d_filter_of, uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count) {
  if (int rc = grouped_filter_check(s, n_queries, k, per_group, group_col, d_queries, filters, d_filter_of, d_out_ids, d_out_dist,
                                    d_out_count))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  const MaskTable tab = filter_table(s, filters, n_queries);
  return search_on_device(s, "ehx_knn_grouped_filter_device", kWhereWhy, n_queries, &st, [&] {
    return grouped_built_locked(s, st, n_queries, d_queries, k, per_group, group_col, tab, nullptr, d_filter_of,
                                ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_knn_grouped_filter(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint32_t per_group,
                           uint32_t group_col, const ehx_filters* filters, const uint32_t* filter_of, uint64_t* out_ids,
                           float* out_dist, uint32_t* out_count) {
  if (int rc = grouped_filter_check(s, n_queries, k, per_group, group_col, queries, filters, filter_of, out_ids, out_dist, out_count))
    return rc;
  if (filter_of)
    if (n_queries)
    if (int rc = check_mask_of(filter_of, n_queries, filters->n_filters)) return rc;   // (before anything is enqueued)
  const MaskTable tab = filter_table(s, filters, n_queries);
  return search_on_device(s, "ehx_knn_grouped_filter", kWhereWhy, n_queries, nullptr, [&]() -> int {
    int rc;
    HostStage& h = s->grouped.host;
    if ((rc = h.up(s->stream, queries, n_queries, s->dims, k, false))) return rc;
    if ((rc = grouped_built_locked(s, s->stream, n_queries, h.q, k, per_group, group_col, tab, filter_of, nullptr, h.out))) return rc;
    return h.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
  });
}

int ehx_range_filter_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, const float* d_radius,
                            uint32_t max_results, const ehx_filters* filters, const uint32_t* d_filter_of, uint64_t* d_out_ids,
                            float* d_out_dist, uint32_t* d_out_count, uint64_t* d_out_total) {
  if (int rc = range_filter_check(s, n_queries, max_results, d_queries, d_radius, filters, d_filter_of, d_out_ids, d_out_dist,
                                  d_out_count))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  const MaskTable tab = filter_table(s, filters, n_queries);
  return search_on_device(s, "ehx_range_filter_device", kWhereWhy, n_queries, &st, [&] {
    return rangem_locked(s, st, n_queries, d_queries, d_radius, max_results, tab, kAllRows, nullptr, d_filter_of,
                         ResultBlock{d_out_ids, d_out_dist, d_out_count, d_out_total, n_queries, max_results});
  });
}

int ehx_range_filter(ehx_space* s, size_t n_queries, const float* queries, const float* radius, uint32_t max_results,
                     const ehx_filters* filters, const uint32_t* filter_of, uint64_t* out_ids, float* out_dist,
                     uint32_t* out_count, uint64_t* out_total) {
  if (int rc = range_filter_check(s, n_queries, max_results, queries, radius, filters, filter_of, out_ids, out_dist, out_count))
    return rc;
  if (filter_of)
    if (n_queries)
    if (int rc = check_mask_of(filter_of, n_queries, filters->n_filters)) return rc;   // (before anything is enqueued)
  const MaskTable tab = filter_table(s, filters, n_queries);
  return search_on_device(s, "ehx_range_filter", kWhereWhy, n_queries, nullptr, [&]() -> int {
    int rc;
    HostStage& h = s->rangem.host;
    if ((rc = h.up(s->stream, queries, n_queries, s->dims, max_results, true, n_queries))) return rc;
    float* d_r = h.q + n_queries * s->dims;
    HIP_TRY(hipMemcpyAsync(d_r, radius, n_queries * sizeof(float), hipMemcpyHostToDevice, s->stream));
    if ((rc = rangem_locked(s, s->stream, n_queries, h.q, d_r, max_results, tab, kAllRows, filter_of, nullptr, h.out))) return rc;
    return h.out.copy_out(s->stream, out_ids, out_dist, out_count, out_total);
  });
}

int ehx_graph_knn_filter_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                const ehx_filters* filters, const uint32_t* d_filter_of, uint32_t route, uint64_t* d_out_ids,
                                float* d_out_dist, uint32_t* d_out_count) {
  if (int rc = graph_filter_check(s, n_queries, k, d_queries, filters, d_filter_of, route, d_out_ids, d_out_dist, d_out_count))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  const MaskTable tab = filter_table(s, filters, n_queries);
  return search_on_device(s, "ehx_graph_knn_filter_device", kWhereWhy, n_queries, &st, [&] {
    return graphm_locked(s, st, n_queries, d_queries, k, tab, kAllRows, nullptr, d_filter_of, route,
                         ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_graph_knn_filter(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const ehx_filters* filters,
                         const uint32_t* filter_of, uint32_t route, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (int rc = graph_filter_check(s, n_queries, k, queries, filters, filter_of, route, out_ids, out_dist, out_count)) return rc;
  if (n_queries)
    if (int rc = check_mask_of(filter_of, n_queries, filters->n_filters)) return rc;   // (before anything is enqueued)
  const MaskTable tab = filter_table(s, filters, n_queries);
  return search_on_device(s, "ehx_graph_knn_filter", kWhereWhy, n_queries, nullptr, [&]() -> int {
    int rc;
    HostStage& h = s->masked.host;
    if ((rc = h.up(s->stream, queries, n_queries, s->dims, k, false))) return rc;
    if ((rc = graphm_locked(s, s->stream, n_queries, h.q, k, tab, kAllRows, filter_of, nullptr, route, h.out))) return rc;
    return h.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
  });
}

// test hook, not part of the ABI: the validation's code for a table of filters, without touching a device
int ehx_test_filter_check(const ehx_filters* filters) { return filter_check(filters); }

// test hook, not part of the ABI: the builder alone, under the search's locks — *out_n = the snapshot of the row count,
// out_words[f * ceil(*out_n / 32) + w] = word w of filter f's bitmap.  The caller's array holds n_filters bitmaps of the
// space's rows, and nothing appends meanwhile.
int ehx_test_filter_bitmaps(ehx_space* s, const ehx_filters* filters, uint32_t* out_words, uint64_t* out_n) {
  if (!out_words) return fail(EHX_EINVAL, "NULL argument");
  return filter_hook(s, "ehx_test_filter_bitmaps", filters, out_n, [&](uint64_t, uint64_t words, uint32_t* dst, hipStream_t st) -> int {
    HIP_TRY(hipMemcpyAsync(out_words, dst, (size_t)filters->n_filters * words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return EHX_OK;
  });
}

// test hook, not part of the ABI (scripts/bench_filter.py): the build kernel alone — `reps` launches back to back over the
// prefix, between two events on the space's stream, behind the upload of the expression and one warm launch; *out_ms = the
// mean of one launch (0 for an empty space), *out_n the snapshot
int ehx_test_filter_build_ms(ehx_space* s, const ehx_filters* filters, uint32_t reps, float* out_ms, uint64_t* out_n) {
  if (!out_ms || !reps) return fail(EHX_EINVAL, "NULL argument");
  *out_ms = 0.f;
  return filter_hook(s, "ehx_test_filter_build_ms", filters, out_n, [&](uint64_t n_pub, uint64_t words, uint32_t* dst, hipStream_t st) -> int {
    const std::shared_ptr<const PackedFilters> pk = pack_filters(filters);   // (the counts the warm launch was given)
    const WhereCols cols = where_cols(s, pk->clauses.data(), pk->n_clauses);
    Event e0, e1;   // (the hook's own, gone with it)
    if (int rc = e0.ensure()) return rc;
    if (int rc = e1.ensure()) return rc;
    HIP_TRY(hipEventRecord(e0, st));
    for (uint32_t i = 0; i < reps; ++i)
      HIP_TRY(launch_filter_bitmaps(cols, s->masked.dFilter.p, pk->n_clauses, pk->n_values, pk->n_filters, n_pub, words, dst, st));
    HIP_TRY(hipEventRecord(e1, st));
    HIP_TRY(hipEventSynchronize(e1));
    HIP_TRY(hipEventElapsedTime(out_ms, e0, e1));
    *out_ms /= (float)reps;
    return EHX_OK;
  });
}

}  // extern "C"
