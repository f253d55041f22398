// Grouped kNN under a label column: ehx_knn_grouped_labeled (host pointers) and ehx_knn_grouped_labeled_device, and over
// stored columns ehx_knn_grouped_by_label*.  Two columns under one length: group_of[r] the entity a row belongs to
// (EHX_GROUP_NONE: a group of its own), label_of[r] the partition — tenant, namespace, collection — it lies in; want[i] the
// partition query i is confined to.  FILTER FIRST, THEN CAP: the first k ELIGIBLE rows among the rows r < n_eff = min(the
// call's ONE snapshot of the row count, n_labels) with label_of[r] == want[i], in (canonical distance, id) order; such a row
// is eligible iff its group is EHX_GROUP_NONE or fewer than per_group rows OF THE SAME PARTITION and group precede it.  Row i
// of the answer is, byte for byte, ehx_knn_grouped_masked_device's for query i alone under the bitmap of its partition
// (include/ehx.h has the contract, k_grouped.hip's header why the answer is exact).  The search is the grouped kNN's
// (grouped_answer, ehx_grouped.cpp: routes, order of the queries, hand-ons, counters); this file keeps what a label column
// adds.  The number of distinct wanted labels is not limited: a call is served in device batches of kSideChunk queries, and
// per batch
//   compaction   the label search's (labeled_plan, ehx_labeled.cpp; a stored column: colindex_plan, read from its index): the
//                batch's distinct wanted labels ("slots"), per slot its rows and its list in masked.dList, for the slots that
//                scan an ascending list and the column's copy behind the head of labeled.dBlock
//   routing      the one rule (filter_routes_cut / _gate, ehx_masked.cpp) with grouped_scan_serves on the prefix, the cut
//                masked_exact_cut(rows) — CARRIED OVER from the bitmap search, not measured for this call — and the gate
//                kLargeKMinQueries, decided by the plan BEFORE the lists are filled: where no slot scans, the batch pays
//                for no tile prefix, no column copy and no second wait.  At most 127 slots can scan (ehx_labeled.cpp).
//   the flush    "the row's label is the query's" (allow_label: the head of the block is every query's wanted label)
// Waits: the device form reads d_want back (one wait for the whole call, the outputs unwritten until then), then per device
// batch the compaction's — once for the counts, a second time only where some slot scans — and radius_knn's one verdict.
// Entry scaffold, host staging: ehx_call.cpp's (search_on_device, HostStage).
#include "ehx_internal.h"

namespace {

constexpr const char* kLabeledGroupedWhy = "filtered grouped search over shards is not built yet";
static_assert(kTabWords == kLabelHead, "the head of the label block holds a word per query of a device batch");

// the union of ehx_knn_grouped_masked's and ehx_knn_labeled's checks, with their codes and in their order
int groupedl_check(const ehx_space* s, size_t nq, uint32_t k, uint32_t per_group, const void* q, const void* group_of,
                   const void* label_of, uint64_t n_labels, const void* want, const void* o_ids, const void* o_dist,
                   const void* o_cnt) {
  if (int rc = grouped_check_head(s, nq, k, per_group, q, group_of, n_labels, o_ids, o_dist, o_cnt)) return rc;
  if (n_labels && !label_of) return fail(EHX_EINVAL, "NULL label_of with n_labels = %llu", (unsigned long long)n_labels);
  if (!want) return fail(EHX_EINVAL, "NULL want");
  return check_batch_size(nq);
}

// ehx_knn_grouped_by_label*: the same checks with their codes and in their order (the columns are the space's: no pointers,
// no length), then the column numbers
int grouped_by_label_check(const ehx_space* s, size_t nq, uint32_t k, uint32_t per_group, const void* q, uint32_t group_col,
                           uint32_t label_col, const void* want, const void* o_ids, const void* o_dist, const void* o_cnt) {
  if (int rc = groupedl_check(s, nq, k, per_group, q, nullptr, nullptr, 0, want, o_ids, o_dist, o_cnt)) return rc;
  if (group_col >= EHX_MAX_COLUMNS || label_col >= EHX_MAX_COLUMNS)
    return fail(EHX_EINVAL, "group_col = %u, label_col = %u: a space has %u columns", group_col, label_col, (unsigned)EHX_MAX_COLUMNS);
  return EHX_OK;
}

// The label search's body (labeled_call, ehx_labeled.cpp: its contract) with the grouped search's routing inputs, and what a
// group column adds.  group_of / label_of: at least min(n_labels, row count) entries each, in host memory (cols_on_host:
// staged in grouped.dLabels and labeled.dCol) or on the device — or, with label_col >= 0, the space's stored columns
// group_col and label_col over the whole prefix; want / d_want: labeled_call's
int groupedl_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, uint32_t per_group,
                    const uint32_t* group_of, const uint32_t* label_of, bool cols_on_host, uint64_t n_labels,
                    const uint32_t* want, const uint32_t* d_want, const ResultBlock& out, int group_col = -1, int label_col = -1) {
  // the ONE read of the row count: the lists name rows below it only, and every later stage sees at least this prefix
  const uint64_t n_pub = s->n.load(std::memory_order_acquire);
  const uint64_t n_eff = label_col >= 0 ? n_pub : std::min<uint64_t>(n_labels, n_pub);
  LabelCall c = {label_of, cols_on_host, label_col, n_eff, want, d_want};
  // routing: the grouped search's under bitmaps (ehx_groupedm.cpp), applied by the plan before it fills the lists
  c.scan_serves = grouped_scan_serves(s, n_eff);
  c.cut = masked_exact_cut(n_pub);
  c.min_scan_queries = kLargeKMinQueries;
  c.fits = grouped_check_ld;
  c.ctr = s->groupedl_ctr;
  const uint32_t* d_group_of = group_of;
  auto stage = [&]() -> int {   // the group column: a stored one resolved, a host one staged
    if (label_col >= 0) return column_as_groups(s, st, (uint32_t)group_col, n_pub, &d_group_of);
    if (!cols_on_host) return EHX_OK;
    if (int rc = s->grouped.dLabels.ensure(std::max<uint64_t>(n_eff, 1))) return rc;
    // (as labeled_call stages the label column: the prefix alone, pageable host memory)
    if (n_eff) HIP_TRY(hipMemcpyAsync(s->grouped.dLabels.p, group_of, n_eff * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    d_group_of = s->grouped.dLabels.p;
    return EHX_OK;
  };
  return labeled_call(s, st, n_pub, nq, c, stage, [&](size_t q0, size_t m, FilterView& v) {
    return grouped_answer(s, st, m, d_queries + q0 * s->dims, k, per_group, d_group_of, v, out.from(q0, m));
  });
}

}  // namespace

extern "C" {

int ehx_knn_grouped_labeled_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                   uint32_t per_group, const uint32_t* d_group_of, const uint32_t* d_label_of,
                                   uint64_t n_labels, const uint32_t* d_want, uint64_t* d_out_ids, float* d_out_dist,
                                   uint32_t* d_out_count) {
  if (int rc = groupedl_check(s, n_queries, k, per_group, d_queries, d_group_of, d_label_of, n_labels, d_want, d_out_ids,
                              d_out_dist, d_out_count))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_knn_grouped_labeled_device", kLabeledGroupedWhy, n_queries, &st, [&] {
    return groupedl_locked(s, st, n_queries, d_queries, k, per_group, d_group_of, d_label_of, false, n_labels, nullptr, d_want,
                           ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_knn_grouped_labeled(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint32_t per_group,
                            const uint32_t* group_of, const uint32_t* label_of, uint64_t n_labels, const uint32_t* want,
                            uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (int rc = groupedl_check(s, n_queries, k, per_group, queries, group_of, label_of, n_labels, want, out_ids, out_dist,
                              out_count))
    return rc;
  return search_on_device(s, "ehx_knn_grouped_labeled", kLabeledGroupedWhy, n_queries, nullptr, [&]() -> int {
    int rc;
    HostStage& h = s->grouped.host;
    if ((rc = h.up(s->stream, queries, n_queries, s->dims, k, false))) return rc;
    if ((rc = groupedl_locked(s, s->stream, n_queries, h.q, k, per_group, group_of, label_of, true, n_labels, want, nullptr,
                              h.out)))
      return rc;
    return h.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
  });
}

int ehx_knn_grouped_by_label_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                    uint32_t per_group, uint32_t group_col, uint32_t label_col, const uint32_t* d_want,
                                    uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count) {
  if (int rc = grouped_by_label_check(s, n_queries, k, per_group, d_queries, group_col, label_col, d_want, d_out_ids, d_out_dist,
                                      d_out_count))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_knn_grouped_by_label_device", kLabeledGroupedWhy, n_queries, &st, [&] {
    return groupedl_locked(s, st, n_queries, d_queries, k, per_group, nullptr, nullptr, false, 0, nullptr, d_want,
                           ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k}, (int)group_col, (int)label_col);
  });
}

int ehx_knn_grouped_by_label(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint32_t per_group,
                             uint32_t group_col, uint32_t label_col, const uint32_t* want, uint64_t* out_ids, float* out_dist,
                             uint32_t* out_count) {
  if (int rc = grouped_by_label_check(s, n_queries, k, per_group, queries, group_col, label_col, want, out_ids, out_dist, out_count))
    return rc;
  return search_on_device(s, "ehx_knn_grouped_by_label", kLabeledGroupedWhy, n_queries, nullptr, [&]() -> int {
    int rc;
    HostStage& h = s->grouped.host;   // (queries up, results down: no column travels)
    if ((rc = h.up(s->stream, queries, n_queries, s->dims, k, false))) return rc;
    if ((rc = groupedl_locked(s, s->stream, n_queries, h.q, k, per_group, nullptr, nullptr, false, 0, want, nullptr, h.out,
                              (int)group_col, (int)label_col)))
      return rc;
    return h.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
  });
}

// test hook, not part of the ABI: queries answered on the scan route, on the list route (by the gate or handed on by the
// scan route), of those the ones whose pool overflowed, scan passes launched, calls
void ehx_test_grouped_labeled_counters(ehx_space* s, uint64_t out[5]) {
  for (int i = 0; i < 5; ++i) out[i] = s ? s->groupedl_ctr[i].load(std::memory_order_relaxed) : 0;
}

}  // extern "C"
