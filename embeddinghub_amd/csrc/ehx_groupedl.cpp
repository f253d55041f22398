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
//   routing      the grouped search's under bitmaps, decided by the plan BEFORE the lists are filled: a slot scans iff the
//                space is flat with plain rows, its int8 scan serves a radius on the prefix, the slot has more than
//                masked_exact_cut(rows) rows and at least kLargeKMinQueries queries of the batch name such slots — otherwise
//                none scans, and the batch pays for no tile prefix, no column copy and no second wait.  At most 127 slots
//                can (ehx_labeled.cpp's argument).  The cut is CARRIED OVER from the bitmap search, not measured for this call.
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

// One device batch of m <= kSideChunk queries under want[0, m) (host memory) over the prefix of n_eff rows of both columns.
// *col_copied: the flush's copy of the label column is in place (made once per call, and only where some slot scans).
// ix: the label column is a stored one — the plan is read from its fresh index (colindex_plan: no launch, no wait), the
// lists are runs of its permutation and the flush's block is the index's.
int groupedl_batch(ehx_space* s, hipStream_t st, uint64_t n_pub, uint64_t n_eff, size_t m, const float* d_queries, uint32_t k,
                   uint32_t per_group, const uint32_t* d_group_of, const uint32_t* d_label_of, const ehx_space::ColIndex* ix,
                   const uint32_t* want, bool* col_copied, const ResultBlock& out) {
  int rc;
  // routing: the grouped search's under bitmaps (ehx_groupedm.cpp), applied by the plan before it fills the lists
  const bool scan_serves = s->params.mode != EHX_MODE_GRAPH && !s->x_perm && n_eff > 0 && i8_serves_radius(s, n_eff);
  LabeledPlan p;
  if (ix) colindex_plan(*ix, m, want, scan_serves, masked_exact_cut(n_pub), kLargeKMinQueries, &p);
  else if ((rc = labeled_plan(s, st, n_eff, m, d_label_of, want, scan_serves, masked_exact_cut(n_pub), kLargeKMinQueries, col_copied, &p)))
    return rc;
  uint32_t* d_block = ix ? ix->dBlock.p : s->labeled.dBlock.p;
  FilterView v;
  v.n_pub = n_pub;
  v.n_eff = n_eff;
  v.n_filters = p.n_slots;
  v.n_allowed = p.n_allowed.data();
  v.off = p.off.data();
  v.filter_of = p.slot_of.data();
  v.scans = p.scans.data();
  v.d_list = ix ? ix->dPerm.p : s->masked.dList.p;
  v.allow = d_block;
  v.allow_label = true;
  v.d_head = d_block;
  v.head_of = p.table.data();
  v.ctr = s->groupedl_ctr;
  return grouped_answer(s, st, m, d_queries, k, per_group, d_group_of, v, out);
}

// an unsharded space, locked shared, scratch_mu held, its device current; everything is enqueued on `st`.  group_of /
// label_of: at least min(n_labels, row count) entries each, in host memory (cols_on_host: staged in grouped.dLabels and
// labeled.dCol) or on the device; want: in host memory, or d_want, read back once (the outputs unwritten until then)
int groupedl_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, uint32_t per_group,
                    const uint32_t* group_of, const uint32_t* label_of, bool cols_on_host, uint64_t n_labels,
                    const uint32_t* want, const uint32_t* d_want, const ResultBlock& out, int group_col = -1, int label_col = -1) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  if ((rc = grouped_check_ld(s))) return rc;   // (before anything is enqueued)
  s->groupedl_ctr[4] += 1;
  // the ONE read of the row count: the lists name rows below it only, and every later stage sees at least this prefix
  const uint64_t n_pub = s->n.load(std::memory_order_acquire);
  const bool stored = label_col >= 0;   // ehx_knn_grouped_by_label*: both columns are the space's, over the whole prefix
  const uint64_t n_eff = stored ? n_pub : std::min<uint64_t>(n_labels, n_pub);   // (row ids are 32 bits wide: n_pub < 2^32)
  if (!stored && (rc = labeled_plan_scratch(s, n_eff))) return rc;
  // (earlier calls' launches on other streams may still read the block, the lists and the staged columns)
  if ((rc = wait_searches_in_flight(s, st))) return rc;
  const uint32_t *d_group_of = group_of, *d_label_of = label_of;
  const ehx_space::ColIndex* ix = nullptr;   // the label column's index, rebuilt here if a write or an append left it stale
  if (stored && ((rc = colindex_ensure(s, st, (uint32_t)label_col, n_pub, &ix)) ||
                 (rc = column_as_groups(s, st, (uint32_t)group_col, n_pub, &d_group_of))))
    return rc;
  if (cols_on_host) {
    if ((rc = s->grouped.dLabels.ensure(std::max<uint64_t>(n_eff, 1))) || (rc = s->labeled.dCol.ensure(std::max<uint64_t>(n_eff, 1))))
      return rc;
    // (labels at or above the prefix are never looked at: they are not even copied; pageable host memory: the runtime
    // stages it before the call returns)
    if (n_eff) {
      HIP_TRY(hipMemcpyAsync(s->grouped.dLabels.p, group_of, n_eff * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(s->labeled.dCol.p, label_of, n_eff * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    d_group_of = s->grouped.dLabels.p;
    d_label_of = s->labeled.dCol.p;
  }
  std::vector<uint32_t> want_read;
  if (!want) {
    want_read.resize(nq);
    HIP_TRY(hipMemcpyAsync(want_read.data(), d_want, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    want = want_read.data();
  }
  bool col_copied = false;
  for (size_t q0 = 0; q0 < nq; q0 += kSideChunk) {
    const size_t m = std::min(kSideChunk, nq - q0);
    if ((rc = groupedl_batch(s, st, n_pub, n_eff, m, d_queries + q0 * s->dims, k, per_group, d_group_of, d_label_of, ix,
                             want + q0, &col_copied, out.from(q0, m))))
      return rc;
  }
  return EHX_OK;
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
