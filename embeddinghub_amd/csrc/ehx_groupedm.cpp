// Grouped kNN under row bitmaps: ehx_knn_grouped_masked (host pointers) and ehx_knn_grouped_masked_device, query i under
// bitmap mask_of[i] of a table (one bitmap is a table of one).  FILTER FIRST, THEN CAP: the first k ELIGIBLE rows among the
// ALLOWED rows of the prefix n_eff = min(the call's ONE snapshot of the row count, n_labels, n_bits) in (canonical distance,
// id) order; an allowed row is eligible iff its label is EHX_GROUP_NONE or fewer than per_group ALLOWED rows of its label
// precede it (include/ehx.h has the contract, k_grouped.hip's header why the answer is exact).  The search is the grouped
// kNN's (grouped_answer, ehx_grouped.cpp: routes, order of the queries, hand-ons, counters); this file keeps what a table
// of bitmaps adds:
//   compaction   the bitmap search's (masked_plan, ehx_masked.cpp) at min(n_bits, n_labels) bits: the row count read once,
//                the bitmaps on the device, every mask's number of allowed rows and its ascending list, mask_of checked;
//                bitmaps that cover no row compact to nothing: every query's range is empty, its page still written
//   routing      per mask, the one rule (filter_routes_cut / _gate, ehx_masked.cpp): grouped_scan_serves on the prefix, the
//                cut masked_exact_cut(rows), the gate kLargeKMinQueries (one query tile of the int8 wave tile)
//   the flush    the batch's one bitmap, or a bitmap per query through the offset words at the head of masked.dBlock
// Entry scaffold, host staging: ehx_call.cpp's (search_on_device, HostStage).
#include "ehx_internal.h"

namespace {

constexpr const char* kFilteredGroupedWhy = "filtered grouped search over shards is not built yet";

}  // namespace

namespace ehx_impl {

int groupedm_check(const ehx_space* s, size_t nq, uint32_t k, uint32_t per_group, const void* q, const void* group_of,
                   uint64_t n_labels, const void* masks, uint32_t n_masks, uint64_t n_bits, const void* mask_of,
                   const void* o_ids, const void* o_dist, const void* o_cnt) {
  int rc = grouped_check_head(s, nq, k, per_group, q, group_of, n_labels, o_ids, o_dist, o_cnt);
  if (rc) return rc;
  if (n_bits && !masks) return fail(EHX_EINVAL, "NULL mask with n_bits = %llu", (unsigned long long)n_bits);
  if ((rc = check_batch_size(nq))) return rc;
  if (nq == 0) return EHX_OK;
  if (n_masks == 0) return fail(EHX_EINVAL, "n_masks is 0 with %zu queries", nq);
  if (n_masks > kMaskedMaxMasks) return fail(EHX_EUNSUPPORTED, "n_masks=%u exceeds %u", n_masks, kMaskedMaxMasks);
  if (n_masks > 1 && !mask_of) return fail(EHX_EINVAL, "NULL mask_of");
  return EHX_OK;
}

// an unsharded space, locked shared, scratch_mu held, its device current; everything is enqueued on `st`.  group_of: at least
// min(n_labels, row count) labels, in host memory (labels_on_host: staged in grouped.dLabels) or on the device; mask_of /
// d_mask_of: masked_plan's
int groupedm_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, uint32_t per_group,
                    const uint32_t* group_of, bool labels_on_host, uint64_t n_labels, const MaskTable& tab, uint64_t n_bits,
                    const uint32_t* mask_of, const uint32_t* d_mask_of, const ResultBlock& out) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  if ((rc = grouped_check_ld(s))) return rc;   // (before anything is enqueued)
  s->groupedm_ctr[4] += 1;
  // a row at or above n_labels is not allowed, as one at or above n_bits: the bitmaps are compacted below both (and below
  // the plan's ONE read of the row count)
  MaskedPlan p;
  if ((rc = masked_plan(s, st, tab, std::min(n_bits, n_labels), nq, mask_of, d_mask_of, &p))) return rc;
  const uint64_t n_eff = p.n_eff;
  const uint32_t* d_group_of = group_of;
  if (labels_on_host) {
    if ((rc = s->grouped.dLabels.ensure(std::max<uint64_t>(n_eff, 1)))) return rc;
    // (masked_plan has ordered `st` behind the earlier calls that may still read the labels; pageable host memory: the
    // runtime stages it before the call returns)
    if (n_eff) HIP_TRY(hipMemcpyAsync(s->grouped.dLabels.p, group_of, n_eff * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    d_group_of = s->grouped.dLabels.p;
  }
  // routing per mask; fewer scanning queries than one query tile of the int8 wave tile: the list route for all
  char scans[kMaskedMaxMasks];
  uint32_t head_of[kMaskedMaxMasks];
  filter_routes_cut(grouped_scan_serves(s, n_eff), masked_exact_cut(p.n_pub), p.n_allowed.data(), p.n_masks, scans);
  filter_routes_gate(p.mask_of, nq, kLargeKMinQueries, p.n_masks, scans);
  FilterView v = masked_view(s, st, p, scans, head_of);
  v.ctr = s->groupedm_ctr;
  return grouped_answer(s, st, nq, d_queries, k, per_group, d_group_of, v, out);
}

}  // namespace ehx_impl

extern "C" {

int ehx_knn_grouped_masked_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                  uint32_t per_group, const uint32_t* d_group_of, uint64_t n_labels, const uint32_t* d_masks,
                                  uint32_t n_masks, uint64_t n_bits, const uint32_t* d_mask_of, uint64_t* d_out_ids,
                                  float* d_out_dist, uint32_t* d_out_count) {
  if (int rc = groupedm_check(s, n_queries, k, per_group, d_queries, d_group_of, n_labels, d_masks, n_masks, n_bits, d_mask_of,
                              d_out_ids, d_out_dist, d_out_count))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_knn_grouped_masked_device", kFilteredGroupedWhy, n_queries, &st, [&] {
    const MaskTable tab = {d_masks, (n_bits + 31) / 32, n_masks, false};
    return groupedm_locked(s, st, n_queries, d_queries, k, per_group, d_group_of, false, n_labels, tab, n_bits, nullptr,
                           d_mask_of, ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_knn_grouped_masked(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint32_t per_group,
                           const uint32_t* group_of, uint64_t n_labels, const uint32_t* masks, uint32_t n_masks,
                           uint64_t n_bits, const uint32_t* mask_of, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (int rc = groupedm_check(s, n_queries, k, per_group, queries, group_of, n_labels, masks, n_masks, n_bits, mask_of, out_ids,
                              out_dist, out_count))
    return rc;
  if (mask_of)
    if (int rc = check_mask_of(mask_of, n_queries, n_masks)) return rc;   // (before anything is enqueued)
  return search_on_device(s, "ehx_knn_grouped_masked", kFilteredGroupedWhy, n_queries, nullptr, [&]() -> int {
    int rc;
    HostStage& h = s->grouped.host;
    if ((rc = h.up(s->stream, queries, n_queries, s->dims, k, false))) return rc;
    const MaskTable tab = {masks, (n_bits + 31) / 32, n_masks, true};
    if ((rc = groupedm_locked(s, s->stream, n_queries, h.q, k, per_group, group_of, true, n_labels, tab, n_bits, mask_of,
                              nullptr, h.out)))
      return rc;
    return h.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
  });
}

// test hook, not part of the ABI: queries answered on the scan route, on the list route (by the gate or handed on by the
// scan route), of those the ones whose pool overflowed, scan passes launched, calls
void ehx_test_grouped_masked_counters(ehx_space* s, uint64_t out[5]) {
  for (int i = 0; i < 5; ++i) out[i] = s ? s->groupedm_ctr[i].load(std::memory_order_relaxed) : 0;
}

}  // extern "C"
