// Exact range search under row bitmaps: ehx_range_masked (host pointers) and ehx_range_masked_device, query i under bitmap
// mask_of[i] of a table (one bitmap is a table of one).  Row r is allowed iff r < n_bits, r is below the call's ONE snapshot
// of the row count and bit r & 31 of word r >> 5 of the query's bitmap is set; the answer is every allowed row whose
// canonical distance is <= the query's radius, ordered by (distance, id), the first max_results written, all of them counted.
//   compaction   the bitmap search's (masked_plan, ehx_masked.cpp): the row count read once, the bitmaps on the device, every
//                mask's number of allowed rows and its ascending list of them, mask_of checked — one wait
//   routing      per device batch of kSideChunk queries, per query through its mask:
//   scan route   masks of more than masked_exact_cut(rows) allowed rows on a space whose int8 scan serves a radius: the
//                unfiltered range search's int8 stage (range_i8_stage, ehx_range.cpp) with the bitmap tested in the scan's
//                flush — the batch's one bitmap, or a bitmap per query through the offset words at the head of masked.dBlock
//                — over the tiles below n_bits.  ONE pass suffices, as it does unfiltered: the radius is fixed, so the
//                threshold is, and the survivors are allowed rows already.  The batch's other queries ride along under a NaN
//                radius, which collects nothing: one scan per device batch.
//   list route   every other query, and the scan route's flagged ones (pool overflow, a bound that does not serve the
//                radius): the canonical distance of every row of the mask's list (range_list_kernel, k_rangem.hip), each
//                slot of the launch with its own list — nothing is regrouped by mask.  A graph space answers from its stored
//                rows here; its graph is not walked.
//   overflow     a list-route query with more than kPoolCap members keeps its exact total and takes its rows from the exact
//                kNN among its mask's list at k = max_results (among_locked), per run of equal masks.
// The cut between the routes is the bitmap kNN's, measured for a k-th distance and not for a radius: a CARRIED-OVER choice.
// scripts/bench_range_masked.py has the routes cross at 0.29 % of 1 M x 768 against the cut's 0.78 %: a cut
// of its own is the follow-up, the kNN's constant is not changed here.
// Entry scaffold, host staging, sub-batch re-runs: ehx_call.cpp's (search_on_device, HostStage, SubsetBufs::rerun).
#include "ehx_internal.h"

namespace {

constexpr const char* kRangeMaskedWhy = "filtered range search over shards is not built yet";

// The list route for the queries sel[0, n) (ascending) of a device batch of m: slot j walks the list of its query's mask.
// counted[j] != 0: query sel[j]'s overflow is in the counters already.
int rangem_list_stage(ehx_space* s, hipStream_t st, const MaskedPlan& p, size_t q0, size_t m, const float* d_queries,
                      const float* d_radius, const std::vector<uint32_t>& sel, const std::vector<uint8_t>& counted,
                      uint32_t max_results, const ResultBlock& o) {
  ehx_space::RangeMasked& w = s->rangem;
  const size_t n = sel.size();
  const bool all = n == m;   // (ascending and distinct: every query, in order)
  auto mask_of = [&](uint32_t i) { return p.mask_of ? p.mask_of[q0 + i] : 0u; };
  int rc;
  if ((rc = s->scr.dQ.ensure(m * s->ld))) return rc;
  if ((rc = s->range.dPool.ensure(n * kPoolCap))) return rc;
  if ((rc = s->range.dCtl.ensure(n))) return rc;
  if (!all && (rc = s->range.dSel.ensure(n))) return rc;
  if ((rc = w.dListOff.ensure(n)) || (rc = w.dListLen.ensure(n))) return rc;
  std::vector<uint64_t> off(n);
  std::vector<uint32_t> len(n);
  uint64_t longest = 0, n_listed = 0;
  for (size_t j = 0; j < n; ++j) {
    const uint32_t mk = mask_of(sel[j]);
    off[j] = p.off.off[mk];
    len[j] = (uint32_t)p.n_allowed[mk];   // (at most the row count, which is below 2^32)
    longest = std::max<uint64_t>(longest, len[j]);
    n_listed += len[j];
  }
  // (searches on other streams have read and written this scratch; this batch's fence makes a Set that rewrites rows in
  // place wait for it in turn)
  if ((rc = wait_searches_in_flight(s, st))) return rc;
  if ((rc = s->clock.begin(st, BatchClock::kOutOfRing))) return rc;
  HIP_TRY(hipMemsetAsync(s->range.dCtl.p, 0, n * sizeof(uint32_t), st));
  // (pageable host memory: the runtime stages it before the call returns)
  if (!all) HIP_TRY(hipMemcpyAsync(s->range.dSel.p, sel.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w.dListOff.p, off.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w.dListLen.p, len.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HIP_TRY(launch_prep_queries(d_queries, (uint32_t)m, s->dims, s->ld, (uint32_t)m, s->metric, s->scr.dQ.p, st));
  RangeListArgs a = {};
  a.Q = s->scr.dQ.p;
  a.rows = rows_view(s, p.n_pub);
  a.radius = d_radius;
  a.sel = all ? nullptr : s->range.dSel.p;
  a.ids = s->masked.dList.p;
  a.list_off = w.dListOff.p;
  a.list_len = w.dListLen.p;
  a.pool = s->range.dPool.p;
  a.pool_cnt = s->range.dCtl.p;
  const uint32_t step = range_list_step_rows(a);
  a.n_blocks = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, (longest + step - 1) / step),
                                            std::max<uint64_t>(1, kRangeGridTarget / n));
  if ((rc = s->clock.scan_begin(st))) return rc;
  if (longest) HIP_TRY(launch_range_list(a, (uint32_t)n, st));   // (every list empty: the empty pools are the answer)
  HIP_TRY(launch_range_emit(s->range.dPool.p, s->range.dCtl.p, a.sel, (uint32_t)n, max_results, o.ids, o.dist, o.cnt, o.total,
                            st));
  if ((rc = s->clock.scan_end(st)) || (rc = s->clock.finish(st))) return rc;
  // the verdict: which pools overflowed (one copy, one wait)
  std::vector<uint32_t> cnt(n);
  HIP_TRY(hipMemcpyAsync(cnt.data(), s->range.dCtl.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  s->n_dist += n_listed;
  std::vector<uint32_t> over;
  uint64_t n_trunc = 0, n_over_new = 0;
  for (size_t j = 0; j < n; ++j) {
    n_trunc += cnt[j] > max_results;
    if (cnt[j] > kPoolCap) {
      over.push_back(sel[j]);
      n_over_new += !counted[j];
    }
  }
  s->rangem_ctr[1] += n;
  s->rangem_ctr[2] += n_over_new;
  s->rangem_ctr[3] += n_trunc;
  s->n_queries += n - over.size();   // (among_locked counts the queries it answers)
  if (over.empty()) return EHX_OK;
  // more than kPoolCap >= max_results members: the top max_results among the mask's list, per run of equal masks (the
  // totals are written already)
  std::stable_sort(over.begin(), over.end(), [&](uint32_t x, uint32_t y) { return mask_of(x) < mask_of(y); });
  for (size_t b = 0; b < over.size();) {
    const uint32_t mk = mask_of(over[b]);
    size_t e = b + 1;
    while (e < over.size() && mask_of(over[e]) == mk) ++e;
    const std::vector<uint32_t> part(over.begin() + b, over.begin() + e);
    if ((rc = w.sub.rerun(
             s, st, d_queries, part, max_results,
             [&](size_t nn, const float* sq, uint64_t* i2, float* d2, uint32_t* c2) {
               return among_locked(s, st, nn, sq, max_results, s->masked.dList.p + p.off.off[mk], nullptr, p.n_allowed[mk], 0,
                                   i2, d2, c2);
             },
             o.ids, o.dist, o.cnt)))
      return rc;
    b = e;
  }
  return EHX_OK;
}

}  // namespace

namespace ehx_impl {

int rangem_check(const ehx_space* s, size_t nq, uint32_t max_results, const void* q, const void* radius, const void* masks,
                 uint32_t n_masks, uint64_t n_bits, const void* mask_of, const void* o_ids, const void* o_dist,
                 const void* o_cnt) {
  int rc = ehx_init(nullptr, 0);   // (no device: EHX_ENODEVICE, whatever else is wrong with the call)
  if (rc) return rc;
  if ((rc = check_batch_call(s, nq, max_results, "max_results", false, o_ids && o_dist && o_cnt && (!nq || (q && radius)))))
    return rc;
  if (n_bits && !masks) return fail(EHX_EINVAL, "NULL mask with n_bits = %llu", (unsigned long long)n_bits);
  if (nq == 0) return EHX_OK;
  if (n_masks == 0) return fail(EHX_EINVAL, "n_masks is 0 with %zu queries", nq);
  if (n_masks > kMaskedMaxMasks) return fail(EHX_EUNSUPPORTED, "n_masks=%u exceeds %u", n_masks, kMaskedMaxMasks);
  if (n_masks > 1 && !mask_of) return fail(EHX_EINVAL, "NULL mask_of");
  return EHX_OK;
}

// an unsharded space, locked shared, scratch_mu held, its device current; everything is enqueued on `st` (mask_of /
// d_mask_of: masked_plan's)
int rangem_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, const float* d_radius, uint32_t max_results,
                  const MaskTable& tab, uint64_t n_bits, const uint32_t* mask_of, const uint32_t* d_mask_of,
                  const ResultBlock& out) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  if ((rc = check_rows_fit_lds(s, "filtered range search"))) return rc;   // (before anything is enqueued)
  s->rangem_ctr[4] += 1;
  MaskedPlan p;
  if ((rc = masked_plan(s, st, tab, n_bits, nq, mask_of, d_mask_of, &p))) return rc;
  ehx_space::RangeMasked& w = s->rangem;
  const bool per_query = p.n_masks > 1;   // one mask: the batch's ONE bitmap in the flush, no offsets
  // The cut is the bitmap kNN's (masked_exact_cut: measured for a k-th distance, profiles/masked_bench.jsonl) — for a radius
  // a CARRIED-OVER choice (the file header has what scripts/bench_range_masked.py measured).
  const uint32_t forced = s->rangem_route.load(std::memory_order_relaxed);   // (test hook: the bench's crossover sweep)
  const uint64_t cut = forced == 1u ? 0 : forced == 2u ? ~0ull : masked_exact_cut(p.n_pub);
  char scans[kMaskedMaxMasks];
  filter_routes_cut(i8_serves_radius(s, p.n_pub), cut, p.n_allowed.data(), p.n_masks, scans);
  std::vector<uint32_t> route, list, offs(per_query ? kTabWords : 0);
  std::vector<uint8_t> counted;
  for (size_t q0 = 0; q0 < nq; q0 += kSideChunk) {
    const size_t m = std::min(kSideChunk, nq - q0);
    const float* q = d_queries + q0 * s->dims;
    const float* r = d_radius + q0;
    const ResultBlock o = out.from(q0, m);
    auto mask_at = [&](size_t j) { return p.mask_of ? p.mask_of[q0 + j] : 0u; };
    route.assign(m, 0u);
    size_t n_scan = 0;
    for (size_t j = 0; j < m; ++j) n_scan += (route[j] = scans[mask_at(j)] ? 1u : 0u);
    list.clear();
    counted.clear();
    if (n_scan) {
      const float* scan_r = r;
      if (n_scan < m) {   // the other queries of the batch collect nothing: a NaN radius
        if ((rc = w.dRadius.ensure(m)) || (rc = w.dScans.ensure(m))) return rc;
        // (pageable host memory: the runtime stages it before the call returns; masked_plan has ordered `st` behind the
        // earlier calls that may still read these buffers and the block)
        HIP_TRY(hipMemcpyAsync(w.dScans.p, route.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(launch_range_scan_radii(r, w.dScans.p, (uint32_t)m, w.dRadius.p, st));
        scan_r = w.dRadius.p;
      }
      if (per_query) {   // the batch's word offsets into the block, in front of the scan
        for (size_t j = 0; j < kTabWords; ++j)   // (padding queries: any bitmap, they collect nothing)
          offs[j] = (uint32_t)(kTabWords + (uint64_t)mask_at(std::min(j, m - 1)) * p.words);
        HIP_TRY(hipMemcpyAsync(s->masked.dBlock.p, offs.data(), kTabWords * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      }
      // (rows at or above n_bits cannot be members: no tile beyond them is scanned)
      const RangeAllow al = {per_query ? s->masked.dBlock.p : p.d_maps, (uint32_t)p.n_eff, per_query, p.n_tiles};
      RangeI8Verdict v;
      if ((rc = range_i8_stage(s, st, p.n_pub, m, q, scan_r, max_results, o, &al, &v))) return rc;
      // (a NaN radius is never flagged: the flagged queries are the scan route's)
      const size_t n_answered = n_scan - v.todo.size();
      s->n_dist += v.n_pairs;
      s->n_queries += n_answered;
      s->rangem_ctr[0] += n_answered;
      s->rangem_ctr[2] += v.n_over;
      s->rangem_ctr[3] += v.n_trunc;
      for (size_t i = 0; i < v.todo.size(); ++i) route[v.todo[i]] = v.counted[i] ? 3u : 2u;
    }
    for (size_t j = 0; j < m; ++j) {
      if (route[j] == 1u) continue;
      list.push_back((uint32_t)j);
      counted.push_back(route[j] == 3u);
    }
    if (list.empty()) continue;
    if ((rc = rangem_list_stage(s, st, p, q0, m, q, r, list, counted, max_results, o))) return rc;
  }
  return EHX_OK;
}

}  // namespace ehx_impl

extern "C" {

int ehx_range_masked(ehx_space* s, size_t n_queries, const float* queries, const float* radius, uint32_t max_results,
                     const uint32_t* masks, uint32_t n_masks, uint64_t n_bits, const uint32_t* mask_of, uint64_t* out_ids,
                     float* out_dist, uint32_t* out_count, uint64_t* out_total) {
  if (int rc = rangem_check(s, n_queries, max_results, queries, radius, masks, n_masks, n_bits, mask_of, out_ids, out_dist,
                            out_count))
    return rc;
  if (mask_of)
    if (int rc = check_mask_of(mask_of, n_queries, n_masks)) return rc;   // (before anything is enqueued)
  return search_on_device(s, "ehx_range_masked", kRangeMaskedWhy, n_queries, nullptr, [&]() -> int {
    int rc;
    HostStage& h = s->rangem.host;
    if ((rc = h.up(s->stream, queries, n_queries, s->dims, max_results, true, n_queries))) return rc;
    float* d_r = h.q + n_queries * s->dims;
    HIP_TRY(hipMemcpyAsync(d_r, radius, n_queries * sizeof(float), hipMemcpyHostToDevice, s->stream));
    const MaskTable tab = {masks, (n_bits + 31) / 32, n_masks, true};
    if ((rc = rangem_locked(s, s->stream, n_queries, h.q, d_r, max_results, tab, n_bits, mask_of, nullptr, h.out))) return rc;
    return h.out.copy_out(s->stream, out_ids, out_dist, out_count, out_total);
  });
}

int ehx_range_masked_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, const float* d_radius,
                            uint32_t max_results, const uint32_t* d_masks, uint32_t n_masks, uint64_t n_bits,
                            const uint32_t* d_mask_of, uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count,
                            uint64_t* d_out_total) {
  if (int rc = rangem_check(s, n_queries, max_results, d_queries, d_radius, d_masks, n_masks, n_bits, d_mask_of, d_out_ids,
                            d_out_dist, d_out_count))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_range_masked_device", kRangeMaskedWhy, n_queries, &st, [&] {
    const MaskTable tab = {d_masks, (n_bits + 31) / 32, n_masks, false};
    return rangem_locked(s, st, n_queries, d_queries, d_radius, max_results, tab, n_bits, nullptr, d_mask_of,
                         ResultBlock{d_out_ids, d_out_dist, d_out_count, d_out_total, n_queries, max_results});
  });
}

// test hook, not part of the ABI: queries answered on the scan route, on the list route, queries whose pool overflowed,
// truncated answers, calls
void ehx_test_range_masked_counters(ehx_space* s, uint64_t out[5]) {
  for (int i = 0; i < 5; ++i) out[i] = s ? s->rangem_ctr[i].load(std::memory_order_relaxed) : 0;
}

// test hook, not part of the ABI: 0 the cut decides the route (the default), 1 the scan route for every non-empty mask where
// the int8 scan serves a radius, 2 the list route for every mask — how scripts/bench_range_masked.py finds where they cross
void ehx_test_range_masked_route(ehx_space* s, uint32_t route) {
  if (s) s->rangem_route.store(route <= 2u ? route : 0u, std::memory_order_relaxed);
}

}  // extern "C"
