// Grouped kNN under row bitmaps: ehx_knn_grouped_masked (host pointers) and ehx_knn_grouped_masked_device, query i under
// bitmap mask_of[i] of a table (one bitmap is a table of one).  FILTER FIRST, THEN CAP: the first k ELIGIBLE rows among the
// ALLOWED rows of the prefix n_eff = min(the call's ONE snapshot of the row count, n_labels, n_bits) in (canonical distance,
// id) order; an allowed row is eligible iff its label is EHX_GROUP_NONE or fewer than per_group ALLOWED rows of its label
// precede it (include/ehx.h has the contract, k_groupedm.hip's header why the answer is exact).
//   compaction   the bitmap search's (masked_plan, ehx_masked.cpp) at min(n_bits, n_labels) bits: the row count read once,
//                the bitmaps on the device, every mask's number of allowed rows and its ascending list, mask_of checked
//   routing      per query through its mask; the queries are ordered scan route first, then by mask (SubsetBufs: gathered,
//                answered, scattered back; skipped when they come in that order)
//   scan route   masks of more than masked_exact_cut(rows) allowed rows on a flat space with plain rows whose int8 scan
//                serves a radius on the prefix, rows of at most grouped_rerank_max_ld() floats, at least kLargeKMinQueries
//                such queries: the falling-radius kNN (radius_knn, ehx_call.cpp) with the bitmap in the int8 scan's flush —
//                the batch's one bitmap, or a bitmap per query through the offset words at the head of masked.dBlock — and
//                grouped_rerank_kernel as its re-rank.  Seed: every query's pool takes a strided-by-rank sample of at most
//                kLargeKSample ids of ITS OWN mask's list (grouped_list_seed_kernel).  Passes: largek_passes(n_eff, growth),
//                the unfiltered grouped search's: a pass never lets more hits through than that search would under the same
//                radius.  (Passes cut by allowed rows seen, as the bitmap kNN's: a follow-up.)
//   list route   everything else — graph spaces (from their stored rows), small spaces, SCAN_F32 / SCAN_F16, small batches,
//                masks at or below the cut — and the queries the scan hands on, under their own mask: grouped_exact's loop
//                with each slab drawn from the mask's list (grouped_list_slab_kernel).  Slab b of a query is entries
//                [b kPoolCap, (b + 1) kPoolCap) of its mask's list, what remains of it, possibly nothing; the loop runs the
//                slabs of the longest list of the device batch, queries of different masks in ONE launch per slab.
// Entry scaffold, host staging, sub-batch re-runs: ehx_call.cpp's (search_on_device, HostStage, SubsetBufs::rerun).
#include "ehx_internal.h"

namespace {

constexpr const char* kGroupedMaskedWhy = "filtered grouped search over shards is not built yet";

// The list route for nq queries, query i under mask gm[i] (host memory) of the plan: any space kind.  count_queries: its
// queries are not in n_queries yet.
int groupedm_list(ehx_space* s, hipStream_t st, const MaskedPlan& p, const uint32_t* gm, size_t nq, const float* d_queries,
                  uint32_t k, uint32_t per_group, const uint32_t* d_group_of, uint64_t* d_ids, float* d_dist, uint32_t* d_count,
                  bool count_queries) {
  ehx_space::Grouped& w = s->grouped;
  ehx_space::GroupedMasked& gw = s->groupedm;
  const size_t cap = std::min(kSideChunk, nq);
  int rc;
  if ((rc = s->scr.dQ.ensure(cap * s->ld)) || (rc = w.dPool.ensure(cap * kPoolCap)) || (rc = w.dCtl.ensure(2 * cap)) ||
      (rc = w.exact.dTop.ensure(cap * kLargeKMax)) || (rc = w.exact.dTopCnt.ensure(cap)) || (rc = w.exact.dRadius.ensure(cap)) ||
      (rc = w.exact.dWork.ensure(cap)) || (rc = gw.dMaskAt.ensure(cap)))
    return rc;
  uint64_t n_listed = 0;
  for (size_t q0 = 0; q0 < nq; q0 += kSideChunk) {
    const size_t m = std::min(kSideChunk, nq - q0);
    uint64_t longest = 0;
    for (size_t j = 0; j < m; ++j) {
      longest = std::max(longest, p.n_allowed[gm[q0 + j]]);
      n_listed += p.n_allowed[gm[q0 + j]];
    }
    const uint64_t n_slabs = std::max<uint64_t>(1, (longest + kPoolCap - 1) / kPoolCap);   // (no row: one empty slab writes the page)
    // (searches on other streams have read and written this scratch; this batch's fence makes a Set that rewrites rows in
    // place wait for it in turn)
    if ((rc = wait_searches_in_flight(s, st))) return rc;
    if ((rc = s->clock.begin(st, BatchClock::kOutOfRing))) return rc;
    HIP_TRY(hipMemsetAsync(w.dCtl.p, 0, 2 * m * sizeof(uint32_t), st));
    // (pageable host memory: the runtime stages it before the call returns)
    HIP_TRY(hipMemcpyAsync(gw.dMaskAt.p, gm + q0, m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(launch_prep_queries(d_queries + q0 * s->dims, (uint32_t)m, s->dims, s->ld, (uint32_t)m, s->metric, s->scr.dQ.p, st));
    GroupedRerankArgs g = {};
    g.group_of = d_group_of;
    g.per_group = per_group;
    RadiusRerankArgs& r = g.r;
    r.Q = s->scr.dQ.p;
    r.rows = rows_view(s, p.n_eff);
    r.radius = w.exact.dRadius.p;
    r.pool = w.dPool.p;
    r.pool_cnt = w.dCtl.p;
    r.ovf = w.dCtl.p + m;
    r.top = w.exact.dTop.p;
    r.top_cnt = w.exact.dTopCnt.p;
    r.work = w.exact.dWork.p;
    r.out_ids = d_ids + q0 * k;
    r.out_dist = d_dist + q0 * k;
    r.out_count = d_count + q0;
    r.nq = (uint32_t)m;
    r.k = k;
    if ((rc = s->clock.scan_begin(st))) return rc;
    for (uint64_t b = 0; b < n_slabs; ++b) {
      if (p.n_tiles)
        HIP_TRY(launch_grouped_list_slab(s->masked.dList.p, p.off, s->masked.dCum.p, p.n_tiles, gw.dMaskAt.p, b, b == 0, w.dPool.p,
                                         w.dCtl.p, r.radius, r.top_cnt, r.work, (uint32_t)m, st));
      else   // (the bitmaps cover no row: nothing was compacted — the grouped kNN's empty slab)
        HIP_TRY(launch_grouped_slab(w.dPool.p, w.dCtl.p, (uint32_t)m, 0, 0, true, r.radius, r.top_cnt, r.work, st));
      r.mode = b + 1 == n_slabs ? kRadiusLast : kRadiusPass;
      HIP_TRY(launch_grouped_rerank(g, st));
    }
    if ((rc = s->clock.scan_end(st)) || (rc = s->clock.finish(st))) return rc;
  }
  if (count_queries) s->n_queries += nq;
  s->n_dist += n_listed;
  return EHX_OK;
}

}  // namespace

namespace ehx_impl {

int groupedm_check(const ehx_space* s, size_t nq, uint32_t k, uint32_t per_group, const void* q, const void* group_of,
                   uint64_t n_labels, const void* masks, uint32_t n_masks, uint64_t n_bits, const void* mask_of,
                   const void* o_ids, const void* o_dist, const void* o_cnt) {
  if (!s) return fail(EHX_EINVAL, "space is NULL");   // (before the device is looked for)
  int rc = ehx_init(nullptr, 0);   // (no device: EHX_ENODEVICE, whatever else is wrong with the call)
  if (rc) return rc;
  if (k == 0) return fail(EHX_EINVAL, "k is 0");
  if (per_group == 0) return fail(EHX_EINVAL, "per_group is 0");
  if (k > EHX_MAX_K_GROUPED) return fail(EHX_EUNSUPPORTED, "k=%u exceeds %u", k, EHX_MAX_K_GROUPED);
  if (!(o_ids && o_dist && o_cnt && (!nq || q))) return fail(EHX_EINVAL, "NULL argument");
  if (n_labels && !group_of) return fail(EHX_EINVAL, "NULL group_of with n_labels = %llu", (unsigned long long)n_labels);
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
  if (s->ld > grouped_rerank_max_ld())   // (before anything is enqueued)
    return fail(EHX_EUNSUPPORTED, "grouped search keeps a prepared query in LDS: rows of %u floats exceed %u", s->ld,
                grouped_rerank_max_ld());
  s->groupedm_ctr[4] += 1;
  ehx_space::GroupedMasked& w = s->groupedm;
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
  const uint32_t n_masks = p.n_masks;
  const bool per_query = n_masks > 1;   // one mask: the batch's ONE bitmap in the flush, no offsets
  // routing, and the order the queries are answered in: the scan route's first, then by mask
  const bool scan_serves = s->params.mode != EHX_MODE_GRAPH && !s->x_perm && n_eff > 0 && i8_serves_radius(s, n_eff);
  bool scans[kMaskedMaxMasks];
  for (uint32_t m = 0; m < n_masks; ++m) scans[m] = scan_serves && p.n_allowed[m] > masked_exact_cut(p.n_pub);
  auto mask_at = [&](size_t i) { return p.mask_of ? p.mask_of[i] : 0u; };
  size_t n_scan = 0;
  for (size_t i = 0; i < nq; ++i) n_scan += scans[mask_at(i)];
  if (n_scan < kLargeKMinQueries) {   // (fewer than one query tile of the int8 wave tile: the list route for all)
    for (uint32_t m = 0; m < n_masks; ++m) scans[m] = false;
    n_scan = 0;
  }
  auto place = [&](uint32_t i) { return (scans[mask_at(i)] ? 0u : kMaskedMaxMasks) + mask_at(i); };
  std::vector<uint32_t> idx(nq), gm(nq);   // gm: the mask of every query in that order
  for (size_t i = 0; i < nq; ++i) idx[i] = (uint32_t)i;
  auto before = [&](uint32_t a, uint32_t b) { return place(a) < place(b); };
  const bool in_order = std::is_sorted(idx.begin(), idx.end(), before);   // (one mask: always)
  if (!in_order) std::stable_sort(idx.begin(), idx.end(), before);
  for (size_t i = 0; i < nq; ++i) gm[i] = mask_at(idx[i]);
  if ((rc = w.dMaskAt.ensure(std::min(kSideChunk, nq)))) return rc;   // (sized once: both routes upload into it)

  auto list = [&](const uint32_t* of, size_t n, const float* q, uint64_t* ids, float* dist, uint32_t* cnt, bool count) {
    return groupedm_list(s, st, p, of, n, q, k, per_group, d_group_of, ids, dist, cnt, count);
  };
  auto answer = [&](size_t, const float* gq, uint64_t* ids, float* dist, uint32_t* cnt) -> int {
    if (n_scan) {
      RadiusKnn c;
      c.passes = largek_passes(n_eff, env().largek_growth);
      c.allow = per_query ? s->masked.dBlock.p : p.d_maps;
      c.allow_bits = (uint32_t)n_eff;
      c.allow_per_query = per_query;
      c.out = ResultBlock{ids, dist, cnt, nullptr, n_scan, k};
      std::vector<uint32_t> offs(per_query ? kTabWords : 0);
      // stage 0 of a device batch [q0, q0 + m): with several masks its queries' word offsets into the block; the mask of
      // every query, and from its list the sample in the query's pool
      c.fill_pool = [&](size_t q0, size_t m, uint64_t* pool, uint32_t* pool_cnt) -> int {
        if (per_query) {
          for (size_t j = 0; j < kTabWords; ++j)   // (padding queries: any bitmap, they collect nothing)
            offs[j] = (uint32_t)(kTabWords + (uint64_t)gm[q0 + std::min(j, m - 1)] * p.words);
          HIP_TRY(hipMemcpyAsync(s->masked.dBlock.p, offs.data(), kTabWords * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        }
        // (pageable host memory: the runtime stages it before the call returns)
        HIP_TRY(hipMemcpyAsync(w.dMaskAt.p, gm.data() + q0, m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(launch_grouped_list_seed(s->masked.dList.p, p.off, s->masked.dCum.p, p.n_tiles, w.dMaskAt.p, pool, pool_cnt,
                                         (uint32_t)m, st));
        return EHX_OK;
      };
      // The scan runs over the tiles that hold the prefix; the flush drops every row at or above n_eff with the rows the
      // bitmap excludes, and the re-rank reads no row (and no label) at or above it
      c.rerank = [&](const RadiusRerankArgs& r, hipStream_t on) {
        GroupedRerankArgs g = {r, d_group_of, per_group};
        g.r.rows.n_rows = n_eff;
        return launch_grouped_rerank(g, on);
      };
      // the flagged queries of a device batch, each under its own mask: ONE sub-batch on the list route
      c.handed = [&](size_t q0, const std::vector<uint32_t>& todo, const float* q, const ResultBlock& o) -> int {
        std::vector<uint32_t> of(todo.size());
        for (size_t i = 0; i < todo.size(); ++i) of[i] = gm[q0 + todo[i]];
        return w.scan.sub.rerun(
            s, st, q, todo, k,
            [&](size_t n, const float* sq, uint64_t* i2, float* d2, uint32_t* c2) {
              return list(of.data(), n, sq, i2, d2, c2, false);   // (the scan batch counted them)
            },
            o.ids, o.dist, o.cnt);
      };
      RadiusKnnTally t;
      const int r = radius_knn(s, st, w.scan, p.n_pub, gq, c, &t);
      for (uint64_t b = 0; b < t.batches; ++b)   // (the int8 scan copy: every query of a batch against every prefix row once)
        count_scan_batch(s, (size_t)std::min<uint64_t>(kSideChunk, t.queries - b * kSideChunk), n_eff, k, 1);
      s->n_i8_queries += t.queries;
      s->n_i8_fallback += t.handed;
      s->groupedm_ctr[0] += t.queries - t.handed;
      s->groupedm_ctr[1] += t.handed;
      s->groupedm_ctr[2] += t.overflowed;
      s->groupedm_ctr[3] += t.batches * c.passes.size();
      if (r) return r;
    }
    if (n_scan == nq) return EHX_OK;
    s->groupedm_ctr[1] += nq - n_scan;
    return list(gm.data() + n_scan, nq - n_scan, gq + n_scan * s->dims, ids + n_scan * k, dist + n_scan * k, cnt + n_scan, true);
  };
  if (in_order) return answer(nq, d_queries, out.ids, out.dist, out.cnt);
  return w.group.rerun(s, st, d_queries, idx, k, answer, out.ids, out.dist, out.cnt);
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
  return search_on_device(s, "ehx_knn_grouped_masked_device", kGroupedMaskedWhy, n_queries, &st, [&] {
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
  return search_on_device(s, "ehx_knn_grouped_masked", kGroupedMaskedWhy, n_queries, nullptr, [&]() -> int {
    int rc;
    HostStage& h = s->groupedm.host;
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
