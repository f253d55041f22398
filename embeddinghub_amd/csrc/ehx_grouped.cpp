// Grouped kNN: ehx_knn_grouped (host pointers) and ehx_knn_grouped_device.  The first k ELIGIBLE rows of the prefix
// n_eff = min(the call's ONE snapshot of the row count, n_labels) in (canonical distance, id) order; a row is eligible iff
// its label is EHX_GROUP_NONE or fewer than per_group rows of its label precede it in that order (include/ehx.h has the
// contract, k_grouped.hip's header the kernels and why the answer is exact).  The labels travel with the call, as a bitmap
// does: nothing is stored with the rows.
//   scan route   flat spaces whose int8 scan serves a radius on the prefix (i8_serves_radius), plain rows (no x_perm), rows
//                of at most grouped_rerank_max_ld() floats, batches of at least kLargeKMinQueries queries, any k <= 256: the
//                falling-radius kNN (radius_knn, ehx_call.cpp) with grouped_rerank_kernel as its re-rank.  Seed: the large-k
//                route's strided sample of <= kLargeKSample rows; passes: largek_passes(n_eff, growth); no bitmap.  The
//                queries it hands on — pool overflow, or a radius the bound does not serve: a sample that cannot reach k
//                groups leaves the radius at +Inf — take the
//   exact route  everything else (graph spaces, which answer from their stored rows; small spaces; SCAN_F32 / SCAN_F16;
//                small batches): grouped_slab_kernel and grouped_rerank_kernel in pass mode over consecutive slabs of
//                kPoolCap rows, the radius falling from +Inf, the last slab in last mode.  Every row's canonical distance is
//                computed once: the exhaustive pass's cost, plus one sort of a slab per query.
// Entry scaffold, host staging, sub-batch re-runs: ehx_call.cpp's (search_on_device, HostStage, SubsetBufs::rerun).
#include "ehx_internal.h"

namespace {

constexpr const char* kGroupedWhy = "grouped search over shards is not built yet";

int grouped_check(const ehx_space* s, size_t nq, uint32_t k, uint32_t per_group, const void* q, const void* group_of,
                  uint64_t n_labels, const void* o_ids, const void* o_dist, const void* o_cnt) {
  if (!s) return fail(EHX_EINVAL, "space is NULL");   // (before the device is looked for)
  int rc = ehx_init(nullptr, 0);   // (no device: EHX_ENODEVICE, whatever else is wrong with the call)
  if (rc) return rc;
  if (k == 0) return fail(EHX_EINVAL, "k is 0");
  if (per_group == 0) return fail(EHX_EINVAL, "per_group is 0");
  if (k > EHX_MAX_K_GROUPED) return fail(EHX_EUNSUPPORTED, "k=%u exceeds %u", k, EHX_MAX_K_GROUPED);
  if (!(o_ids && o_dist && o_cnt && (!nq || q))) return fail(EHX_EINVAL, "NULL argument");
  if (n_labels && !group_of) return fail(EHX_EINVAL, "NULL group_of with n_labels = %llu", (unsigned long long)n_labels);
  return check_batch_size(nq);
}
static_assert(EHX_MAX_K_GROUPED == kLargeKMax, "the re-rank carries one key per thread");
static_assert(EHX_GROUP_NONE == kGroupNone, "the header's label of a row that is a group of its own");

}  // namespace

namespace ehx_impl {

int grouped_exact(ehx_space* s, hipStream_t st, uint64_t n_eff, size_t nq, const float* d_queries, uint32_t k, uint32_t per_group,
                  const uint32_t* d_group_of, uint64_t* d_ids, float* d_dist, uint32_t* d_count, bool count_queries) {
  ehx_space::Grouped& w = s->grouped;
  const size_t cap = std::min(kSideChunk, nq);
  int rc;
  if ((rc = s->scr.dQ.ensure(cap * s->ld)) || (rc = w.dPool.ensure(cap * kPoolCap)) || (rc = w.dCtl.ensure(2 * cap)) ||
      (rc = w.exact.dTop.ensure(cap * kLargeKMax)) || (rc = w.exact.dTopCnt.ensure(cap)) || (rc = w.exact.dRadius.ensure(cap)) ||
      (rc = w.exact.dWork.ensure(cap)))
    return rc;
  const uint64_t n_slabs = std::max<uint64_t>(1, (n_eff + kPoolCap - 1) / kPoolCap);   // (no row: one empty slab writes the page)
  for (size_t q0 = 0; q0 < nq; q0 += kSideChunk) {
    const size_t m = std::min(kSideChunk, nq - q0);
    // (searches on other streams have read and written this scratch; this batch's fence makes a Set that rewrites rows in
    // place wait for it in turn)
    if ((rc = wait_searches_in_flight(s, st))) return rc;
    if ((rc = s->clock.begin(st, BatchClock::kOutOfRing))) return rc;
    HIP_TRY(hipMemsetAsync(w.dCtl.p, 0, 2 * m * sizeof(uint32_t), st));
    HIP_TRY(launch_prep_queries(d_queries + q0 * s->dims, (uint32_t)m, s->dims, s->ld, (uint32_t)m, s->metric, s->scr.dQ.p, st));
    GroupedRerankArgs g = {};
    g.group_of = d_group_of;
    g.per_group = per_group;
    RadiusRerankArgs& r = g.r;
    r.Q = s->scr.dQ.p;
    r.rows = rows_view(s, n_eff);
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
      const uint64_t row0 = b * kPoolCap;
      const uint32_t n = (uint32_t)std::min<uint64_t>(kPoolCap, n_eff - std::min(n_eff, row0));
      HIP_TRY(launch_grouped_slab(w.dPool.p, w.dCtl.p, (uint32_t)m, row0, n, b == 0, r.radius, r.top_cnt, r.work, st));
      r.mode = b + 1 == n_slabs ? kRadiusLast : kRadiusPass;
      HIP_TRY(launch_grouped_rerank(g, st));
    }
    if ((rc = s->clock.scan_end(st)) || (rc = s->clock.finish(st))) return rc;
  }
  if (count_queries) s->n_queries += nq;
  s->n_dist += (uint64_t)nq * n_eff;
  return EHX_OK;
}

}  // namespace ehx_impl

namespace {

// an unsharded space, locked shared, scratch_mu held, its device current; everything is enqueued on `st`.  n_pub: the call's
// ONE read of the row count; d_group_of: at least min(n_pub, n_labels) labels on the device
int grouped_locked(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const float* d_queries, uint32_t k,
                   uint32_t per_group, const uint32_t* d_group_of, uint64_t n_labels, const ResultBlock& out) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  if (s->ld > grouped_rerank_max_ld())   // (before anything is enqueued)
    return fail(EHX_EUNSUPPORTED, "grouped search keeps a prepared query in LDS: rows of %u floats exceed %u", s->ld,
                grouped_rerank_max_ld());
  s->grouped_ctr[4] += 1;
  const uint64_t n_eff = std::min(n_pub, n_labels);
  const bool scan = s->params.mode != EHX_MODE_GRAPH && !s->x_perm && nq >= kLargeKMinQueries && n_eff > 0 &&
                    i8_serves_radius(s, n_eff);
  if (!scan) {
    s->grouped_ctr[1] += nq;
    return grouped_exact(s, st, n_eff, nq, d_queries, k, per_group, d_group_of, out.ids, out.dist, out.cnt);
  }
  RadiusKnn c;
  c.passes = largek_passes(n_eff, env().largek_growth);
  c.seed_stride = (n_eff + kLargeKSample - 1) / kLargeKSample;
  c.n_sample = (uint32_t)((n_eff + c.seed_stride - 1) / c.seed_stride);
  c.out = out;
  c.exact = [&](size_t n, const float* sq, uint64_t* oi, float* od, uint32_t* oc) {
    return grouped_exact(s, st, n_eff, n, sq, k, per_group, d_group_of, oi, od, oc, false);   // (the scan batch counted them)
  };
  // The scan runs on the snapshot's rows — a row's place inside its tile of the scan copy is not its id's, so the copy cannot
  // be cut at a row count of its own — over the tiles that hold the prefix; the re-rank reads no row at or above n_eff, so
  // what the last of those tiles holds beyond the prefix never becomes a key (and its label is never looked up)
  c.rerank = [&](const RadiusRerankArgs& r, hipStream_t on) {
    GroupedRerankArgs g = {r, d_group_of, per_group};
    g.r.rows.n_rows = n_eff;
    return launch_grouped_rerank(g, on);
  };
  RadiusKnnTally t;
  rc = radius_knn(s, st, s->grouped.scan, n_pub, d_queries, c, &t);
  for (uint64_t b = 0; b < t.batches; ++b)   // (the int8 scan copy: every query of a batch against every row once)
    count_scan_batch(s, (size_t)std::min<uint64_t>(kSideChunk, t.queries - b * kSideChunk), n_eff, k, 1);
  s->n_i8_queries += t.queries;
  s->n_i8_fallback += t.handed;
  s->grouped_ctr[0] += t.queries - t.handed;
  s->grouped_ctr[1] += t.handed;
  s->grouped_ctr[2] += t.overflowed;
  s->grouped_ctr[3] += t.batches * c.passes.size();
  return rc;
}

// host pointers in, host pointers out, on the space's stream (on_device): the labels of the prefix staged in grouped.dLabels
int grouped_host_locked(ehx_space* s, size_t nq, const float* queries, uint32_t k, uint32_t per_group, const uint32_t* group_of,
                        uint64_t n_labels, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  int rc;
  ehx_space::Grouped& w = s->grouped;
  const uint64_t n_pub = s->n.load(std::memory_order_acquire);   // the ONE read of the row count
  const uint64_t n_eff = std::min(n_pub, n_labels);
  if ((rc = w.dLabels.ensure(std::max<uint64_t>(n_eff, 1))) || (rc = w.host.up(s->stream, queries, nq, s->dims, k, false))) return rc;
  // (earlier calls' launches on other streams may still read the labels)
  if ((rc = wait_searches_in_flight(s, s->stream))) return rc;
  // (pageable host memory: the runtime stages it before the call returns)
  if (n_eff) HIP_TRY(hipMemcpyAsync(w.dLabels.p, group_of, n_eff * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
  if ((rc = grouped_locked(s, s->stream, n_pub, nq, w.host.q, k, per_group, w.dLabels.p, n_eff, w.host.out))) return rc;
  return w.host.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
}

}  // namespace

extern "C" {

int ehx_knn_grouped_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k, uint32_t per_group,
                           const uint32_t* d_group_of, uint64_t n_labels, uint64_t* d_out_ids, float* d_out_dist,
                           uint32_t* d_out_count) {
  if (int rc = grouped_check(s, n_queries, k, per_group, d_queries, d_group_of, n_labels, d_out_ids, d_out_dist, d_out_count))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_knn_grouped_device", kGroupedWhy, n_queries, &st, [&] {
    return grouped_locked(s, st, s->n.load(std::memory_order_acquire), n_queries, d_queries, k, per_group, d_group_of, n_labels,
                          ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_knn_grouped(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint32_t per_group,
                    const uint32_t* group_of, uint64_t n_labels, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (int rc = grouped_check(s, n_queries, k, per_group, queries, group_of, n_labels, out_ids, out_dist, out_count)) return rc;
  return search_on_device(s, "ehx_knn_grouped", kGroupedWhy, n_queries, nullptr, [&] {
    return grouped_host_locked(s, n_queries, queries, k, per_group, group_of, n_labels, out_ids, out_dist, out_count);
  });
}

// test hook, not part of the ABI: queries answered on the scan route, handed to the exact route (by the gate or by the scan
// route), of those the ones whose pool overflowed, scan passes launched, calls
void ehx_test_grouped_counters(ehx_space* s, uint64_t out[5]) {
  for (int i = 0; i < 5; ++i) out[i] = s ? s->grouped_ctr[i].load(std::memory_order_relaxed) : 0;
}

}  // extern "C"
