// Exact kNN on the int8 radius scan under a radius that falls (radius_knn, ehx_call.cpp): the first k rows — of ALL rows
// (the flat chain's route for EHX_MAX_K < k <= kLargeKMax, ehx_largek.cpp) or of the rows a bitmap ALLOWS (the bitmap
// search's scan route, ehx_masked.cpp) — in (canonical distance, id) order: the exhaustive pass's answer, or
// ehx_knn_among's with the ascending list of allowed rows, byte for byte.
//   radius_seed_kernel     a strided sample of <= kLargeKSample row ids into every query's pool
//   radius_rerank_kernel   once for the seed and once per pass: the pool's canonical distances, cut at the radius, sorted
//                          (pool_rerank_sorted, k_exact_common.h — the range search's re-rank), merged with the query's
//                          carried keys; the best <= k carried on, the radius lowered; behind the last pass the output page
// Every distance comes from the exact paths' one row walk (walk_row), the keys from dist_key and the page from emit_page.
//
// The carried keys live in top[q][kLargeKMax] as EXACT (distance, id) keys, ascending: a pool that held them would gather
// their rows again behind every pass.  A pass re-ranks its own hits only and merges the two sorted lists by rank: a hit's
// place is its index plus the carried keys below it, a carried key's place its index plus the hits below it (binary
// searches in LDS; keys are distinct because ids are, so equal distances fall in id order).  The pool is empty again for
// the next pass.
//
// Why the answer is exact.  "Rows" below are all rows of the prefix searched, or — with a bitmap in the scan's flush, which
// drops every other row before it takes a pool slot — the ALLOWED rows; nothing else differs between the two routes.
//   * A search that knows a radius r with "the k-th distance is <= r" needs no certificate: flat_scan_i8_kernel under the
//     threshold range_thr_kernel maps r to keeps every row with D <= r (k_range.hip's header).  The exact k-th distance
//     over ANY k rows is such an r.  The first r is the k-th distance of a sample (+Inf while it gives fewer than k:
//     range_thr_kernel marks the query and the host answers it exactly) — the seed's, re-ranked here in seed mode, or the
//     bitmap route's sample of allowed rows, which the host sends through the list scan (ehx_masked.cpp); either way the
//     sample carries NOTHING, its rows enter the answer through their own pass like every other row.
//   * Passes cover disjoint tile ranges and a tile's rows are hit at most once per pass: a row enters a pool at most once,
//     and never meets its own key in the carried list.
//   * Let m be a true member of the answer and r* the radius behind the last pass.  Every radius is the k-th distance of k
//     rows of the prefix seen, hence >= the true k-th distance >= D(m); the radius only falls, so the radius r_j its own
//     pass ran under is >= r* >= D(m): the scan keeps m and the cut at r_j does not drop it.  It leaves the carried list only
//     when k rows precede it in (distance, id) order — then it is no member.  By induction the merged list behind the last
//     pass holds every member, in order.
//   * Distances are canonical, so a loose threshold costs time, never correctness.
//   * A query whose pool overflowed (ovf = 1, sticky: its radius becomes NaN, later passes collect nothing for it) or which
//     the bound does not serve (ovf = 2: NaN or non-positive u, infinite radius, non-finite margin) writes nothing here: the
//     host answers it exactly — the exhaustive pass at k, or the exact kNN among the whole list of allowed rows.
#include "ehx_kernels.h"

namespace ehx {

namespace {

constexpr uint32_t kRadiusThreads = 256;
static_assert(kLargeKMax <= kRadiusThreads, "one thread per carried key and per surviving hit");
static_assert(3u * kLargeKMax <= kPoolCap, "hits | carried | merged share the pool's LDS image");

}  // namespace

// one workgroup per query: pool[q][i] = i * stride for i < n_sample (the key's high half is not looked at)
__global__ __launch_bounds__(256) void radius_seed_kernel(uint64_t* __restrict__ pool, uint32_t* __restrict__ pool_cnt,
                                                          uint64_t stride, uint32_t n_sample) {
  const uint32_t q = blockIdx.x;
  for (uint32_t i = threadIdx.x; i < n_sample; i += 256u) pool[(size_t)q * kPoolCap + i] = (uint64_t)i * stride;
  if (threadIdx.x == 0) pool_cnt[q] = n_sample;
}

// One workgroup per query (file header).  LDS: the pool's 32 KiB of keys and the prepared query; behind the sort the first
// <= k hits stay at keys[0, kLargeKMax), the carried keys go to [kLargeKMax, 2 kLargeKMax), the merged list to
// [2 kLargeKMax, 3 kLargeKMax) — later hits than the k-th are no members and may be overwritten.
template <bool HALFX, int METRIC>
__global__ __launch_bounds__(kRadiusThreads) void radius_rerank_kernel(const RadiusRerankArgs a) {
  extern __shared__ float4 radius_lds[];
  uint64_t* keys = (uint64_t*)radius_lds;   // (pool_rerank_sorted's image: the sorted keys at its head)
  const uint32_t tid = threadIdx.x, q = blockIdx.x;
  const bool seed = a.mode == kRadiusSeed;
  const uint32_t flag = seed ? 0u : a.ovf[q];
  if (flag) {
    // (an overflowed pool: a NaN radius maps to -inf, the later passes collect nothing for the query)
    if (flag == 1u && tid == 0) a.radius[q] = __builtin_nanf("");
    return;
  }
  const uint32_t cnt = a.pool_cnt[q];
  if (cnt > kPoolCap) return;   // (the scan's flag is about to land or has: the host reads it behind the last pass)
  const float r = seed ? __builtin_inff() : a.radius[q];
  const uint32_t total = pool_rerank_sorted<HALFX ? kLayoutF16 : kLayoutF32, METRIC, kRadiusThreads>(
      radius_lds, a.rows, a.Q + (size_t)q * a.rows.ld, a.pool + (size_t)q * kPoolCap, cnt, r, tid);
  if (seed) {
    // the sample gives the first radius and nothing else
    if (tid == 0) {
      a.radius[q] = total >= a.k ? ordered_to_f32((uint32_t)(keys[a.k - 1] >> 32)) : __builtin_inff();
      a.pool_cnt[q] = 0;
      a.top_cnt[q] = 0;
      a.work[q] = cnt;
    }
    return;
  }
  const uint32_t nh = total < a.k ? total : a.k;   // hits that can still be members: keys[0, nh)
  const uint32_t have = a.top_cnt[q];
  const uint32_t nc = have < a.k ? have : a.k;     // (never more than k: this kernel wrote it)
  uint64_t* carried = keys + kLargeKMax;
  uint64_t* merged = keys + 2u * kLargeKMax;
  uint64_t* tq = a.top + (size_t)q * kLargeKMax;
  uint64_t c = kKeyInf;
  if (tid < nc) {
    c = tq[tid];
    carried[tid] = c;
  }
  __syncthreads();
  const uint32_t n_out = nh + nc < a.k ? nh + nc : a.k;
  if (tid < nh) {
    const uint64_t h = keys[tid];
    const uint32_t at = tid + lower_bound_lds(carried, nc, h);
    if (at < n_out) merged[at] = h;
  }
  if (tid < nc) {
    const uint32_t at = tid + lower_bound_lds(keys, nh, c);
    if (at < n_out) merged[at] = c;
  }
  __syncthreads();
  if (a.mode == kRadiusLast) {
    emit_page([&](uint32_t i) { return merged[i]; }, n_out, a.k, a.out_ids + (size_t)q * a.k, a.out_dist + (size_t)q * a.k,
              a.out_count + q, 0, tid, kRadiusThreads);
  } else {
    if (tid < n_out) tq[tid] = merged[tid];
    if (tid == 0) {
      a.top_cnt[q] = n_out;
      a.pool_cnt[q] = 0;
      // (every key held is <= r: the k-th of them is the new, smaller or equal, radius)
      if (n_out >= a.k) a.radius[q] = ordered_to_f32((uint32_t)(merged[a.k - 1] >> 32));
    }
  }
  if (tid == 0) a.work[q] += cnt;
}

namespace {

const decltype(&radius_rerank_kernel<false, 0>) kRadiusRerankFns[6] = {   // [half * 3 + metric]
    radius_rerank_kernel<false, 0>, radius_rerank_kernel<false, 1>, radius_rerank_kernel<false, 2>,
    radius_rerank_kernel<true, 0>,  radius_rerank_kernel<true, 1>,  radius_rerank_kernel<true, 2>};
DynLdsAttr g_radius_lds;

}  // namespace

hipError_t launch_radius_seed(uint64_t* pool, uint32_t* pool_cnt, uint32_t nq, uint64_t n_rows, uint64_t stride,
                              uint32_t n_sample, hipStream_t st) {
  if (nq == 0) return hipSuccess;
  // (every sampled id is a row: (n_sample - 1) * stride < n_rows)
  if (n_sample == 0 || n_sample > kLargeKSample || stride == 0 || (uint64_t)(n_sample - 1) * stride >= n_rows)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(radius_seed_kernel, dim3(nq), dim3(256), 0, st, pool, pool_cnt, stride, n_sample);
  return hipGetLastError();
}

hipError_t launch_radius_rerank(const RadiusRerankArgs& a, hipStream_t st) {
  return launch_pool_rerank(kRadiusRerankFns, g_radius_lds, a, a.k != 0 && a.k <= kLargeKMax && a.mode <= kRadiusSeed && !a.rows.x_perm,
                            kRadiusThreads, st);
}

}  // namespace ehx
