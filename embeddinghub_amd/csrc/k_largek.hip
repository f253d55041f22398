// Exact kNN for EHX_MAX_K < k <= kLargeKMax at batch rate (ehx_largek.cpp): the first k rows in (canonical distance, id)
// order — the exhaustive pass's answer, byte for byte — found by the int8 radius scan under a radius that falls.
//   largek_seed_kernel     a strided sample of <= kLargeKSample row ids into every query's pool
//   largek_rerank_kernel   once for the seed and once per pass: the pool's canonical distances, cut at the radius, sorted,
//                          merged with the query's carried keys; the best <= k carried on, the radius lowered; behind the
//                          last pass the output page
// Every distance comes from the exact paths' one row walk (walk_row, k_exact_common.h) through the pool re-rank the range
// and bitmap searches use (rerank_pool_cut, block_sort_lds), the keys from dist_key and the page from emit_page.
//
// What differs from masked_rerank_kernel (k_masked.hip).  The carried list is up to 256 keys long, and a pool that held it
// would gather its rows again behind every pass.  Here the carried keys live in top[q][kLargeKMax] as EXACT (distance, id)
// keys, ascending; a pass re-ranks its own hits only and merges the two sorted lists by rank: a hit's place is its index
// plus the carried keys below it, a carried key's place its index plus the hits below it (binary searches in LDS; keys are
// distinct because ids are).  The pool is empty again for the next pass.
//
// Why the answer is exact (k_masked.hip's argument, with "rows" for "allowed rows").
//   * A search that knows a radius r with "the k-th distance is <= r" needs no certificate: flat_scan_i8_kernel under the
//     threshold range_thr_kernel maps r to keeps every row with D <= r (k_range.hip's header).  The exact k-th distance
//     over ANY k rows is such an r.  The first r is the k-th distance of the seed's sample (+Inf while it gives fewer than
//     k: range_thr_kernel marks the query and the host answers it exhaustively); the sample carries NOTHING, its rows
//     enter the answer through their own pass like every other row.
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
//     host answers it with the exhaustive pass at k.
#include "ehx_kernels.h"

namespace ehx {

namespace {

constexpr uint32_t kLargeKThreads = 256;
static_assert(kLargeKMax <= kLargeKThreads, "one thread per carried key and per surviving hit");
static_assert(3u * kLargeKMax <= kPoolCap, "hits | carried | merged share the pool's LDS image");

// the number of keys[0, n) below `key` (keys ascending, distinct from `key`)
__device__ __forceinline__ uint32_t keys_below(const uint64_t* keys, uint32_t n, uint64_t key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

}  // namespace

// one workgroup per query: pool[q][i] = i * stride for i < n_sample (the key's high half is not looked at)
__global__ __launch_bounds__(256) void largek_seed_kernel(uint64_t* __restrict__ pool, uint32_t* __restrict__ pool_cnt,
                                                          uint64_t stride, uint32_t n_sample) {
  const uint32_t q = blockIdx.x;
  for (uint32_t i = threadIdx.x; i < n_sample; i += 256u) pool[(size_t)q * kPoolCap + i] = (uint64_t)i * stride;
  if (threadIdx.x == 0) pool_cnt[q] = n_sample;
}

// One workgroup per query (file header).  LDS: the pool's 32 KiB of keys and the prepared query; behind the sort the first
// <= k hits stay at keys[0, kLargeKMax), the carried keys go to [kLargeKMax, 2 kLargeKMax), the merged list to
// [2 kLargeKMax, 3 kLargeKMax) — later hits than the k-th are no members and may be overwritten.
template <bool HALFX, int METRIC>
__global__ __launch_bounds__(kLargeKThreads) void largek_rerank_kernel(const LargeKRerankArgs a) {
  extern __shared__ float4 largek_lds[];
  uint64_t* keys = (uint64_t*)largek_lds;             // [kPoolCap]
  float* qs = (float*)(keys + kPoolCap);              // [ld]
  uint32_t& kept_s = *(uint32_t*)(qs + a.rows.ld);
  const uint32_t tid = threadIdx.x, q = blockIdx.x;
  const int lane = (int)(tid & 63u);
  const bool seed = a.mode == kLargeKSeed;
  const uint32_t flag = seed ? 0u : a.ovf[q];
  if (flag) {
    // (an overflowed pool: a NaN radius maps to -inf, the later passes collect nothing for the query)
    if (flag == 1u && tid == 0) a.radius[q] = __builtin_nanf("");
    return;
  }
  const uint32_t cnt = a.pool_cnt[q];
  if (cnt > kPoolCap) return;   // (the scan's flag is about to land or has: the host reads it behind the last pass)
  const float r = seed ? __builtin_inff() : a.radius[q];
  constexpr int LAYOUT = HALFX ? kLayoutF16 : kLayoutF32;
  stage_query_lds<LAYOUT>(qs, a.Q + (size_t)q * a.rows.ld, a.rows.ld, tid, kLargeKThreads);
  if (tid == 0) kept_s = 0;
  __syncthreads();
  const uint32_t kept = rerank_pool_cut<LAYOUT, METRIC, kLargeKThreads>(a.rows, qs, a.pool + (size_t)q * kPoolCap, cnt, r, keys, tid);
  if (lane == 0 && kept) atomicAdd(&kept_s, kept);
  uint32_t m = 2;
  while (m < cnt) m <<= 1;
  for (uint32_t i = cnt + tid; i < m; i += kLargeKThreads) keys[i] = kKeyInf;
  __syncthreads();
  block_sort_lds<kLargeKThreads>(keys, m, tid);
  const uint32_t total = kept_s;
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
    const uint32_t at = tid + keys_below(carried, nc, h);
    if (at < n_out) merged[at] = h;
  }
  if (tid < nc) {
    const uint32_t at = tid + keys_below(keys, nh, c);
    if (at < n_out) merged[at] = c;
  }
  __syncthreads();
  if (a.mode == kLargeKLast) {
    emit_page([&](uint32_t i) { return merged[i]; }, n_out, a.k, a.out_ids + (size_t)q * a.k, a.out_dist + (size_t)q * a.k,
              a.out_count + q, 0, tid, kLargeKThreads);
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

typedef void (*LargeKRerankFn)(const LargeKRerankArgs);
const LargeKRerankFn kLargeKRerankFns[6] = {   // [half * 3 + metric]
    largek_rerank_kernel<false, 0>, largek_rerank_kernel<false, 1>, largek_rerank_kernel<false, 2>,
    largek_rerank_kernel<true, 0>,  largek_rerank_kernel<true, 1>,  largek_rerank_kernel<true, 2>};
DynLdsAttr g_largek_lds;

}  // namespace

hipError_t launch_largek_seed(uint64_t* pool, uint32_t* pool_cnt, uint32_t nq, uint64_t n_rows, uint64_t stride,
                              uint32_t n_sample, hipStream_t st) {
  if (nq == 0) return hipSuccess;
  // (every sampled id is a row: (n_sample - 1) * stride < n_rows)
  if (n_sample == 0 || n_sample > kLargeKSample || stride == 0 || (uint64_t)(n_sample - 1) * stride >= n_rows)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(largek_seed_kernel, dim3(nq), dim3(256), 0, st, pool, pool_cnt, stride, n_sample);
  return hipGetLastError();
}

hipError_t launch_largek_rerank(const LargeKRerankArgs& a, hipStream_t st) {
  if (a.nq == 0) return hipSuccess;
  if (a.k == 0 || a.k > kLargeKMax || a.mode > kLargeKSeed || (a.rows.ld & 3u) || a.rows.ld > range_rerank_max_ld() ||
      a.rows.x_perm || a.rows.metric < 0 || a.rows.metric > 2)
    return hipErrorInvalidValue;
  const size_t lds = kPoolCap * sizeof(uint64_t) + (size_t)a.rows.ld * sizeof(float) + 16u;
  hipError_t e = g_largek_lds.ensure(kLargeKRerankFns, 6, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kLargeKRerankFns[(a.rows.x_half ? 3 : 0) + a.rows.metric], dim3(a.nq), dim3(kLargeKThreads), lds, st, a);
  return hipGetLastError();
}

}  // namespace ehx
