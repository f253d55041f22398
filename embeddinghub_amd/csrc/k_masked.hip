// Exact kNN under a row bitmap (ehx_knn_masked*): the first k of the ALLOWED rows in (canonical distance, id) order — the
// answer of ehx_knn_among with the ascending list of allowed rows, byte for byte.
//   masked_count_kernel    allowed rows of every 256-row tile (8 words of the bitmap)
//   masked_prefix_kernel   their exclusive prefix, cum[0 .. n_tiles] (cum[n_tiles] = the number of allowed rows)
//   masked_fill_kernel     the ascending list of allowed row ids
//   masked_sample_kernel   every stride-th allowed id by rank: the sample whose exact k-th distance is the first radius
//   masked_radius_kernel   radius[q] = the sample's k-th distance (+Inf while the sample gave fewer than k)
//   masked_rerank_kernel   scan route, once per pass: the pool's canonical distances, cut at the radius, sorted; the best
//                          <= k carried into the next pass, the radius lowered; behind the last pass the output page
// Every distance comes from the exact paths' one row walk (walk_row, k_exact_common.h) through the pool re-rank it shares
// with the range search (rerank_pool_cut, block_sort_lds), the keys from dist_key and the page from emit_page.
//
// The scan route (ehx_masked.cpp).  A search that knows a radius r with "the masked k-th distance is <= r" needs no
// certificate: flat_scan_i8_kernel under the threshold range_thr_kernel maps r to keeps every row with D <= r (k_range.hip's
// header), and its flush drops the rows the bitmap does not allow before they take a pool slot.  The k-th exact distance
// over ANY subset of the allowed rows is such an r: the subset's k nearest are k allowed rows within r.  The first r is the
// k-th distance of a sample of <= 256 allowed rows; the rows are then scanned in passes over disjoint tile ranges, and
// behind every pass this file's re-rank computes the canonical distances of the pool — the <= k keys carried from earlier
// passes and the pass's hits — drops what lies above r (or is NaN), sorts the rest by (distance, id), keeps the best <= k
// at the head of the pool and lowers r to their k-th distance when k are held.  The radius only ever falls.
//
// Why the answer is exact and nothing is collected twice.
//   * Passes cover disjoint tiles and a tile's rows are hit at most once per pass, so a row enters a pool at most once; the
//     sample's rows give the radius only and enter a pool through their own pass like every other row.
//   * Let m be a true member of the answer and r* the radius behind the last pass.  Every radius is the k-th distance of k
//     allowed rows, hence >= the true masked k-th distance >= D(m); the radius r_j its own pass j ran under is >= r*
//     >= D(m), so the scan keeps it (soundness of the threshold) and the re-rank does not cut it at the radius.  It leaves a
//     pool only when k allowed rows precede it in (distance, id) order — then it is no member.  By induction over the
//     passes the pool behind the last pass holds every member, in order.
//   * A query whose pool overflowed (ovf = 1, sticky: its radius becomes NaN, so later passes collect nothing for it) or
//     which the bound does not serve (ovf = 2, range_thr_kernel) writes nothing here: the host answers it with the exact
//     kNN among the whole list.
#include "ehx_kernels.h"

namespace ehx {

namespace {

constexpr uint32_t kMaskedThreads = 256;

// word w of the bitmap cut at n_bits (bits of the last word beyond n_bits and words beyond it read as 0)
__device__ __forceinline__ uint32_t mask_word(const uint32_t* __restrict__ mask, uint64_t w, uint64_t n_bits) {
  const uint64_t lo = w << 5;
  if (lo >= n_bits) return 0u;
  uint32_t v = mask[w];
  const uint64_t left = n_bits - lo;
  if (left < 32) v &= (1u << (uint32_t)left) - 1u;
  return v;
}

}  // namespace

// one lane per tile
__global__ __launch_bounds__(256) void masked_count_kernel(const uint32_t* __restrict__ mask, uint64_t n_bits, uint32_t n_tiles,
                                                           uint32_t* __restrict__ cum) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= n_tiles) return;
  uint32_t c = 0;
  for (uint32_t w = 0; w < 8; ++w) c += (uint32_t)__builtin_popcount(mask_word(mask, (uint64_t)t * 8u + w, n_bits));
  cum[t] = c;
}

// ONE workgroup: cum[0 .. n_tiles) counts -> exclusive prefix in place, cum[n_tiles] = the total.  Blocks of 1024 tiles,
// a running carry between them (n_tiles <= 2^24: at most 16 384 steps of a kernel that runs once per call).
__global__ __launch_bounds__(1024) void masked_prefix_kernel(uint32_t* __restrict__ cum, uint32_t n_tiles) {
  __shared__ uint32_t wave_sum[16];
  __shared__ uint32_t carry_s;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (uint32_t t0 = 0; t0 < n_tiles; t0 += 1024u) {
    const uint32_t t = t0 + tid;
    const uint32_t c = t < n_tiles ? cum[t] : 0u;
    uint32_t incl = c;   // inclusive scan across the wave
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
      if ((int)lane >= d) incl += o;
    }
    if (lane == 63u) wave_sum[w] = incl;
    __syncthreads();
    uint32_t before = carry_s;
    for (uint32_t i = 0; i < w; ++i) before += wave_sum[i];
    if (t < n_tiles) cum[t] = before + incl - c;
    __syncthreads();
    if (tid == 1023u) carry_s = before + incl;
    __syncthreads();
  }
  if (tid == 0) cum[n_tiles] = carry_s;
}

// one workgroup per tile, one lane per row: list[cum[tile] + rank inside the tile] = row id
__global__ __launch_bounds__(256) void masked_fill_kernel(const uint32_t* __restrict__ mask, uint64_t n_bits,
                                                          const uint32_t* __restrict__ cum, uint64_t* __restrict__ list) {
  const uint32_t tile = blockIdx.x, tid = threadIdx.x;
  const uint32_t wi = tid >> 5, bit = tid & 31u;
  uint32_t before = 0, mine = 0;
  for (uint32_t w = 0; w < 8; ++w) {   // (the tile's 8 words: 32 bytes, the same for every lane)
    const uint32_t v = mask_word(mask, (uint64_t)tile * 8u + w, n_bits);
    if (w < wi) before += (uint32_t)__builtin_popcount(v);
    if (w == wi) mine = v;
  }
  if (!((mine >> bit) & 1u)) return;
  const uint32_t rank = before + (uint32_t)__builtin_popcount(mine & ((1u << bit) - 1u));
  list[(uint64_t)cum[tile] + rank] = (uint64_t)tile * 256u + tid;
}

__global__ __launch_bounds__(256) void masked_sample_kernel(const uint64_t* __restrict__ list, uint64_t n_allowed,
                                                            uint64_t stride, uint64_t* __restrict__ sample) {
  const uint64_t i = threadIdx.x;
  if (i * stride < n_allowed) sample[i] = list[i * stride];
}

__global__ __launch_bounds__(256) void masked_radius_kernel(const float* __restrict__ dist, const uint32_t* __restrict__ cnt,
                                                            uint32_t nq, uint32_t k, float* __restrict__ radius) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= nq) return;
  radius[q] = cnt[q] >= k ? dist[(size_t)q * k + (k - 1)] : __builtin_inff();
}

// One workgroup per query (file header).  The pool holds keys whose low halves are row ids: (distance, id) of the rows
// carried, (S_lower, id) of this pass's hits.
template <bool HALFX, int METRIC>
__global__ __launch_bounds__(kMaskedThreads) void masked_rerank_kernel(const MaskedRerankArgs a) {
  extern __shared__ float4 masked_lds[];
  uint64_t* keys = (uint64_t*)masked_lds;             // [kPoolCap]
  float* qs = (float*)(keys + kPoolCap);              // [ld]
  uint32_t& kept_s = *(uint32_t*)(qs + a.rows.ld);
  const uint32_t tid = threadIdx.x, q = blockIdx.x;
  const int lane = (int)(tid & 63u);
  const uint32_t flag = a.ovf[q];
  if (flag) {
    // (an overflowed pool: a NaN radius maps to -inf, the later passes collect nothing for the query)
    if (flag == 1u && tid == 0) a.radius[q] = __builtin_nanf("");
    return;
  }
  const uint32_t have = a.pool_cnt[q];
  if (have > kPoolCap) return;   // (the scan's flag is about to land or has: the host reads it behind the last pass)
  const uint32_t cnt = have;
  const float r = a.radius[q];
  constexpr int LAYOUT = HALFX ? kLayoutF16 : kLayoutF32;
  stage_query_lds<LAYOUT>(qs, a.Q + (size_t)q * a.rows.ld, a.rows.ld, tid, kMaskedThreads);
  if (tid == 0) kept_s = 0;
  __syncthreads();
  uint64_t* pq = a.pool + (size_t)q * kPoolCap;
  const uint32_t kept = rerank_pool_cut<LAYOUT, METRIC, kMaskedThreads>(a.rows, qs, pq, cnt, r, keys, tid);
  if (lane == 0 && kept) atomicAdd(&kept_s, kept);
  uint32_t m = 2;
  while (m < cnt) m <<= 1;
  for (uint32_t i = cnt + tid; i < m; i += kMaskedThreads) keys[i] = kKeyInf;
  __syncthreads();
  block_sort_lds<kMaskedThreads>(keys, m, tid);
  const uint32_t total = kept_s;
  const uint32_t keep = total < a.k ? total : a.k;
  if (a.last) {
    emit_page([&](uint32_t i) { return keys[i]; }, keep, a.k, a.out_ids + (size_t)q * a.k, a.out_dist + (size_t)q * a.k,
              a.out_count + q, 0, tid, kMaskedThreads);
  } else {
    for (uint32_t i = tid; i < keep; i += kMaskedThreads) pq[i] = keys[i];
    if (tid == 0) {
      a.pool_cnt[q] = keep;
      // (every kept distance is <= r: the k-th of them is the new, smaller or equal, radius)
      if (total >= a.k) a.radius[q] = ordered_to_f32((uint32_t)(keys[a.k - 1] >> 32));
    }
  }
  if (tid == 0) a.work[q] += cnt;
}

namespace {

typedef void (*MaskedRerankFn)(const MaskedRerankArgs);
const MaskedRerankFn kMaskedRerankFns[6] = {   // [half * 3 + metric]
    masked_rerank_kernel<false, 0>, masked_rerank_kernel<false, 1>, masked_rerank_kernel<false, 2>,
    masked_rerank_kernel<true, 0>,  masked_rerank_kernel<true, 1>,  masked_rerank_kernel<true, 2>};
DynLdsAttr g_masked_lds;

}  // namespace

hipError_t launch_masked_compact(const uint32_t* mask, uint64_t n_bits, uint32_t n_tiles, uint32_t* cum, uint64_t* list,
                                 hipStream_t st) {
  if (n_tiles == 0) return hipSuccess;
  hipLaunchKernelGGL(masked_count_kernel, dim3((n_tiles + 255u) / 256u), dim3(256), 0, st, mask, n_bits, n_tiles, cum);
  hipLaunchKernelGGL(masked_prefix_kernel, dim3(1), dim3(1024), 0, st, cum, n_tiles);
  hipLaunchKernelGGL(masked_fill_kernel, dim3(n_tiles), dim3(256), 0, st, mask, n_bits, cum, list);
  return hipGetLastError();
}

hipError_t launch_masked_sample(const uint64_t* list, uint64_t n_allowed, uint64_t stride, uint64_t* sample, hipStream_t st) {
  if (n_allowed == 0) return hipSuccess;
  if (stride == 0 || (n_allowed + stride - 1) / stride > 256) return hipErrorInvalidValue;
  hipLaunchKernelGGL(masked_sample_kernel, dim3(1), dim3(256), 0, st, list, n_allowed, stride, sample);
  return hipGetLastError();
}

hipError_t launch_masked_radius(const float* dist, const uint32_t* cnt, uint32_t nq, uint32_t k, float* radius,
                                hipStream_t st) {
  if (nq == 0) return hipSuccess;
  if (k == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(masked_radius_kernel, dim3((nq + 255u) / 256u), dim3(256), 0, st, dist, cnt, nq, k, radius);
  return hipGetLastError();
}

hipError_t launch_masked_rerank(const MaskedRerankArgs& a, hipStream_t st) {
  if (a.nq == 0) return hipSuccess;
  if (a.k == 0 || a.k > kPoolCap || (a.rows.ld & 3u) || a.rows.ld > range_rerank_max_ld() || a.rows.x_perm || a.rows.metric < 0 ||
      a.rows.metric > 2)
    return hipErrorInvalidValue;
  const size_t lds = kPoolCap * sizeof(uint64_t) + (size_t)a.rows.ld * sizeof(float) + 16u;
  hipError_t e = g_masked_lds.ensure(kMaskedRerankFns, 6, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kMaskedRerankFns[(a.rows.x_half ? 3 : 0) + a.rows.metric], dim3(a.nq), dim3(kMaskedThreads), lds, st, a);
  return hipGetLastError();
}

}  // namespace ehx
