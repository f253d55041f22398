// Exact kNN under a row bitmap (ehx_knn_masked*): the first k of the ALLOWED rows in (canonical distance, id) order — the
// answer of ehx_knn_among with the ascending list of allowed rows, byte for byte.  This file compacts the bitmap:
//   masked_count_kernel    allowed rows of every 256-row tile (8 words of the bitmap)
//   masked_prefix_kernel   their exclusive prefix, cum[0 .. n_tiles] (cum[n_tiles] = the number of allowed rows)
//   masked_fill_kernel     the ascending list of allowed row ids
//   masked_sample_kernel   every stride-th allowed id by rank: the sample whose exact k-th distance is the first radius
//   masked_radius_kernel   radius[q] = that distance, from the list scan's answer over the sample (+Inf while it gave fewer
//                          than k)
// The list serves the exact route (k_among.hip) and the host's pass plan; the scan route (ehx_masked.cpp) is the falling-
// radius kNN of k_radius.hip with the bitmap in the int8 scan's flush and this first radius — that file's header has the
// re-rank kernel and the argument why the answer is exact, "allowed rows" being its rows.
#include "ehx_kernels.h"

namespace ehx {

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

}  // namespace ehx
