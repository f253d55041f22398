// The block-wide exclusive prefix of the compactions: rows_prefix_kernel (k_masked.hip) and colindex_scan_kernel (k_colindex.hip).
#pragma once
#include "ehx_kernels.h"

namespace ehx {

// row[0, n) counts -> their exclusive prefix in place, on top of `carry` (lane 0's value counts alone); with `total`,
// row[n] = carry + their sum.  A workgroup of WG lanes, every lane calls it: chunks of WG entries, a running carry between
// them (n <= 2^24: at most 16 384 steps at 1024 lanes, of kernels that run once per call).  LDS: WG / 64 + 1 words.
template <uint32_t WG>
__device__ __forceinline__ void block_prefix(uint32_t* __restrict__ row, uint32_t n, uint32_t carry, bool total) {
  __shared__ uint32_t wave_sum[WG / 64u];
  __shared__ uint32_t carry_s;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  if (tid == 0) carry_s = carry;
  __syncthreads();
  for (uint32_t t0 = 0; t0 < n; t0 += WG) {
    const uint32_t t = t0 + tid;
    const uint32_t c = t < n ? row[t] : 0u;
    uint32_t incl = c;   // inclusive scan across the wave
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
      if ((int)lane >= d) incl += o;
    }
    if (lane == 63u) wave_sum[w] = incl;
    __syncthreads();
    uint32_t before = carry_s;
    for (uint32_t i = 0; i < w; ++i) before += wave_sum[i];
    if (t < n) row[t] = before + incl - c;
    __syncthreads();
    if (tid == WG - 1u) carry_s = before + incl;
    __syncthreads();
  }
  if (total && tid == 0) row[n] = carry_s;
}

}  // namespace ehx
