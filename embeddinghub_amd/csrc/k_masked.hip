// Exact kNN under row bitmaps (ehx_knn_masked*: one bitmap; ehx_knn_masked_multi*: a table, one per query): the first k of
// the ALLOWED rows in (canonical distance, id) order — the answer of ehx_knn_among with the ascending list of allowed rows,
// byte for byte.  This file compacts the bitmaps, every one of a table in one set of launches, the mask a grid dimension
// (one bitmap: a table of one, used where it lies — the row stride is never applied):
//   masked_count_kernel    allowed rows of every 256-row tile (8 words of the bitmap) of every mask
//   rows_prefix_kernel     their exclusive prefix per mask, cum[m][0 .. n_tiles] (cum[m][n_tiles] = mask m's allowed rows);
//                          the label compaction (k_labeled.hip) and the column index (k_colindex.hip) launch it too
//   masked_fill_kernel     the ascending lists of allowed row ids, mask m's at list + off[m] (the host places them back to
//                          back from the counts it read)
//   masked_sample_kernel   every mask's sample, every sample_stride(allowed)-th allowed id by rank: its exact k-th distance is
//                          the first radius (launched for the scan route only)
//   masked_radius_kernel   radius[q] = that distance, from the list scan's answer over the sample of the query's own mask
//                          (+Inf while it gave fewer than k)
// The lists serve the exact route (k_among.hip) and the host's pass plan; the scan route (ehx_masked.cpp) is the falling-
// radius kNN of k_radius.hip with the bitmap in the int8 scan's flush (one for the batch, or one per query: k_flati8.hip)
// and this first radius — that file's header has the re-rank kernel and the argument why the answer is exact, "allowed
// rows" being its rows.
#include "k_prefix.h"

namespace ehx {

// one lane per tile, blockIdx.y = mask
__global__ __launch_bounds__(256) void masked_count_kernel(const uint32_t* __restrict__ maps, uint64_t stride, uint64_t n_bits,
                                                           uint32_t n_tiles, uint32_t* __restrict__ cum) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x, m = blockIdx.y;
  if (t >= n_tiles) return;
  const uint32_t* mask = maps + (size_t)m * stride;
  uint32_t c = 0;
  for (uint32_t w = 0; w < 8; ++w) c += (uint32_t)__builtin_popcount(mask_word(mask, (uint64_t)t * 8u + w, n_bits));
  cum[(size_t)m * (n_tiles + 1u) + t] = c;
}

// ONE workgroup per row of counts: cum[row][0 .. n) -> exclusive prefix in place, cum[row][n] = the total (block_prefix,
// k_prefix.h).  Every compaction's: the tiles of a bitmap, of a scanning label, the label boundaries of a column index.
__global__ __launch_bounds__(1024) void rows_prefix_kernel(uint32_t* __restrict__ cum_all, uint32_t n) {
  block_prefix<1024>(cum_all + (size_t)blockIdx.x * (n + 1u), n, 0u, true);
}

// one workgroup per (tile, mask), one lane per row: list[off[mask] + cum[mask][tile] + rank inside the tile] = row id
__global__ __launch_bounds__(256) void masked_fill_kernel(const uint32_t* __restrict__ maps, uint64_t stride, uint64_t n_bits,
                                                          uint32_t n_tiles, const uint32_t* __restrict__ cum,
                                                          const MaskedOffsets off, uint64_t* __restrict__ list) {
  const uint32_t tile = blockIdx.x, m = blockIdx.y, tid = threadIdx.x;
  const uint32_t* mask = maps + (size_t)m * stride;
  const uint32_t wi = tid >> 5, bit = tid & 31u;
  uint32_t before = 0, mine = 0;
  for (uint32_t w = 0; w < 8; ++w) {   // (the tile's 8 words: 32 bytes, the same for every lane)
    const uint32_t v = mask_word(mask, (uint64_t)tile * 8u + w, n_bits);
    if (w < wi) before += (uint32_t)__builtin_popcount(v);
    if (w == wi) mine = v;
  }
  if (!((mine >> bit) & 1u)) return;
  const uint32_t rank = before + (uint32_t)__builtin_popcount(mine & ((1u << bit) - 1u));
  list[off.off[m] + cum[(size_t)m * (n_tiles + 1u) + tile] + rank] = (uint64_t)tile * 256u + tid;
}

// one workgroup per mask: mask m's sample (write_sample, ehx_kernels.h) at sample + 256 m
__global__ __launch_bounds__(256) void masked_sample_kernel(const uint64_t* __restrict__ list, const MaskedOffsets off,
                                                            const uint32_t* __restrict__ cum, uint32_t n_tiles,
                                                            uint64_t* __restrict__ sample) {
  const uint32_t m = blockIdx.x;
  write_sample(list + off.off[m], cum[(size_t)m * (n_tiles + 1u) + n_tiles], sample + (size_t)m * 256u);
}

__global__ __launch_bounds__(256) void masked_radius_kernel(const float* __restrict__ dist, const uint32_t* __restrict__ cnt,
                                                            uint32_t nq, uint32_t k, float* __restrict__ radius) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= nq) return;
  radius[q] = cnt[q] >= k ? dist[(size_t)q * k + (k - 1)] : __builtin_inff();
}

hipError_t launch_masked_count(const uint32_t* maps, uint64_t stride, uint32_t n_masks, uint64_t n_bits, uint32_t n_tiles,
                               uint32_t* cum, hipStream_t st) {
  if (n_tiles == 0 || n_masks == 0) return hipSuccess;
  if (n_masks > kMaskedMaxMasks || (n_masks > 1 && stride < (n_bits + 31) / 32)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(masked_count_kernel, dim3((n_tiles + 255u) / 256u, n_masks), dim3(256), 0, st, maps, stride, n_bits,
                     n_tiles, cum);
  return launch_rows_prefix(cum, n_masks, n_tiles, st);
}

hipError_t launch_rows_prefix(uint32_t* cum, uint32_t rows, uint32_t n, hipStream_t st) {
  if (rows == 0 || n == 0) return hipSuccess;
  hipLaunchKernelGGL(rows_prefix_kernel, dim3(rows), dim3(1024), 0, st, cum, n);
  return hipGetLastError();
}

hipError_t launch_masked_fill(const uint32_t* maps, uint64_t stride, uint32_t n_masks, uint64_t n_bits, uint32_t n_tiles,
                              const uint32_t* cum, const MaskedOffsets& off, uint64_t* list, hipStream_t st) {
  if (n_tiles == 0 || n_masks == 0) return hipSuccess;
  if (n_masks > kMaskedMaxMasks || (n_masks > 1 && stride < (n_bits + 31) / 32)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(masked_fill_kernel, dim3(n_tiles, n_masks), dim3(256), 0, st, maps, stride, n_bits, n_tiles, cum, off, list);
  return hipGetLastError();
}

hipError_t launch_masked_samples(const uint64_t* list, const MaskedOffsets& off, const uint32_t* cum, uint32_t n_masks,
                                 uint32_t n_tiles, uint64_t* sample, hipStream_t st) {
  if (n_tiles == 0 || n_masks == 0) return hipSuccess;
  if (n_masks > kMaskedMaxMasks) return hipErrorInvalidValue;
  hipLaunchKernelGGL(masked_sample_kernel, dim3(n_masks), dim3(256), 0, st, list, off, cum, n_tiles, sample);
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
