// Grouped kNN under row bitmaps (ehx_knn_grouped_masked*, ehx_groupedm.cpp): the first k ELIGIBLE rows among the ALLOWED rows
// of the prefix — filter first, then cap.  The search is the grouped kNN's (k_grouped.hip: grouped_rerank_kernel, unchanged)
// fed from the bitmaps' compacted lists (k_masked.hip: mask m's ascending allowed ids at list + off[m], their number at
// cum[m][n_tiles]); this file holds the two kernels that fill a query's pool from the list of ITS OWN bitmap:
//   grouped_list_seed_kernel   the scan route's sample: every stride-th allowed id by rank, stride = ceil(allowed /
//                              kLargeKSample), at most kLargeKSample of them; the seed-mode re-rank makes the first radius of it
//   grouped_list_slab_kernel   the list route's "pass": entries [b kPoolCap, (b + 1) kPoolCap) of the list, as many as remain
//                              (possibly none: the re-rank keeps its carried keys through an empty pool); in front of the
//                              first slab the radius +Inf and nothing carried, as grouped_slab_kernel leaves them
// mask_at[q] is the bitmap of query q of the device batch.  Both are a copy of at most 32 KiB per query: nothing to tune.
//
// Why the answer is exact: k_grouped.hip's argument with "rows" read as "allowed rows".  The allowed rows of a query are a
// FIXED set S — the bitmap is not a function of the search — so cap(S), the greedy over S in key order, is the contract's
// answer, and every step of the argument (a row dropped by a cap or a cut never returns in a superset; the k-th kept key of
// any subset of S bounds the true one from above) speaks of subsets of S only.  The scan's flush drops every row outside S
// before it takes a pool slot, the lists hold S alone, so no row outside S ever reaches a cap: it neither appears nor counts.
#include "ehx_kernels.h"

namespace ehx {

namespace {

// mask m's number of allowed rows (0 for a mask the table does not hold: nothing is read through it)
__device__ __forceinline__ uint64_t allowed_of(const uint32_t* __restrict__ cum, uint32_t n_tiles, uint32_t m) {
  return m < kMaskedMaxMasks ? (uint64_t)cum[(size_t)m * (n_tiles + 1u) + n_tiles] : 0ull;
}

}  // namespace

// one workgroup per query (launch_grouped_list_seed)
__global__ __launch_bounds__(256) void grouped_list_seed_kernel(const uint64_t* __restrict__ list, const MaskedOffsets off,
                                                                const uint32_t* __restrict__ cum, uint32_t n_tiles,
                                                                const uint32_t* __restrict__ mask_at,
                                                                uint64_t* __restrict__ pool, uint32_t* __restrict__ pool_cnt) {
  const uint32_t q = blockIdx.x, m = mask_at[q];
  const uint64_t n_allowed = allowed_of(cum, n_tiles, m);
  const uint64_t stride = (n_allowed + kLargeKSample - 1u) / kLargeKSample;
  const uint32_t n_sample = stride ? (uint32_t)((n_allowed + stride - 1u) / stride) : 0u;   // (<= kLargeKSample <= kPoolCap)
  const uint64_t* mine = list + (m < kMaskedMaxMasks ? off.off[m] : 0ull);
  for (uint32_t i = threadIdx.x; i < n_sample; i += 256u) pool[(size_t)q * kPoolCap + i] = mine[(uint64_t)i * stride];
  if (threadIdx.x == 0) pool_cnt[q] = n_sample;
}

// one workgroup per query (launch_grouped_list_slab)
__global__ __launch_bounds__(256) void grouped_list_slab_kernel(const uint64_t* __restrict__ list, const MaskedOffsets off,
                                                                const uint32_t* __restrict__ cum, uint32_t n_tiles,
                                                                const uint32_t* __restrict__ mask_at, uint64_t slab,
                                                                uint32_t first, uint64_t* __restrict__ pool,
                                                                uint32_t* __restrict__ pool_cnt, float* __restrict__ radius,
                                                                uint32_t* __restrict__ top_cnt, uint32_t* __restrict__ work) {
  const uint32_t q = blockIdx.x, m = mask_at[q];
  const uint64_t n_allowed = allowed_of(cum, n_tiles, m), at = slab * kPoolCap;
  const uint64_t left = at < n_allowed ? n_allowed - at : 0ull;
  const uint32_t n = left < kPoolCap ? (uint32_t)left : kPoolCap;
  const uint64_t* mine = list + (m < kMaskedMaxMasks ? off.off[m] : 0ull) + at;
  for (uint32_t i = threadIdx.x; i < n; i += 256u) pool[(size_t)q * kPoolCap + i] = mine[i];
  if (threadIdx.x == 0) {
    pool_cnt[q] = n;
    if (first) {
      radius[q] = __builtin_inff();
      top_cnt[q] = 0;
      work[q] = 0;
    }
  }
}

hipError_t launch_grouped_list_seed(const uint64_t* list, const MaskedOffsets& off, const uint32_t* cum, uint32_t n_tiles,
                                    const uint32_t* mask_at, uint64_t* pool, uint32_t* pool_cnt, uint32_t nq, hipStream_t st) {
  if (nq == 0) return hipSuccess;
  if (!list || !cum || !mask_at || !pool || !pool_cnt || n_tiles == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(grouped_list_seed_kernel, dim3(nq), dim3(256), 0, st, list, off, cum, n_tiles, mask_at, pool, pool_cnt);
  return hipGetLastError();
}

hipError_t launch_grouped_list_slab(const uint64_t* list, const MaskedOffsets& off, const uint32_t* cum, uint32_t n_tiles,
                                    const uint32_t* mask_at, uint64_t slab, bool first, uint64_t* pool, uint32_t* pool_cnt,
                                    float* radius, uint32_t* top_cnt, uint32_t* work, uint32_t nq, hipStream_t st) {
  if (nq == 0) return hipSuccess;
  if (!list || !cum || !mask_at || !pool || !pool_cnt || n_tiles == 0 || (first && (!radius || !top_cnt || !work)))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(grouped_list_slab_kernel, dim3(nq), dim3(256), 0, st, list, off, cum, n_tiles, mask_at, slab,
                     first ? 1u : 0u, pool, pool_cnt, radius, top_cnt, work);
  return hipGetLastError();
}

}  // namespace ehx
