// Grouped kNN under a label column (ehx_knn_grouped_labeled*, ehx_groupedl.cpp): the first k ELIGIBLE rows among the rows that
// carry the query's wanted label — filter first, then cap.  The search is the grouped kNN's (k_grouped.hip:
// grouped_rerank_kernel, unchanged) fed from the label compaction's lists (k_labeled.hip: every wanted label's row ids back
// to back in one array).  This file holds the two kernels that fill a query's pool from ITS OWN label's list, the
// counterparts of k_groupedm.hip's pair; query q's list is list[start[q], end[q]), both read from a per-batch device array
// the host fills from the plan — so any number of lists fits one launch, and queries of one label name the same range:
//   grouped_range_seed_kernel   the scan route's sample: every stride-th id of the range by rank, stride = ceil(len /
//                               kLargeKSample), at most kLargeKSample of them (a scanning label's list is ascending, so the
//                               sample spreads over the id space as the unfiltered search's does); the seed-mode re-rank
//                               makes the first radius of it
//   grouped_range_slab_kernel   the list route's "pass": entries [b kPoolCap, (b + 1) kPoolCap) of the range, as many as
//                               remain (possibly none: the re-rank keeps its carried keys through an empty pool, and an empty
//                               range still has its page written); in front of the first slab the radius +Inf, nothing
//                               carried, work 0, as grouped_slab_kernel leaves them
// Both are a copy of at most 32 KiB per query: nothing to tune.
//
// Why the answer is exact: k_grouped.hip's argument with "rows" read as "the rows of the query's label", as k_groupedm.hip
// states it for a bitmap.  Those rows are a FIXED set S — the label column is not a function of the search — so cap(S), the
// greedy over S in key order, is the contract's answer, and every step of the argument speaks of subsets of S only.  The
// scan's flush drops every row outside S before it takes a pool slot, the ranges hold S alone, so no row outside S ever
// reaches a cap: it neither appears nor counts.  cap_k(A u B) = cap_k(cap_k(A) u cap_k(B)) holds for ANY split of S into
// slabs, so the list route's answer does not depend on the order of a list (a label that does not scan is listed in any order).
#include "ehx_kernels.h"

namespace ehx {

// one workgroup per query (launch_grouped_range_seed)
__global__ __launch_bounds__(256) void grouped_range_seed_kernel(const uint64_t* __restrict__ list,
                                                                 const uint64_t* __restrict__ start,
                                                                 const uint64_t* __restrict__ end,
                                                                 uint64_t* __restrict__ pool, uint32_t* __restrict__ pool_cnt) {
  const uint32_t q = blockIdx.x;
  const uint64_t b = start[q], e = end[q];
  const uint64_t len = e > b ? e - b : 0ull;
  const uint64_t stride = (len + kLargeKSample - 1u) / kLargeKSample;
  const uint32_t n_sample = stride ? (uint32_t)((len + stride - 1u) / stride) : 0u;   // (<= kLargeKSample <= kPoolCap)
  const uint64_t* mine = list + b;
  for (uint32_t i = threadIdx.x; i < n_sample; i += 256u) pool[(size_t)q * kPoolCap + i] = mine[(uint64_t)i * stride];
  if (threadIdx.x == 0) pool_cnt[q] = n_sample;
}

// one workgroup per query (launch_grouped_range_slab)
__global__ __launch_bounds__(256) void grouped_range_slab_kernel(const uint64_t* __restrict__ list,
                                                                 const uint64_t* __restrict__ start,
                                                                 const uint64_t* __restrict__ end, uint64_t slab,
                                                                 uint32_t first, uint64_t* __restrict__ pool,
                                                                 uint32_t* __restrict__ pool_cnt, float* __restrict__ radius,
                                                                 uint32_t* __restrict__ top_cnt, uint32_t* __restrict__ work) {
  const uint32_t q = blockIdx.x;
  const uint64_t b = start[q], e = end[q];
  const uint64_t len = e > b ? e - b : 0ull, at = slab * kPoolCap;
  const uint64_t left = at < len ? len - at : 0ull;
  const uint32_t n = left < kPoolCap ? (uint32_t)left : kPoolCap;
  const uint64_t* mine = list + b + at;
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

hipError_t launch_grouped_range_seed(const uint64_t* list, const uint64_t* start, const uint64_t* end, uint64_t* pool,
                                     uint32_t* pool_cnt, uint32_t nq, hipStream_t st) {
  if (nq == 0) return hipSuccess;
  if (!list || !start || !end || !pool || !pool_cnt) return hipErrorInvalidValue;
  hipLaunchKernelGGL(grouped_range_seed_kernel, dim3(nq), dim3(256), 0, st, list, start, end, pool, pool_cnt);
  return hipGetLastError();
}

hipError_t launch_grouped_range_slab(const uint64_t* list, const uint64_t* start, const uint64_t* end, uint64_t slab,
                                     bool first, uint64_t* pool, uint32_t* pool_cnt, float* radius, uint32_t* top_cnt,
                                     uint32_t* work, uint32_t nq, hipStream_t st) {
  if (nq == 0) return hipSuccess;
  if (!list || !start || !end || !pool || !pool_cnt || (first && (!radius || !top_cnt || !work))) return hipErrorInvalidValue;
  hipLaunchKernelGGL(grouped_range_slab_kernel, dim3(nq), dim3(256), 0, st, list, start, end, slab, first ? 1u : 0u, pool,
                     pool_cnt, radius, top_cnt, work);
  return hipGetLastError();
}

}  // namespace ehx
