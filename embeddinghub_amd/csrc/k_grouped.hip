// Grouped kNN (ehx_knn_grouped*, ehx_grouped.cpp), unfiltered, under row bitmaps and under a label column: the first k
// ELIGIBLE rows of the rows searched in (canonical distance, id) order, a row being eligible iff its label is kGroupNone or
// fewer than per_group ("m") rows of its label precede it in that order.  The falling-radius kNN of k_radius.hip with a cap
// per label in its re-rank.  Whatever names a query's rows — nothing, a bitmap, a wanted label — the host turns it into ONE
// shape: query q searches list[start[q], end[q]), start and end read from a per-batch device array, so any number of lists
// fits one launch and queries under one filter name the same range; list == nullptr is the identity list (entry i is row i),
// which makes the unfiltered search the range [0, n_eff).
//   grouped_range_seed_kernel   the scan route's sample: every stride-th entry of the range by rank, stride = ceil(len /
//                               kLargeKSample), at most kLargeKSample of them (a scanning filter's list is ascending, so the
//                               sample spreads over the id space; the identity list gives rows 0, stride, 2 stride, ...);
//                               the seed-mode re-rank makes the first radius of it
//   grouped_range_slab_kernel   the list route's "pass": entries [b kPoolCap, (b + 1) kPoolCap) of the range, as many as
//                               remain (possibly none: the re-rank keeps its carried keys through an empty pool, and an empty
//                               range — which reads nothing, whatever list is — still has its page written); in front of the
//                               first slab the radius +Inf, nothing carried, work 0.  Both are a copy of at most 32 KiB per
//                               query: nothing to tune.
//   grouped_rerank_kernel   radius_rerank_kernel's modes and arguments plus the labels: the pool's canonical distances, cut
//                           at the radius and sorted (pool_rerank_sorted, unchanged), then
//                             A  the sorted hits capped — at most m per label — and cut at k,
//                             B  merged by rank with the carried keys, the merged list of at most 2 k keys capped AGAIN
//                                (a carried key may be displaced by m nearer hits of its label) and cut at k;
//                           the k-th key kept is the new radius.  Seed mode: the k-th key of the capped sample is the first
//                           radius (+Inf while the capped sample holds fewer than k); nothing is carried from the sample.
// Every distance comes from walk_row, the keys from dist_key and the page from emit_page, as in k_radius.hip.
//
// The cap of an ascending list (cap_sorted): the labels of its entries are fetched into LDS, (label << 32 | position) is
// sorted (block_sort_lds), an entry's rank in its label is its sorted index minus its segment's start (lower_bound_lds);
// it is kept iff that rank is below m or the label is kGroupNone (such rows are never ranked against one another); a
// prefix sum over the keep bits in position order compacts the first k kept.
//
// Why the answer is exact.  The rows a query may return — the prefix, its allowed rows, the rows of its label — are a FIXED
// set S: neither a bitmap nor a label column is a function of the search.  cap(S) below is "S in key order, every row
// dropped that is not among the first m of its label in S", cap_k(S) its first k entries; every step speaks of subsets of S
// only.  The scan's flush drops every row outside S before it takes a pool slot and the ranges hold S alone, so no row
// outside S ever reaches a cap: it neither appears nor counts (FILTER FIRST, THEN CAP).
//   * "At most m per label" is a partition matroid: greedy by ascending key over any set S keeps exactly the rows that are
//     among the first m of their label in S — cap(S) — and the answer over S is cap_k(S).
//   * A row that is not among the first m of its label in S is not among them in any superset of S: m nearer rows of its
//     label stay nearer.
//   * A row with k kept rows before it in S has at least k kept rows before it in any superset: per label, the kept rows
//     below x number min(m, rows of that label below x), which only grows as S grows (kGroupNone rows: each its own label).
//   * So rows dropped by a cap or by a cut at k never return: cap_k(A u B) = cap_k(cap_k(A) u cap_k(B)).  A is a pass's
//     hits, B the carried list: step B above computes the right side.
//   * The k-th key kept over ANY subset of S bounds the true k-th eligible distance from above (third point), so
//     every radius is such a bound, the scan under it keeps every member (k_radius.hip's header: the threshold keeps every
//     row with D <= r), and the cut at the radius drops none.
//   * The rest is k_radius.hip's induction over passes: a member leaves the carried list only when a cap or a cut drops it,
//     and then it is no member.  The list route runs the same kernel over the slabs of ALL of S, radius +Inf first; the
//     identity above holds for any split of S into slabs, in any order, so its answer does not depend on the order of a
//     list (a filter that does not scan may be listed in any order).
//   * Flagged queries (pool overflow, a radius the bound does not serve) write nothing here: the host answers them on the
//     list route.
#include "ehx_kernels.h"

namespace ehx {

namespace {

constexpr uint32_t kGroupedThreads = 256;
constexpr uint32_t kKeepWords = kPoolCap / 32;   // keep bits of a capped list, one per position
static_assert(kLargeKMax <= kGroupedThreads, "one thread per carried key and per capped hit");
static_assert(kKeepWords == 2 * 64, "one wave sums the keep words, two per lane");

// LDS behind pool_rerank_sorted's image (the sorted hits stay at its head): the cap's sort image [kPoolCap], the capped hits
// [kLargeKMax], the carried keys [kLargeKMax], the merged list [2 kLargeKMax], the capped merged list [kLargeKMax], the keep
// bits [kKeepWords] and their exclusive prefix sums [kKeepWords + 1] (the last: the total), padded to 16 bytes
constexpr size_t kGroupedExtraBytes =
    (kPoolCap + 5u * kLargeKMax) * sizeof(uint64_t) + ((2u * kKeepWords + 1u) * sizeof(uint32_t) + 15u) / 16u * 16u;
__host__ __device__ constexpr size_t grouped_rerank_lds_bytes(uint32_t ld) { return pool_rerank_lds_bytes(ld) + kGroupedExtraBytes; }
constexpr uint32_t kGroupedMaxLd = (uint32_t)((kMaxLds - grouped_rerank_lds_bytes(0)) / sizeof(float)) & ~31u;
static_assert(grouped_rerank_lds_bytes(kGroupedMaxLd) <= kMaxLds, "the kernel's LDS fits one CU");
static_assert(kGroupedMaxLd >= 16384, "rows of every width the int8 scan serves are re-ranked");
static_assert(pool_rerank_lds_bytes(32) % sizeof(uint64_t) == 0, "the extra block holds 8-byte keys");

// The cap of src[0, n), ascending (distance, id) keys of rows below the labels' length, n <= kPoolCap: dst[0, min(kept, k))
// = the first k kept keys, in order; returns kept.  gk [kPoolCap], bits [kKeepWords], pre [kKeepWords + 1]: scratch.  Ends
// behind a barrier.
template <uint32_t T>
__device__ __forceinline__ uint32_t cap_sorted(const uint64_t* src, uint32_t n, const uint32_t* __restrict__ group_of,
                                               uint32_t per_group, uint32_t k, uint64_t* gk, uint32_t* bits, uint32_t* pre,
                                               uint64_t* dst, uint32_t tid) {
  for (uint32_t i = tid; i < n; i += T) gk[i] = ((uint64_t)group_of[(uint32_t)src[i]] << 32) | i;
  for (uint32_t w = tid; w < kKeepWords; w += T) bits[w] = 0;
  pad_and_sort_lds<T>(gk, n, tid);   // (a barrier in front of the sort and one behind its last step)
  for (uint32_t j = tid; j < n; j += T) {
    const uint64_t e = gk[j];
    const uint32_t label = (uint32_t)(e >> 32), pos = (uint32_t)e;
    const bool keep = label == kGroupNone || j - lower_bound_lds(gk, n, (uint64_t)label << 32) < per_group;
    if (keep) atomicOr(&bits[pos >> 5], 1u << (pos & 31u));
  }
  __syncthreads();
  if (tid < 64u) {   // wave 0: lane l sums words 2 l and 2 l + 1
    const uint32_t c0 = (uint32_t)__builtin_popcount(bits[2u * tid]), c1 = (uint32_t)__builtin_popcount(bits[2u * tid + 1u]);
    uint32_t incl = c0 + c1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d, 64);
      if ((int)tid >= d) incl += up;
    }
    pre[2u * tid] = incl - c0 - c1;
    pre[2u * tid + 1u] = incl - c1;
    if (tid == 63u) pre[kKeepWords] = incl;
  }
  __syncthreads();
  for (uint32_t p = tid; p < n; p += T) {
    const uint32_t w = bits[p >> 5], b = 1u << (p & 31u);
    if (w & b) {
      const uint32_t at = pre[p >> 5] + (uint32_t)__builtin_popcount(w & (b - 1u));
      if (at < k) dst[at] = src[p];
    }
  }
  __syncthreads();
  return pre[kKeepWords];
}

}  // namespace

// entry i of query q's range: list[start + i], or row start + i of the identity list
__device__ __forceinline__ uint64_t range_entry(const uint64_t* __restrict__ list, uint64_t at) { return list ? list[at] : at; }

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
  for (uint32_t i = threadIdx.x; i < n_sample; i += 256u) pool[(size_t)q * kPoolCap + i] = range_entry(list, b + (uint64_t)i * stride);
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
  for (uint32_t i = threadIdx.x; i < n; i += 256u) pool[(size_t)q * kPoolCap + i] = range_entry(list, b + at + i);
  if (threadIdx.x == 0) {
    pool_cnt[q] = n;
    if (first) {
      radius[q] = __builtin_inff();
      top_cnt[q] = 0;
      work[q] = 0;
    }
  }
}

// One workgroup per query (file header); the control flow in front of the re-rank is radius_rerank_kernel's.
template <int LAYOUT, int METRIC>
__global__ __launch_bounds__(kGroupedThreads) void grouped_rerank_kernel(const GroupedRerankArgs g) {
  extern __shared__ float4 grouped_lds[];
  const RadiusRerankArgs& a = g.r;
  uint64_t* keys = (uint64_t*)grouped_lds;   // (pool_rerank_sorted's image: the sorted keys at its head)
  uint64_t* gk = (uint64_t*)((unsigned char*)grouped_lds + pool_rerank_lds_bytes(a.rows.ld));
  uint64_t* hits = gk + kPoolCap;
  uint64_t* carried = hits + kLargeKMax;
  uint64_t* merged = carried + kLargeKMax;
  uint64_t* best = merged + 2u * kLargeKMax;
  uint32_t* bits = (uint32_t*)(best + kLargeKMax);
  uint32_t* pre = bits + kKeepWords;
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
  const uint32_t total = pool_rerank_sorted<LAYOUT, METRIC, kGroupedThreads>(
      grouped_lds, a.rows, a.Q + (size_t)q * a.rows.ld, a.pool + (size_t)q * kPoolCap, cnt, r, tid);
  // A: the hits capped, cut at k
  const uint32_t kept = cap_sorted<kGroupedThreads>(keys, total, g.group_of, g.per_group, a.k, gk, bits, pre, hits, tid);
  const uint32_t nh = kept < a.k ? kept : a.k;
  if (seed) {
    // the capped sample gives the first radius and nothing else
    if (tid == 0) {
      a.radius[q] = nh >= a.k ? ordered_to_f32((uint32_t)(hits[a.k - 1] >> 32)) : __builtin_inff();
      a.pool_cnt[q] = 0;
      a.top_cnt[q] = 0;
      a.work[q] = cnt;
    }
    return;
  }
  // B: merged by rank with the carried keys (distinct keys: ids are), capped again, cut at k
  const uint32_t have = a.top_cnt[q];
  const uint32_t nc = have < a.k ? have : a.k;   // (never more than k: this kernel wrote it)
  uint64_t* tq = a.top + (size_t)q * kLargeKMax;
  uint64_t c = kKeyInf;
  if (tid < nc) {
    c = tq[tid];
    carried[tid] = c;
  }
  __syncthreads();
  if (tid < nh) {
    const uint64_t h = hits[tid];
    merged[tid + lower_bound_lds(carried, nc, h)] = h;
  }
  if (tid < nc) merged[tid + lower_bound_lds(hits, nh, c)] = c;
  __syncthreads();
  const uint32_t kept2 = cap_sorted<kGroupedThreads>(merged, nh + nc, g.group_of, g.per_group, a.k, gk, bits, pre, best, tid);
  const uint32_t n_out = kept2 < a.k ? kept2 : a.k;
  if (a.mode == kRadiusLast) {
    emit_page([&](uint32_t i) { return best[i]; }, n_out, a.k, a.out_ids + (size_t)q * a.k, a.out_dist + (size_t)q * a.k,
              a.out_count + q, 0, tid, kGroupedThreads);
  } else {
    if (tid < n_out) tq[tid] = best[tid];
    if (tid == 0) {
      a.top_cnt[q] = n_out;
      a.pool_cnt[q] = 0;
      // (every key held is <= r: the k-th of them is the new, smaller or equal, radius)
      if (n_out >= a.k) a.radius[q] = ordered_to_f32((uint32_t)(best[a.k - 1] >> 32));
    }
  }
  if (tid == 0) a.work[q] += cnt;
}

namespace {

const decltype(&grouped_rerank_kernel<0, 0>) kGroupedRerankFns[9] = {   // [layout * 3 + metric]
    grouped_rerank_kernel<kLayoutF32, 0>,  grouped_rerank_kernel<kLayoutF32, 1>,  grouped_rerank_kernel<kLayoutF32, 2>,
    grouped_rerank_kernel<kLayoutF16, 0>,  grouped_rerank_kernel<kLayoutF16, 1>,  grouped_rerank_kernel<kLayoutF16, 2>,
    grouped_rerank_kernel<kLayoutPerm, 0>, grouped_rerank_kernel<kLayoutPerm, 1>, grouped_rerank_kernel<kLayoutPerm, 2>};
DynLdsAttr g_grouped_lds;

}  // namespace

uint32_t grouped_rerank_max_ld() { return kGroupedMaxLd; }

// (list may be nullptr: the identity list)
hipError_t launch_grouped_range_seed(const uint64_t* list, const uint64_t* start, const uint64_t* end, uint64_t* pool,
                                     uint32_t* pool_cnt, uint32_t nq, hipStream_t st) {
  if (nq == 0) return hipSuccess;
  if (!start || !end || !pool || !pool_cnt) return hipErrorInvalidValue;
  hipLaunchKernelGGL(grouped_range_seed_kernel, dim3(nq), dim3(256), 0, st, list, start, end, pool, pool_cnt);
  return hipGetLastError();
}

hipError_t launch_grouped_range_slab(const uint64_t* list, const uint64_t* start, const uint64_t* end, uint64_t slab,
                                     bool first, uint64_t* pool, uint32_t* pool_cnt, float* radius, uint32_t* top_cnt,
                                     uint32_t* work, uint32_t nq, hipStream_t st) {
  if (nq == 0) return hipSuccess;
  if (!start || !end || !pool || !pool_cnt || (first && (!radius || !top_cnt || !work))) return hipErrorInvalidValue;
  hipLaunchKernelGGL(grouped_range_slab_kernel, dim3(nq), dim3(256), 0, st, list, start, end, slab, first ? 1u : 0u, pool,
                     pool_cnt, radius, top_cnt, work);
  return hipGetLastError();
}

hipError_t launch_grouped_rerank(const GroupedRerankArgs& g, hipStream_t st) {
  const RadiusRerankArgs& a = g.r;
  if (a.nq == 0) return hipSuccess;
  if (a.k == 0 || a.k > kLargeKMax || a.mode > kRadiusSeed || g.per_group == 0 || (!g.group_of && a.rows.n_rows) ||
      (a.rows.ld & 31u) || a.rows.ld > kGroupedMaxLd || a.rows.metric < 0 || a.rows.metric > 2)
    return hipErrorInvalidValue;
  const size_t lds = grouped_rerank_lds_bytes(a.rows.ld);
  hipError_t e = g_grouped_lds.ensure(kGroupedRerankFns, 9, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kGroupedRerankFns[row_layout(a.rows.x_half, a.rows.x_perm) * 3 + a.rows.metric], dim3(a.nq),
                     dim3(kGroupedThreads), lds, st, g);
  return hipGetLastError();
}

}  // namespace ehx
