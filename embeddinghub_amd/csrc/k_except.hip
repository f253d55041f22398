// kNN with per-query exclusion lists (ehx_knn_except*, ehx_except.cpp): row i of the answer is the first k rows in (canonical
// distance, id) order among the rows of the prefix that query i's list does NOT name — ehx_knn_masked's answer under the
// complement bitmap of the list, byte for byte.  The falling-radius kNN of k_radius.hip with the listed rows dropped in its
// re-rank; the int8 scan in front of it is untouched and knows nothing of the lists.
//   except_lists_kernel    once per device batch: every query's list — 64-bit ids, unsorted, with repeats, with ids at or
//                          beyond the prefix — becomes ascending unique 32-bit row ids in the call's scratch (a bitonic sort
//                          in LDS; the passes would otherwise each sort it again)
//   except_rerank_kernel   radius_rerank_kernel's modes and arguments plus the lists.  The order of work is the design:
//                            1  the query's sorted list into LDS (at most 16 KiB)
//                            2  the pool's keys read, each row id looked up in the list by binary search in LDS
//                            3  the survivors compacted into the pool's LDS image
//                            4  ONLY THEN rows are walked: the survivors' canonical distances (walk_row, dist_key), cut at the
//                               radius, sorted (staged_rerank_sorted, k_exact_common.h), merged by rank with the carried keys,
//                               the radius lowered or the page written (radius_carry_or_emit, ehx_kernels.h)
//                          An excluded row's bytes are never fetched: a user with 1000 seen items near their vector costs 1000
//                          searches in LDS, not 1000 rows of HBM traffic.
// Matrix instructions have no place here: every distance is the oracle's non-fused fp32 order (k_canon.h); the matrix cores
// work in the int8 scan in front.
//
// Why the answer is exact.  k_radius.hip's argument with "rows" read as ALLOWED rows — the rows of the prefix the query's list
// does not name, a fixed set: the list is no function of the search.
//   * Every radius is the k-th distance of k allowed rows (the seed's: of the allowed rows of the sample, +Inf while they
//     number fewer than k — range_thr_kernel then marks the query and the host answers it exactly), so it is at least the
//     true k-th allowed distance.
//   * The scan keeps every row with D <= r, allowed or not; the re-rank drops exactly the listed rows (a sorted unique list
//     and a binary search: a row is dropped iff its id is in the list) and cuts the others at r.  So a true member m, whose
//     D(m) is at most every radius there ever is, reaches the carried list in its own pass and leaves it only when k allowed
//     rows precede it: the induction over passes is k_radius.hip's.
//   * Excluded rows take pool slots.  A pool that overflows flags the query (sticky, as there), and the host answers it on
//     the exact route: this kernel over the slabs of ALL rows, the radius falling from +Inf — every allowed row passes one
//     re-rank, so the answer does not depend on a threshold at all.
#include "ehx_kernels.h"

namespace ehx {

namespace {

constexpr uint32_t kExceptThreads = 256;
constexpr uint32_t kExceptPer = kPoolCap / kExceptThreads;   // pool entries, or list entries, per thread
static_assert(kExceptMaxList == kPoolCap, "one list is one pool: excluded rows alone never need more than one pool");
static_assert(kExceptPer * kExceptThreads == kPoolCap && kExceptPer <= 32, "a thread's keep bits fit a word");

// LDS of the re-rank: pool_rerank_sorted's image (keys | prepared query | counter), then the sorted list, then the waves' sums
constexpr size_t kExceptExtraBytes = kExceptMaxList * sizeof(uint32_t) + 16u;
__host__ __device__ constexpr size_t except_rerank_lds_bytes(uint32_t ld) { return pool_rerank_lds_bytes(ld) + kExceptExtraBytes; }
constexpr uint32_t kExceptMaxLd = (uint32_t)((kMaxLds - except_rerank_lds_bytes(0)) / sizeof(float)) & ~31u;
static_assert(except_rerank_lds_bytes(kExceptMaxLd) <= kMaxLds, "the kernel's LDS fits one CU");
static_assert(kExceptMaxLd >= 16384, "rows of every width the int8 scan serves are re-ranked");
static_assert(pool_rerank_lds_bytes(32) % 16 == 0, "the list begins aligned");

// whether the ascending array a[0, n) holds id
__device__ __forceinline__ bool list_holds(const uint32_t* a, uint32_t n, uint32_t id) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && a[lo] == id;
}

// Exclusive prefix sum of one count per thread over the workgroup; *total: the sum.  sums: kExceptThreads / 64 words of LDS.
// A barrier inside: what the threads read before the call is read by all of them when it returns.
__device__ __forceinline__ uint32_t block_offsets(uint32_t mine, uint32_t* sums, uint32_t tid, uint32_t* total) {
  uint32_t incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(incl, d, 64);
    if ((int)(tid & 63u) >= d) incl += up;
  }
  if ((tid & 63u) == 63u) sums[tid >> 6] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < kExceptThreads / 64u; ++w) {
    const uint32_t s = sums[w];
    before += w < (tid >> 6) ? s : 0u;
    all += s;
  }
  *total = all;
  return before + incl - mine;
}

}  // namespace

// one workgroup per query (file header); thread t files entries [t kExceptPer, (t + 1) kExceptPer) of the sorted image
__global__ __launch_bounds__(kExceptThreads) void except_lists_kernel(const uint64_t* __restrict__ excl_ids,
                                                                      const uint64_t* __restrict__ excl_off, uint64_t n_rows,
                                                                      uint32_t* __restrict__ sorted,
                                                                      uint32_t* __restrict__ sorted_cnt) {
  __shared__ uint32_t ids[kExceptMaxList];
  __shared__ uint32_t sums[kExceptThreads / 64u];
  const uint32_t tid = threadIdx.x, q = blockIdx.x;
  const uint64_t b = excl_off[q], e = excl_off[q + 1];
  const uint64_t len = e > b ? e - b : 0ull;
  const uint32_t n = len < kExceptMaxList ? (uint32_t)len : kExceptMaxList;
  // (an id at or beyond the prefix names no row: it sorts behind every row id, with the padding)
  for (uint32_t i = tid; i < n; i += kExceptThreads) {
    const uint64_t id = excl_ids[b + i];
    ids[i] = id < n_rows ? (uint32_t)id : 0xFFFFFFFFu;
  }
  pad_and_sort_lds<kExceptThreads>(ids, n, tid);   // (a barrier in front of the sort and one behind its last step)
  uint32_t keep = 0, mine = 0;
#pragma unroll
  for (uint32_t j = 0; j < kExceptPer; ++j) {
    const uint32_t i = tid * kExceptPer + j;
    const uint32_t v = i < n ? ids[i] : 0xFFFFFFFFu;
    if (v != 0xFFFFFFFFu && (i == 0 || ids[i - 1] != v)) {
      keep |= 1u << j;
      ++mine;
    }
  }
  uint32_t total;
  uint32_t at = block_offsets(mine, sums, tid, &total);
  uint32_t* out = sorted + (size_t)q * kExceptMaxList;
#pragma unroll
  for (uint32_t j = 0; j < kExceptPer; ++j)
    if (keep & (1u << j)) out[at++] = ids[tid * kExceptPer + j];
  if (tid == 0) sorted_cnt[q] = total;
}

// One workgroup per query (file header); the control flow in front of the re-rank is radius_rerank_kernel's.
template <int LAYOUT, int METRIC>
__global__ __launch_bounds__(kExceptThreads) void except_rerank_kernel(const ExceptRerankArgs e) {
  extern __shared__ float4 except_lds[];
  const RadiusRerankArgs& a = e.r;
  uint64_t* keys = (uint64_t*)except_lds;   // (the pool image: the survivors' ids, then their sorted keys, at its head)
  float* qs = (float*)(keys + kPoolCap);
  uint32_t* kept_s = (uint32_t*)(qs + a.rows.ld);
  uint32_t* list = (uint32_t*)((unsigned char*)except_lds + pool_rerank_lds_bytes(a.rows.ld));
  uint32_t* sums = list + kExceptMaxList;
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
  // 1: the list and the prepared query into LDS
  const uint32_t slot = e.list_of ? e.list_of[q] : q;
  const uint32_t have = e.sorted_cnt[slot];
  const uint32_t n_list = have < kExceptMaxList ? have : kExceptMaxList;
  const uint32_t* __restrict__ src = e.sorted + (size_t)slot * kExceptMaxList;
  for (uint32_t i = tid; i < n_list; i += kExceptThreads) list[i] = src[i];
  stage_query_lds<LAYOUT>(qs, a.Q + (size_t)q * a.rows.ld, a.rows.ld, tid, kExceptThreads);
  if (tid == 0) *kept_s = 0;
  // 2: the pool's row ids into registers (coalesced: entry j kExceptThreads + tid), each looked up in the list
  const uint64_t* __restrict__ pool = a.pool + (size_t)q * kPoolCap;
  uint32_t id[kExceptPer];
#pragma unroll
  for (uint32_t j = 0; j < kExceptPer; ++j) {
    const uint32_t i = j * kExceptThreads + tid;
    id[j] = i < cnt ? (uint32_t)pool[i] : 0u;
  }
  __syncthreads();
  uint32_t keep = 0, mine = 0;
#pragma unroll
  for (uint32_t j = 0; j < kExceptPer; ++j) {
    if (j * kExceptThreads + tid < cnt && !list_holds(list, n_list, id[j])) {
      keep |= 1u << j;
      ++mine;
    }
  }
  // 3: the survivors compacted into the image (any order: the sort behind the walk orders them)
  uint32_t n_live;
  uint32_t at = block_offsets(mine, sums, tid, &n_live);
#pragma unroll
  for (uint32_t j = 0; j < kExceptPer; ++j)
    if (keep & (1u << j)) keys[at++] = id[j];
  __syncthreads();
  // 4: only the survivors' rows are read
  const uint32_t total = staged_rerank_sorted<LAYOUT, METRIC, kExceptThreads>(except_lds, a.rows, n_live, r, tid);
  radius_carry_or_emit<kExceptThreads>(a, keys, total, n_live, q, tid);
}

namespace {

const decltype(&except_rerank_kernel<0, 0>) kExceptRerankFns[9] = {   // [layout * 3 + metric]
    except_rerank_kernel<kLayoutF32, 0>,  except_rerank_kernel<kLayoutF32, 1>,  except_rerank_kernel<kLayoutF32, 2>,
    except_rerank_kernel<kLayoutF16, 0>,  except_rerank_kernel<kLayoutF16, 1>,  except_rerank_kernel<kLayoutF16, 2>,
    except_rerank_kernel<kLayoutPerm, 0>, except_rerank_kernel<kLayoutPerm, 1>, except_rerank_kernel<kLayoutPerm, 2>};
DynLdsAttr g_except_lds;

}  // namespace

uint32_t except_rerank_max_ld() { return kExceptMaxLd; }

hipError_t launch_except_lists(const uint64_t* excl_ids, const uint64_t* excl_off, uint32_t nq, uint64_t n_rows,
                               uint32_t* sorted, uint32_t* sorted_cnt, hipStream_t st) {
  if (nq == 0) return hipSuccess;
  // (excl_ids may be nullptr when every list is empty: nothing is read through it then)
  if (!excl_off || !sorted || !sorted_cnt || n_rows > 0xFFFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(except_lists_kernel, dim3(nq), dim3(kExceptThreads), 0, st, excl_ids, excl_off, n_rows, sorted, sorted_cnt);
  return hipGetLastError();
}

hipError_t launch_except_rerank(const ExceptRerankArgs& e, hipStream_t st) {
  const RadiusRerankArgs& a = e.r;
  if (a.nq == 0) return hipSuccess;
  if (a.k == 0 || a.k > kLargeKMax || a.mode > kRadiusSeed || !e.sorted || !e.sorted_cnt || (a.rows.ld & 31u) ||
      a.rows.ld > kExceptMaxLd || a.rows.metric < 0 || a.rows.metric > 2)
    return hipErrorInvalidValue;
  const size_t lds = except_rerank_lds_bytes(a.rows.ld);
  hipError_t err = g_except_lds.ensure(kExceptRerankFns, 9, lds);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(kExceptRerankFns[row_layout(a.rows.x_half, a.rows.x_perm) * 3 + a.rows.metric], dim3(a.nq),
                     dim3(kExceptThreads), lds, st, e);
  return hipGetLastError();
}

}  // namespace ehx
