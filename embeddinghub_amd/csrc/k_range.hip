// Exact range search (ehx_range*): every row whose canonical (oracle-order) distance D(q, x) is <= radius[q], ordered by
// (distance, id), the first max_results of them written and ALL of them counted.
//   range_exact_kernel    every row's canonical distance, any layout (fp32 / binary16 / block-permuted rows); the rows
//                         inside the radius are appended to the query's pool, kPoolCap (distance, id) keys
//   range_emit_kernel     one workgroup per query: the pool sorted in LDS, the page and the counts written
//   range_thr_kernel      int8 path: the caller's radius -> the int8 filter scan's score threshold (derivation below)
//   range_rerank_kernel   int8 path: canonical distances of the scan's survivors, cut at the radius, sorted, emitted
//   range_iota_kernel     0, 1, 2, ... (a graph space's overflow fall-back lists every row for launch_among)
// Every distance comes from the exact paths' one row walk (walk_row, k_exact_common.h), which also holds the row layouts,
// the on-the-fly cosine scaling, the keys and the page writer.
//
// One counter serves as pool fill, overflow flag and total: a row inside the radius ALWAYS adds 1 to pool_cnt[q] and is
// stored only while its slot is below kPoolCap, so pool_cnt[q] is the exact number of rows inside the radius whatever
// happens, and pool_cnt[q] > kPoolCap says that the pool is incomplete (the host then answers the query with the exact kNN
// pipeline at k = max_results <= kPoolCap: the answer is the top max_results of the whole space, the total stays).
//
// The threshold of the int8 scan (range_thr_kernel).  The scan keeps every (row, query) with S_lower <= thr[q]
// (k_flati8.hip), S_lower a certified lower bound of the row's score S, and the query's (u, v) of
// launch_prep_queries_i8 map a score to a distance, D = u S + v with u > 0.  The re-rank of the kNN engine
// (rerank256_kernel) rests on one statement about every row x of the space and every score s:
//     (C)   S_lower(x) >= s   and   lb(s) - cert_margin(scale = max(|d|, |lb(s)|)) > d      ==>      D(q, x) > d,
// with lb(s) = fma(u, s, v): a row whose lower bound maps to a distance more than the margin above d is not within d.
// Range search needs the contrapositive at d = r: D(q, x) <= r must imply S_lower(x) <= thr, i.e. thr must be chosen so
// that EVERY s > thr satisfies the second premise of (C) at d = r.  Direction by direction:
//   1. f(L) = L - base - 2e-6 max(|r|, |L|, qn, 1) (cert_margin's form, base >= 0 independent of L) is increasing in L
//      with slope >= 1 - 2e-6, so it suffices to find ONE L* with f(L*) > r: every lb >= L* then has f(lb) > r.
//   2. m = cert_margin(scale = |r|) = base + 2e-6 max(|r|, qn, 1).  L* = r + 1.001 m: |L*| <= |r| + 1.001 m, hence
//      f(L*) >= r + 1.001 m - base - 2e-6 max(|r|, qn, 1) - 2e-6 * 1.001 m = r + m (0.001 - 2.002e-6) > r   (m > 0).
//      L* is then moved UP by two units in its last place: the fp32 evaluation only ever errs towards a larger threshold.
//   3. lb(s) >= L* for every s > thr: t = (L* - v) / u is two roundings away from the real quotient (relative 2^-23);
//      thr = t + 4.8e-7 |t| lies above the real quotient by more than that, so u s + v > L* in real arithmetic for
//      every s > thr, and the single rounding of the fma is monotone and L* is a float: fma(u, s, v) >= L*.
//   A larger threshold is always sound (more survivors, all of them re-ranked in the oracle's arithmetic and cut at the
//   radius there); a smaller one could hide a member.  Every step above rounds outward, i.e. up.
//   Not bounded by this: u NaN or not positive (a query the filter cannot bound), a radius of +-Inf, a margin or quotient
//   that is not finite (max_sumsq Inf / NaN) — those queries are MARKED (ovf[q] = 2) and scanned under -inf: the exact
//   kernel answers them.  A NaN radius has no members: -inf, not marked, the empty pool is its answer.  Padding queries keep
//   the -inf launch_prep_queries_i8 gave them.
#include "ehx_kernels.h"

namespace ehx {

namespace {

constexpr uint32_t kEmitThreads = 256;

}  // namespace

// Grid (query slots, blocks): slot j answers query sel[j] (sel == nullptr: j); block b walks steps b, b + gridDim.y, ...
// of the rows [0, n_rows), a step being 256 rows (fp32 rows: one lane per row) or 64 rows (binary16 and block-permuted rows: a
// 4-lane group per row) of walk_row.  The prepared query sits in LDS (permuted like the rows for the block-permuted layout).
// A wave reserves the slots of its members with one atomic.
template <int LAYOUT, int METRIC>
__global__ __launch_bounds__(256) void range_exact_kernel(const RangeArgs a) {
  constexpr uint32_t kStep = walk_rows<LAYOUT, true>(256);
  extern __shared__ float4 range_lds[];
  float* qs = (float*)range_lds;
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t j = blockIdx.x;
  const uint32_t q = a.sel ? a.sel[j] : j;
  const float r = a.radius[q];
  if (!(r == r)) return;   // a NaN radius has no members (the same in every lane: the whole workgroup leaves)
  stage_query_lds<LAYOUT>(qs, a.Q + (size_t)q * a.rows.ld, a.rows.ld, tid, 256);
  __syncthreads();
  uint64_t* pool = a.pool + (size_t)j * kPoolCap;
  const uint32_t slot0 = walk_slot<LAYOUT, true>(tid);
  for (uint64_t p0 = (uint64_t)blockIdx.y * kStep; p0 < a.rows.n_rows; p0 += (uint64_t)gridDim.y * kStep) {
    const uint64_t id = p0 + (uint64_t)slot0;
    bool mine;
    const float d = walk_row<LAYOUT, METRIC, true>(a.rows, qs, id, id < a.rows.n_rows, tid, &mine);
    const bool in = mine && d <= r;   // (a NaN distance compares false: never a member)
    const unsigned long long mask = __ballot(in);
    if (mask) {
      const uint32_t n_in = (uint32_t)__builtin_popcountll(mask);
      uint32_t base = 0;
      if (lane == (int)__builtin_ctzll(mask)) base = atomicAdd(&a.pool_cnt[j], n_in);
      base = (uint32_t)__shfl((int)base, (int)__builtin_ctzll(mask), 64);
      const uint32_t slot = base + (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
      if (in && slot < kPoolCap) pool[slot] = dist_key(d, (uint32_t)id, true);
    }
  }
}

// One workgroup per query slot: the pool's keys (canonical already) sorted, the page written; total[q] = the counter.  A
// slot whose pool overflowed writes its total only: the exact kNN pipeline writes its row.
__global__ __launch_bounds__(kEmitThreads) void range_emit_kernel(const uint64_t* __restrict__ pool,
                                                                  const uint32_t* __restrict__ pool_cnt,
                                                                  const uint32_t* __restrict__ sel, uint32_t max_results,
                                                                  uint64_t* __restrict__ out_ids,
                                                                  float* __restrict__ out_dist,
                                                                  uint32_t* __restrict__ out_count,
                                                                  uint64_t* __restrict__ out_total) {
  __shared__ uint64_t keys[kPoolCap];
  const uint32_t tid = threadIdx.x, j = blockIdx.x;
  const uint32_t q = sel ? sel[j] : j;
  const uint32_t cnt = pool_cnt[j];
  if (tid == 0 && out_total) out_total[q] = cnt;
  if (cnt > kPoolCap) return;
  for (uint32_t i = tid; i < cnt; i += kEmitThreads) keys[i] = pool[(size_t)j * kPoolCap + i];
  pad_and_sort_lds<kEmitThreads>(keys, cnt, tid);
  emit_page([&](uint32_t i) { return keys[i]; }, cnt, max_results, out_ids + (size_t)q * max_results,
            out_dist + (size_t)q * max_results, out_count + q, 0, tid, kEmitThreads);
}

// One lane per query: the threshold of the file header.  ovf[q] = 2 marks a query the bound does not serve.
__global__ __launch_bounds__(256) void range_thr_kernel(const float* __restrict__ radius, const float2* __restrict__ quv,
                                                        const float* __restrict__ max_sumsq, uint32_t nq, uint32_t dims,
                                                        int metric, float* __restrict__ thr, uint32_t* __restrict__ ovf) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= nq) return;   // (padding queries keep -inf)
  const float r = radius[q];
  const float2 uv = quv[q];
  float t = -__builtin_inff();
  bool mark = false;
  if (r == r) {
    if (__builtin_isinf(r) || !(uv.x > 0.0f) || __builtin_isinf(uv.x)) {
      mark = true;
    } else {
      const float qn = metric == 0 ? uv.y : (metric == 1 ? uv.x * uv.x : 1.0f);
      const float m = cert_margin(metric, dims, qn, max_sumsq ? *max_sumsq : __builtin_inff(), fabsf(r));
      float L = r + 1.001f * m;
      L += fabsf(L) * 2.4e-7f;                 // two units in the last place, upward
      t = (L - uv.y) / uv.x;
      t += fabsf(t) * 4.8e-7f;                 // above the real quotient
      if (!(t == t) || __builtin_isinf(t) || !(m == m)) {
        mark = true;
        t = -__builtin_inff();
      }
    }
  }
  thr[q] = t;
  if (mark) ovf[q] = 2u;
}

// One workgroup per query: the survivors of the int8 scan — pool keys (S_lower, id), unsorted, each row at most once —
// get their canonical distances from the stored rows (walk_row; fp32: one lane per row, binary16: a 4-lane group per
// row), those above the radius are dropped, the rest sorted by (distance, id) and emitted; kept[q] = how many stayed = the exact total (every member is in
// the pool: header).  A query that is flagged (pool overflow, or marked by range_thr_kernel) writes nothing here.
template <bool HALFX, int METRIC>
__global__ __launch_bounds__(kEmitThreads) void range_rerank_kernel(const RangeRerankArgs a) {
  extern __shared__ float4 range_lds[];
  uint64_t* keys = (uint64_t*)range_lds;   // (pool_rerank_sorted's image: the sorted keys at its head)
  const uint32_t tid = threadIdx.x, q = blockIdx.x;
  if (a.ovf[q]) return;
  const uint32_t cnt = a.pool_cnt[q] < kPoolCap ? a.pool_cnt[q] : kPoolCap;
  const uint32_t total = pool_rerank_sorted<HALFX ? kLayoutF16 : kLayoutF32, METRIC, kEmitThreads>(
      range_lds, a.rows, a.Q + (size_t)q * a.rows.ld, a.pool + (size_t)q * kPoolCap, cnt, a.radius[q], tid);
  if (tid == 0) {
    a.kept[q] = total;
    if (a.out_total) a.out_total[q] = total;
  }
  emit_page([&](uint32_t i) { return keys[i]; }, total, a.max_results, a.out_ids + (size_t)q * a.max_results,
            a.out_dist + (size_t)q * a.max_results, a.out_count + q, 0, tid, kEmitThreads);
}

__global__ __launch_bounds__(256) void range_iota_kernel(uint64_t* __restrict__ out, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n) out[i] = i;
}

namespace {

typedef void (*RangeFn)(const RangeArgs);
const RangeFn kExactFns[9] = {   // [layout * 3 + metric]
    range_exact_kernel<kLayoutF32, 0>,  range_exact_kernel<kLayoutF32, 1>,  range_exact_kernel<kLayoutF32, 2>,
    range_exact_kernel<kLayoutF16, 0>,  range_exact_kernel<kLayoutF16, 1>,  range_exact_kernel<kLayoutF16, 2>,
    range_exact_kernel<kLayoutPerm, 0>, range_exact_kernel<kLayoutPerm, 1>, range_exact_kernel<kLayoutPerm, 2>};
const decltype(&range_rerank_kernel<false, 0>) kRerankFns[6] = {   // [half * 3 + metric]
    range_rerank_kernel<false, 0>, range_rerank_kernel<false, 1>, range_rerank_kernel<false, 2>,
    range_rerank_kernel<true, 0>,  range_rerank_kernel<true, 1>,  range_rerank_kernel<true, 2>};
DynLdsAttr g_exact_lds, g_rerank_lds;

}  // namespace

uint32_t range_step_rows(const RangeArgs& a) { return row_layout(a.rows.x_half, a.rows.x_perm) == kLayoutF32 ? 256u : 64u; }

uint32_t range_rerank_max_ld() { return (uint32_t)((kMaxLds - pool_rerank_lds_bytes(0)) / sizeof(float)) & ~31u; }

hipError_t launch_range_exact(const RangeArgs& a, uint32_t n_slots, hipStream_t st) {
  if (n_slots == 0 || a.rows.n_rows == 0) return hipSuccess;
  if (a.n_blocks == 0 || a.n_blocks > 65535u || (a.rows.ld & 31u) || a.rows.metric < 0 || a.rows.metric > 2) return hipErrorInvalidValue;
  const size_t lds = (size_t)a.rows.ld * sizeof(float);
  if (lds > kMaxLds) return hipErrorInvalidValue;
  hipError_t e = g_exact_lds.ensure(kExactFns, 9, lds);
  if (e != hipSuccess) return e;
  const int fn = row_layout(a.rows.x_half, a.rows.x_perm) * 3 + a.rows.metric;
  hipLaunchKernelGGL(kExactFns[fn], dim3(n_slots, a.n_blocks), dim3(256), lds, st, a);
  return hipGetLastError();
}

hipError_t launch_range_emit(const uint64_t* pool, const uint32_t* pool_cnt, const uint32_t* sel, uint32_t n_slots,
                             uint32_t max_results, uint64_t* out_ids, float* out_dist, uint32_t* out_count,
                             uint64_t* out_total, hipStream_t st) {
  if (n_slots == 0) return hipSuccess;
  if (max_results == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(range_emit_kernel, dim3(n_slots), dim3(kEmitThreads), 0, st, pool, pool_cnt, sel, max_results, out_ids,
                     out_dist, out_count, out_total);
  return hipGetLastError();
}

hipError_t launch_range_thr(const float* radius, const float2* quv, const float* max_sumsq, uint32_t nq, uint32_t dims,
                            int metric, float* thr, uint32_t* ovf, hipStream_t st) {
  if (nq == 0) return hipSuccess;
  hipLaunchKernelGGL(range_thr_kernel, dim3((nq + 255u) / 256u), dim3(256), 0, st, radius, quv, max_sumsq, nq, dims, metric,
                     thr, ovf);
  return hipGetLastError();
}

hipError_t launch_range_rerank(const RangeRerankArgs& a, hipStream_t st) {
  return launch_pool_rerank(kRerankFns, g_rerank_lds, a, a.max_results != 0, kEmitThreads, st);
}

hipError_t launch_range_iota(uint64_t* out, uint64_t n, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(range_iota_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, out, n);
  return hipGetLastError();
}

}  // namespace ehx
