// Exact range search under row bitmaps (ehx_range_masked*), the list route: every row of a query's OWN list — its mask's
// ascending list of allowed rows (k_masked.hip's compaction) — whose canonical (oracle-order) distance is <= radius[q].
//   range_list_kernel         the canonical distance of every listed row, any layout (fp32 / binary16 / block-permuted rows);
//                             the rows inside the radius are appended to the slot's pool, kPoolCap (distance, id) keys
//   range_scan_radii_kernel   the radii the int8 scan of a device batch runs under: NaN for the queries it does not answer
// The kernel is the unfiltered search's exact kernel (k_range.hip) with the row ids read from a list: every distance comes
// from the exact paths' one row walk (walk_row, k_exact_common.h), the keys from dist_key, and one counter serves as pool
// fill, overflow flag and total, as k_range.hip's header has it — a member ALWAYS adds 1 to pool_cnt[j] and is stored only
// while its slot is below kPoolCap.  launch_range_emit (k_range.hip) sorts the pools and writes the pages.
#include "ehx_kernels.h"

namespace ehx {

// Grid (query slots, blocks): slot j answers query sel[j] (sel == nullptr: j) over the list ids[list_off[j] ..
// list_off[j] + list_len[j]); block b walks steps b, b + gridDim.y, ... of it, a step being 256 entries (fp32 rows: one lane
// per row) or 64 entries (binary16 and block-permuted rows: a 4-lane group per row, whose lanes read the one entry together)
// of walk_row.  The grid is sized from the longest list of the launch: the blocks of a shorter list that have no step leave
// before the query is staged.  The prepared query sits in LDS (permuted like the rows for the block-permuted layout).  A wave
// reserves the slots of its members with one atomic.
template <int LAYOUT, int METRIC>
__global__ __launch_bounds__(256) void range_list_kernel(const RangeListArgs a) {
  constexpr uint32_t kStep = walk_rows<LAYOUT, true>(256);
  extern __shared__ float4 rangem_lds[];
  float* qs = (float*)rangem_lds;
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t j = blockIdx.x;
  const uint32_t q = a.sel ? a.sel[j] : j;
  const float r = a.radius[q];
  if (!(r == r)) return;   // a NaN radius has no members (the same in every lane: the whole workgroup leaves)
  const uint64_t len = a.list_len[j];
  if ((uint64_t)blockIdx.y * kStep >= len) return;   // (a shorter list than the launch's longest: nothing to do)
  const uint64_t* __restrict__ list = a.ids + a.list_off[j];
  stage_query_lds<LAYOUT>(qs, a.Q + (size_t)q * a.rows.ld, a.rows.ld, tid, 256);
  __syncthreads();
  uint64_t* pool = a.pool + (size_t)j * kPoolCap;
  const uint32_t slot0 = walk_slot<LAYOUT, true>(tid);
  for (uint64_t e0 = (uint64_t)blockIdx.y * kStep; e0 < len; e0 += (uint64_t)gridDim.y * kStep) {
    const uint64_t e = e0 + (uint64_t)slot0;
    const uint64_t id = e < len ? list[e] : ~0ull;   // (the same in the four lanes of a group)
    bool mine;
    const float d = walk_row<LAYOUT, METRIC, true>(a.rows, qs, id, e < len && id < a.rows.n_rows, tid, &mine);
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

__global__ __launch_bounds__(256) void range_scan_radii_kernel(const float* __restrict__ radius,
                                                               const uint32_t* __restrict__ scans, uint32_t nq,
                                                               float* __restrict__ out) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q < nq) out[q] = scans[q] ? radius[q] : __builtin_nanf("");
}

namespace {

typedef void (*RangeListFn)(const RangeListArgs);
const RangeListFn kListFns[9] = {   // [layout * 3 + metric]
    range_list_kernel<kLayoutF32, 0>,  range_list_kernel<kLayoutF32, 1>,  range_list_kernel<kLayoutF32, 2>,
    range_list_kernel<kLayoutF16, 0>,  range_list_kernel<kLayoutF16, 1>,  range_list_kernel<kLayoutF16, 2>,
    range_list_kernel<kLayoutPerm, 0>, range_list_kernel<kLayoutPerm, 1>, range_list_kernel<kLayoutPerm, 2>};
DynLdsAttr g_list_lds;

}  // namespace

uint32_t range_list_step_rows(const RangeListArgs& a) {
  return row_layout(a.rows.x_half, a.rows.x_perm) == kLayoutF32 ? 256u : 64u;
}

hipError_t launch_range_list(const RangeListArgs& a, uint32_t n_slots, hipStream_t st) {
  if (n_slots == 0 || a.rows.n_rows == 0) return hipSuccess;
  if (a.n_blocks == 0 || a.n_blocks > 65535u || (a.rows.ld & 31u) || a.rows.metric < 0 || a.rows.metric > 2) return hipErrorInvalidValue;
  const size_t lds = (size_t)a.rows.ld * sizeof(float);
  if (lds > kMaxLds) return hipErrorInvalidValue;
  hipError_t e = g_list_lds.ensure(kListFns, 9, lds);
  if (e != hipSuccess) return e;
  const int fn = row_layout(a.rows.x_half, a.rows.x_perm) * 3 + a.rows.metric;
  hipLaunchKernelGGL(kListFns[fn], dim3(n_slots, a.n_blocks), dim3(256), lds, st, a);
  return hipGetLastError();
}

hipError_t launch_range_scan_radii(const float* radius, const uint32_t* scans, uint32_t nq, float* out, hipStream_t st) {
  if (nq == 0) return hipSuccess;
  hipLaunchKernelGGL(range_scan_radii_kernel, dim3((nq + 255u) / 256u), dim3(256), 0, st, radius, scans, nq, out);
  return hipGetLastError();
}

}  // namespace ehx
