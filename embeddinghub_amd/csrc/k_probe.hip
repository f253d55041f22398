// Exact kNN under a per-query SET of stored labels (ehx_knn_by_labels*): the list-major scan.
// The composed route — every query replicated once per wanted label, among_list_kernel per (query, label) pair — reads a
// list's rows from HBM once per pair that names it.  Here the host groups the batch's (query, want-slot) pairs by label
// (ehx_probe.cpp) and hands the kernel a WORK LIST:
//   probe_tile_kernel   one workgroup of 256 per item = (a range [lo, hi) of the column index's permutation, up to 8 pairs
//                       that all name that label).  The item's prepared queries are gathered BY INDEX into LDS, then the
//                       range goes through LDS in steps of 8 rows — 32 lanes stage a row with 16-byte loads into plain,
//                       scaled fp32 (stage_row_lds: whatever the stored layout) — and each of the 64 four-lane groups
//                       evaluates one (row, pair) with canon_dist from LDS.  Every 64 rows each wave merges the new keys
//                       of its two pairs into their best-64 lists (registers).  A row makes one trip through the memory
//                       system per 8 pairs; the items of one label are adjacent in the grid, so the others find it in L2.
//   probe_fill_kernel   kKeyInf into the key lists: the blocks no item writes — an absent or repeated label, a slot beyond
//                       the query's count, a chunk beyond a list's end — must read as empty in the merge.
// out[query][slot * n_chunks + chunk][64] is the layout launch_flat_merge reads with n_want * n_chunks lists per query; the
// page floor is per QUERY (two pairs of one item may belong to different queries, or to the same one).
// LDS, dynamic: [8][ld + 4] queries | [8][ld + 4] rows | [8][64] keys — 16 (ld + 4) floats + 4096 bytes: 53 504 bytes at
// ld = 768 (three workgroups per CU), and rows of up to probe_max_ld() = 2464 floats fit the CU's 160 KB.
// No matrix instruction: the answer is defined as the canonical walk's bytes (k_canon.h), which an MFMA product is not.
#include "ehx_kernels.h"

namespace ehx {

namespace {

constexpr uint32_t kLdsPad = 4;   // floats behind every LDS row: the 8 rows a 32-lane group reads fall into 32 banks
constexpr uint32_t kStepRows = 8; // rows staged per step: with 8 pairs, one (row, pair) per 4-lane group

}  // namespace

template <int LAYOUT, int METRIC>
__global__ __launch_bounds__(256) void probe_tile_kernel(const ProbeArgs a) {
  constexpr uint32_t P = kProbeTilePairs, R = kStepRows;
  static_assert(P * R == 64 && P == 8, "one (row, pair) per 4-lane group; two pairs per wave");
  extern __shared__ float4 probe_lds[];
  __shared__ uint32_t row_id[R], row_ok[R];
  const uint32_t lds = a.rows.ld + kLdsPad;
  float* qs = (float*)probe_lds;                  // [P][lds] the pairs' prepared queries
  float* xs = qs + (size_t)P * lds;               // [R][lds] this step's rows
  uint64_t* keys = (uint64_t*)(xs + (size_t)R * lds);   // [P][64] the keys of 64 rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const ProbeItem& it = a.items[blockIdx.x];
  const uint32_t np = it.n_pairs < P ? it.n_pairs : P;
  const uint64_t lo = it.lo;
  const uint64_t hi = it.hi < a.n_perm ? it.hi : a.n_perm;   // (never read beyond the permutation)
  const uint32_t ld4 = a.rows.ld >> 2, lds4 = lds >> 2;
  for (uint32_t i = tid; i < P * ld4; i += 256) {
    const uint32_t pi = i / ld4, c = i - pi * ld4;
    const uint32_t q = pi < np ? it.q[pi] : ~0u;
    ((float4*)qs)[pi * lds4 + c] = q < a.nq ? ((const float4*)a.Q)[(size_t)q * ld4 + c] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  constexpr bool scale = METRIC == 2;
  constexpr int metric01 = METRIC == 0 ? 0 : 1;
  const bool paged = a.floor != nullptr;
  const int g = tid >> 2, sub = tid & 3;
  const uint32_t pr = (uint32_t)g & (R - 1), pp = (uint32_t)g / R;   // this group's row slot and pair
  const uint32_t my_q = pp < np ? it.q[pp] : ~0u;
  const bool pair_ok = my_q < a.nq;
  const uint64_t fl = (paged && pair_ok) ? a.floor[my_q] : 0ull;
  const uint32_t sr = (uint32_t)tid >> 5, sl = (uint32_t)tid & 31u;  // staging: row slot, lane within the row's 32
  uint64_t best[2] = {kKeyInf, kKeyInf};          // pairs wave and wave + 4
  for (uint64_t c0 = lo; c0 < hi; c0 += 64u) {
    keys[tid] = kKeyInf;
    keys[tid + 256] = kKeyInf;
    for (uint32_t st = 0; st < 64u / R && c0 + st * R < hi; ++st) {
      const uint64_t p = c0 + st * R + sr;
      const uint64_t id = p < hi ? a.perm[p] : ~0ull;
      const bool ok = id < a.rows.n_rows;
      if (sl == 0) {
        row_id[sr] = (uint32_t)id;
        row_ok[sr] = ok ? 1u : 0u;
      }
      // (a row that is not staged leaves stale floats behind: its pairs' keys are dropped)
      if (ok) stage_row_lds<LAYOUT, scale>((float4*)xs + sr * lds4, a.rows, id, sl, 32);
      __syncthreads();
      const float d = canon_dist(metric01, qs + (size_t)pp * lds, xs + (size_t)pr * lds, 1.0f, false, a.rows.dims, sub);
      if (sub == 0) keys[pp * 64 + st * R + pr] = dist_key_paged(d, row_id[pr], row_ok[pr] != 0 && pair_ok, paged, fl);
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) best[j] = keep_best64(best[j], keys[(wave + 4 * j) * 64 + lane], lane);
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const uint32_t pi = (uint32_t)wave + 4u * j;
    if (pi >= np) continue;
    const uint32_t q = it.q[pi], slot = it.slot[pi];
    if (q < a.nq && slot < a.n_want && it.chunk < a.n_chunks)   // (an item names a block of `out` or writes nothing)
      a.out[(((size_t)q * a.n_want + slot) * a.n_chunks + it.chunk) * 64 + lane] = best[j];
  }
}

__global__ __launch_bounds__(256) void probe_fill_kernel(uint64_t* __restrict__ out, size_t n_keys) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_keys; i += (size_t)gridDim.x * 256) out[i] = kKeyInf;
}

namespace {

constexpr size_t kProbeKeyBytes = (size_t)kProbeTilePairs * 64 * sizeof(uint64_t);
size_t probe_lds(uint32_t ld) { return (size_t)(kProbeTilePairs + kStepRows) * (ld + kLdsPad) * sizeof(float) + kProbeKeyBytes; }

typedef void (*ProbeFn)(const ProbeArgs);
#define EHX_PROBE_FNS(K) \
  {K<kLayoutF32, 0>, K<kLayoutF32, 1>, K<kLayoutF32, 2>, K<kLayoutF16, 0>, K<kLayoutF16, 1>, K<kLayoutF16, 2>, \
   K<kLayoutPerm, 0>, K<kLayoutPerm, 1>, K<kLayoutPerm, 2>}
const ProbeFn kProbeFns[9] = EHX_PROBE_FNS(probe_tile_kernel);   // [layout * 3 + metric]
#undef EHX_PROBE_FNS
DynLdsAttr g_probe_lds;

}  // namespace

// the longest row stride whose tiles fit: 16 (ld + 4) floats + the key area <= 160 KB, ld a multiple of 32
uint32_t probe_max_ld() {
  const size_t floats = (kMaxLds - kProbeKeyBytes) / sizeof(float) / (kProbeTilePairs + kStepRows);
  return (uint32_t)((floats - kLdsPad) & ~(size_t)31);
}

hipError_t launch_probe(const ProbeArgs& a, hipStream_t st) {
  if (a.n_items == 0) return hipSuccess;
  if (a.nq == 0 || a.n_want == 0 || a.n_chunks == 0 || a.n_chunks > kProbeMaxChunks || (a.rows.ld & 31u) ||
      a.rows.ld > probe_max_ld() || a.rows.metric < 0 || a.rows.metric > 2)
    return hipErrorInvalidValue;
  const size_t lds = probe_lds(a.rows.ld);
  hipError_t e = g_probe_lds.ensure(kProbeFns, 9, lds);
  if (e != hipSuccess) return e;
  const int fn = row_layout(a.rows.x_half, a.rows.x_perm) * 3 + a.rows.metric;
  hipLaunchKernelGGL(kProbeFns[fn], dim3(a.n_items), dim3(256), lds, st, a);
  return hipGetLastError();
}

hipError_t launch_probe_fill(uint64_t* out, size_t n_keys, hipStream_t st) {
  if (n_keys == 0) return hipSuccess;
  const uint32_t grid = (uint32_t)std::min<size_t>((n_keys + 255) / 256, 4096);
  hipLaunchKernelGGL(probe_fill_kernel, dim3(grid), dim3(256), 0, st, out, n_keys);
  return hipGetLastError();
}

}  // namespace ehx
