// Exact kNN among a caller's list of row ids (ehx_knn_among*): the canonical (oracle-order) distance of every listed row,
// the best 64 (distance, id) keys per workgroup — out[q][block][64], the layout launch_flat_merge reads — and the page
// writer that turns a query's merged keys into ids / distances / count.
//   among_list_kernel   one query per workgroup, the rows read straight from HBM: a gather, bound by what the memory
//                       system delivers for random whole rows.  Serves the per-query lists; with AmongArgs::cand_end
//                       (a run-time field: the same nine functions) two queries may name the same list.
//   among_tile_kernel   ONE list shared by every query: a workgroup stages 8 gathered rows in LDS and applies them to a tile
//                       of 8 queries before it moves on, so a row makes one trip through the memory system per 8 pairs
//                       (and the workgroups of the other query tiles, resident together, find it in L2).
// The list kernel takes every distance from the exact paths' one row walk (walk_row, k_exact_common.h), the tile kernel
// from canon_dist over the rows it staged; keys, best-64 lists and the page come from the same header.  The row layouts
// are those gather_rows_kernel (k_bykey.hip) reads: fp32 rows as stored, binary16 rows widened exactly, single-copy graph
// rows in the search copy's block order.  Cosine rows are scaled by inv_norm — one rounding per element, hnswlib-python's
// stored normalised row — on the fly (list kernel) or as they are staged (tile kernel).
#include "ehx_kernels.h"

namespace ehx {

namespace {

typedef _Float16 half8_t __attribute__((ext_vector_type(8)));

constexpr uint32_t kLdsPad = 4;   // floats behind every LDS row: the 8 rows a 32-lane group reads fall into 32 banks

}  // namespace

// Grid (queries, blocks): block b of query q walks steps b, b + gridDim.y, ... of the query's list until its end, a step
// being 256 rows (fp32 rows: one lane per row) or 64 rows (binary16 and block-permuted rows: a 4-lane group per row) of
// walk_row.  The grid is sized from a hint of the longest list; a hint that is too small costs time, never rows.  The
// query sits in LDS (permuted like the rows for the block-permuted layout).
template <int LAYOUT, int METRIC>
__global__ __launch_bounds__(256) void among_list_kernel(const AmongArgs a) {
  constexpr uint32_t kStep = walk_rows<LAYOUT, true>(256);
  extern __shared__ float4 among_lds[];
  __shared__ uint64_t keys[256];
  float* qs = (float*)among_lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t q = blockIdx.x;
  uint64_t lo = 0, hi = a.n_cand;
  if (a.cand_off) {
    lo = a.cand_off[q];
    hi = a.cand_end ? a.cand_end[q] : a.cand_off[q + 1];   // (cand_end: queries that share a list name the same range)
    hi = hi < a.n_cand ? hi : a.n_cand;   // (the device form cannot check its offsets: never read beyond the id array)
  }
  stage_query_lds<LAYOUT>(qs, a.Q + (size_t)q * a.rows.ld, a.rows.ld, tid, 256);
  __syncthreads();
  const uint64_t fl = a.floor ? a.floor[q] : 0ull;
  const bool paged = a.floor != nullptr;
  const uint32_t slot = walk_slot<LAYOUT, true>(tid);
  const bool writer = walk_by_lane<LAYOUT, true>() || (tid & 3) == 0;   // this lane files its slot's key
  uint64_t best = kKeyInf;
  for (uint64_t p0 = lo + (uint64_t)blockIdx.y * kStep; p0 < hi; p0 += (uint64_t)gridDim.y * kStep) {
    const uint64_t p = p0 + (uint64_t)slot;
    const uint64_t id = p < hi ? a.cand_ids[p] : ~0ull;
    bool mine;
    const float d = walk_row<LAYOUT, METRIC, true>(a.rows, qs, id, id < a.rows.n_rows, tid, &mine);
    if (writer) keys[slot] = dist_key_paged(d, (uint32_t)id, mine, paged, fl);
    __syncthreads();
    if ((uint32_t)wave < kStep / 64u) best = keep_best64(best, keys[tid], lane);
    __syncthreads();
  }
  if (kStep > 64u) {   // the four waves' lists -> wave 0
    keys[tid] = best;
    __syncthreads();
    if (wave == 0)
      for (int w = 1; w < 4; ++w) {
        const uint64_t rv = keys[w * 64 + 63 - lane];
        best = wave_bitonic_merge64(best < rv ? best : rv, lane);
      }
  }
  if (wave == 0) a.out[((size_t)q * gridDim.y + blockIdx.y) * 64 + lane] = best;
}

// Grid (query tiles, blocks), the query tile fastest: the workgroups that read the same chunks of the shared list run
// together.  Block b walks chunks b, b + gridDim.y, ... of 64 list entries; a chunk goes through LDS in 8 steps of
// kAmongTileRows rows — 32 lanes stage a row with 16-byte loads into plain, scaled fp32 (whatever the stored layout), then
// each of the 64 four-lane groups evaluates one (row, query) pair with canon_dist from LDS.  After the chunk every wave
// merges the 64 new keys of its two queries into their best-64 lists (registers).
template <int LAYOUT, int METRIC>
__global__ __launch_bounds__(256) void among_tile_kernel(const AmongArgs a) {
  constexpr uint32_t QT = kAmongTileQ, R = kAmongTileRows;
  static_assert(QT * R == 64 && QT == 8, "one (row, query) pair per 4-lane group; two queries per wave");
  extern __shared__ float4 among_lds[];
  __shared__ uint32_t row_id[R], row_ok[R];
  const uint32_t lds = a.rows.ld + kLdsPad;
  float* qs = (float*)among_lds;                  // [QT][lds] the tile's prepared queries
  float* xs = qs + (size_t)QT * lds;              // [R][lds] this step's rows
  uint64_t* keys = (uint64_t*)(xs + (size_t)R * lds);   // [QT][64] this chunk's keys
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t q0 = blockIdx.x * QT;
  const uint32_t nqt = a.nq - q0 < QT ? a.nq - q0 : QT;
  const uint32_t ld4 = a.rows.ld >> 2, lds4 = lds >> 2;
  for (uint32_t i = tid; i < QT * ld4; i += 256) {
    const uint32_t qi = i / ld4, c = i - qi * ld4;
    ((float4*)qs)[qi * lds4 + c] =
        qi < nqt ? ((const float4*)a.Q)[(size_t)(q0 + qi) * ld4 + c] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  constexpr bool scale = METRIC == 2;
  constexpr int metric01 = METRIC == 0 ? 0 : 1;
  const bool paged = a.floor != nullptr;
  const int g = tid >> 2, sub = tid & 3;
  const uint32_t pr = (uint32_t)g & (R - 1), pq = (uint32_t)g / R;   // this group's pair: row slot, query of the tile
  const uint64_t fl = (paged && pq < nqt) ? a.floor[q0 + pq] : 0ull;
  const uint32_t sr = (uint32_t)tid >> 5, sl = (uint32_t)tid & 31u;  // staging: row slot, lane within the row's 32
  uint64_t best[2] = {kKeyInf, kKeyInf};          // queries wave and wave + 4 of the tile
  for (uint64_t c0 = (uint64_t)blockIdx.y * 64u; c0 < a.n_cand; c0 += (uint64_t)gridDim.y * 64u) {
    keys[tid] = kKeyInf;
    keys[tid + 256] = kKeyInf;
    for (uint32_t st = 0; st < 64u / R && c0 + st * R < a.n_cand; ++st) {
      const uint64_t p = c0 + st * R + sr;
      const uint64_t id = p < a.n_cand ? a.cand_ids[p] : ~0ull;
      const bool ok = id < a.rows.n_rows;
      if (sl == 0) {
        row_id[sr] = (uint32_t)id;
        row_ok[sr] = ok ? 1u : 0u;
      }
      if (ok) {   // (a row that is not staged leaves stale floats behind: its pairs' keys are dropped)
        const float inv = scale ? a.rows.inv_norm[id] : 1.0f;
        float4* dst = (float4*)xs + sr * lds4;
        if (LAYOUT == kLayoutF16) {
          const half8_t* x = (const half8_t*)((const _Float16*)a.rows.X + (size_t)id * a.rows.ld);
          for (uint32_t c = sl; c < (a.rows.dims + 7u) >> 3; c += 32) {
            const half8_t h = x[c];
            float4 v0 = make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
            float4 v1 = make_float4((float)h[4], (float)h[5], (float)h[6], (float)h[7]);
            if (scale) {
              v0 = scale_f4(v0, inv);
              v1 = scale_f4(v1, inv);
            }
            dst[2 * c] = v0;
            dst[2 * c + 1] = v1;
          }
        } else if (LAYOUT == kLayoutPerm) {
          // a 16-float block of the search copy's order: four 16-byte loads, the 4 x 4 transpose undone (search_copy_pos)
          const float4* x = (const float4*)((const float*)a.rows.X + (size_t)id * a.rows.ld);
          for (uint32_t b = sl; b < (a.rows.dims + 15u) >> 4; b += 32) {
            float4 v0 = x[4 * b], v1 = x[4 * b + 1], v2 = x[4 * b + 2], v3 = x[4 * b + 3];
            if (scale) {
              v0 = scale_f4(v0, inv);
              v1 = scale_f4(v1, inv);
              v2 = scale_f4(v2, inv);
              v3 = scale_f4(v3, inv);
            }
            dst[4 * b] = make_float4(v0.x, v1.x, v2.x, v3.x);
            dst[4 * b + 1] = make_float4(v0.y, v1.y, v2.y, v3.y);
            dst[4 * b + 2] = make_float4(v0.z, v1.z, v2.z, v3.z);
            dst[4 * b + 3] = make_float4(v0.w, v1.w, v2.w, v3.w);
          }
        } else {
          const float4* x = (const float4*)((const float*)a.rows.X + (size_t)id * a.rows.ld);
          for (uint32_t c = sl; c < (a.rows.dims + 3u) >> 2; c += 32) dst[c] = scale ? scale_f4(x[c], inv) : x[c];
        }
      }
      __syncthreads();
      const float d = canon_dist(metric01, qs + (size_t)pq * lds, xs + (size_t)pr * lds, 1.0f, false, a.rows.dims, sub);
      if (sub == 0) keys[pq * 64 + st * R + pr] = dist_key_paged(d, row_id[pr], row_ok[pr] != 0 && pq < nqt, paged, fl);
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) best[j] = keep_best64(best[j], keys[(wave + 4 * j) * 64 + lane], lane);
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const uint32_t qi = (uint32_t)wave + 4u * j;
    if (qi < nqt) a.out[((size_t)(q0 + qi) * gridDim.y + blockIdx.y) * 64 + lane] = best[j];
  }
}

// One wave per query: a page of results from the query's merged keys (ascending, exact canonical distances): columns
// [out_offset, out_offset + k) of a row of out_stride entries (emit_page).
__global__ __launch_bounds__(64) void among_emit_kernel(const uint64_t* __restrict__ merged, uint32_t k,
                                                        uint32_t out_stride, uint32_t out_offset,
                                                        uint64_t* __restrict__ out_ids, float* __restrict__ out_dist,
                                                        uint32_t* __restrict__ out_count) {
  const uint32_t lane = threadIdx.x, q = blockIdx.x;
  const uint64_t key = merged[(size_t)q * 64 + lane];
  const uint32_t nvalid = (uint32_t)__builtin_popcountll(__ballot(key != kKeyInf));
  emit_page([&](uint32_t) { return key; }, nvalid, k, out_ids + (size_t)q * out_stride, out_dist + (size_t)q * out_stride,
            out_count + q, out_offset, lane, 64);
}

namespace {

size_t among_tile_lds(uint32_t ld) {
  return (size_t)(kAmongTileQ + kAmongTileRows) * (ld + kLdsPad) * sizeof(float) + (size_t)kAmongTileQ * 64 * sizeof(uint64_t);
}

typedef void (*AmongFn)(const AmongArgs);
#define EHX_AMONG_FNS(K) \
  {K<kLayoutF32, 0>, K<kLayoutF32, 1>, K<kLayoutF32, 2>, K<kLayoutF16, 0>, K<kLayoutF16, 1>, K<kLayoutF16, 2>, \
   K<kLayoutPerm, 0>, K<kLayoutPerm, 1>, K<kLayoutPerm, 2>}
const AmongFn kTileFns[9] = EHX_AMONG_FNS(among_tile_kernel);   // [layout * 3 + metric]
const AmongFn kListFns[9] = EHX_AMONG_FNS(among_list_kernel);
#undef EHX_AMONG_FNS
DynLdsAttr g_tile_lds, g_list_lds;

int among_layout(const AmongArgs& a) { return row_layout(a.rows.x_half, a.rows.x_perm); }

}  // namespace

bool among_tiled(const AmongArgs& a) { return a.cand_off == nullptr && among_tile_lds(a.rows.ld) <= kMaxLds; }

uint32_t among_max_ld() { return (uint32_t)(kMaxLds / sizeof(float)); }   // among_list_kernel keeps one prepared query in LDS

uint32_t among_step_rows(const AmongArgs& a) { return among_tiled(a) ? 64u : (among_layout(a) == kLayoutF32 ? 256u : 64u); }

hipError_t launch_among(const AmongArgs& a, hipStream_t st) {
  if (a.nq == 0 || a.n_blocks == 0 || a.n_blocks > 65535u || (a.rows.ld & 31u) || a.rows.metric < 0 || a.rows.metric > 2)
    return hipErrorInvalidValue;
  const int fn = among_layout(a) * 3 + a.rows.metric;
  if (among_tiled(a)) {
    const size_t lds = among_tile_lds(a.rows.ld);
    hipError_t e = g_tile_lds.ensure(kTileFns, 9, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kTileFns[fn], dim3((a.nq + kAmongTileQ - 1) / kAmongTileQ, a.n_blocks), dim3(256), lds, st, a);
  } else {
    const size_t lds = (size_t)a.rows.ld * sizeof(float);
    if (lds > kMaxLds) return hipErrorInvalidValue;
    hipError_t e = g_list_lds.ensure(kListFns, 9, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kListFns[fn], dim3(a.nq, a.n_blocks), dim3(256), lds, st, a);
  }
  return hipGetLastError();
}

hipError_t launch_among_emit(const uint64_t* merged, uint32_t nq, uint32_t k, uint32_t out_stride, uint32_t out_offset,
                             uint64_t* out_ids, float* out_dist, uint32_t* out_count, hipStream_t st) {
  if (nq == 0) return hipSuccess;
  if (k == 0 || k > 64) return hipErrorInvalidValue;
  hipLaunchKernelGGL(among_emit_kernel, dim3(nq), dim3(64), 0, st, merged, k, out_stride, out_offset, out_ids, out_dist,
                     out_count);
  return hipGetLastError();
}

}  // namespace ehx
