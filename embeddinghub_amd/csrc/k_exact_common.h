// What the exact paths share (k_flat.hip: rerank / exhaustive / single-query kernels; k_among.hip; k_range.hip): where the
// stored rows are (RowsView), their three layouts, the ONE walk from a prepared query to a stored row in the oracle's
// arithmetic, the (distance, id) key with its NaN rule, the running best-64 list, the re-rank of a pool and its sort, and the page writer with its sentinel
// rule.  Included by ehx_kernels.h behind k_canon.h — the one statement of that arithmetic, whose walkers (canon_dist,
// canon_dist_lane_t, canon_dist_group_t) the walk here calls and never restates — ahead of the launch arguments that embed
// a RowsView.
#pragma once

namespace ehx {

// layout of the stored rows: fp32 as stored, binary16 (widened exactly), fp32 in the search copy's block order (single-copy
// graph spaces, search_copy_pos)
enum { kLayoutF32 = 0, kLayoutF16 = 1, kLayoutPerm = 2 };
__host__ __device__ inline int row_layout(uint32_t x_half, uint32_t x_perm) {
  return x_half ? kLayoutF16 : (x_perm ? kLayoutPerm : kLayoutF32);
}

constexpr size_t kMaxLds = 160u * 1024u;   // LDS of one CU: the most one workgroup can have
constexpr uint32_t kPoolCap = 4096;        // candidate keys one query can collect in one pass (overflow: query flagged)

// where the rows of a space are, for one search (host: rows_view, ehx_call.cpp)
struct RowsView {
  const void* X;          // [cap][ld] stored rows
  const float* inv_norm;  // [cap] (cosine: the rows are scaled by it on the fly — hnswlib-python's stored normalised row)
  uint64_t n_rows;        // the search's snapshot of the row count: an id at or above it is no row
  uint32_t dims, ld;      // ld: row stride in elements, % 32 == 0
  uint32_t x_half;        // rows stored as binary16
  uint32_t x_perm;        // fp32 rows stored in the search copy's block order
  int metric;             // EHX_METRIC_*: 0 L2^2, 1 inner product, 2 cosine
};

// the prepared query qv[0, ld) into LDS, permuted like the rows for the block-permuted layout
template <int LAYOUT>
__device__ __forceinline__ void stage_query_lds(float* qs, const float* __restrict__ qv, uint32_t ld, uint32_t tid,
                                                uint32_t nthreads) {
  for (uint32_t m = tid; m < ld; m += nthreads) qs[LAYOUT == kLayoutPerm ? search_copy_pos(m) : m] = qv[m];
}

// ---- the row walk ----
// LANE: one lane per row where the layout has such a walk (fp32 rows: canon_dist_lane_t, 16-byte loads through its register
// ring); otherwise, and always with !LANE, a 4-lane group per row (fp32 / binary16: canon_dist; block-permuted:
// canon_dist_group_t).  A workgroup of T threads therefore takes walk_rows(T) rows per step, thread tid the row of slot
// walk_slot(tid).
constexpr int kMetricRt = -1;   // METRIC of a kernel that is not instantiated per metric: RowsView::metric decides (group walk
                                // of plain rows only)
template <int LAYOUT, bool LANE>
__host__ __device__ constexpr bool walk_by_lane() { return LANE && LAYOUT == kLayoutF32; }
template <int LAYOUT, bool LANE>
__host__ __device__ constexpr uint32_t walk_rows(uint32_t nthreads) { return walk_by_lane<LAYOUT, LANE>() ? nthreads : nthreads / 4u; }
template <int LAYOUT, bool LANE>
__device__ __forceinline__ uint32_t walk_slot(uint32_t tid) { return walk_by_lane<LAYOUT, LANE>() ? tid : tid >> 2; }

// Canonical distance from the prepared query q (LDS or global; permuted for kLayoutPerm) to row `id`, for thread tid.  ok:
// `id` is a row (the same in the four lanes of a group: they walk it together); a row that is not is not read.  *mine: this
// lane reports the row's result (every lane of a lane walk, sub-lane 0 of a group).
template <int LAYOUT, int METRIC, bool LANE>
__device__ __forceinline__ float walk_row(const RowsView& v, const float* __restrict__ q, uint64_t id, bool ok, uint32_t tid,
                                          bool* mine) {
  constexpr bool by_lane = walk_by_lane<LAYOUT, LANE>();
  const int sub = (int)(tid & 3u);
  *mine = ok && (by_lane || sub == 0);
  if (!ok) return 0.0f;
  const int metric = METRIC == kMetricRt ? v.metric : METRIC;
  const bool scale = metric == 2;
  const int metric01 = metric == 0 ? 0 : 1;
  const float xs = scale ? v.inv_norm[id] : 1.0f;
  if constexpr (LAYOUT == kLayoutF16) {
    return canon_dist(metric01, q, (const __half*)v.X + (size_t)id * v.ld, xs, scale, v.dims, sub);
  } else if constexpr (LAYOUT == kLayoutF32 && !by_lane) {
    return canon_dist(metric01, q, (const float*)v.X + (size_t)id * v.ld, xs, scale, v.dims, sub);
  } else {
    static_assert(METRIC != kMetricRt, "the lane walk and the block-permuted walk are instantiated per metric");
    constexpr int m01 = METRIC == 0 ? 0 : 1;
    constexpr bool sc = METRIC == 2;
    const float* x = (const float*)v.X + (size_t)id * v.ld;
    if constexpr (by_lane) return canon_dist_lane_t<m01, sc>(q, x, xs, v.dims);
    else return canon_dist_group_t<m01, sc>(q, x, sub, v.dims, xs);
  }
}

// ---- keys ----
// (ordered distance, id): unsigned order == (distance asc, id asc).  A NaN distance — a row or query holding NaN — is
// never a neighbour, nor is a row that is none (!ok): kKeyInf.
__device__ __forceinline__ uint64_t dist_key(float d, uint32_t id, bool ok) {
  return (ok && d == d) ? (((uint64_t)f32_to_ordered(d) << 32) | id) : kKeyInf;
}
// paging (k > 64): only keys strictly above the previous page's last (floor) count
__device__ __forceinline__ uint64_t dist_key_paged(float d, uint32_t id, bool ok, bool paged, uint64_t floor) {
  uint64_t key = dist_key(d, id, ok);
  if (paged && key <= floor) key = kKeyInf;
  return key;
}

// the 64 smallest of (best, 64 unsorted keys), ascending across the wave
__device__ __forceinline__ uint64_t keep_best64(uint64_t best, uint64_t key, int lane) {
  key = wave_sort64(key, lane);
  const uint64_t rv = __shfl(key, 63 - lane, 64);
  return wave_bitonic_merge64(best < rv ? best : rv, lane);
}

// ---- a pool of candidates, re-ranked (k_range.hip, k_radius.hip) ----
// Canonical distances of the pool's rows for a workgroup of T threads: pool[0, cnt) are keys whose low halves are row ids
// (each row at most once), qs the prepared query in LDS; keys[i] = the (distance, id) key of entry i, kKeyInf where the
// distance lies above r or is NaN.  Returns, in every lane of a wave, how many entries that wave's lanes kept.
template <int LAYOUT, int METRIC, uint32_t T>
__device__ __forceinline__ uint32_t rerank_pool_cut(const RowsView& rows, const float* qs, const uint64_t* __restrict__ pool,
                                                    uint32_t cnt, float r, uint64_t* keys, uint32_t tid) {
  const bool writer = walk_by_lane<LAYOUT, true>() || (tid & 3u) == 0;   // this lane files its slot's key
  uint32_t kept = 0;
  for (uint32_t i0 = 0; i0 < cnt; i0 += walk_rows<LAYOUT, true>(T)) {
    const uint32_t i = i0 + walk_slot<LAYOUT, true>(tid);
    const uint32_t id = i < cnt ? (uint32_t)pool[i] : ~0u;   // (the same in the four lanes of a group)
    bool mine;
    const float d = walk_row<LAYOUT, METRIC, true>(rows, qs, id, id < rows.n_rows, tid, &mine);
    const bool in = mine && d <= r;   // (a NaN distance compares false: never a member)
    if (i < cnt && writer) keys[i] = dist_key(d, id, in);
    kept += (uint32_t)__builtin_popcountll(__ballot(in));
  }
  return kept;
}

// ascending bitonic sort of keys[0, m) in LDS, m a power of two >= 2, by a whole workgroup of T threads
template <uint32_t T>
__device__ __forceinline__ void block_sort_lds(uint64_t* keys, uint32_t m, uint32_t tid) {
  for (uint32_t k = 2; k <= m; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = tid; t < (m >> 1); t += T) {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));   // the pair (i, i + j)
        const uint64_t a = keys[i], b = keys[i + j];
        const bool up = (i & k) == 0;
        if ((a > b) == up) {
          keys[i] = b;
          keys[i + j] = a;
        }
      }
      __syncthreads();
    }
  }
}

// keys[0, n) padded with kKeyInf to the power of two the sort runs over, and sorted
template <uint32_t T>
__device__ __forceinline__ void pad_and_sort_lds(uint64_t* keys, uint32_t n, uint32_t tid) {
  uint32_t m = 2;
  while (m < n) m <<= 1;
  for (uint32_t i = n + tid; i < m; i += T) keys[i] = kKeyInf;
  __syncthreads();
  block_sort_lds<T>(keys, m, tid);
}

// One query's pool re-ranked by its workgroup of T threads, whose whole LDS is the launch's pool_rerank_lds_bytes(rows.ld):
// the keys [kPoolCap] | the prepared query q_row, staged here, [ld] | a counter.  Behind it (uint64_t*)lds holds the
// (distance, id) keys of the entries within r, ascending, kKeyInf behind them; returns how many there are.
__host__ __device__ constexpr size_t pool_rerank_lds_bytes(uint32_t ld) {
  return kPoolCap * sizeof(uint64_t) + (size_t)ld * sizeof(float) + 16u;
}
template <int LAYOUT, int METRIC, uint32_t T>
__device__ __forceinline__ uint32_t pool_rerank_sorted(float4* lds, const RowsView& rows, const float* __restrict__ q_row,
                                                       const uint64_t* __restrict__ pool, uint32_t cnt, float r, uint32_t tid) {
  uint64_t* keys = (uint64_t*)lds;
  float* qs = (float*)(keys + kPoolCap);
  uint32_t& kept_s = *(uint32_t*)(qs + rows.ld);
  stage_query_lds<LAYOUT>(qs, q_row, rows.ld, tid, T);
  if (tid == 0) kept_s = 0;
  __syncthreads();
  const uint32_t kept = rerank_pool_cut<LAYOUT, METRIC, T>(rows, qs, pool, cnt, r, keys, tid);
  if ((tid & 63u) == 0 && kept) atomicAdd(&kept_s, kept);
  pad_and_sort_lds<T>(keys, cnt, tid);   // (at least one barrier: every wave's count has landed)
  return kept_s;
}

// ---- a page of results ----
// Columns [offset, offset + k) of one query's output row from its ascending keys, nvalid of them real: entry i < min(nvalid,
// k) is key_at(i)'s (id, distance), the entries behind are id ~0 / +Inf, and the count of a page after the first (offset > 0)
// is added to the earlier pages'.  The caller's threads take entries first, first + step, ...; thread `first == 0` writes
// the count.
template <class KeyAt>
__device__ __forceinline__ void emit_page(KeyAt key_at, uint32_t nvalid, uint32_t k, uint64_t* __restrict__ row_ids,
                                          float* __restrict__ row_dist, uint32_t* __restrict__ row_count, uint32_t offset,
                                          uint32_t first, uint32_t step) {
  const uint32_t cnt = nvalid < k ? nvalid : k;
  for (uint32_t i = first; i < k; i += step) {
    const bool ok = i < cnt;
    const uint64_t key = ok ? key_at(i) : kKeyInf;
    row_ids[offset + i] = ok ? (uint64_t)(uint32_t)key : ~0ull;
    row_dist[offset + i] = ok ? ordered_to_f32((uint32_t)(key >> 32)) : __builtin_inff();
  }
  if (first == 0) *row_count = (offset ? *row_count : 0u) + cnt;
}

}  // namespace ehx
