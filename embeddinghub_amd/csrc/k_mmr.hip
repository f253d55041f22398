// MMR re-ranking of candidate lists on the device (ehx_mmr_select_device, ehx_knn_mmr*): from the c <= 256 candidates
// (id_j, dq_j) of a query, greedily the k that are near the query and not near each other — include/ehx.h has the contract,
// ehx_mmr.cpp the host side.
//   mmr_select_kernel   one workgroup of 256 threads per query; thread j owns candidate j (its rank).  Everything the greedy
//                       loop keeps is in LDS; the only global traffic is candidate rows in and min(k, c) results out.
// LDS (mmr_lds_bytes): the prepared pivot [ld] | the block the canonical norm is summed from [1024] | ids [256] | one key per
// wave [4] | dq [256] | near [256] | picked [256] | the pivot's inverse norm.
// Per pick after the first, while mu = 1 - lambda is not 0:
//   stage   the last pick's row becomes the query: gathered from its stored layout (the cases of gather_rows_kernel,
//           k_bykey.hip: the bytes ehx_get_by_id returns), padded, for cosine normalised with the canonical sequential norm
//           (squares into LDS, one lane adds them in order: prep_query_row's sum, k_prep_query.h), and laid out as
//           stage_query_lds lays a prepared query out — so pair(a, b) is byte for byte what ehx_knn_by_ids_device reports;
//   sweep   every unpicked candidate's distance to it from the exact paths' ONE row walk (walk_row, k_exact_common.h): 256
//           rows per step with one lane per row (fp32 rows), 64 with a 4-lane group per row (binary16 and block-permuted
//           rows); the lane that reports a row lowers near[] of its candidate (a NaN never does);
//   pick    thread j forms cost_j = a_j - b_j, every operation rounded on its own, and packs (orderable bits of cost + 0.0f,
//           rank) into one 64-bit key, NaN above +Inf; the minimum — shuffles within a wave, four keys through LDS — is the
//           next pick and the next pivot.
// The first pick is the lowest rank that is a row; lambda == 1 (mu == 0), k == 1 and c <= 1 never sweep.
#include "k_prep_query.h"

namespace ehx {

namespace {

typedef _Float16 half4_t __attribute__((ext_vector_type(4)));

constexpr uint32_t kMmrThreads = 256;
static_assert(kMmrThreads == kMmrMaxFetch, "thread j owns candidate j");
constexpr uint32_t kNormBlock = 1024;   // floats the canonical norm is summed from at a time (prep_query_row's block)

__host__ __device__ constexpr size_t mmr_lds_bytes(uint32_t ld) {
  return ((size_t)ld + kNormBlock + 3u * kMmrMaxFetch + 4u) * sizeof(float) + ((size_t)kMmrMaxFetch + 4u) * sizeof(uint64_t);
}

// (orderable bits of cost + 0.0f, rank): unsigned order == (cost ascending as IEEE values, -0 == +0, NaN behind +Inf; rank)
__device__ __forceinline__ uint64_t mmr_key(float cost, uint32_t rank) {
  const uint32_t o = cost == cost ? f32_to_ordered(ex_add(cost, 0.0f)) : 0xFFFFFFFFu;
  return ((uint64_t)o << 32) | rank;
}

}  // namespace

template <int LAYOUT, int METRIC>
__global__ __launch_bounds__(kMmrThreads) void mmr_select_kernel(const MmrArgs a) {
  constexpr uint32_t kStep = walk_rows<LAYOUT, true>(kMmrThreads);
  extern __shared__ float4 mmr_lds[];
  float* qs = (float*)mmr_lds;                           // [ld] the prepared pivot (permuted for kLayoutPerm)
  float* sq = qs + a.rows.ld;                            // [kNormBlock]
  uint64_t* ids = (uint64_t*)(sq + kNormBlock);          // [256]
  uint64_t* wkey = ids + kMmrMaxFetch;                   // [4]
  float* dq = (float*)(wkey + 4);                        // [256]
  float* near = dq + kMmrMaxFetch;                       // [256]
  uint32_t* picked = (uint32_t*)(near + kMmrMaxFetch);   // [256] picked, or no candidate at all
  float* inv_s = (float*)(picked + kMmrMaxFetch);
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t q = blockIdx.x;
  const uint32_t dims = a.rows.dims, ld = a.rows.ld;
  uint32_t c = a.cand_count[q];
  c = c < a.fetch_k ? c : a.fetch_k;
  // an id at or above the row count is no candidate: never picked, never a pivot, never read
  const uint64_t my_id = tid < c ? a.cand_ids[(size_t)q * a.fetch_k + tid] : ~0ull;
  const bool is_row = my_id < a.rows.n_rows;
  ids[tid] = my_id;
  dq[tid] = tid < c ? a.cand_dist[(size_t)q * a.fetch_k + tid] : 0.0f;
  near[tid] = __builtin_inff();
  picked[tid] = is_row ? 0u : 1u;
  const uint32_t wave_rows = (uint32_t)__builtin_popcountll(__ballot(is_row));
  if (lane == 0) wkey[wave] = wave_rows;
  __syncthreads();
  const uint32_t n_rows_in = (uint32_t)(wkey[0] + wkey[1] + wkey[2] + wkey[3]);
  __syncthreads();   // (the first pick writes wkey again)
  const uint32_t n_pick = a.k < n_rows_in ? a.k : n_rows_in;
  const float lambda = a.lambda, mu = ex_sub(1.0f, lambda);
  uint64_t* __restrict__ out_ids = a.out_ids + (size_t)q * a.k;
  float* __restrict__ out_dist = a.out_dist + (size_t)q * a.k;
  uint32_t p = 0;
  for (uint32_t t = 0; t < n_pick; ++t) {
    if (t > 0 && mu != 0.0f) {
      // ---- stage the pivot: row ids[p] as ehx_get_by_id returns it, zeros behind dims, at the places the walk reads ----
      const uint64_t pid = ids[p];
      for (uint32_t c4 = tid; c4 < (ld >> 2); c4 += kMmrThreads) {
        float4 v;
        if (LAYOUT == kLayoutF16) {
          const half4_t h = ((const half4_t*)((const _Float16*)a.rows.X + (size_t)pid * ld))[c4];
          v = make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
        } else {
          v = ((const float4*)((const float*)a.rows.X + (size_t)pid * ld))[c4];
        }
        // (element m of the row is stored at search_copy_pos(m) of a block-permuted row, and the map is its own inverse)
        const uint32_t m0 = 4u * c4;
        if ((LAYOUT == kLayoutPerm ? search_copy_pos(m0) : m0) >= dims) v.x = 0.0f;
        if ((LAYOUT == kLayoutPerm ? search_copy_pos(m0 + 1) : m0 + 1) >= dims) v.y = 0.0f;
        if ((LAYOUT == kLayoutPerm ? search_copy_pos(m0 + 2) : m0 + 2) >= dims) v.z = 0.0f;
        if ((LAYOUT == kLayoutPerm ? search_copy_pos(m0 + 3) : m0 + 3) >= dims) v.w = 0.0f;
        ((float4*)qs)[c4] = v;
      }
      __syncthreads();
      if (METRIC == 2) {
        float sum = 0.0f;   // (thread 0's)
        for (uint32_t base = 0; base < dims; base += kNormBlock) {
          const uint32_t m = dims - base < kNormBlock ? dims - base : kNormBlock;
          for (uint32_t i = tid; i < m; i += kMmrThreads) {
            const float v = qs[LAYOUT == kLayoutPerm ? search_copy_pos(base + i) : base + i];
            sq[i] = ex_mul(v, v);
          }
          __syncthreads();
          if (tid == 0) sum = seq_sum_lds_from(sum, sq, m);
          __syncthreads();
        }
        if (tid == 0) *inv_s = inv_norm_of(sum);
        __syncthreads();
        const float inv = *inv_s;
        for (uint32_t i = tid; i < ld; i += kMmrThreads) qs[i] = ex_mul(qs[i], inv);
        __syncthreads();
      }
      // ---- sweep: near[j] = min(near[j], pair(id_j, id_p)) for every unpicked j ----
      for (uint32_t i0 = 0; i0 < c; i0 += kStep) {
        const uint32_t i = i0 + walk_slot<LAYOUT, true>(tid);   // (the same in the four lanes of a group)
        const bool todo = i < c && picked[i] == 0;
        bool mine;
        const float d = walk_row<LAYOUT, METRIC, true>(a.rows, qs, todo ? ids[i] : ~0ull, todo, tid, &mine);
        if (mine && d < near[i]) near[i] = d;
      }
      __syncthreads();
    }
    // ---- pick: the unpicked candidate least by (cost, rank); the first pick is the lowest rank ----
    uint64_t key = kKeyInf;
    if (picked[tid] == 0) {
      if (t == 0) {
        key = tid;
      } else {
        const float ca = lambda == 0.0f ? 0.0f : ex_mul(lambda, dq[tid]);
        const float cb = mu == 0.0f ? 0.0f : ex_mul(mu, near[tid]);
        key = mmr_key(ex_sub(ca, cb), tid);
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const uint64_t other = __shfl_xor(key, o, 64);
      key = other < key ? other : key;
    }
    if (lane == 0) wkey[wave] = key;
    __syncthreads();
    key = wkey[0];
    for (int w = 1; w < 4; ++w) key = wkey[w] < key ? wkey[w] : key;
    p = (uint32_t)key;   // (t < n_pick: an unpicked row is left, so the minimum is a candidate's key)
    if (tid == p) {
      picked[p] = 1u;
      out_ids[t] = ids[p];
      out_dist[t] = dq[p];
    }
    __syncthreads();
  }
  for (uint32_t t = n_pick + tid; t < a.k; t += kMmrThreads) {
    out_ids[t] = ~0ull;
    out_dist[t] = __builtin_inff();
  }
  if (tid == 0) a.out_count[q] = n_pick;
}

namespace {

typedef void (*MmrFn)(const MmrArgs);
#define EHX_MMR_FNS(K) \
  {K<kLayoutF32, 0>, K<kLayoutF32, 1>, K<kLayoutF32, 2>, K<kLayoutF16, 0>, K<kLayoutF16, 1>, K<kLayoutF16, 2>, \
   K<kLayoutPerm, 0>, K<kLayoutPerm, 1>, K<kLayoutPerm, 2>}
const MmrFn kMmrFns[9] = EHX_MMR_FNS(mmr_select_kernel);   // [layout * 3 + metric]
#undef EHX_MMR_FNS
DynLdsAttr g_mmr_lds;

}  // namespace

uint32_t mmr_max_ld() { return (uint32_t)((kMaxLds - mmr_lds_bytes(0)) / sizeof(float)) & ~31u; }

hipError_t launch_mmr_select(const MmrArgs& a, hipStream_t st) {
  if (a.nq == 0) return hipSuccess;
  if (a.k == 0 || a.k > a.fetch_k || a.fetch_k > kMmrMaxFetch || (a.rows.ld & 31u) || a.rows.ld > mmr_max_ld() ||
      a.rows.metric < 0 || a.rows.metric > 2)
    return hipErrorInvalidValue;
  const size_t lds = mmr_lds_bytes(a.rows.ld);
  hipError_t e = g_mmr_lds.ensure(kMmrFns, 9, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kMmrFns[row_layout(a.rows.x_half, a.rows.x_perm) * 3 + a.rows.metric], dim3(a.nq), dim3(kMmrThreads), lds,
                     st, a);
  return hipGetLastError();
}

}  // namespace ehx
