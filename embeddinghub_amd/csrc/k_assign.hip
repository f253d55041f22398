// Nearest-centroid assignment (ehx_assign_device, ehx_kmeans_device; ehx_assign.cpp): the transpose of the scans — millions
// of stored rows against a few thousand centroids, ONE argmin kept per row, the N x C products never written.  include/ehx.h
// has the definition (the centroid plays the query of the canonical distance), DESIGN.md §e.33 the margin's derivation.
//   centroid_stats_kernel  |c|^2 of every prepared centroid (launch_prep_queries' output: padded, cosine normalised) and the
//                          call's flag "a centroid is not finite".
//   assign_filter_kernel   the hot path, fp32 matrix cores.  Plain fp32 and binary16 rows; block-permuted single-copy graph
//                          rows take the exact kernel only.
//   assign_exact_kernel    the canonical route: the rows the filter could not certify, or every row where it may not run.
//   label_keys / lloyd_divide / count_moved   the glue of the centroid sums and of a Lloyd step.
//
// The filter.  A workgroup of 4 waves owns a tile of TM = 32 RB rows (RB = 4, 2 or 1: the most whose tile fits) and loads it
// from HBM ONCE into LDS as fp32 — binary16 widened (exact), cosine rows scaled by inv_norm with the one rounding the walk
// gives them, columns at and beyond dims zero — at a row stride of ld + 4 floats.  Then ALL centroid tiles of 128 stream
// past it in slabs of 32 k-values, double-buffered through LDS with 16-byte loads ([2][128][36] floats; the loads of slab
// s + 1 are in flight while slab s is multiplied; one barrier per slab).  At C <= 4096 the prepared centroids stay in L2:
// the row tile is the only HBM stream.
//   split     wave w owns centroids [32 w, 32 w + 32) of the tile and ALL RB row blocks: RB accumulators of 32 x 32.  The
//             centroids are the instruction's M side and the rows its N side, so a lane's 16 results are 16 centroids of ONE
//             row (lane & 31), and the argmin starts inside the lane.
//   shape     v_mfma_f32_32x32x2_f32: per 16-byte LDS read of an operand it issues four instructions of 2 k-values — lane half
//             h reads k = 8 j + 4 h .. + 3 of both operands, and the k-order inside a slab is permuted the same way on both
//             sides, which a dot product does not see.  Against 16x16x4 the 32 x 32 tile reads each operand half as often per
//             product (1 + RB reads feed 4 RB instructions), and its 16 RB accumulator registers are no pressure at one
//             workgroup of 4 waves per CU, which is what the LDS allows anyway.
//   epilogue  behind a centroid tile's last slab, per row block, in registers: score = |c|^2 - 2 x.c (L2^2) or -x.c (inner
//             product, cosine), which ranks like the real distance; the lane's running (best, its centroid, best of the
//             others), centroids at or beyond n_centroids skipped.  Ties keep the lower centroid.
//   meeting   behind the last tile the two lane halves meet by one shuffle, the four waves through LDS, merged in wave
//             order; no atomics.
//   verdict   row certified iff second - best > margin(row) (assign_margin below); its label is the winner and its distance
//             ONE canonical walk of (winner, row) over the tile still in LDS, the winner's prepared centroid read from L2.
//             Every other row — a row that is not finite, a call whose centroids are not — is appended to the call's list
//             through a wave-aggregated counter: one vector atomic per wave.
// Sizes are choices (128-centroid tiles, 32-deep slabs, the + 4 padding), none of them measured.
#include "ehx_kernels.h"

namespace ehx {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));

constexpr uint32_t kAsgThreads = 256;
constexpr uint32_t kAsgTileC = 128;              // centroids of a tile: 32 per wave (the prepared centroids are padded to it)
constexpr uint32_t kAsgBK = 32;                  // k-values of a slab
constexpr uint32_t kAsgSlabLd = kAsgBK + 4;      // floats between two centroids of a slab in LDS
constexpr uint32_t kAsgPad = 4;                  // floats behind a row of the tile in LDS
constexpr uint32_t kAsgExactBlock = 8;           // centroids a row is walked against at once (canon_dist_lane_multi)
constexpr uint32_t kAsgNone = 0xFFFFFFFFu;       // EHX_ASSIGN_NONE

static_assert(kAssignTileC == kAsgTileC, "the host pads the prepared centroids to the filter's tile");

// slabs [2][128][36] | per wave and row (best, second, centroid) [4][TM][3] | |x|^2 [TM] | 16 words | the row tile
__host__ __device__ constexpr size_t assign_filter_lds_bytes(uint32_t ld, uint32_t tm) {
  return sizeof(float) * (2u * kAsgTileC * kAsgSlabLd + 12u * tm + tm + 16u + (size_t)tm * (ld + kAsgPad));
}
constexpr uint32_t kAsgMaxLd = (uint32_t)((kMaxLds - assign_filter_lds_bytes(0, 32)) / (32u * sizeof(float)) - kAsgPad) & ~31u;
static_assert(assign_filter_lds_bytes(kAsgMaxLd, 32) <= kMaxLds, "the smallest row tile fits one CU");
constexpr uint32_t kAsgExactMaxLd = (uint32_t)(kMaxLds / (kAsgExactBlock * sizeof(float))) & ~31u;

// The certificate's margin: certified iff second - best > margin.  With u = 2^-24, n = dims, nx >= |x| and nc >= every |c| up
// to the factors folded into 1.05 (DESIGN.md §e.33 derives every term):
//   W = (nx + nc)^2 (L2^2)  |  nx nc (inner product, cosine)
//   |filter score - real score|            <= (2 n + 2) u' W    any accumulation order, every operation within 2 u
//   |canonical distance - real distance|   <= (n + 3) u' W + 6 u'   (the 6 u': the joins around 1 - sum; not L2^2)
//   margin = 2 (both) = (6 n + 10) u' W + 12 u', times 1.05 for u' / u, the norms' own rounding and this evaluation,
//   plus the underflow term 8 n 2^-126 (nx + nc + 2): inputs, products and sums that a flush to zero may have moved.
// W at or above 1e30 (a square may overflow), or anything not finite: +Inf, nothing is certified.
template <int METRIC>
__device__ __forceinline__ float assign_margin(uint32_t dims, float xn2, float cmax2) {
  const float nx = __builtin_sqrtf(xn2), nc = __builtin_sqrtf(cmax2), n = (float)dims;
  const float W = METRIC == 0 ? (nx + nc) * (nx + nc) : nx * nc;
  if (!(W < 1e30f)) return __builtin_inff();
  const float u = 5.9604645e-8f;
  return 1.05f * ((6.0f * n + 10.0f) * u * W + (METRIC == 0 ? 0.0f : 12.0f * u)) + 8.0f * n * 1.1754944e-38f * (nx + nc + 2.0f);
}

// (best, second, centroid) of one row: a further score, in ascending centroid order — a tie keeps the lower centroid and
// closes the gap; a NaN compares false and is no candidate (a call that could hold one is never certified)
__device__ __forceinline__ void asg_take(float s, uint32_t c, float& best, float& second, uint32_t& bc) {
  if (s < best) {
    second = best;
    best = s;
    bc = c;
  } else if (s < second) {
    second = s;
  }
}
// ... and two such triples over disjoint centroids
__device__ __forceinline__ void asg_merge(float ob, float os, uint32_t oc, float& best, float& second, uint32_t& bc) {
  const bool other = ob < best || (ob == best && oc < bc);
  const float lose = other ? best : ob, s2 = other ? os : second;
  if (other) {
    best = ob;
    bc = oc;
  }
  second = lose < s2 ? lose : s2;
}

}  // namespace

// one wave per prepared centroid (padding rows too: their |c|^2 is 0)
__global__ __launch_bounds__(256) void centroid_stats_kernel(const float* __restrict__ cent, uint32_t c_rows, uint32_t n_cent,
                                                             uint32_t ld, float* __restrict__ cn2, uint32_t* __restrict__ bad) {
  const uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (c >= c_rows) return;
  float s = 0.0f;
  for (uint32_t m = lane; m < ld; m += 64) {
    const float v = cent[(size_t)c * ld + m];
    s += v * v;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
  if (lane == 0) {
    cn2[c] = s;
    if (c < n_cent && !(s < __builtin_inff())) atomicOr(bad, 1u);   // (an Inf or NaN component, or a norm that overflows)
  }
}

template <int RB, bool HALFX, int METRIC>
__global__ __launch_bounds__(kAsgThreads) void assign_filter_kernel(const AssignArgs a) {
  constexpr uint32_t TM = 32u * RB;
  constexpr int m01 = METRIC == 0 ? 0 : 1;
  extern __shared__ float4 assign_lds[];
  float* cs = (float*)assign_lds;                                  // [2][128][36]
  float* red_f = cs + 2u * kAsgTileC * kAsgSlabLd;                 // [4][TM][2] best, second
  uint32_t* red_c = (uint32_t*)(red_f + 8u * TM);                  // [4][TM]
  float* xn2_s = (float*)(red_c + 4u * TM);                        // [TM]
  float* misc = xn2_s + TM;                                        // [16]: the waves' maxima of |c|^2
  float* xs = misc + 16;                                           // [TM][ld + 4]
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6, h = lane >> 5, l31 = lane & 31u;
  const uint32_t ld = a.rows.ld, dims = a.rows.dims, xld = ld + kAsgPad;
  const uint32_t r_base = blockIdx.x * TM;                         // (relative to row0)
  const bool cent_bad = *a.bad != 0;

  // ---- the row tile, once ----
  {
    constexpr uint32_t kE = HALFX ? 8 : 4;                         // elements of a 16-byte unit as stored
    const uint32_t upr = ld / kE;
    for (uint32_t i = tid; i < TM * upr; i += kAsgThreads) {
      const uint32_t r = i / upr, un = i - r * upr, m0 = un * kE;
      float v[kE];
#pragma unroll
      for (uint32_t j = 0; j < kE; ++j) v[j] = 0.0f;
      if (r_base + r < a.n_rows) {
        const uint64_t id = a.row0 + r_base + r;
        const float sc = METRIC == 2 ? a.rows.inv_norm[id] : 1.0f;
        const float4 raw = *(const float4*)((const char*)a.rows.X + ((size_t)id * ld + m0) * (HALFX ? 2 : 4));
        if (HALFX) {
          const half8_t hv = *(const half8_t*)&raw;
#pragma unroll
          for (uint32_t j = 0; j < kE; ++j) v[j] = (float)hv[j];
        } else {
          v[0] = raw.x, v[1] = raw.y, v[2] = raw.z, v[3] = raw.w;
        }
#pragma unroll
        for (uint32_t j = 0; j < kE; ++j) v[j] = m0 + j < dims ? (METRIC == 2 ? ex_mul(v[j], sc) : v[j]) : 0.0f;
      }
#pragma unroll
      for (uint32_t j = 0; j < kE; j += 4) *(float4*)(xs + (size_t)r * xld + m0 + j) = make_float4(v[j], v[j + 1], v[j + 2], v[j + 3]);
    }
  }
  // the largest |c|^2 of the call (every workgroup for itself: C <= 4096 words from L2)
  {
    float mx = 0.0f;
    for (uint32_t c = tid; c < a.n_cent; c += kAsgThreads) mx = fmaxf(mx, a.cn2[c]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d, 64));
    if (lane == 0) misc[w] = mx;
  }
  __syncthreads();
  // |x|^2 of the tile's rows as the filter sees them: 256 / TM threads per row, any order (the margin covers it)
  {
    constexpr uint32_t G = kAsgThreads / TM;
    const uint32_t r = tid / G, g = tid % G;
    float s = 0.0f;
    for (uint32_t m = g; m < ld / 4u; m += G) {
      const float4 v = *(const float4*)(xs + (size_t)r * xld + 4u * m);
      s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
#pragma unroll
    for (uint32_t d = G >> 1; d > 0; d >>= 1) s += __shfl_xor(s, (int)d, 64);
    if (g == 0) xn2_s[r] = s;
  }

  float best[RB], second[RB];
  uint32_t bc[RB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) best[rb] = second[rb] = __builtin_inff(), bc[rb] = kAsgNone;

  if (!cent_bad) {
    // ---- every centroid tile past the row tile ----
    const uint32_t nks = ld / kAsgBK, n_ct = (a.n_cent + kAsgTileC - 1) / kAsgTileC, n_slabs = nks * n_ct;
    f32x16 acc[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[rb][j] = 0.0f;
    // slab s = (tile s / nks, k-slab s % nks): thread t moves 16-byte pieces t, t + 256, ... of its [128][32] floats (macros:
    // the staged pieces stay in registers)
    float4 st0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), st1 = st0, st2 = st0, st3 = st0;
    const float* src = a.cent + (size_t)(tid >> 3) * ld + 4u * (tid & 7u);          // piece t of slab (0, 0); piece t + 256 j: 32 j centroids on
    float* dst = cs + (tid >> 3) * kAsgSlabLd + 4u * (tid & 7u);
#define EHX_ASG_SLAB_LOAD(S)                                                                                    \
  {                                                                                                             \
    const uint32_t ct_ = (S) / nks, ks_ = (S) - ct_ * nks;                                                      \
    const float* p_ = src + (size_t)ct_ * kAsgTileC * ld + ks_ * kAsgBK;                                        \
    st0 = *(const float4*)p_;                                                                              \
    st1 = *(const float4*)(p_ + (size_t)32u * ld);                                                         \
    st2 = *(const float4*)(p_ + (size_t)64u * ld);                                                         \
    st3 = *(const float4*)(p_ + (size_t)96u * ld);                                                         \
  }
#define EHX_ASG_SLAB_STORE(BUF)                                                                                 \
  {                                                                                                             \
    float* d_ = dst + (size_t)(BUF) * kAsgTileC * kAsgSlabLd;                                                   \
    *(float4*)d_ = st0;                                                                                    \
    *(float4*)(d_ + 32u * kAsgSlabLd) = st1;                                                               \
    *(float4*)(d_ + 64u * kAsgSlabLd) = st2;                                                               \
    *(float4*)(d_ + 96u * kAsgSlabLd) = st3;                                                               \
  }
    EHX_ASG_SLAB_LOAD(0u)
    EHX_ASG_SLAB_STORE(0u)
    __syncthreads();
    uint32_t ct = 0, ks = 0;
    for (uint32_t s = 0; s < n_slabs; ++s) {
      if (s + 1 < n_slabs) EHX_ASG_SLAB_LOAD(s + 1u)
      const float* cw = cs + (size_t)(s & 1u) * kAsgTileC * kAsgSlabLd + (w * 32u + l31) * kAsgSlabLd + 4u * h;
      const float* xw = xs + (size_t)l31 * xld + ks * kAsgBK + 4u * h;
#pragma unroll
      for (uint32_t j8 = 0; j8 < kAsgBK / 8u; ++j8) {
        const float4 c4 = *(const float4*)(cw + 8u * j8);
        float4 x4[RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) x4[rb] = *(const float4*)(xw + (size_t)rb * 32u * xld + 8u * j8);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(c4.x, x4[rb].x, acc[rb], 0, 0, 0);
          acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(c4.y, x4[rb].y, acc[rb], 0, 0, 0);
          acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(c4.z, x4[rb].z, acc[rb], 0, 0, 0);
          acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(c4.w, x4[rb].w, acc[rb], 0, 0, 0);
        }
      }
      if (ks + 1 == nks) {
        // the tile's epilogue: result j of a lane is centroid 8 (j >> 2) + 4 h + (j & 3) of the wave's 32, row l31 of the block
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const uint32_t c0 = ct * kAsgTileC + w * 32u + 8u * g + 4u * h;
          const float4 cn = METRIC == 0 ? *(const float4*)(a.cn2 + c0) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if (c0 + i < a.n_cent) {
#pragma unroll
              for (int rb = 0; rb < RB; ++rb) {
                const float dot = acc[rb][4 * g + i];
                const float cni = i == 0 ? cn.x : i == 1 ? cn.y : i == 2 ? cn.z : cn.w;
                asg_take(METRIC == 0 ? cni - 2.0f * dot : -dot, c0 + i, best[rb], second[rb], bc[rb]);
              }
            }
          }
        }
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
          for (int j = 0; j < 16; ++j) acc[rb][j] = 0.0f;
        ks = 0;
        ct += 1;
      } else {
        ks += 1;
      }
      if (s + 1 < n_slabs) EHX_ASG_SLAB_STORE((s + 1u) & 1u)
      __syncthreads();   // (slab s + 1 has landed, and nobody reads slab s any more)
    }
#undef EHX_ASG_SLAB_LOAD
#undef EHX_ASG_SLAB_STORE
  }

  // ---- the lane halves meet, then the waves ----
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    const float ob = __shfl_xor(best[rb], 32, 64), os = __shfl_xor(second[rb], 32, 64);
    const uint32_t oc = (uint32_t)__shfl_xor((int)bc[rb], 32, 64);
    asg_merge(ob, os, oc, best[rb], second[rb], bc[rb]);
    if (h == 0) {
      const uint32_t at = w * TM + (uint32_t)rb * 32u + l31;
      red_f[2u * at] = best[rb];
      red_f[2u * at + 1u] = second[rb];
      red_c[at] = bc[rb];
    }
  }
  __syncthreads();
  if (tid < TM) {
    const uint32_t i = r_base + tid;
    float b = red_f[2u * tid], s2 = red_f[2u * tid + 1u];
    uint32_t c = red_c[tid];
#pragma unroll
    for (uint32_t ww = 1; ww < 4; ++ww) asg_merge(red_f[2u * (ww * TM + tid)], red_f[2u * (ww * TM + tid) + 1u], red_c[ww * TM + tid], b, s2, c);
    const float cmax2 = fmaxf(fmaxf(misc[0], misc[1]), fmaxf(misc[2], misc[3]));
    const bool row = i < a.n_rows;
    const bool cert = row && c != kAsgNone && (s2 - b > assign_margin<METRIC>(dims, xn2_s[tid], cmax2));
    if (cert) {
      a.label[i] = c;
      if (a.dist) a.dist[i] = canon_dist_lane_t<m01, false, false>(a.cent + (size_t)c * ld, xs + (size_t)tid * xld, 1.0f, dims);
    }
    // the rest goes on the call's list: one atomic per wave
    const unsigned long long un = __ballot(row && !cert), ok = __ballot(cert);
    uint32_t base = 0;
    if (lane == 0) {
      if (un) base = atomicAdd(&a.ctl[0], (uint32_t)__builtin_popcountll(un));
      if (ok) atomicAdd(&a.ctl[1], (uint32_t)__builtin_popcountll(ok));
    }
    base = (uint32_t)__shfl((int)base, 0, 64);
    if (row && !cert) a.list[base + (uint32_t)__builtin_popcountll(un & ((1ull << lane) - 1ull))] = i;
  }
}

// The canonical route.  A workgroup takes walk_rows rows per step (fp32 rows: a lane per row; binary16 and block-permuted
// rows: a 4-lane group) and walks each against ALL centroids, kAsgExactBlock at a time staged in LDS as a query is staged;
// the minimum over the (distance, centroid) keys is the answer, ties to the lower centroid, a NaN distance no candidate.
template <int LAYOUT, int METRIC>
__global__ __launch_bounds__(kAsgThreads) void assign_exact_kernel(const AssignArgs a, uint32_t n_work, uint32_t listed) {
  constexpr bool kMulti = LAYOUT == kLayoutF32;
  constexpr uint32_t kStep = walk_rows<LAYOUT, true>(kAsgThreads);
  constexpr int m01 = METRIC == 0 ? 0 : 1;
  extern __shared__ float4 assign_lds[];
  float* qs = (float*)assign_lds;   // [kAsgExactBlock][ld]
  const uint32_t tid = threadIdx.x, ld = a.rows.ld, dims = a.rows.dims;
  for (uint32_t base = blockIdx.x * kStep; base < n_work; base += gridDim.x * kStep) {
    const uint32_t at = base + walk_slot<LAYOUT, true>(tid);   // (the same in the four lanes of a group)
    const bool ok = at < n_work;
    const uint32_t i = ok ? (listed ? a.list[at] : at) : 0u;
    const uint64_t id = a.row0 + i;
    uint64_t best = kKeyInf;
    for (uint32_t c0 = 0; c0 < a.n_cent; c0 += kAsgExactBlock) {
      __syncthreads();   // (everyone is done with the last block)
      for (uint32_t j = 0; j < kAsgExactBlock; ++j)   // (rows behind n_centroids are the padding's zeros)
        stage_query_lds<LAYOUT>(qs + (size_t)j * ld, a.cent + (size_t)(c0 + j) * ld, ld, tid, kAsgThreads);
      __syncthreads();
      const uint32_t nb = a.n_cent - c0 < kAsgExactBlock ? a.n_cent - c0 : kAsgExactBlock;
      if constexpr (kMulti) {
        if (ok) {
          float d[kAsgExactBlock];
          const float sc = METRIC == 2 ? a.rows.inv_norm[id] : 1.0f;
          canon_dist_lane_multi<m01, METRIC == 2, (int)kAsgExactBlock>(qs, ld, (const float*)a.rows.X + (size_t)id * ld, sc, dims, d);
#pragma unroll
          for (uint32_t j = 0; j < kAsgExactBlock; ++j) {
            const uint64_t key = dist_key(d[j], c0 + j, j < nb);
            best = key < best ? key : best;
          }
        }
      } else {
        for (uint32_t j = 0; j < nb; ++j) {
          bool mine;
          const float d = walk_row<LAYOUT, METRIC, true>(a.rows, qs + (size_t)j * ld, id, ok, tid, &mine);
          const uint64_t key = dist_key(d, c0 + j, mine);
          best = key < best ? key : best;
        }
      }
    }
    if (ok && (kMulti || (tid & 3u) == 0)) {
      a.label[i] = best == kKeyInf ? kAsgNone : (uint32_t)best;
      if (a.dist) a.dist[i] = best == kKeyInf ? __builtin_nanf("") : ordered_to_f32((uint32_t)(best >> 32));
    }
  }
}

// keys of the sums' sort: a label that names a centroid, else n_cent (<= 4096: two 8-bit digits)
__global__ __launch_bounds__(256) void label_keys_kernel(const uint32_t* __restrict__ label, uint32_t n, uint32_t n_cent,
                                                         uint32_t* __restrict__ keys) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) keys[i] = label[i] < n_cent ? label[i] : n_cent;
}

// one Lloyd step's divide: new_c = fl(sum_c / fl32(count_c)) where count_c > 0, else the centroid keeps its bytes
__global__ __launch_bounds__(256) void lloyd_divide_kernel(const float* __restrict__ sums, const uint32_t* __restrict__ count,
                                                           uint32_t n_cent, uint32_t dims, float* __restrict__ cent) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= (size_t)n_cent * dims) return;
  const uint32_t n = count[i / dims];
  if (n) cent[i] = ex_div(sums[i], (float)n);
}

// *moved += rows whose label differs; one atomic per wave
__global__ __launch_bounds__(256) void count_moved_kernel(const uint32_t* __restrict__ was, const uint32_t* __restrict__ is,
                                                          uint32_t n, uint32_t* __restrict__ moved) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const unsigned long long m = __ballot(i < n && was[i] != is[i]);
  if ((threadIdx.x & 63u) == 0 && m) atomicAdd(moved, (uint32_t)__builtin_popcountll(m));
}

namespace {

typedef void (*AssignFilterFn)(const AssignArgs);
typedef void (*AssignExactFn)(const AssignArgs, uint32_t, uint32_t);
#define EHX_ASG_FILTER(RB) \
  {assign_filter_kernel<RB, false, 0>, assign_filter_kernel<RB, false, 1>, assign_filter_kernel<RB, false, 2>, \
   assign_filter_kernel<RB, true, 0>, assign_filter_kernel<RB, true, 1>, assign_filter_kernel<RB, true, 2>}
const AssignFilterFn kFilterFns[3][6] = {EHX_ASG_FILTER(1), EHX_ASG_FILTER(2), EHX_ASG_FILTER(4)};   // [log2 RB][half * 3 + metric]
#undef EHX_ASG_FILTER
#define EHX_ASG_EXACT(L) assign_exact_kernel<L, 0>, assign_exact_kernel<L, 1>, assign_exact_kernel<L, 2>
const AssignExactFn kExactFns[9] = {EHX_ASG_EXACT(kLayoutF32), EHX_ASG_EXACT(kLayoutF16), EHX_ASG_EXACT(kLayoutPerm)};
#undef EHX_ASG_EXACT
DynLdsAttr g_filter_lds[3], g_exact_lds;

bool assign_args_ok(const AssignArgs& a) {
  return a.n_cent && a.n_cent <= kAssignMaxCentroids && (a.rows.ld & 31u) == 0 && a.rows.metric >= 0 && a.rows.metric <= 2 &&
         a.cent && a.cn2 && a.bad && a.label && a.list && a.ctl && a.row0 + a.n_rows <= a.rows.n_rows;
}

}  // namespace

uint32_t assign_max_ld() { return kAsgMaxLd; }
uint32_t assign_exact_max_ld() { return kAsgExactMaxLd; }

hipError_t launch_centroid_stats(const float* cent, uint32_t c_rows, uint32_t n_cent, uint32_t ld, float* cn2, uint32_t* bad,
                                 hipStream_t st) {
  hipLaunchKernelGGL(centroid_stats_kernel, dim3((c_rows + 3) / 4), dim3(256), 0, st, cent, c_rows, n_cent, ld, cn2, bad);
  return hipGetLastError();
}

hipError_t launch_assign_filter(const AssignArgs& a, hipStream_t st) {
  if (a.n_rows == 0) return hipSuccess;
  if (!assign_args_ok(a) || a.rows.x_perm || a.rows.ld > kAsgMaxLd) return hipErrorInvalidValue;
  int lg = 2;   // the largest row tile that fits
  while (lg > 0 && assign_filter_lds_bytes(a.rows.ld, 32u << lg) > kMaxLds) --lg;
  const uint32_t tm = 32u << lg;
  const size_t lds = assign_filter_lds_bytes(a.rows.ld, tm);
  hipError_t e = g_filter_lds[lg].ensure(kFilterFns[lg], 6, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kFilterFns[lg][(a.rows.x_half ? 3 : 0) + a.rows.metric], dim3((a.n_rows + tm - 1) / tm), dim3(kAsgThreads), lds,
                     st, a);
  return hipGetLastError();
}

hipError_t launch_assign_exact(const AssignArgs& a, uint32_t n_work, bool listed, int n_cus, hipStream_t st) {
  if (n_work == 0) return hipSuccess;
  if (!assign_args_ok(a) || a.rows.ld > kAsgExactMaxLd || n_work > a.n_rows) return hipErrorInvalidValue;
  const int layout = row_layout(a.rows.x_half, a.rows.x_perm);
  const uint32_t step = layout == kLayoutF32 ? kAsgThreads : kAsgThreads / 4u;
  const size_t lds = (size_t)kAsgExactBlock * a.rows.ld * sizeof(float);
  hipError_t e = g_exact_lds.ensure(kExactFns, 9, lds);
  if (e != hipSuccess) return e;
  const uint32_t want = (n_work + step - 1) / step, cap = 8u * (uint32_t)(n_cus > 0 ? n_cus : 1);
  hipLaunchKernelGGL(kExactFns[layout * 3 + a.rows.metric], dim3(want < cap ? want : cap), dim3(kAsgThreads), lds, st, a, n_work,
                     listed ? 1u : 0u);
  return hipGetLastError();
}

hipError_t launch_label_keys(const uint32_t* label, uint32_t n, uint32_t n_cent, uint32_t* keys, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(label_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, st, label, n, n_cent, keys);
  return hipGetLastError();
}

hipError_t launch_lloyd_divide(const float* sums, const uint32_t* count, uint32_t n_cent, uint32_t dims, float* cent, hipStream_t st) {
  hipLaunchKernelGGL(lloyd_divide_kernel, dim3((uint32_t)(((size_t)n_cent * dims + 255) / 256)), dim3(256), 0, st, sums, count, n_cent,
                     dims, cent);
  return hipGetLastError();
}

hipError_t launch_count_moved(const uint32_t* was, const uint32_t* is, uint32_t n, uint32_t* moved, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(count_moved_kernel, dim3((n + 255) / 256), dim3(256), 0, st, was, is, n, moved);
  return hipGetLastError();
}

}  // namespace ehx
