// The oracle's distance arithmetic, stated ONCE: every canonical distance of the engine — prepared query to stored row,
// stored row to stored row — is built from the pieces of this header, and nothing outside it may restate any of them.
// Included by ehx_kernels.h (which every kernel file includes), ahead of k_exact_common.h's row walk.
//
// The order is hnswlib's SSE kernels' (space_l2.h / space_ip.h; oracle/hnsw_oracle.hpp restates them):
//   * canon_body: a row is a body of whole 16- (or, up to 16 dims, 4-) float pieces and a scalar tail;
//   * canon_term: one element is one product and one add, NOT fused (the library is built with -ffp-contract=off);
//   * over the body, element m feeds partial sum m & 3, in the order of m: four strided sums;
//   * canon_hsum: ((p0 + p1) + p2) + p3;
//   * EHX_CANON_RUN: the tail is one more sum, element after element;
//   * EHX_CANON_FINISH / canon_finish: body and tail are joined, and an inner product becomes the distance 1 - sum.
// metric01: 0 = L2^2, 1 = 1 - inner product.  For cosine the stored row is normalised on the fly (x * inv_norm, one
// rounding — hnswlib-python's normalize_vector) and the query arrives normalised.
// The walkers differ only in who plays the four SSE lanes and how the row reaches them: a 4-lane group over plain fp32 or
// binary16 rows (canon_dist), one lane with 16-byte loads (canon_dist_lane_t), a 4-lane group over the block-permuted
// search copy (canon_dist_group_t, _pair, _quad; wave_group_dists hands a wave's rows to them), one lane over two rows of
// the search copy (row_row_dist).
#pragma once

namespace ehx {

// Exactly-rounded single operations.  HIP's __fmul_rn/__fadd_rn are plain * and + (contractible) and __fsqrt_rn is the
// approximate native sqrt, so they are NOT used; the library relies on -ffp-contract=off and on hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt for / and sqrt.
__device__ __forceinline__ float ex_add(float a, float b) { return a + b; }
__device__ __forceinline__ float ex_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float ex_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float ex_div(float a, float b) { return a / b; }
__device__ __forceinline__ float ex_sqrt(float a) { return __builtin_sqrtf(a); }

// ---- the pieces ----
// elements [0, body) go through the four strided sums, [body, dims) through the tail
__host__ __device__ inline uint32_t canon_body(uint32_t dims) {
  if ((dims & 15u) == 0 || (dims & 3u) == 0) return dims;
  if (dims > 16) return dims & ~15u;
  if (dims > 4) return dims & ~3u;
  return 0;
}

// One element's term is one product and one add, not fused: L2^2 multiplies the difference of the operands by itself, the
// inner product one operand by the other.  canon_lhs is the product's left factor; the 16-byte steps below form their four
// left factors first and then their four terms.
template <int METRIC01>
__device__ __forceinline__ float canon_lhs(float q, float x) { return METRIC01 == 0 ? ex_sub(q, x) : q; }
template <int METRIC01>
__device__ __forceinline__ float canon_term(float acc, float lhs, float x) {
  return ex_add(acc, ex_mul(lhs, METRIC01 == 0 ? lhs : x));
}

__device__ __forceinline__ float canon_hsum(float p0, float p1, float p2, float p3) {
  return ex_add(ex_add(ex_add(p0, p1), p2), p3);
}

// The join, stated once as the macro EHX_CANON_FINISH.  It ends the walker that expands it (it returns).  RES: the body's
// sum, an lvalue; TAIL: a statement that adds the tail's terms to the float `tail` (declared here, 0 before it) — an
// EHX_CANON_RUN — run only where the row has a tail.  hnswlib 0.5.x's residual variants of the inner product turn both
// halves into distances (1 - sum) and combine them as  res + res_tail - 1.0f  (space_ip.h; oracle/hnsw_oracle.hpp:ip_dist).
// (Macros and not functions, like the ring below: with the tail loop or the join behind a call — a function, a functor —
// the compiler lays the walkers' blocks out differently and the kernels' register use moves; as text they compile to the
// code of the hand-written tails they replace.)
#define EHX_CANON_FINISH(METRIC01, RES, BODY, DIMS, TAIL)                                                         \
  if ((BODY) != (DIMS)) {                                                                                         \
    float tail = 0.0f;                                                                                            \
    TAIL                                                                                                          \
    if ((METRIC01) != 0 && (BODY)) return ex_sub(ex_add(ex_sub(1.0f, RES), ex_sub(1.0f, tail)), 1.0f);            \
    RES = (BODY) ? ex_add(RES, tail) : tail;                                                                      \
  }                                                                                                               \
  if ((METRIC01) != 0) RES = ex_sub(1.0f, RES);                                                                   \
  return RES;
// a whole row (body == dims): the join of a sum with no tail
#define EHX_CANON_FINISH_WHOLE(METRIC01, RES) EHX_CANON_FINISH(METRIC01, RES, 0u, 0u, ;)
__device__ __forceinline__ float canon_finish(int metric01, float res) { EHX_CANON_FINISH_WHOLE(metric01, res) }

// row element load: fp32 rows as stored, fp16 rows widened exactly (every half is a float)
__device__ __forceinline__ float ld_row(const float* x, uint32_t m) { return x[m]; }
__device__ __forceinline__ float ld_row(const __half* x, uint32_t m) { return __half2float(x[m]); }

// position of element m of a row inside the search copy / the permuted query
__host__ __device__ inline uint32_t search_copy_pos(uint32_t m) { return (m & ~15u) + ((m & 3u) << 2) + ((m >> 2) & 3u); }

// One sum over the elements LO, LO + STEP, ... below HI, in that order, added to ACC: a tail (STEP 1) or one SSE lane's share
// of the body (STEP 4).  PERM: the operands are in the search copy's block order.  Either operand is multiplied by its scale
// first when its flag says so (a multiplication by 1.0f is exact).  A is the query side (L2^2: a - b), B the stored row;
// B_FIRST: the row's element is loaded before the query's (the query-to-row walkers; row_row_dist loads xa, then xb).
// METRIC01 may be a runtime value: the test sits around the term, per element.
#define EHX_CANON_RUN(METRIC01, PERM, ACC, A, SA, SCALE_A, B, SB, SCALE_B, B_FIRST, LO, HI, STEP)        \
  for (uint32_t m_ = (LO); m_ < (HI); m_ += (STEP)) {                                                   \
    const uint32_t pos_ = (PERM) ? search_copy_pos(m_) : m_;                                            \
    float av_, bv_;                                                                                     \
    if (B_FIRST) bv_ = (SCALE_B) ? ex_mul(ld_row(B, pos_), SB) : ld_row(B, pos_);                       \
    av_ = (SCALE_A) ? ex_mul(ld_row(A, pos_), SA) : ld_row(A, pos_);                                    \
    if (!(B_FIRST)) bv_ = (SCALE_B) ? ex_mul(ld_row(B, pos_), SB) : ld_row(B, pos_);                    \
    if ((METRIC01) == 0) ACC = canon_term<0>(ACC, canon_lhs<0>(av_, bv_), bv_);                         \
    else ACC = canon_term<1>(ACC, canon_lhs<1>(av_, bv_), bv_);                                         \
  }

// x * xs per element: four multiplies, or two packed ones (v_pk_mul_f32: IEEE, one rounding per element like the scalar form)
__device__ __forceinline__ float4 scale_s4(float4 xv, float xs) {
  xv.x = ex_mul(xv.x, xs);
  xv.y = ex_mul(xv.y, xs);
  xv.z = ex_mul(xv.z, xs);
  xv.w = ex_mul(xv.w, xs);
  return xv;
}
__device__ __forceinline__ float4 scale_f4(float4 xv, float xs) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const f32x2 sc = {xs, xs};
  f32x2 lo = {xv.x, xv.y}, hi = {xv.z, xv.w};
  lo = lo * sc;
  hi = hi * sc;
  return make_float4(lo.x, lo.y, hi.x, hi.y);
}

// 16 bytes of a plain row: element j feeds partial sum j
template <int METRIC01, bool SCALE>
__device__ __forceinline__ void canon_lane_step(float4 xv, const float4 qv, float xscale, float& p0, float& p1,
                                                float& p2, float& p3) {
  if (SCALE) xv = scale_s4(xv, xscale);
  const float l0 = canon_lhs<METRIC01>(qv.x, xv.x), l1 = canon_lhs<METRIC01>(qv.y, xv.y),
              l2 = canon_lhs<METRIC01>(qv.z, xv.z), l3 = canon_lhs<METRIC01>(qv.w, xv.w);
  p0 = canon_term<METRIC01>(p0, l0, xv.x);
  p1 = canon_term<METRIC01>(p1, l1, xv.y);
  p2 = canon_term<METRIC01>(p2, l2, xv.z);
  p3 = canon_term<METRIC01>(p3, l3, xv.w);
}

// 16 bytes of the search copy: the first NCOMP inputs of ONE partial sum P, in order (a macro: see EHX_CANON_FINISH)
#define EHX_CANON_PIECE(METRIC01, QV, XV, P, NCOMP)                                                           \
  {                                                                                                           \
    const float l0_ = canon_lhs<METRIC01>(QV.x, XV.x), l1_ = canon_lhs<METRIC01>(QV.y, XV.y),                 \
                l2_ = canon_lhs<METRIC01>(QV.z, XV.z), l3_ = canon_lhs<METRIC01>(QV.w, XV.w);                 \
    P = canon_term<METRIC01>(P, l0_, XV.x);                                                                   \
    if ((NCOMP) > 1) P = canon_term<METRIC01>(P, l1_, XV.y);                                                  \
    if ((NCOMP) > 2) P = canon_term<METRIC01>(P, l2_, XV.z);                                                  \
    if ((NCOMP) > 3) P = canon_term<METRIC01>(P, l3_, XV.w);                                                  \
  }
template <int METRIC01, bool SCALE = false>
__device__ __forceinline__ void canon_group_step(float4 xv, const float4 qv, float& p, int ncomp = 4, float xs = 1.0f) {
  if (SCALE) xv = scale_f4(xv, xs);
  EHX_CANON_PIECE(METRIC01, qv, xv, p, ncomp)
}

// ---- the register ring ----
// A lane's walk over the n 16-byte pieces x4[0], x4[S], x4[2 S], ... of its row, in order.
//
// The walk is HBM-latency bound unless many loads are in flight per lane (a row is ld*4 contiguous
// bytes = ld/32 cache lines that nobody else touches; the plain loop compiles to ONE 16-byte load in
// flight per lane): the first nblk * kLaneBlk pieces are cut into blocks of kLaneBlk 16-byte loads and a ring of three
// register blocks keeps two blocks in flight ahead of the block being accumulated.  Measured on the
// graph bench (profiles/r01_m_*): 16-24 loads in flight per lane are enough — kLaneBlk 8 and 16 are
// within 3 % of each other, 4 is 6 % slower at d=768 — because past that point the random row gathers
// are bound by what the memory system delivers for this pattern (scripts/ubench/gather_rows.hip:
// 27 lanes x private rows, 4 waves per CU: 4.2-4.5 TB/s; deeper queues thrash the 32-KiB L1).
// The accumulation order is unchanged (block after block, 16 bytes after 16 bytes), so the result is
// bit-identical to the plain loop.
// The schedule is ONE macro, instantiated by the lane walker (S = 1: the row's pieces are contiguous; four partial sums) and
// by the group walker (S = 4: every fourth piece is the lane's; one partial sum).  ACC(R, b) accumulates ring block b, whose
// pieces are in R; STEP(xv, m) accumulates piece m.  (A macro and not a function over functors: with functors the compiler
// schedules the steady state differently — two block loads back to back — where this text gives the code of the two
// hand-written rings it replaces.)
// Contract: ACC and STEP are statement macros of the walker (they end their own statements; the schedule writes no
// semicolon after them).  The expansion is one braced block that declares r0, r1, r2, b, rem, m, nblk_ and n_ in it, so
// the walker must not pass expressions that use those names; ACC and STEP see the walker's own variables (its partial
// sums, q4, the scale).
#ifndef EHX_LANE_BLK
#define EHX_LANE_BLK 8
#endif
constexpr int kLaneBlk = EHX_LANE_BLK;  // 16-byte loads per ring block (8: 128 B = one cache line per lane)

#define EHX_RING_LOAD(S, X4, R, B) \
  _Pragma("unroll") for (int i_ = 0; i_ < kLaneBlk; ++i_) R[i_] = X4[((size_t)(B) * kLaneBlk + i_) * S];
#define EHX_CANON_RING(S, X4, NBLK, N, ACC, STEP)                                                                 \
  {                                                                                                               \
    constexpr int BL_ = kLaneBlk;                                                                                 \
    const uint32_t nblk_ = (NBLK);                                                                                \
    float4 r0[BL_], r1[BL_], r2[BL_];                                                                             \
    uint32_t b = 0;                                                                                               \
    if (nblk_ >= 2) {                                                                                             \
      EHX_RING_LOAD(S, X4, r0, 0)                                                                                 \
      EHX_RING_LOAD(S, X4, r1, 1)                                                                                 \
      /* steady state: three blocks accumulated per trip, every load two blocks ahead of its use, no branches */  \
      for (; b + 5 <= nblk_; b += 3) {                                                                            \
        EHX_RING_LOAD(S, X4, r2, b + 2)                                                                           \
        ACC(r0, b)                                                                                                \
        EHX_RING_LOAD(S, X4, r0, b + 3)                                                                           \
        ACC(r1, b + 1)                                                                                            \
        EHX_RING_LOAD(S, X4, r1, b + 4)                                                                           \
        ACC(r2, b + 2)                                                                                            \
      }                                                                                                           \
      const uint32_t rem = nblk_ - b; /* 2, 3 or 4 blocks left; r0 / r1 hold blocks b / b+1 */                    \
      if (rem >= 3) { EHX_RING_LOAD(S, X4, r2, b + 2) }                                                           \
      ACC(r0, b)                                                                                                  \
      if (rem == 4) { EHX_RING_LOAD(S, X4, r0, b + 3) }                                                           \
      ACC(r1, b + 1)                                                                                              \
      if (rem >= 3) { ACC(r2, b + 2) }                                                                            \
      if (rem == 4) { ACC(r0, b + 3) }                                                                            \
    } else if (nblk_ == 1) {                                                                                      \
      EHX_RING_LOAD(S, X4, r0, 0)                                                                                 \
      ACC(r0, 0)                                                                                                  \
    }                                                                                                             \
    /* the pieces after the last full block (fewer than kLaneBlk with a ring), four loads at a time */            \
    uint32_t m = nblk_ * BL_;                                                                                     \
    const uint32_t n_ = (N);                                                                                      \
    for (; m + 4 <= n_; m += 4) {                                                                                 \
      const float4 t0 = X4[m * S], t1 = X4[(m + 1) * S], t2 = X4[(m + 2) * S], t3 = X4[(m + 3) * S];              \
      STEP(t0, m)                                                                                                 \
      STEP(t1, m + 1)                                                                                             \
      STEP(t2, m + 2)                                                                                             \
      STEP(t3, m + 3)                                                                                             \
    }                                                                                                             \
    for (; m < n_; ++m) STEP(X4[m * S], m)                                                                        \
  }

// ---- the walkers ----
// A 4-lane group over a plain row: lane `sub` plays SSE lane `sub`; all 4 lanes of the group must be active.  Result valid
// in sub-lane 0.
template <typename XT>
__device__ __forceinline__ float canon_dist(int metric, const float* __restrict__ q,
                                            const XT* __restrict__ x, float xscale, bool scale_x,
                                            uint32_t dims, int sub) {
  const uint32_t body = canon_body(dims);
  float part = 0.0f;
  if (metric == 0) { EHX_CANON_RUN(0, false, part, q, 1.0f, false, x, xscale, scale_x, true, sub, body, 4) }
  else { EHX_CANON_RUN(1, false, part, q, 1.0f, false, x, xscale, scale_x, true, sub, body, 4) }
  // horizontal sum in lane order within the 4-lane group
  const float t1 = __shfl_down(part, 1, 4), t2 = __shfl_down(part, 2, 4), t3 = __shfl_down(part, 3, 4);
  float res = canon_hsum(part, t1, t2, t3);  // (the result is valid in sub-lane 0)
  EHX_CANON_FINISH(metric, res, body, dims,
                   if (metric == 0) { EHX_CANON_RUN(0, false, tail, q, 1.0f, false, x, xscale, scale_x, true, body, dims, 1) }
                   else { EHX_CANON_RUN(1, false, tail, q, 1.0f, false, x, xscale, scale_x, true, body, dims, 1) })
}

// ONE lane: the lane keeps the 4 SSE partial sums itself and walks its row with 16-byte loads through the ring (q may live
// in LDS).  Used by the graph search and the graph insertion, where every lane owns one neighbour row.  Requires 16-byte
// aligned q and x (row stride ld % 4 == 0).  !RING: few registers, four loads in flight.
template <int METRIC01, bool SCALE, bool RING = true>
__device__ __forceinline__ float canon_dist_lane_t(const float* __restrict__ q, const float* __restrict__ x,
                                                   float xscale, uint32_t dims) {
  const uint32_t body = canon_body(dims);
  float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f, p3 = 0.0f;
  constexpr int BL = kLaneBlk;
  const float4* q4 = (const float4*)q;
  const float4* x4 = (const float4*)x;
#define EHX_LANE_ACC(R, B)                                         \
  _Pragma("unroll") for (int i_ = 0; i_ < BL; ++i_)                \
      canon_lane_step<METRIC01, SCALE>(R[i_], q4[(size_t)(B) * BL + i_], xscale, p0, p1, p2, p3);
#define EHX_LANE_STEP(XV, M) canon_lane_step<METRIC01, SCALE>(XV, q4[M], xscale, p0, p1, p2, p3);
  EHX_CANON_RING(1, x4, RING ? body / (4u * BL) : 0u, body / 4u, EHX_LANE_ACC, EHX_LANE_STEP)
#undef EHX_LANE_ACC
#undef EHX_LANE_STEP
  float res = canon_hsum(p0, p1, p2, p3);
  EHX_CANON_FINISH(METRIC01, res, body, dims, EHX_CANON_RUN(METRIC01, false, tail, q, 1.0f, false, x, xscale, SCALE, true, body, dims, 1))
}

// A 4-LANE GROUP over a row of the graph-mode SEARCH COPY (launch_make_search_copy: inside every 16-float block the four
// inputs of SSE partial sum j are 16 contiguous bytes; cosine rows are stored normalised).  Lane `sub` of the group plays
// SSE lane `sub`: per block it loads ONE float4 — the group reads the block as one coalesced 64-byte piece — and adds
// its four products to its partial sum in order.  qp is the query permuted the same way (LDS).  All four
// lanes of the group must be active; every lane returns the full result.
// SCALE (single-copy graph spaces: the rows are stored raw and permuted, not normalised): every element of
// the row is multiplied by xscale first — hnswlib-python's stored normalised row x * inv_norm, one rounding per element,
// formed on the fly; the products with the query then see exactly the values the normalised copy held.
template <int METRIC01, bool SCALE = false>
__device__ __forceinline__ float canon_dist_group_t(const float* __restrict__ qp, const float* __restrict__ xs, int sub,
                                                    uint32_t dims, float xscale = 1.0f) {
  const uint32_t body = canon_body(dims);
  float p = 0.0f;
  constexpr int BL = kLaneBlk;
  const uint32_t n16 = body / 16u;             // full 16-float blocks: one float4 per lane each
  const uint32_t nblk = n16 / BL;              // ring blocks
  const float4* x4 = (const float4*)xs + sub;  // block t of this lane: x4[4 t]
  const float4* q4 = (const float4*)qp + sub;
  // (SCALE: the ring block's query pieces are read from LDS together, ahead of its products — left to the scheduler,
  // the scaled walk reads one piece, waits for it, multiplies, and pays the LDS latency once per 16-float block)
#define EHX_GRP_ACC(R, B)                                                                                            \
  if (SCALE) {                                                                                                       \
    float4 qv_[BL];                                                                                                  \
    _Pragma("unroll") for (int i_ = 0; i_ < BL; ++i_) qv_[i_] = q4[((size_t)(B) * BL + i_) * 4];                      \
    _Pragma("unroll") for (int i_ = 0; i_ < BL; ++i_) R[i_] = scale_f4(R[i_], xscale);                               \
    _Pragma("unroll") for (int i_ = 0; i_ < BL; ++i_) canon_group_step<METRIC01, false>(R[i_], qv_[i_], p, 4, 1.0f); \
  } else {                                                                                                           \
    _Pragma("unroll") for (int i_ = 0; i_ < BL; ++i_)                                                                \
      canon_group_step<METRIC01, false>(R[i_], q4[((size_t)(B) * BL + i_) * 4], p, 4, 1.0f);                         \
  }
#define EHX_GRP_STEP(XV, T) canon_group_step<METRIC01, SCALE>(XV, q4[(T) * 4], p, 4, xscale);
  EHX_CANON_RING(4, x4, nblk, n16, EHX_GRP_ACC, EHX_GRP_STEP)
#undef EHX_GRP_ACC
#undef EHX_GRP_STEP
  // the 4-float pieces of a last, partial block (body % 16 / 4 of them): components 0..rem4-1
  const int rem4 = (int)((body & 15u) >> 2);
  if (rem4) canon_group_step<METRIC01, SCALE>(x4[n16 * 4], q4[n16 * 4], p, rem4, xscale);
  // horizontal sum in SSE-lane order, formed by every lane of the group
  const float t0 = __shfl(p, 0, 4), t1 = __shfl(p, 1, 4), t2 = __shfl(p, 2, 4), t3 = __shfl(p, 3, 4);
  float res = canon_hsum(t0, t1, t2, t3);
  EHX_CANON_FINISH(METRIC01, res, body, dims, EHX_CANON_RUN(METRIC01, true, tail, qp, 1.0f, false, xs, xscale, SCALE, true, body, dims, 1))
}

// Two rows of exactly 16 * N16 floats by one 4-lane group, all 2 * N16 loads of the lane in flight before the first
// product (a 128-dim row is ONE ring block of canon_dist_group_t: with more than 16 fresh neighbours the second pass
// would wait a second memory round trip).  Same arithmetic and order per row as canon_dist_group_t.
template <int METRIC01, int N16, bool SCALE = false>
__device__ __forceinline__ void canon_dist_group_pair(const float* __restrict__ qp, const float* __restrict__ xa,
                                                      const float* __restrict__ xb, int sub, float& res_a, float& res_b,
                                                      float sa = 1.0f, float sb = 1.0f) {
  const float4* a4 = (const float4*)xa + sub;
  const float4* b4 = (const float4*)xb + sub;
  const float4* q4 = (const float4*)qp + sub;
  float4 ra[N16], rb[N16];
#pragma unroll
  for (int i = 0; i < N16; ++i) ra[i] = a4[i * 4];
#pragma unroll
  for (int i = 0; i < N16; ++i) rb[i] = b4[i * 4];
  float pa = 0.0f, pb = 0.0f;
#pragma unroll
  for (int i = 0; i < N16; ++i) canon_group_step<METRIC01, SCALE>(ra[i], q4[i * 4], pa, 4, sa);
#pragma unroll
  for (int i = 0; i < N16; ++i) canon_group_step<METRIC01, SCALE>(rb[i], q4[i * 4], pb, 4, sb);
  const float a0 = __shfl(pa, 0, 4), a1 = __shfl(pa, 1, 4), a2 = __shfl(pa, 2, 4), a3 = __shfl(pa, 3, 4);
  const float b0 = __shfl(pb, 0, 4), b1 = __shfl(pb, 1, 4), b2 = __shfl(pb, 2, 4), b3 = __shfl(pb, 3, 4);
  res_a = canon_finish(METRIC01, canon_hsum(a0, a1, a2, a3));
  res_b = canon_finish(METRIC01, canon_hsum(b0, b1, b2, b3));
}

// Four rows of exactly 16 * N16 floats (N16 <= 8: rows of up to 128 dims) by one 4-lane group, all 4 * N16 loads of the lane
// in flight before the first product: 64 rows per pass of a wave (the wide graph walk, k_graphw.hip, evaluates up to 64
// fresh rows per merge — one memory round trip instead of two).  Same arithmetic and order per row as canon_dist_group_t.
template <int METRIC01, int N16, bool SCALE = false>
__device__ __forceinline__ void canon_dist_group_quad(const float* __restrict__ qp, const float* const (&x)[4], int sub,
                                                      float (&res)[4], const float (&sc)[4]) {
  const float4* q4 = (const float4*)qp + sub;
  float4 r[4][N16];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float4* x4 = (const float4*)x[j] + sub;
#pragma unroll
    for (int i = 0; i < N16; ++i) r[j][i] = x4[i * 4];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float p = 0.0f;
#pragma unroll
    for (int i = 0; i < N16; ++i) canon_group_step<METRIC01, SCALE>(r[j][i], q4[i * 4], p, 4, sc[j]);
    const float t0 = __shfl(p, 0, 4), t1 = __shfl(p, 1, 4), t2 = __shfl(p, 2, 4), t3 = __shfl(p, 3, 4);
    res[j] = canon_finish(METRIC01, canon_hsum(t0, t1, t2, t3));
  }
}

// Two STORED rows by one lane, both read from the SEARCH COPY (k_misc.hip: cosine rows already normalised — the product
// hnswlib stores — and every 16-float block permuted so that piece j holds the four inputs of SSE partial sum j in order).
// Piece j of a block therefore feeds partial sum j with its four products one after the other: the same additions in the
// same order as walking the raw rows 16 bytes at a time, and the graph insertion needs neither the raw rows nor their norms
// (fp16 row storage: the search copy is made from the rounded rows).
// sa / sb: per-row scales applied to the elements on the fly (single-copy graph spaces, cosine: the rows are stored
// raw; x * inv_norm is the normalised row hnswlib-python stores, one rounding per element).  1.0f: the rows as stored
// (a multiplication by one is exact).
__device__ __forceinline__ float row_row_dist(int metric01, const float* __restrict__ xa, const float* __restrict__ xb,
                                              uint32_t dims, float sa = 1.0f, float sb = 1.0f) {
  const uint32_t body = canon_body(dims);
  float p[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  auto step = [&](float4 a, float4 b, float& acc, int ncomp) {
    a = scale_s4(a, sa);
    b = scale_s4(b, sb);
    if (metric01 == 0) EHX_CANON_PIECE(0, a, b, acc, ncomp)
    else EHX_CANON_PIECE(1, a, b, acc, ncomp)
  };
  const float4* a4 = (const float4*)xa;
  const float4* b4 = (const float4*)xb;
  const uint32_t n16 = body / 16u;
  // two blocks (sixteen 16-byte pieces of both rows) requested before the first is used: a one-piece-per-trip
  // loop keeps ONE load in flight and pays the cache latency dims/4 times
  uint32_t t = 0;
  for (; t + 2 <= n16; t += 2) {
    float4 ra[8], rb[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      ra[i] = a4[t * 4 + i];
      rb[i] = b4[t * 4 + i];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) step(ra[i], rb[i], p[i & 3], 4);
  }
  for (; t < n16; ++t) {
#pragma unroll
    for (int j = 0; j < 4; ++j) step(a4[t * 4 + j], b4[t * 4 + j], p[j], 4);
  }
  const int rem4 = (int)((body & 15u) >> 2);  // 4-float pieces of a last, partial block: components 0..rem4-1
  if (rem4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) step(a4[n16 * 4 + j], b4[n16 * 4 + j], p[j], rem4);
  }
  float res = canon_hsum(p[0], p[1], p[2], p[3]);
  // (the tail loads xa's element before xb's and tests the metric per element, as this walker always did)
  EHX_CANON_FINISH(metric01, res, body, dims,
                   EHX_CANON_RUN(metric01, true, tail, xa, sa, true, xb, sb, true, false, body, dims, 1))
}

// Canonical distances of the search-copy rows ids_l[0..count) (LDS) to the permuted query qs (LDS), by one wave:
// lane p (< count) returns the distance of row p, other lanes +inf.  16 rows per pass, one 4-lane group per row
// (canon_dist_group_t); rows of 32 / 64 / 96 / 128 / 192 / 256 dims go 32 per pass, two per group, with the loads
// of both rows in flight together (canon_dist_group_pair) — at 128 dims and 27 fresh neighbours per expansion that is
// one memory round trip per expansion instead of two (6.25 M x 128-class workloads: -20 % kernel time).
// xscale (optional): per-row scale applied to the row's elements on the fly (single-copy graph spaces, cosine:
// inv_norm) — nullptr: the rows are used as stored.
// QUAD (the wide graph walk): more than 32 rows of 32 / 64 / 96 / 128 dims go 64 per pass, four per group.
template <int METRIC01, bool SCALE, bool QUAD = false>
__device__ __forceinline__ float wave_group_dists_t(const float* __restrict__ qs, const float* __restrict__ Xs, uint32_t ld,
                                                    uint32_t dims, const uint32_t* ids_l, uint32_t count, int lane,
                                                    const float* __restrict__ xscale) {
  float mine = __builtin_inff();
  const bool pairable = dims <= 256 && (dims == 32 || dims == 64 || dims == 96 || dims == 128 || dims == 192 || dims == 256);
  if (QUAD && pairable && dims <= 128 && count > 32) {   // (count <= 64: one pass)
    const uint32_t r0 = (uint32_t)lane >> 2;
    const float* x[4];
    float sc[4], res[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t rj = r0 + 16u * (uint32_t)j;
      const uint32_t id = ids_l[rj < count ? rj : r0];   // a missing row: the group's first one again, result dropped
      sc[j] = SCALE ? __hip_atomic_load(xscale + id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT) : 1.0f;
      x[j] = Xs + (size_t)id * ld;
    }
    const int sub = lane & 3;
    switch (dims) {
      case 32: canon_dist_group_quad<METRIC01, 2, SCALE>(qs, x, sub, res, sc); break;
      case 64: canon_dist_group_quad<METRIC01, 4, SCALE>(qs, x, sub, res, sc); break;
      case 96: canon_dist_group_quad<METRIC01, 6, SCALE>(qs, x, sub, res, sc); break;
      default: canon_dist_group_quad<METRIC01, 8, SCALE>(qs, x, sub, res, sc); break;
    }
    const int src = (lane & 15) << 2;
    const float g0 = __shfl(res[0], src, 64), g1 = __shfl(res[1], src, 64), g2 = __shfl(res[2], src, 64),
                g3 = __shfl(res[3], src, 64);
    if ((uint32_t)lane < count) mine = (lane & 32) ? ((lane & 16) ? g3 : g2) : ((lane & 16) ? g1 : g0);
    return mine;
  }
  if (pairable && count > 16) {
    for (uint32_t base = 0; base < count; base += 32) {
      const uint32_t ra = base + ((uint32_t)lane >> 2), rb = ra + 16;
      float res_a = __builtin_inff(), res_b = __builtin_inff();
      if (ra < count) {
        const bool have_b = rb < count;  // a missing second row: the first one again, result dropped
        const uint32_t ia = ids_l[ra], ib = ids_l[have_b ? rb : ra];
        const float sa = SCALE ? __hip_atomic_load(xscale + ia, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT) : 1.0f;
        const float sb = SCALE ? __hip_atomic_load(xscale + ib, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT) : 1.0f;
        const float* xa = Xs + (size_t)ia * ld;
        const float* xb = Xs + (size_t)ib * ld;
        const int sub = lane & 3;
        switch (dims) {
          case 32: canon_dist_group_pair<METRIC01, 2, SCALE>(qs, xa, xb, sub, res_a, res_b, sa, sb); break;
          case 64: canon_dist_group_pair<METRIC01, 4, SCALE>(qs, xa, xb, sub, res_a, res_b, sa, sb); break;
          case 96: canon_dist_group_pair<METRIC01, 6, SCALE>(qs, xa, xb, sub, res_a, res_b, sa, sb); break;
          case 128: canon_dist_group_pair<METRIC01, 8, SCALE>(qs, xa, xb, sub, res_a, res_b, sa, sb); break;
          case 192: canon_dist_group_pair<METRIC01, 12, SCALE>(qs, xa, xb, sub, res_a, res_b, sa, sb); break;
          default: canon_dist_group_pair<METRIC01, 16, SCALE>(qs, xa, xb, sub, res_a, res_b, sa, sb); break;
        }
        if (!have_b) res_b = __builtin_inff();
      }
      const float got_a = __shfl(res_a, (lane & 15) << 2, 64), got_b = __shfl(res_b, (lane & 15) << 2, 64);
      if (((uint32_t)lane & ~31u) == base && (uint32_t)lane < count) mine = (lane & 16) ? got_b : got_a;
    }
    return mine;
  }
  for (uint32_t base = 0; base < count; base += 16) {
    const uint32_t r = base + ((uint32_t)lane >> 2);
    float res = __builtin_inff();
    if (r < count) {
      const uint32_t id = ids_l[r];
      // (the scale is requested FIRST, as an ordered load: it is the oldest entry of the load queue when the first
      // product needs it — sunk below the row's ring loads it would be the youngest, and waiting for it would drain
      // the ring)
      const float xsc = SCALE ? __hip_atomic_load(xscale + id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT) : 1.0f;
      res = canon_dist_group_t<METRIC01, SCALE>(qs, Xs + (size_t)id * ld, lane & 3, dims, xsc);
    }
    const float got = __shfl(res, (lane & 15) << 2, 64);
    if (((uint32_t)lane & ~15u) == base && (uint32_t)lane < count) mine = got;
  }
  return mine;
}
template <int METRIC01, bool QUAD = false>
__device__ __forceinline__ float wave_group_dists(const float* __restrict__ qs, const float* __restrict__ Xs, uint32_t ld,
                                                  uint32_t dims, const uint32_t* ids_l, uint32_t count, int lane,
                                                  const float* __restrict__ xscale = nullptr) {
  if (METRIC01 == 1 && xscale) return wave_group_dists_t<METRIC01, true, QUAD>(qs, Xs, ld, dims, ids_l, count, lane, xscale);
  return wave_group_dists_t<METRIC01, false, QUAD>(qs, Xs, ld, dims, ids_l, count, lane, nullptr);
}

}  // namespace ehx
