// Boosted kNN (ehx_knn_boosted*, ehx_knn_decay*, ehx_boost.cpp): the first k rows of the prefix in ascending (score, id) order,
//     score(q, i) = fl32( D(q, i) + fl32( w[q] * p[i] ) ),
// D the canonical distance (walk_row), p[i] a number stored beside the row — a caller's float array (kBoostArray) or the
// linear decay (float)min(|col[i] - origin|, span) of a stored column (kBoostColumn) — w[q] >= 0 and finite.  The multiply and
// the add are two roundings (__fmul_rn, __fadd_rn: no FMA); a NaN score is never a neighbour (dist_key).  The falling-radius
// kNN of k_radius.hip, ranking on the score while the int8 scan in front of it, untouched, keeps bounding the DISTANCE.
//   boost_floor_kernel    array form, once per call: p_min, the least non-NaN penalty of the prefix, by an ordered-uint
//                         atomicMin; the last workgroup to finish decodes it and raises the flag (p_min = -Inf, or no finite
//                         penalty at all): the host then answers the call on the exact route.  The column form has p >= 0 and
//                         takes p_min = 0 without looking.
//   boost_rerank_kernel   radius_rerank_kernel's modes and arguments plus the penalties.  The order of work is the design:
//                           1  the pool's row ids into registers, the prepared query into LDS
//                           2  their penalties gathered FIRST — 4 bytes per entry — and b = fl(w p) formed
//                           3  L2 (D >= 0 or NaN): an entry whose b alone exceeds the score radius is dropped, as is, under
//                              every metric, one whose b is NaN; the survivors compacted into the pool's LDS image as (b, id)
//                           4  ONLY THEN rows are walked (walk_row: a lane per fp32 row, a 4-lane group otherwise), the scores
//                              formed, cut at the score radius, filed as (score, id) keys (dist_key), sorted (block_sort_lds)
//                           5  merged by rank with the carried keys, the k-th score the new score radius or, behind the last
//                              pass, the page written: radius_carry_or_emit (ehx_kernels.h), handed the SCORE radii as its radii
//                           6  the distance radius for the next pass's threshold, from the score radius (below)
// Matrix instructions have no place here: every distance is the oracle's non-fused fp32 order (k_canon.h); the matrix cores
// work in the int8 scan in front.
//
// Two radii per query.  R = score_r[q] is the exact k-th score held.  r.radius[q] — the only radius radius_knn and
// range_thr_kernel see — takes the distance radius Dr with
//     (S)   fl(D + bmin) <= R   ==>   D <= Dr,        bmin = fl(w p_min).
// Rounding is monotone and w >= 0, so p[i] >= p_min gives fl(w p[i]) >= bmin and score(q, i) >= fl(D + bmin): by (S) every row
// with score <= R has D <= Dr, and the scan under the threshold range_thr_kernel maps Dr to keeps it.
//   Dr = fl(t + m),   t = fl(R - bmin),   m = max(2^-21 fl(|R| + |t|), 1e-30).
// Proof of (S), all quantities finite (else Dr is not finite: below).  Let s = fl(D + bmin) <= R.  Round-to-nearest puts the
// real sum x = D + bmin at most half the gap above s, and s <= R, so x <= R + h with h half the gap above R: h <= 2^-24 |R|
// for a normal R, 2^-150 otherwise.  With T = R - bmin (real), D = x - bmin <= T + h.  t = fl(T) is within 2^-24 |t| of T (a
// difference in the subnormal range is exact).  So D <= t + 2^-24 (|R| + |t|) + 2^-150 =: t + need.  g = fl(|R| + |t|) >=
// (1 - 2^-24)(|R| + |t|); 2^-21 g is exact once g >= 2^-100 (a power of two times a normal number, no underflow), and below
// that need < 2^-123 < 1e-30.  Either way m >= 7.9 need (need <= 2^-24 (|R| + |t|) + 2^-150, m >= 2^-21 (1 - 2^-24)(|R| + |t|)
// or m = 1e-30).  The last add rounds down by at most 2^-24 |t + m| <= 2^-24 (|t| + m) <= need + 2^-24 m, so
// Dr >= t + m - need - 2^-24 m >= t + need >= D.  In units in the last place: m is 8 ulps of max(|R|, |t|), up to a factor of
// two — Dr lies within 16 ulps of max(|R|, |t|) above t; with no penalties (bmin = 0, t = R) within 16 ulps of the large-k
// route's radius.  A looser Dr costs time, never correctness.
// Dr not finite (R = +Inf: fewer than k scores held; an overflow of R - bmin): the query is marked, ovf = 2 — what
// range_thr_kernel does with such a radius anyway — and the host answers it on the exact route.
//
// Why the answer is exact.  k_radius.hip's argument with "distance" read as "score" for the carried list and the cut:
//   * Every R is the k-th score of k rows of the prefix (the seed's: of the sample; +Inf while it holds fewer than k rows with a
//     score), so R >= the true k-th score >= score(m) for every true member m, and R only falls: a pass's R is the k-th of a
//     list merged from the one before.  By (S) D(m) <= Dr for the Dr made of every such R, so the scan keeps m in its own pass;
//     step 3 drops only rows whose score exceeds R or is NaN, and the cut at R does not drop m either.
//   * Passes cover disjoint tile ranges, a row enters a pool at most once and never meets its own key in the carried list; the
//     sample carries nothing.
//   * m leaves the carried list only when k rows precede it in (score, id) order — then it is no member.  By induction the
//     merged list behind the last pass holds every member, in order; keys are distinct because ids are, so equal scores fall in
//     id order.
//   * A query whose pool overflowed (ovf = 1, sticky: its distance radius becomes NaN) or which is marked (ovf = 2) writes
//     nothing here: the host answers it on the exact route — this kernel over slabs of ALL rows of the prefix, R falling from
//     +Inf, flag == nullptr: every row passes one re-rank, the answer depends on no threshold and no p_min.
#include "ehx_kernels.h"

namespace ehx {

namespace {

constexpr uint32_t kBoostThreads = 256;
constexpr uint32_t kBoostPer = kPoolCap / kBoostThreads;   // pool entries per thread
static_assert(kBoostPer * kBoostThreads == kPoolCap && kBoostPer <= 32, "a thread's keep bits fit a word");

// LDS of the re-rank: pool_rerank_sorted's image (keys | prepared query | counter), then the waves' sums
__host__ __device__ constexpr size_t boost_rerank_lds_bytes(uint32_t ld) { return pool_rerank_lds_bytes(ld) + 16u; }
constexpr uint32_t kBoostMaxLd = (uint32_t)((kMaxLds - boost_rerank_lds_bytes(0)) / sizeof(float)) & ~31u;
static_assert(boost_rerank_lds_bytes(kBoostMaxLd) <= kMaxLds, "the kernel's LDS fits one CU");
static_assert(kBoostMaxLd >= 16384, "rows of every width the int8 scan serves are re-ranked");

// the penalty of row id
template <int FORM>
__device__ __forceinline__ float boost_penalty(const BoostRerankArgs& e, uint32_t id) {
  if constexpr (FORM == kBoostArray) {
    return e.penalty[id];
  } else {
    const uint32_t c = e.col[id];
    const uint32_t d = c > e.origin ? c - e.origin : e.origin - c;   // (unsigned: no wrap)
    return __uint2float_rn(d < e.span ? d : e.span);
  }
}

// Exclusive prefix sum of one count per thread over the workgroup; *total: the sum.  sums: kBoostThreads / 64 words of LDS.
// A barrier inside: what the threads wrote before the call is visible to all of them when it returns.
__device__ __forceinline__ uint32_t boost_offsets(uint32_t mine, uint32_t* sums, uint32_t tid, uint32_t* total) {
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
  for (uint32_t w = 0; w < kBoostThreads / 64u; ++w) {
    const uint32_t s = sums[w];
    before += w < (tid >> 6) ? s : 0u;
    all += s;
  }
  *total = all;
  return before + incl - mine;
}

}  // namespace

// Grid-stride over p[0, n) (file header).  state: kBoostFloorWords words, {~0, 0, 0, 0} on entry.
__global__ __launch_bounds__(256) void boost_floor_kernel(const float* __restrict__ p, uint64_t n, uint32_t* __restrict__ state) {
  uint32_t best = 0xFFFFFFFFu;   // (no non-NaN value orders this high: +Inf is 0xFF800000)
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
    const float v = p[i];
    if (v == v) {
      const uint32_t o = f32_to_ordered(v);
      best = o < best ? o : best;
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const uint32_t other = __shfl_xor(best, d, 64);
    best = other < best ? other : best;
  }
  if ((threadIdx.x & 63u) == 0 && best != 0xFFFFFFFFu) atomicMin(&state[0], best);
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0 && atomicAdd(&state[1], 1u) == gridDim.x - 1u) {
    __threadfence();
    const uint32_t o = atomicMin(&state[0], 0xFFFFFFFFu);   // (an atomic read: every workgroup's minimum has landed)
    const float p_min = o == 0xFFFFFFFFu ? __builtin_inff() : ordered_to_f32(o);
    state[3] = __float_as_uint(p_min);
    state[2] = __builtin_isinf(p_min) ? 1u : 0u;
  }
}

// One workgroup per query (file header); the control flow in front of the re-rank is radius_rerank_kernel's.
template <int LAYOUT, int METRIC, int FORM>
__global__ __launch_bounds__(kBoostThreads) void boost_rerank_kernel(const BoostRerankArgs e) {
  extern __shared__ float4 boost_lds[];
  const RadiusRerankArgs& a = e.r;
  uint64_t* keys = (uint64_t*)boost_lds;   // (the pool image: the survivors' (b, id), then their sorted keys, at its head)
  float* qs = (float*)(keys + kPoolCap);
  uint32_t* kept_s = (uint32_t*)(qs + a.rows.ld);
  uint32_t* sums = (uint32_t*)((unsigned char*)boost_lds + pool_rerank_lds_bytes(a.rows.ld));
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
  const float R = seed ? __builtin_inff() : e.score_r[q];
  const float w = e.weight ? e.weight[e.weight_of ? e.weight_of[q] : q] : 1.0f;
  stage_query_lds<LAYOUT>(qs, a.Q + (size_t)q * a.rows.ld, a.rows.ld, tid, kBoostThreads);
  if (tid == 0) *kept_s = 0;
  // 1, 2: the pool's row ids (coalesced: entry j kBoostThreads + tid), then their penalties — no row is read yet
  const uint64_t* __restrict__ pool = a.pool + (size_t)q * kPoolCap;
  uint32_t id[kBoostPer];
  float b[kBoostPer];
#pragma unroll
  for (uint32_t j = 0; j < kBoostPer; ++j) {
    const uint32_t i = j * kBoostThreads + tid;
    id[j] = i < cnt ? (uint32_t)pool[i] : 0xFFFFFFFFu;
  }
  uint32_t keep = 0, mine = 0;
#pragma unroll
  for (uint32_t j = 0; j < kBoostPer; ++j) {
    // (an id at or beyond the penalties' prefix — the scan's last tile may hold some — is not searched: nothing is read for it)
    const bool is_row = id[j] < e.n_penalty;
    b[j] = is_row ? __fmul_rn(w, boost_penalty<FORM>(e, id[j])) : __builtin_nanf("");
    // 3: fl(D + b) >= b where D >= 0; a NaN b is a NaN score whatever D is
    if (METRIC == 0 ? b[j] <= R : b[j] == b[j]) {
      keep |= 1u << j;
      ++mine;
    }
  }
  uint32_t n_live;
  uint32_t at = boost_offsets(mine, sums, tid, &n_live);
#pragma unroll
  for (uint32_t j = 0; j < kBoostPer; ++j)
    if (keep & (1u << j)) keys[at++] = ((uint64_t)__float_as_uint(b[j]) << 32) | id[j];
  __syncthreads();
  // 4: only the survivors' rows are read.  An entry is read by the lanes that walk it, in front of the walk, and its key
  // written behind it.
  const bool writer = walk_by_lane<LAYOUT, true>() || (tid & 3u) == 0;
  uint32_t kept = 0;
  for (uint32_t i0 = 0; i0 < n_live; i0 += walk_rows<LAYOUT, true>(kBoostThreads)) {
    const uint32_t i = i0 + walk_slot<LAYOUT, true>(tid);
    const uint64_t ent = i < n_live ? keys[i] : kKeyInf;   // (the same in the four lanes of a group)
    const uint32_t row = (uint32_t)ent;
    bool me;
    const float d = walk_row<LAYOUT, METRIC, true>(a.rows, qs, row, i < n_live, tid, &me);
    const float score = __fadd_rn(d, __uint_as_float((uint32_t)(ent >> 32)));
    const bool in = me && score <= R;   // (a NaN score compares false: never a member)
    if (i < n_live && writer) keys[i] = dist_key(score, row, in);
    kept += (uint32_t)__builtin_popcountll(__ballot(in));
  }
  if ((tid & 63u) == 0 && kept) atomicAdd(kept_s, kept);
  pad_and_sort_lds<kBoostThreads>(keys, n_live, tid);   // (at least one barrier: every wave's count has landed)
  const uint32_t total = *kept_s;
  // 5: the merge is the falling-radius re-rank's, on the score radii
  RadiusRerankArgs on_scores = a;
  on_scores.radius = e.score_r;
  radius_carry_or_emit<kBoostThreads>(on_scores, keys, total, n_live, q, tid);
  // 6: the distance radius the next pass is scanned under (file header: (S))
  if (e.flag && a.mode != kRadiusLast && tid == 0) {
    const float Rn = e.score_r[q];   // (this thread wrote it, or left it as it was)
    const float t = __fsub_rn(Rn, __fmul_rn(w, e.floor ? *e.floor : 0.0f));
    const float m = fmaxf(__fmul_rn(__fadd_rn(fabsf(Rn), fabsf(t)), 0x1p-21f), 1e-30f);
    const float Dr = __fadd_rn(t, m);
    a.radius[q] = Dr;
    if (!(Dr == Dr) || __builtin_isinf(Dr)) e.flag[q] = 2u;
  }
}

namespace {

typedef void (*BoostRerankFn)(const BoostRerankArgs);
#define EHX_BOOST_FNS(L) \
  boost_rerank_kernel<L, 0, 0>, boost_rerank_kernel<L, 0, 1>, boost_rerank_kernel<L, 1, 0>, boost_rerank_kernel<L, 1, 1>, \
      boost_rerank_kernel<L, 2, 0>, boost_rerank_kernel<L, 2, 1>
const BoostRerankFn kBoostRerankFns[18] = {   // [(layout * 3 + metric) * 2 + form]
    EHX_BOOST_FNS(kLayoutF32), EHX_BOOST_FNS(kLayoutF16), EHX_BOOST_FNS(kLayoutPerm)};
#undef EHX_BOOST_FNS
DynLdsAttr g_boost_lds;

}  // namespace

uint32_t boost_rerank_max_ld() { return kBoostMaxLd; }

hipError_t launch_boost_floor(const float* p, uint64_t n, uint32_t* state, int n_cus, hipStream_t st) {
  if (!p || !state || n == 0) return hipErrorInvalidValue;
  // (4 workgroups per CU at most; every thread at least one value while there are that many)
  const uint64_t want = (n + 255u) / 256u, most = (uint64_t)(n_cus > 0 ? n_cus : 1) * 4u;
  hipLaunchKernelGGL(boost_floor_kernel, dim3((uint32_t)(want < most ? want : most)), dim3(256), 0, st, p, n, state);
  return hipGetLastError();
}

hipError_t launch_boost_rerank(const BoostRerankArgs& e, hipStream_t st) {
  const RadiusRerankArgs& a = e.r;
  if (a.nq == 0) return hipSuccess;
  if (a.k == 0 || a.k > kLargeKMax || a.mode > kRadiusSeed || !e.score_r || e.score_r == a.radius || (a.rows.ld & 31u) ||
      a.rows.ld > kBoostMaxLd || a.rows.metric < 0 || a.rows.metric > 2 || (e.form != kBoostArray && e.form != kBoostColumn) ||
      (e.n_penalty && !(e.form == kBoostArray ? (const void*)e.penalty : (const void*)e.col)) || e.n_penalty > a.rows.n_rows ||
      a.rows.n_rows > 0xFFFFFFFFull)
    return hipErrorInvalidValue;
  const size_t lds = boost_rerank_lds_bytes(a.rows.ld);
  hipError_t err = g_boost_lds.ensure(kBoostRerankFns, 18, lds);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(kBoostRerankFns[(row_layout(a.rows.x_half, a.rows.x_perm) * 3 + a.rows.metric) * 2 + e.form], dim3(a.nq),
                     dim3(kBoostThreads), lds, st, e);
  return hipGetLastError();
}

}  // namespace ehx
