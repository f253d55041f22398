// Predicate filters on stored columns (ehx_where.cpp): the bitmaps of a call's n_preds <= 64 predicates over the prefix of
// n_rows < 2^32 rows, in ONE pass over the columns, written where the bitmap searches' compaction (k_masked.hip) reads a table:
// bitmap p at dst + p * words, words = ceil(n_rows / 32), bit r & 31 of word r >> 5 set iff predicate p allows row r.
//   where_bitmaps_kernel   a workgroup of 256 lanes (4 waves) per span of kWhereSpan = 1024 rows, four 256-row tiles.  In round
//                          j lane t holds row span + 256 j + t: it loads the row's value from every column that SOME predicate
//                          of the call names and that is live — once, 4 bytes per lane, a wave 256 contiguous bytes — and
//                          keeps the four rounds' values in registers (at most 16).  A column nobody names is not read; one
//                          that is not live is the constant 0xFFFFFFFF.  The workgroup copies the call's predicates into LDS
//                          once, so no dependent load from global memory stands in the loop.  The loop over predicates and
//                          terms is wave-uniform (every lane reads the same LDS word, made scalar by readfirstlane); a
//                          term is two unsigned compares per round, the column picked by a SCALAR BRANCH on its number (no
//                          indexed register array, no select chain).  __ballot gives 64 bits of
//                          predicate p per wave and round: two words, which lane 0 puts into LDS at [p][8 j + 2 wave].  Behind
//                          ONE barrier the workgroup stores the 32 words of every predicate's span: consecutive lanes write
//                          consecutive words, so a wave's store instruction writes 128 contiguous bytes of each of two
//                          predicates (never 8-byte pieces strided by `words`).
// Rows at or above n_rows load nothing and fail every predicate — that of no terms included — so the bits at or above n_rows in
// the last word are 0; words at or above `words` are not written.  Every store is an ordinary vector store.
// LDS: 64 predicates x 32 words of bitmap = 8 KB and 64 x 33 words of predicates = 8448 bytes, 16 640 bytes per workgroup,
// whatever n_preds is.  Registers: 16 values, 4 verdicts; no scratch.
// Algorithmic traffic: 4 x (columns named and live) x n_rows bytes in, n_preds x n_rows / 8 bytes out.
#include "ehx_kernels.h"

namespace ehx {

namespace {
constexpr uint32_t kWhereThreads = 256, kWhereRounds = kWhereSpan / kWhereThreads,
                   kWhereSpanWords = kWhereSpan / 32;
static_assert(kWhereRounds == 4 && kWhereSpanWords == 32, "a span is four rounds of 256 rows, 32 words of a bitmap");
static_assert(kWhereMaxCols == 4, "the branch below names four columns");
// a row's values: four named registers — the wave-uniform column number of a term branches to the compares that name its
// register (an indexed array would live in scratch; a chain of selects costs three vector instructions per round and term)
struct WhereVals {
  uint32_t c0, c1, c2, c3;
};
__device__ __forceinline__ uint32_t where_load(const WhereCols& cols, uint32_t c, bool live, uint64_t r) {
  return (live && ((cols.named >> c) & 1u)) ? cols.p[c][r] : 0xFFFFFFFFu;
}
__device__ __forceinline__ WhereVals where_row(const WhereCols& cols, bool live, uint64_t r) {
  return {where_load(cols, 0, live, r), where_load(cols, 1, live, r), where_load(cols, 2, live, r), where_load(cols, 3, live, r)};
}
__device__ __forceinline__ uint32_t where_uniform(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
// lo <= x <= hi, inverted by flag bit 0 (lo > hi: no x lies inside): two vector compares, the rest on the lane masks
__device__ __forceinline__ bool where_holds(uint32_t x, const WhereTerm& tm) {
  return (x >= tm.lo && x <= tm.hi) != ((tm.flags & 1u) != 0u);
}
// one term over the four rounds' values of ONE column
#define EHX_WHERE_TERM(c)                      \
  ok0 = ok0 && where_holds(v0.c, tm);          \
  ok1 = ok1 && where_holds(v1.c, tm);          \
  ok2 = ok2 && where_holds(v2.c, tm);          \
  ok3 = ok3 && where_holds(v3.c, tm)
}

__global__ __launch_bounds__(256) void where_bitmaps_kernel(WhereCols cols, const WherePred* __restrict__ preds, uint32_t n_preds,
                                                            uint64_t n_rows, uint64_t words, uint32_t* __restrict__ dst) {
  __shared__ uint32_t bits[kMaskedMaxMasks * kWhereSpanWords];
  __shared__ uint32_t table[kMaskedMaxMasks * (sizeof(WherePred) / sizeof(uint32_t))];
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const uint64_t span0 = (uint64_t)blockIdx.x * kWhereSpan;
  const uint64_t r0 = span0 + tid, r1 = r0 + kWhereThreads, r2 = r1 + kWhereThreads, r3 = r2 + kWhereThreads;
  const bool live0 = r0 < n_rows, live1 = r1 < n_rows, live2 = r2 < n_rows, live3 = r3 < n_rows;
  const WhereVals v0 = where_row(cols, live0, r0), v1 = where_row(cols, live1, r1), v2 = where_row(cols, live2, r2),
                  v3 = where_row(cols, live3, r3);
  // the call's predicates, once per workgroup, beside the column loads in flight
  constexpr uint32_t kPredWords = sizeof(WherePred) / sizeof(uint32_t);
  for (uint32_t i = tid; i < n_preds * kPredWords; i += kWhereThreads) table[i] = reinterpret_cast<const uint32_t*>(preds)[i];
  __syncthreads();
  for (uint32_t p = 0; p < n_preds; ++p) {
    bool ok0 = live0, ok1 = live1, ok2 = live2, ok3 = live3;
    const uint32_t* pw = table + p * kPredWords;
    const uint32_t n_terms = where_uniform(pw[0]);
    for (uint32_t t = 0; t < n_terms; ++t) {
      const uint32_t* tw = pw + 1u + 4u * t;   // (every lane reads the same words: a broadcast, made scalar again)
      const WhereTerm tm = {where_uniform(tw[0]), where_uniform(tw[1]), where_uniform(tw[2]), where_uniform(tw[3])};
      // (the column number is wave-uniform: a scalar branch to the copy of the compares that names its registers)
      switch (tm.col) {
        case 0u: EHX_WHERE_TERM(c0); break;
        case 1u: EHX_WHERE_TERM(c1); break;
        case 2u: EHX_WHERE_TERM(c2); break;
        default: EHX_WHERE_TERM(c3); break;
      }
    }
    const unsigned long long b0 = __ballot(ok0), b1 = __ballot(ok1), b2 = __ballot(ok2), b3 = __ballot(ok3);
    if (lane == 0u) {   // round j's 64 bits of wave w: words 8 j + 2 w and the next of the span
      uint32_t* o = bits + p * kWhereSpanWords + 2u * wave;
      o[0] = (uint32_t)b0, o[1] = (uint32_t)(b0 >> 32);
      o[8] = (uint32_t)b1, o[9] = (uint32_t)(b1 >> 32);
      o[16] = (uint32_t)b2, o[17] = (uint32_t)(b2 >> 32);
      o[24] = (uint32_t)b3, o[25] = (uint32_t)(b3 >> 32);
    }
  }
  __syncthreads();
  const uint64_t word0 = span0 / 32u;
  for (uint32_t i = tid; i < n_preds * kWhereSpanWords; i += kWhereThreads) {
    const uint64_t w = word0 + (i & (kWhereSpanWords - 1u));
    if (w < words) dst[(uint64_t)(i / kWhereSpanWords) * words + w] = bits[i];
  }
}

hipError_t launch_where_bitmaps(const WhereCols& cols, const WherePred* preds, uint32_t n_preds, uint64_t n_rows, uint64_t words,
                                uint32_t* dst, hipStream_t st) {
  if (n_rows == 0 || n_preds == 0) return hipSuccess;
  if (n_rows > 0xFFFFFFFFull || n_preds > kMaskedMaxMasks || words != (n_rows + 31) / 32) return hipErrorInvalidValue;
  hipLaunchKernelGGL(where_bitmaps_kernel, dim3((uint32_t)((n_rows + kWhereSpan - 1) / kWhereSpan)), dim3(kWhereThreads), 0, st, cols,
                     preds, n_preds, n_rows, words, dst);
  return hipGetLastError();
}

}  // namespace ehx
