// Boolean filters on stored columns (ehx_filter.cpp): the bitmaps of a call's n_filters <= 64 filters — each an OR of clauses,
// a clause an AND of at most 8 terms, a term an unsigned range or a set-membership test — over the prefix of n_rows < 2^32
// rows, in ONE pass over the columns, written where the bitmap searches' compaction (k_masked.hip) reads a table: bitmap f at
// dst + f * words, words = ceil(n_rows / 32), bit r & 31 of word r >> 5 set iff filter f allows row r.
//   filter_bitmaps_kernel  k_where.hip's frame: a workgroup of 256 lanes (4 waves) per span of kWhereSpan = 1024 rows, four
//                          256-row tiles; in round j lane t holds row span + 256 j + t and loads its value from every column
//                          SOME clause names and that is live, once, and keeps the four rounds' values in 16 named registers.
//                          A column nobody names is not read; one that is not live is the constant 0xFFFFFFFF.  The workgroup
//                          copies the call's expression into LDS once: the clauses (ehx_pred's 33 words each), the packed
//                          sets of the IN terms, the filters' runs.  The loop over clauses and terms is wave-uniform
//                          (readfirstlane makes the LDS words scalars); a term's column is picked by a SCALAR BRANCH on its
//                          number.
//                          EVERY CLAUSE IS EVALUATED ONCE, however many filters share it: __ballot gives 64 bits of clause c
//                          per wave and round, which lane 0 puts into LDS at cw[c][8 j + 2 wave].  Behind ONE barrier the
//                          filters' words are ORed from the clause words, lane-parallel over (filter, word): lane i of a
//                          pass holds word i & 31 of filter i >> 5, reads its run's clause words and stores the OR — a
//                          wave's store instruction writes 128 contiguous bytes of each of two filters.  A filter of no
//                          clause ORs nothing and still WRITES its zero words: the compaction reads the whole table.
//   IN terms               the term's set lies sorted and de-duplicated in LDS at vals[lo, lo + hi) (ehx_filter.cpp packs it).
//                          Each lane runs an UNSIGNED branchless binary search for its value: ceil(log2(len)) steps whose
//                          count is wave-uniform, one divergent LDS read per step and round, then one equality compare.
//                          A set of length 0 reads nothing (a scalar branch): the term is false, true under NOT.
// Rows at or above n_rows load nothing and fail every clause — one of no terms, a NOT IN and a negated empty range included
// — so they fail every filter: the bits at or above n_rows in the last word are 0; words at or above `words` are not written.
// Every store is an ordinary vector store from plain C++.
// LDS: 128 clauses x 33 words = 16 896 bytes, 4096 values = 16 384 bytes, 64 runs x 2 words = 512 bytes (one array, packed
// in that order as the host packs it), and 128 x 32 clause words = 16 384 bytes: 50 176 bytes per workgroup, whatever the
// call holds — three workgroups on a CU's 160 KB.  Registers: 16 values, 4 verdicts, 4 search cursors; no scratch, no spill.
// Algorithmic traffic: 4 x (columns named and live) x n_rows bytes in, n_filters x n_rows / 8 bytes out.
#include "ehx_kernels.h"

namespace ehx {

namespace {
constexpr uint32_t kFilterThreads = 256, kFilterSpanWords = kWhereSpan / 32;
constexpr uint32_t kClauseWords = sizeof(WherePred) / sizeof(uint32_t);
static_assert(kWhereSpan / kFilterThreads == 4 && kFilterSpanWords == 32, "a span is four rounds of 256 rows, 32 words of a bitmap");
static_assert(kWhereMaxCols == 4, "the branch below names four columns");
static_assert(kClauseWords == 33, "a clause is n_terms and eight terms of four words");
static_assert((kFilterExprWords + kFilterMaxClauses * kFilterSpanWords) * sizeof(uint32_t) == 50176, "the LDS the header states");
struct FilterVals {
  uint32_t c0, c1, c2, c3;
};
__device__ __forceinline__ uint32_t filter_load(const WhereCols& cols, uint32_t c, bool live, uint64_t r) {
  return (live && ((cols.named >> c) & 1u)) ? cols.p[c][r] : 0xFFFFFFFFu;
}
__device__ __forceinline__ FilterVals filter_row(const WhereCols& cols, bool live, uint64_t r) {
  return {filter_load(cols, 0, live, r), filter_load(cols, 1, live, r), filter_load(cols, 2, live, r), filter_load(cols, 3, live, r)};
}
__device__ __forceinline__ uint32_t filter_uniform(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
// one term over the four rounds' values x0..x3 of ONE column: tm.lo / tm.hi are a range's ends, or — kFilterTermIn — where
// the term's sorted set starts in `vals` and how many values it holds
__device__ __forceinline__ void filter_term(const WhereTerm& tm, const uint32_t* vals, uint32_t x0, uint32_t x1, uint32_t x2,
                                            uint32_t x3, bool& ok0, bool& ok1, bool& ok2, bool& ok3) {
  const bool neg = (tm.flags & 1u) != 0u;
  bool h0, h1, h2, h3;
  if (tm.flags & kFilterTermIn) {   // (wave-uniform)
    h0 = h1 = h2 = h3 = false;
    if (tm.hi) {   // (wave-uniform; an empty set reads nothing)
      const uint32_t* set = vals + tm.lo;
      // the last position whose value is <= x, if set[0] <= x: the answer stays in [b, b + n)
      uint32_t b0 = 0, b1 = 0, b2 = 0, b3 = 0;
      for (uint32_t n = tm.hi; n > 1u;) {
        const uint32_t half = n >> 1;
        b0 += set[b0 + half] <= x0 ? half : 0u;
        b1 += set[b1 + half] <= x1 ? half : 0u;
        b2 += set[b2 + half] <= x2 ? half : 0u;
        b3 += set[b3 + half] <= x3 ? half : 0u;
        n -= half;
      }
      h0 = set[b0] == x0, h1 = set[b1] == x1, h2 = set[b2] == x2, h3 = set[b3] == x3;
    }
  } else {   // lo <= x <= hi (lo > hi: no x lies inside)
    h0 = x0 >= tm.lo && x0 <= tm.hi, h1 = x1 >= tm.lo && x1 <= tm.hi;
    h2 = x2 >= tm.lo && x2 <= tm.hi, h3 = x3 >= tm.lo && x3 <= tm.hi;
  }
  ok0 = ok0 && (h0 != neg), ok1 = ok1 && (h1 != neg), ok2 = ok2 && (h2 != neg), ok3 = ok3 && (h3 != neg);
}
#define EHX_FILTER_TERM(c) filter_term(tm, vals, v0.c, v1.c, v2.c, v3.c, ok0, ok1, ok2, ok3)
}

// expr: the call's expression in DEVICE memory, packed — n_clauses x 33 words of clauses | n_values values | n_filters x
// (first clause, number of clauses) — and checked on the host: every run inside the clauses, every set inside the values
__global__ __launch_bounds__(256) void filter_bitmaps_kernel(WhereCols cols, const uint32_t* __restrict__ expr, uint32_t n_clauses,
                                                             uint32_t n_values, uint32_t n_filters, uint64_t n_rows,
                                                             uint64_t words, uint32_t* __restrict__ dst) {
  __shared__ uint32_t ex[kFilterExprWords];
  __shared__ uint32_t cw[kFilterMaxClauses * kFilterSpanWords];
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const uint64_t span0 = (uint64_t)blockIdx.x * kWhereSpan;
  const uint64_t r0 = span0 + tid, r1 = r0 + kFilterThreads, r2 = r1 + kFilterThreads, r3 = r2 + kFilterThreads;
  const bool live0 = r0 < n_rows, live1 = r1 < n_rows, live2 = r2 < n_rows, live3 = r3 < n_rows;
  const FilterVals v0 = filter_row(cols, live0, r0), v1 = filter_row(cols, live1, r1), v2 = filter_row(cols, live2, r2),
                   v3 = filter_row(cols, live3, r3);
  // the call's expression, once per workgroup, beside the column loads in flight
  const uint32_t n_expr = n_clauses * kClauseWords + n_values + 2u * n_filters;
  for (uint32_t i = tid; i < n_expr; i += kFilterThreads) ex[i] = expr[i];
  __syncthreads();
  const uint32_t* vals = ex + n_clauses * kClauseWords;
  const uint32_t* runs = vals + n_values;
  for (uint32_t c = 0; c < n_clauses; ++c) {
    bool ok0 = live0, ok1 = live1, ok2 = live2, ok3 = live3;
    const uint32_t* pw = ex + c * kClauseWords;
    const uint32_t n_terms = filter_uniform(pw[0]);
    for (uint32_t t = 0; t < n_terms; ++t) {
      const uint32_t* tw = pw + 1u + 4u * t;   // (every lane reads the same words: a broadcast, made scalar again)
      const WhereTerm tm = {filter_uniform(tw[0]), filter_uniform(tw[1]), filter_uniform(tw[2]), filter_uniform(tw[3])};
      // (the column number is wave-uniform: a scalar branch to the copy of the term that names its registers)
      switch (tm.col) {
        case 0u: EHX_FILTER_TERM(c0); break;
        case 1u: EHX_FILTER_TERM(c1); break;
        case 2u: EHX_FILTER_TERM(c2); break;
        default: EHX_FILTER_TERM(c3); break;
      }
    }
    const unsigned long long b0 = __ballot(ok0), b1 = __ballot(ok1), b2 = __ballot(ok2), b3 = __ballot(ok3);
    if (lane == 0u) {   // round j's 64 bits of wave w: words 8 j + 2 w and the next of the span
      uint32_t* o = cw + c * kFilterSpanWords + 2u * wave;
      o[0] = (uint32_t)b0, o[1] = (uint32_t)(b0 >> 32);
      o[8] = (uint32_t)b1, o[9] = (uint32_t)(b1 >> 32);
      o[16] = (uint32_t)b2, o[17] = (uint32_t)(b2 >> 32);
      o[24] = (uint32_t)b3, o[25] = (uint32_t)(b3 >> 32);
    }
  }
  __syncthreads();
  // the filters' words: the OR of their runs' clause words (none: zero), every word below `words` written
  const uint64_t word0 = span0 / 32u;
  for (uint32_t i = tid; i < n_filters * kFilterSpanWords; i += kFilterThreads) {
    const uint32_t f = i / kFilterSpanWords, sw = i & (kFilterSpanWords - 1u);
    const uint32_t first = runs[2u * f], n = runs[2u * f + 1u];
    uint32_t acc = 0u;
    for (uint32_t c = 0; c < n; ++c) acc |= cw[(first + c) * kFilterSpanWords + sw];
    const uint64_t w = word0 + sw;
    if (w < words) dst[(uint64_t)f * words + w] = acc;
  }
}

hipError_t launch_filter_bitmaps(const WhereCols& cols, const uint32_t* expr, uint32_t n_clauses, uint32_t n_values,
                                 uint32_t n_filters, uint64_t n_rows, uint64_t words, uint32_t* dst, hipStream_t st) {
  if (n_rows == 0 || n_filters == 0) return hipSuccess;
  if (n_rows > 0xFFFFFFFFull || n_filters > kMaskedMaxMasks || n_clauses > kFilterMaxClauses || n_values > kFilterMaxValues ||
      words != (n_rows + 31) / 32)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(filter_bitmaps_kernel, dim3((uint32_t)((n_rows + kWhereSpan - 1) / kWhereSpan)), dim3(kFilterThreads), 0, st, cols,
                     expr, n_clauses, n_values, n_filters, n_rows, words, dst);
  return hipGetLastError();
}

}  // namespace ehx
