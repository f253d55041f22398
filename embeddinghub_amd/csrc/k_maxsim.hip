// MaxSim ("late interaction") scoring on the device (ehx_maxsim_select_device, ehx_knn_maxsim*): a query is a bag of up to 32
// vectors, an entity the rows that carry one value of a stored column, and score(e) = sum over the query's vectors of the
// least canonical distance among e's rows — include/ehx.h has the contract, ehx_maxsim.cpp the host side.
//   maxsim_score_kernel   one workgroup of 256 threads per query.  Global traffic: the candidate labels in, log2(L) probes
//                         of the index per label, the candidates' rows (once from HBM per slab, again from cache per further
//                         block of query vectors), min(k, scored) results out.
//   maxsim_labels_kernel  ehx_knn_maxsim*'s glue: the grouped search's row ids -> their labels, laid out as a candidate block.
// LDS (maxsim_lds_bytes): keys [1024] | run starts [1024] | run lengths [1024] | run labels [1024] | a slab's exclusive
// prefix sums [kSlab + 1] and a counter | the slab's table of minima [kSlab][32] | kNT prepared query vectors [kNT][ld].
//   prologue  the candidate labels become 64-bit keys in LDS, are sorted (block_sort_lds, the grouped cap's sort) and
//             deduplicated; every distinct label other than kGroupNone is looked up in the index's ascending labels and, if a
//             row carries it, kept as (start, length, label) of its run in the permutation.
//   slabs     kSlab kept candidates at a time.  Wave 0 prefix-sums the slab's run lengths: the slab is ONE flat list of rows,
//             and flat position r belongs to the candidate whose prefix interval holds it (a binary search over at most kSlab
//             + 1 words of LDS) — an entity of 1 000 rows and sixty of 3 load the lanes evenly.
//   blocks    the query's vectors go through LDS kNT at a time, each laid out as stage_query_lds lays a query out (absent
//             vectors of the last block: zeros, their results dropped).  Plain fp32 rows: a lane takes a flat position, loads
//             the row's 16-byte pieces once and runs them against all kNT staged vectors (canon_dist_lane_multi, k_canon.h:
//             kNT x 4 partial sums in registers, the vectors' pieces as LDS broadcast reads).  Binary16 and block-permuted
//             rows: a 4-lane group per row, vector by vector through walk_row.
//   minima    every result lowers m[candidate][vector] by an LDS atomic minimum on its orderable bits; a NaN is skipped.
//             The minimum does not depend on the order, so the table — and the answer — is deterministic.
//   scores    behind a slab's last block one thread per candidate adds its T minima in vector order, every add rounded on
//             its own, and files (orderable bits of the score, label) as the candidate's key; a NaN score: kKeyInf.
//   epilogue  the keys are sorted (the same sort) and the first k written by emit_page.
// No matrix instructions: an MFMA product sums in its own order, and every distance here is the oracle's byte.
#include "ehx_kernels.h"

namespace ehx {

namespace {

constexpr uint32_t kMaxsimThreads = 256;
constexpr uint32_t kNT = 8;      // query vectors a row is run against per pass over its pieces
constexpr uint32_t kSlab = 64;   // candidates whose rows form one flat list
static_assert(kSlab <= 64, "one wave prefix-sums a slab's run lengths");
static_assert(kMaxsimMaxTokens % kNT == 0, "whole blocks of query vectors");

constexpr uint32_t kOrdInf = 0xFF800000u;   // f32_to_ordered(+Inf)

__host__ __device__ constexpr size_t maxsim_lds_bytes(uint32_t ld) {
  return kMaxsimMaxCand * (sizeof(uint64_t) + 3u * sizeof(uint32_t)) + (kSlab + 4u) * sizeof(uint32_t) +
         (size_t)kSlab * kMaxsimMaxTokens * sizeof(uint32_t) + (size_t)kNT * ld * sizeof(float);
}
constexpr uint32_t kMaxsimMaxLd = (uint32_t)((kMaxLds - maxsim_lds_bytes(0)) / (kNT * sizeof(float))) & ~31u;
static_assert(maxsim_lds_bytes(kMaxsimMaxLd) <= kMaxLds, "the kernel's LDS fits one CU");
static_assert(maxsim_lds_bytes(0) % 16 == 0, "the staged vectors are read 16 bytes at a time");

// number of entries of the ascending global array a[0, n) that are < key
__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t* __restrict__ a, uint32_t n, uint32_t key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

}  // namespace

template <int LAYOUT, int METRIC>
__global__ __launch_bounds__(kMaxsimThreads) void maxsim_score_kernel(const MaxsimArgs a) {
  constexpr bool kMulti = LAYOUT == kLayoutF32;   // the lane multi-walker; else a 4-lane group per row, vector by vector
  constexpr uint32_t kStep = kMulti ? kMaxsimThreads : kMaxsimThreads / 4u;
  constexpr int m01 = METRIC == 0 ? 0 : 1;
  extern __shared__ float4 maxsim_lds[];
  uint64_t* keys = (uint64_t*)maxsim_lds;              // [1024] the sorted labels, then the scored candidates' keys
  uint32_t* run_start = (uint32_t*)(keys + kMaxsimMaxCand);   // [1024]
  uint32_t* run_len = run_start + kMaxsimMaxCand;      // [1024]
  uint32_t* run_label = run_len + kMaxsimMaxCand;      // [1024]
  uint32_t* pre = run_label + kMaxsimMaxCand;          // [kSlab + 1]
  uint32_t* n_keep_s = pre + kSlab + 1u;               // (+ 2 words of padding)
  uint32_t* mins = pre + kSlab + 4u;                   // [kSlab][32] orderable bits
  float* qs = (float*)(mins + kSlab * kMaxsimMaxTokens);   // [kNT][ld]
  const uint32_t tid = threadIdx.x, q = blockIdx.x;
  const uint32_t ld = a.rows.ld, dims = a.rows.dims;
  uint32_t T = a.token_count ? a.token_count[q] : a.n_tokens;
  T = T < a.n_tokens ? T : a.n_tokens;
  uint32_t nc = a.cand_count[q];
  nc = T == 0 ? 0u : (nc < a.n_cand ? nc : a.n_cand);
  // ---- prologue: distinct labels, looked up ----
  for (uint32_t i = tid; i < nc; i += kMaxsimThreads) keys[i] = a.cand[(size_t)q * a.n_cand + i];
  if (tid == 0) *n_keep_s = 0;
  pad_and_sort_lds<kMaxsimThreads>(keys, nc, tid);   // (a barrier in front of the sort and one behind its last step)
  for (uint32_t i = tid; i < nc; i += kMaxsimThreads) {
    const uint32_t label = (uint32_t)keys[i];
    if (label == kGroupNone || (i > 0 && (uint32_t)keys[i - 1] == label)) continue;
    const uint32_t at = lower_bound_u32(a.labels, a.n_labels, label);
    if (at >= a.n_labels || a.labels[at] != label) continue;
    const uint32_t b = a.start[at], e = a.start[at + 1];
    if (e <= b) continue;
    const uint32_t slot = atomicAdd(n_keep_s, 1u);   // (any order: the keys are sorted at the end)
    run_start[slot] = b;
    run_len[slot] = e - b;
    run_label[slot] = label;
  }
  __syncthreads();
  const uint32_t n_keep = *n_keep_s;
  __syncthreads();   // (the keys are rewritten from here on)
  unsigned long long walked = 0;   // (thread 0's)
  for (uint32_t c0 = 0; c0 < n_keep; c0 += kSlab) {
    const uint32_t ns = n_keep - c0 < kSlab ? n_keep - c0 : kSlab;
    if (tid < 64u) {   // wave 0: exclusive prefix sums of the slab's run lengths (their total is below 2^32: distinct labels)
      const uint32_t len = tid < ns ? run_len[c0 + tid] : 0u;
      uint32_t incl = len;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if ((int)tid >= d) incl += up;
      }
      if (tid < kSlab) pre[tid] = incl - len;
      if (tid == 63u) pre[kSlab] = incl;
    }
    for (uint32_t i = tid; i < ns * kMaxsimMaxTokens; i += kMaxsimThreads) mins[i] = kOrdInf;
    __syncthreads();
    const uint32_t total = pre[kSlab];
    if (tid == 0) walked += total;
    for (uint32_t tb = 0; tb < T; tb += kNT) {
      const uint32_t nt = T - tb < kNT ? T - tb : kNT;
      for (uint32_t j = 0; j < kNT; ++j) {
        if (j < nt) {
          stage_query_lds<LAYOUT>(qs + (size_t)j * ld, a.Q + ((size_t)q * a.n_tokens + tb + j) * ld, ld, tid, kMaxsimThreads);
        } else if (kMulti) {   // (the multi-walker runs all kNT: zeros, results dropped)
          for (uint32_t m = tid; m < ld; m += kMaxsimThreads) qs[(size_t)j * ld + m] = 0.0f;
        }
      }
      __syncthreads();
      for (uint32_t r0 = 0; r0 < total; r0 += kStep) {
        const uint32_t r = r0 + (kMulti ? tid : tid >> 2);   // (the same in the four lanes of a group)
        const bool ok = r < total;
        uint32_t c = 0;
        uint64_t id = ~0ull;
        if (ok) {
          // the candidate whose interval [pre[c], pre[c + 1]) holds r: the last c with pre[c] <= r (empty runs are not kept)
          uint32_t lo = 0, hi = ns;
          while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (pre[mid] <= r) lo = mid;
            else hi = mid;
          }
          c = lo;
          id = a.perm[(size_t)run_start[c0 + c] + (r - pre[c])];
        }
        uint32_t* mrow = mins + c * kMaxsimMaxTokens + tb;
        if constexpr (kMulti) {
          if (ok) {
            float d[kNT];
            const float xs = METRIC == 2 ? a.rows.inv_norm[id] : 1.0f;
            canon_dist_lane_multi<m01, METRIC == 2, (int)kNT>(qs, ld, (const float*)a.rows.X + (size_t)id * ld, xs, dims, d);
#pragma unroll
            for (uint32_t j = 0; j < kNT; ++j)
              if (j < nt && d[j] == d[j]) atomicMin(&mrow[j], f32_to_ordered(d[j]));
          }
        } else {
          for (uint32_t j = 0; j < nt; ++j) {
            bool mine;
            const float d = walk_row<LAYOUT, METRIC, false>(a.rows, qs + (size_t)j * ld, id, ok, tid, &mine);
            if (mine && d == d) atomicMin(&mrow[j], f32_to_ordered(d));
          }
        }
      }
      __syncthreads();   // (the block's minima have landed; the next block restages qs)
    }
    // ---- the slab's scores: m_0 + m_1 + ... in vector order ----
    if (tid < ns) {
      const uint32_t* mrow = mins + tid * kMaxsimMaxTokens;
      float score = ordered_to_f32(mrow[0]);
      for (uint32_t t = 1; t < T; ++t) score = ex_add(score, ordered_to_f32(mrow[t]));
      // (score + 0.0f: -0 and +0 are one value, one key)
      keys[c0 + tid] = score == score ? (((uint64_t)f32_to_ordered(ex_add(score, 0.0f)) << 32) | run_label[c0 + tid]) : kKeyInf;
    }
    __syncthreads();
  }
  // ---- epilogue ----
  pad_and_sort_lds<kMaxsimThreads>(keys, n_keep, tid);
  const uint32_t n_valid = lower_bound_lds(keys, n_keep, kKeyInf);   // (NaN scores sort behind every answer)
  emit_page([&](uint32_t i) { return keys[i]; }, n_valid, a.k, a.out_ids + (size_t)q * a.k, a.out_score + (size_t)q * a.k,
            a.out_count + q, 0, tid, kMaxsimThreads);
  if (tid == 0 && a.work) {
    atomicAdd(&a.work[0], (unsigned long long)n_keep);
    atomicAdd(&a.work[1], walked);
  }
}

// one workgroup per query (launch_maxsim_labels)
__global__ __launch_bounds__(256) void maxsim_labels_kernel(const uint64_t* __restrict__ ids, const uint32_t* __restrict__ cnt,
                                                            const uint32_t* __restrict__ col, uint64_t n_rows,
                                                            const uint32_t* __restrict__ base,
                                                            const uint32_t* __restrict__ token_count, uint32_t n_tokens,
                                                            uint32_t fetch_k, uint32_t* __restrict__ cand,
                                                            uint32_t* __restrict__ cand_count) {
  const uint32_t q = blockIdx.x;
  uint32_t T = token_count ? token_count[q] : n_tokens;
  T = T < n_tokens ? T : n_tokens;
  const uint32_t first = base ? base[q] : q * n_tokens;
  for (uint32_t i = threadIdx.x; i < T * fetch_k; i += 256u) {
    const uint32_t v = first + i / fetch_k, j = i % fetch_k;
    uint32_t label = kGroupNone;
    if (cnt && j < cnt[v]) {
      const uint64_t id = ids[(size_t)v * fetch_k + j];
      if (id < n_rows) label = col[id];
    }
    cand[(size_t)q * n_tokens * fetch_k + i] = label;
  }
  if (threadIdx.x == 0) cand_count[q] = T * fetch_k;
}

namespace {

typedef void (*MaxsimFn)(const MaxsimArgs);
#define EHX_MAXSIM_FNS(K) \
  {K<kLayoutF32, 0>, K<kLayoutF32, 1>, K<kLayoutF32, 2>, K<kLayoutF16, 0>, K<kLayoutF16, 1>, K<kLayoutF16, 2>, \
   K<kLayoutPerm, 0>, K<kLayoutPerm, 1>, K<kLayoutPerm, 2>}
const MaxsimFn kMaxsimFns[9] = EHX_MAXSIM_FNS(maxsim_score_kernel);   // [layout * 3 + metric]
#undef EHX_MAXSIM_FNS
DynLdsAttr g_maxsim_lds;

}  // namespace

uint32_t maxsim_max_ld() { return kMaxsimMaxLd; }

hipError_t launch_maxsim_score(const MaxsimArgs& a, hipStream_t st) {
  if (a.nq == 0) return hipSuccess;
  if (a.k == 0 || a.k > kMaxsimMaxCand || a.n_cand > kMaxsimMaxCand || a.n_tokens == 0 || a.n_tokens > kMaxsimMaxTokens ||
      (a.rows.ld & 31u) || a.rows.ld > kMaxsimMaxLd || a.rows.metric < 0 || a.rows.metric > 2 || !a.cand || !a.cand_count ||
      (a.n_labels && (!a.labels || !a.start || !a.perm)))
    return hipErrorInvalidValue;
  const size_t lds = maxsim_lds_bytes(a.rows.ld);
  hipError_t e = g_maxsim_lds.ensure(kMaxsimFns, 9, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kMaxsimFns[row_layout(a.rows.x_half, a.rows.x_perm) * 3 + a.rows.metric], dim3(a.nq), dim3(kMaxsimThreads),
                     lds, st, a);
  return hipGetLastError();
}

hipError_t launch_maxsim_labels(const uint64_t* ids, const uint32_t* cnt, const uint32_t* col, uint64_t n_rows,
                                const uint32_t* base, const uint32_t* token_count, uint32_t nq, uint32_t n_tokens,
                                uint32_t fetch_k, uint32_t* cand, uint32_t* cand_count, hipStream_t st) {
  if (nq == 0) return hipSuccess;
  if (!cand || !cand_count || n_tokens == 0 || fetch_k == 0 || (cnt && (!ids || (!col && n_rows)))) return hipErrorInvalidValue;
  hipLaunchKernelGGL(maxsim_labels_kernel, dim3(nq), dim3(256), 0, st, ids, cnt, col, n_rows, base, token_count, n_tokens,
                     fetch_k, cand, cand_count);
  return hipGetLastError();
}

}  // namespace ehx
