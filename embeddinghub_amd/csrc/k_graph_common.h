// The pieces the graph walks share (k_graph.hip: the strict, hnswlib-order-identical walk; k_graphw.hip: the wide
// walk, several expansions per step; k_graphm.hip: the strict walk under a row bitmap) — one copy of each:
//   GraphLds            the LDS layout: carve() in the kernels, bytes() for the launchers
//   load_query          one-query form's preparation of the raw query, query row -> LDS in search-copy order
//   greedy_descent      entry point + upper levels maxlevel..1, with the NaN rule
//   rank_by_counting    rank of a lane's key among the keys of batch[] (strict walk; the wide walk keeps the same loop
//                       in place — k_graphw.hip, merge_keys, says why)
//   merge_sorted_into_R in-place, top-down merge of <= 64 ranked keys into the result list R
//   finish_query        visited bitmap back to all-zero, the k results, counters, done_flag
// The level-0 loops — where the walks differ — stay in their own files.
#pragma once
#include "ehx_env.h"
#include "ehx_kernels.h"
#include "k_prep_query.h"

namespace ehx {
namespace {

constexpr uint32_t kOrdNaN = 0xFFFFFFFFu;  // ordered key above +inf: a NaN entry point seeding level 0, never returned

// Both walks run their R bookkeeping on ONE wave: the LDS accesses of a wave execute in order, so wave_lds_sync() (a
// compiler-level fence) orders write -> read across lanes, and wave-uniform values that come out of a shuffle or LDS
// go through wave_uniform() (readfirstlane) so that the loop bookkeeping runs on the scalar unit.  Both were A/B
// switches once (a real barrier, a shuffle from lane 0); the switches are gone, these are the forms that shipped.

// -DEHX_GRAPH_PROFILE (ablation builds, scripts/gpu_graph_profile.sh): per-phase wall-clock ticks (100 MHz) of the
// level-0 loop, summed over all query waves into the counters behind the four work counters (finish_query).  Strict
// walk, [4..11]: pick next node | adjacency + visited | row fetch + distances | rank fresh keys | decide next + request |
// insertion points | move R | tail.  Wide walk, [5..11]: k_graphw.hip.
struct GraphProf {
#ifdef EHX_GRAPH_PROFILE
  unsigned long long t[8] = {0, 0, 0, 0, 0, 0, 0, 0}, last = wall_clock64();
  __device__ __forceinline__ void mark(int i) {
    const unsigned long long now = wall_clock64();
    t[i] += now - last;
    last = now;
  }
#else
  __device__ __forceinline__ void mark(int) {}
#endif
};

// work counters of one query as SURVEY §8d (n_steps: the wide walk's steps)
struct WalkCounters {
  unsigned long long n_dist = 0, n_hops0 = 0, n_hops_up = 0, n_pf_hit = 0, n_steps = 0;
};

// LDS of one query: qs[ld] f32 (the query, search-copy order) | R[ef_cap] u64 (the result list) | S[64] u64 (sorted
// fresh keys) | batch[64] u64 | ids[n_ids] u32 (64; the wide walk holds 32 per expansion of a step) | F[ef_cap] u8,
// padded to 16 (slots of R a fresh key lands on, during a merge) | the wide walk's helper wave: hd[32] f32 (its
// distances), ctrl[2] u32 in 16 bytes ((count, first slot) of the pass; ~0: done) | 64 bytes of slack.
// carve() and bytes() walk the same fields in the same order.
struct GraphLds {
  float* qs;
  uint64_t *R, *S, *batch;
  uint32_t* ids;
  uint8_t* F;
  float* hd;
  volatile uint32_t* ctrl;

  __device__ __forceinline__ void carve(char* smem, uint32_t ld, uint32_t ef_cap, uint32_t n_ids) {
    qs = (float*)smem;
    R = (uint64_t*)(qs + ld);
    S = R + ef_cap;
    batch = S + 64;
    ids = (uint32_t*)(batch + 64);
    F = (uint8_t*)(ids + n_ids);
    hd = (float*)(F + (((size_t)ef_cap + 15) & ~(size_t)15));
    ctrl = (volatile uint32_t*)(hd + 32);
  }
  static constexpr size_t bytes(uint32_t ld, uint32_t ef_cap, uint32_t n_ids) {
    size_t b = (size_t)ld * sizeof(float);                 // qs
    b += (size_t)ef_cap * sizeof(uint64_t);                // R
    b += 64 * sizeof(uint64_t);                            // S
    b += 64 * sizeof(uint64_t);                            // batch
    b += (size_t)n_ids * sizeof(uint32_t);                 // ids
    b += ((size_t)ef_cap + 15) & ~(size_t)15;              // F
    b += 32 * sizeof(float);                               // hd
    b += 16;                                               // ctrl
    return b + 64;
  }
};
constexpr uint32_t graph_n_ids(uint32_t width) { return width > 2 ? 32 * width : 64; }

// Prefetch-style load: a relaxed atomic load (wavefront scope: no cache-policy bits) is an ordered memory
// reference for the compiler, so it is issued where it is written — a plain load whose first use comes an
// LDS-heavy phase later is a candidate for the compiler's code sinking, which would expose the HBM round
// trip the early issue is meant to overlap.
__device__ __forceinline__ uint32_t load_here(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// value of a 64-bit register in lane l (wave-uniform l)
__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
  return ((uint64_t)hi << 32) | lo;
}

// The query row into LDS, in search-copy order, by the NWAVES waves of the workgroup (wave wv, lane lane).  One query per
// call in one launch (a.q_raw): the raw query comes from host-visible memory and is prepared here, by wave 0, into the
// device scratch row the loads below read (the same arithmetic as prep_queries_kernel: identical bytes).
template <int NWAVES>
__device__ __forceinline__ void load_query(const GraphArgs& a, float* qs, uint32_t qi, int wv, int lane) {
  if ((NWAVES == 1 || wv == 0) && a.q_raw) {
    prep_query_row(a.q_raw, 1u, a.dims, a.ld, a.metric, const_cast<float*>(a.Q), 0u, lane);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  }
  if (NWAVES > 1) __syncthreads();   // (the prepared query row is wave 0's work)
  for (uint32_t i = NWAVES == 1 ? (uint32_t)lane : threadIdx.x; i < a.ld; i += 64 * NWAVES)
    qs[search_copy_pos(i)] = a.Q[(size_t)qi * a.ld + i];
  if (NWAVES > 1) __syncthreads();
  else wave_lds_sync();
}

// Entry point and upper levels maxlevel..1: greedy descent — scan the current node's list in stored order and move to
// the FIRST strictly-closest neighbour, repeat until no improvement.  A NaN distance is no neighbour: the
// descent treats it as +inf (never strictly smaller), and a NaN entry point the descent could not leave (nan_seed) seeds
// level 0 with the largest key, where it is expanded once and never returned.  Adds to c.n_dist and c.n_hops_up.
struct Descent {
  uint32_t cur;    // where level 0 starts (wave-uniform, as the rest)
  float curdist;
  bool nan_seed;
};
template <int METRIC01>
__device__ __forceinline__ Descent greedy_descent(const GraphArgs& a, const GraphLds& L, int lane, WalkCounters& c) {
  uint32_t cur = a.entry_point;
  if (lane == 0) L.ids[0] = cur;
  wave_lds_sync();
  float curdist = wave_uniform(wave_group_dists<METRIC01>(L.qs, a.Xs, a.ld, a.dims, L.ids, 1, lane, a.xscale));
  c.n_dist += 1;
  bool nan_seed = curdist != curdist;
  if (nan_seed) curdist = __builtin_inff();
  for (int level = a.max_level; level >= 1; --level) {
    bool changed = true;
    while (changed) {
      changed = false;
      const uint32_t us = a.up_start[cur];
      const uint32_t* lst = a.up_lists + ((size_t)us + (uint32_t)(level - 1)) * a.M;
      uint32_t nb = kNoNode;
      if (lane < (int)a.M) nb = lst[lane];
      const uint32_t cnt = __builtin_popcountll(__ballot(nb != kNoNode));  // lists are packed from slot 0
      c.n_hops_up += 1;
      if (lane < (int)cnt) L.ids[lane] = nb;
      wave_lds_sync();
      c.n_dist += cnt;
      float m = wave_group_dists<METRIC01>(L.qs, a.Xs, a.ld, a.dims, L.ids, cnt, lane, a.xscale);
      if (m != m) m = __builtin_inff();
      uint32_t mi = (uint32_t)lane;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {  // first strictly-smaller minimum in stored order
        const float od = __shfl_xor(m, o, 64);
        const uint32_t oi = __shfl_xor(mi, o, 64);
        if (od < m || (od == m && oi < mi)) {
          m = od;
          mi = oi;
        }
      }
      m = wave_uniform(m);  // (the butterfly leaves the minimum in every lane)
      mi = wave_uniform(mi);
      if (m < curdist) {
        curdist = m;
        cur = wave_uniform(L.ids[mi]);
        changed = true;
        nan_seed = false;
      }
      wave_lds_sync();
    }
  }
  return {cur, curdist, nan_seed};
}

// Rank of mykey among batch[0..n) by counting (keys are distinct: the id is part of the key).  Sixteen keys per trip,
// all LDS reads issued before the first compare (a one-key-per-trip loop pays the LDS latency n times); batch[n..64)
// holds +inf, which never counts.
__device__ __forceinline__ uint32_t rank_by_counting(const uint64_t* batch, uint32_t n, uint64_t mykey) {
  uint32_t rank = 0;
  for (uint32_t j = 0; j < n; j += 16) {
    uint64_t kb[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) kb[u] = batch[j + u];
#pragma unroll
    for (int u = 0; u < 16; ++u) rank += kb[u] < mykey ? 1u : 0u;
  }
  return rank;
}

// Merge of n (<= 64) fresh keys into R: lane p with has holds one of them, mykey, of rank `rank` among them.  They are
// sorted through S, their insertion points found by binary search, and R is updated IN PLACE, driven by the
// DESTINATION: fresh key i lands at fpos = ps_i + i (distinct, ascending); a destination slot no fresh key lands on
// receives the old entry whose index is the slot minus the number of fresh keys landing below it.  F flags the landing
// slots, so per 64 slots that number is one ballot + a lane-prefix popcount — no per-entry search.  Top down: a chunk
// reads only slots at or below its own, which are still untouched.  Only [first insertion point, nR) is touched.
// PROF_POINTS / PROF_MOVED: the caller's profile slots for "insertion points found" and "R moved".
template <int PROF_POINTS, int PROF_MOVED>
__device__ __forceinline__ void merge_sorted_into_R(const GraphLds& L, uint32_t ef, uint64_t mykey, bool has, uint32_t rank,
                                                    uint32_t n, uint32_t& nR, uint32_t& scan_from, int lane,
                                                    GraphProf& prof) {
  uint64_t* R = L.R;
  if (has) L.S[rank] = mykey;
  wave_lds_sync();
  uint64_t skey = kKeyInf;
  uint32_t ps = kNoNode;
  if ((uint32_t)lane < n) {
    skey = L.S[lane];  // the lane-th smallest fresh key
    ps = lower_bound_lds(R, nR, skey);
  }
  // insertion point of the smallest fresh key (lane 0).  readfirstlane, not a shuffle: the value is wave-uniform
  // and everything derived from it (nR, the scan positions, the loop bounds) then lives in scalar registers
  const uint32_t p0 = wave_uniform(ps);
  prof.mark(PROF_POINTS);
  if (p0 < ef) {
    const uint32_t new_nR = nR + n < ef ? nR + n : ef;
    const uint32_t fpos = ps + (uint32_t)lane;
    const bool lands = (uint32_t)lane < n && fpos < ef;
    if (lands) L.F[fpos] = 1;
    wave_lds_sync();
    for (uint32_t dhi = new_nR; dhi > p0;) {
      const uint32_t dlo = dhi - p0 > 64 ? dhi - 64 : p0;
      const uint32_t dpos = dlo + (uint32_t)lane;
      const bool in = dpos < dhi;
      const bool taken = in && L.F[dpos] != 0;
      const uint64_t occ = __ballot(taken);
      const uint32_t below = (uint32_t)__builtin_popcountll(__ballot(lands && fpos < dlo));
      const uint32_t cnt = below + (uint32_t)__builtin_popcountll(occ & ((1ull << lane) - 1ull));
      const bool mv = in && !taken;
      uint64_t kj = 0;
      if (mv) kj = R[dpos - cnt];
      wave_lds_sync();
      if (mv) R[dpos] = kj;
      wave_lds_sync();
      dhi = dlo;
    }
    if (lands) {
      R[fpos] = skey;
      L.F[fpos] = 0;
    }
    wave_lds_sync();
    nR = new_nR;
    if (p0 < scan_from) scan_from = p0;
  }
  prof.mark(PROF_MOVED);
}

// End of a query, by its walking wave.  Leaves the visited bitmap all-zero: clears the words of the logged rows (or
// everything, if the log overflowed; vislog_cap == 0 is the A/B mode in which the host clears the bitmaps with a memset
// before every launch).  Writes the k closest of R (already sorted by (dist, id); a NaN seed, if still there, is R's last
// entry and is not returned), adds the work counters — WIDE: n_steps at [4]; profile builds: the phase ticks behind them —
// and, in the one-launch form, tells the spinning host thread.
// (the first half of it, for a walk with an epilogue of its own: k_graphm.hip)
__device__ __forceinline__ void clear_visited(uint32_t vislog_cap, uint32_t vis_words, int lane, uint32_t* vis,
                                              const uint32_t* vlog, uint32_t n_logged) {
  // (the log was written by other lanes, through global memory: a real fence, once per query)
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  if (vislog_cap == 0) {
  } else if (n_logged <= vislog_cap) {
    for (uint32_t i = lane; i < n_logged; i += 64) vis[vlog[i] >> 5] = 0u;
  } else {
    for (uint32_t i = lane; i < vis_words; i += 64) vis[i] = 0u;
  }
}

template <bool WIDE>
__device__ __forceinline__ void finish_query(const GraphArgs& a, const uint64_t* R, uint32_t nR, uint32_t qi, int lane,
                                             uint32_t* vis, const uint32_t* vlog, uint32_t n_logged, const WalkCounters& c,
                                             const GraphProf& prof) {
  clear_visited(a.vislog_cap, a.vis_words, lane, vis, vlog, n_logged);
  uint32_t cnt = nR < a.k ? nR : a.k;
  if (cnt && (uint32_t)(R[cnt - 1] >> 32) == kOrdNaN) cnt -= 1;
  for (uint32_t j = lane; j < a.k; j += 64) {
    const bool ok = j < cnt;
    a.out_ids[(size_t)qi * a.k + j] = ok ? (uint64_t)((uint32_t)(R[j] & 0xFFFFFFFFull) >> 1) : ~0ull;
    a.out_dist[(size_t)qi * a.k + j] = ok ? ordered_to_f32((uint32_t)(R[j] >> 32)) : __builtin_inff();
  }
  if (lane == 0) {
    a.out_count[qi] = cnt;
    atomicAdd(&a.counters[0], c.n_dist);
    atomicAdd(&a.counters[1], c.n_hops0);
    atomicAdd(&a.counters[2], c.n_hops_up);
    atomicAdd(&a.counters[3], c.n_pf_hit);
    if (WIDE) atomicAdd(&a.counters[4], c.n_steps);
#ifdef EHX_GRAPH_PROFILE
    for (int i = 0; i < (WIDE ? 7 : 8); ++i) atomicAdd(&a.counters[(WIDE ? 5 : 4) + i], prof.t[i]);
#endif
  }
  if (a.done_flag) {   // one-launch form: the results above went to host-visible memory
    __threadfence_system();
    __builtin_amdgcn_s_waitcnt(0);
    if (lane == 0) __hip_atomic_store(a.done_flag, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

using GraphKernel = void (*)(const GraphArgs);

}  // namespace
}  // namespace ehx
