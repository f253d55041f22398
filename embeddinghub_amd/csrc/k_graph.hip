// Graph-mode search: HNSW-style greedy descent + level-0 best-first search over an HBM-resident
// graph, one wavefront per query.
//
// Replaces hnswlib::HierarchicalNSW::searchKnn / searchBaseLayerST (call site
// embeddinghub/embeddingstore/index.cc:41; algorithm restated in oracle/hnsw_oracle.hpp):
//   * upper levels maxlevel..1: greedy descent — scan the current node's list in stored order and
//     move to the FIRST strictly-closest neighbour, repeat until no improvement;
//   * level 0: best-first search bounded by ef.  hnswlib keeps two heaps (candidates, results) and a
//     lowerBound; here ONE sorted list R of at most ef (distance, id, expanded) keys lives in LDS:
//     the next node to expand is the closest unexpanded entry of R, the search ends when R has no
//     unexpanded entry.  This is equivalent to the two-heap formulation whenever distances are
//     distinct: every candidate is inserted into the result heap at the same moment, a candidate
//     evicted from the results has distance >= lowerBound and can never be expanded, and processing a
//     node's neighbours as one batch (R <- ef smallest of R u batch) keeps exactly the elements the
//     one-by-one insertion keeps.
//
// Layout re-designed for the GPU (SURVEY Appendix A.3 describes hnswlib's AoS element block):
//   * adj0[n][2M] u32, padded with 0xFFFFFFFF, stored order preserved: one 128-B line per expansion;
//   * upper levels: up_start[n] (index of the node's first upper list or ~0), up_lists[*][M];
//   * vectors: the space's row-major X plus a SEARCH COPY Xs (k_misc.hip: every 16-float block permuted
//     so that the four inputs of SSE partial sum j are contiguous; cosine rows normalised): a 4-lane
//     group reads a row in coalesced 64-byte pieces and lane j accumulates partial sum j — the canonical
//     (oracle-order) arithmetic, so on an imported graph the traversal, the returned ids and the
//     distances are bit-identical to the oracle;
//   * visited set: one bit per row per in-flight query in HBM (n/8 bytes per query — 1.25 MB at 10 M
//     rows, 1.3 GB for a 1024-query batch out of 288 GB), test-and-set with atomicOr.  The bitmap is all-zero
//     between launches: a query logs every row it marks (vislog, 48 ef + 256 entries) and clears exactly those
//     words when it is done — a few thousand stores instead of a 1.3-GB memset per batch (a query that outgrows
//     its log clears its whole bitmap instead);
//   * work counters as SURVEY §8d: n_dist = rows actually fetched, n_hops0 / n_hops_up = expansions.
//
// The LDS layout, the query prologue, the greedy descent, the ranking (rank_by_counting) and the merge of fresh keys into R and the query
// epilogue are k_graph_common.h's (shared with the wide walk, k_graphw.hip); the 64-lane sort and the binary search
// are ehx_kernels.h's.  This file is the strict level-0 loop and the launcher.
#include "k_graph_common.h"

namespace ehx {

size_t graph_lds_bytes(uint32_t ld, uint32_t ef_cap, uint32_t width) { return GraphLds::bytes(ld, ef_cap, graph_n_ids(width)); }

// (Measured and not shipped, the switches are gone.  Round 3 capped the registers so that 3 or 4 waves share a SIMD
// (amdgpu_waves_per_eu): the compiler spills 79-535 registers per lane (it keeps the row walk's register rings alive across
// the LDS phases); at batch 1024 a SIMD holds one wave anyway (graph kernel history, round 3).  Two more
// switches selected branches that never shipped and are deleted with them: one private row of X per lane instead of
// 4-lane groups on the search copy, and deciding the next node only after the merge.
// Round 4 built a HELPER wave per query — rows 16.. of every distance batch on a second SIMD, same arithmetic, bit-identical
// — and measured -1..2 % at batch 1024, +1..3 % at 2048 (profiles/r04_j_graph_*_helper{0,1}.jsonl): the row phase is bound
// by the memory system, not by the loads one wave keeps in flight.  Removed in round 6; the lever that pays at batch 1024 is
// fewer dependent steps per query: k_graphw.hip.  Round 6 re-measured the helper on THIS walk at short rows, where it does
// pay for the wide walk's 64-row passes: 6.25 M x 128, batch 1024, ef 50 / 200 / 800: 0.324 / 0.377 / 0.354 -> 0.294 / 0.344 /
// 0.331 of 8 TB/s (profiles/r06_l_graph_6250k128_help{0,1}.jsonl) — an expansion's <= 32 rows are ONE pass and one round
// trip either way, the split only adds two barriers.  Not in the library.)
template <int METRIC01>
__global__ __launch_bounds__(64) void graph_search_kernel(const GraphArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const uint32_t qi = blockIdx.x;
  GraphLds L;
  L.carve(smem, a.ld, a.ef_cap, 64);
  uint64_t* R = L.R;
  uint64_t* batch = L.batch;
  uint32_t* ids_l = L.ids;
  uint32_t* vis = a.visited + (size_t)qi * a.vis_words;
  uint32_t* vlog = a.vislog + (size_t)qi * a.vislog_cap;
  uint32_t n_logged = 0;  // rows marked visited so far (wave-uniform)
  for (uint32_t i = lane; i < a.ef_cap; i += 64) L.F[i] = 0;
  load_query<1>(a, L.qs, qi, 0, lane);

  WalkCounters ctr;
  // ---- entry point and upper levels ----
  const Descent top = greedy_descent<METRIC01>(a, L, lane, ctr);
  const uint32_t cur = top.cur;

  // ---- level 0: best-first, ef bounded ----
  // Per expansion the dependent chain is: adjacency row -> visited words -> neighbour rows -> merge.
  //  * The adjacency row of the node most likely to be expanded next (c2, the second-closest
  //    unexpanded entry of R) is requested before this expansion's row fetches.  Right after the
  //    distances — BEFORE the merge — the next node is known for certain (c2, or the closest fresh
  //    neighbour if that is closer): c2's visited words, or the fresh node's adjacency row and then
  //    its visited words, are requested there and fly while R is merged.  On a confirmed c2 only the
  //    row fetch is left on the chain.  The traversal order is unchanged.
  //  * visited: the test is an agent-scope atomic LOAD, the set a fire-and-forget atomicOr (an
  //    adjacency list holds distinct ids — hnswlib invariant, checked on import — so the lanes of one
  //    expansion never race on the same BIT, and the same wave's later loads of a word observe its
  //    earlier atomics: per-location coherence).  The speculative words are loaded after this
  //    expansion's atomicOrs in program order and nothing else touches the bitmap before they are used.
  //  * merge: the fresh keys are ranked by counting (broadcast LDS reads, no shuffle network), their
  //    insertion points found by binary search, and R is updated IN PLACE from the top down, touching
  //    only [first insertion point, nR), one ballot + prefix popcount per 64 slots: nothing at all when
  //    no fresh key beats the current worst.
  const uint32_t ef = a.ef;
  uint32_t nR = 1;
  if (lane == 0) {
    R[0] = ((uint64_t)(top.nan_seed ? kOrdNaN : f32_to_ordered(top.curdist)) << 32) | ((uint64_t)cur << 1);
    atomicOr(&vis[cur >> 5], 1u << (cur & 31));
    if (a.vislog_cap) vlog[0] = cur;
  }
  n_logged = 1;
  wave_lds_sync();
  uint32_t scan_from = 0;  // every entry of R before this index is expanded
  uint32_t pf_node = kNoNode, pf_nb = kNoNode, pf_word = 0;
  GraphProf prof;
  for (;;) {
    // closest unexpanded entry (and the one after it): 128 entries per trip (both LDS reads in flight
    // together), the two keys taken out of the registers with readlane — one LDS latency per trip
    uint32_t idx = kNoNode, idx2 = kNoNode;
    uint64_t kidx = 0, kidx2 = kKeyInf;
    for (uint32_t base = scan_from & ~63u; base < nR && idx2 == kNoNode; base += 128) {
      const uint32_t i0 = base + lane, i1 = i0 + 64;
      const uint64_t v0 = i0 < nR ? R[i0] : 1ull;  // beyond nR: "expanded"
      const uint64_t v1 = i1 < nR ? R[i1] : 1ull;
      uint64_t m0 = __ballot(!(v0 & 1ull)), m1 = __ballot(!(v1 & 1ull));
#pragma unroll
      for (int pick = 0; pick < 2; ++pick) {
        if (pick == 0 ? idx != kNoNode : (idx == kNoNode || idx2 != kNoNode)) continue;
        uint32_t at = kNoNode;
        uint64_t key = 0;
        if (m0) {
          const int l = __builtin_ctzll(m0);
          m0 &= m0 - 1;
          at = base + (uint32_t)l;
          key = readlane64(v0, l);
        } else if (m1) {
          const int l = __builtin_ctzll(m1);
          m1 &= m1 - 1;
          at = base + 64 + (uint32_t)l;
          key = readlane64(v1, l);
        }
        if (at == kNoNode) continue;
        if (pick == 0) {
          idx = at;
          kidx = key;
        } else {
          idx2 = at;
          kidx2 = key;
        }
      }
    }
    if (idx == kNoNode) break;
    prof.mark(0);
    const uint32_t c = (uint32_t)(kidx & 0xFFFFFFFFull) >> 1;
    const uint32_t c2 = idx2 != kNoNode ? (uint32_t)(kidx2 & 0xFFFFFFFFull) >> 1 : kNoNode;
    wave_lds_sync();
    if (lane == 0) R[idx] |= 1ull;
    ctr.n_hops0 += 1;
    // neighbours (stored order) and their visited words
    uint32_t nb = kNoNode, word = 0;
    if (c == pf_node) {
      nb = pf_nb;
      word = pf_word;
    } else {  // first expansion only
      if (lane < (int)a.M0) nb = a.adj0[(size_t)c * a.M0 + lane];
      if (nb != kNoNode) word = __hip_atomic_load(&vis[nb >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const bool fresh = nb != kNoNode && !(word & (1u << (nb & 31)));
    if (fresh) (void)__hip_atomic_fetch_or(&vis[nb >> 5], 1u << (nb & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    pf_node = c2;
    pf_nb = kNoNode;
    if (c2 != kNoNode && lane < (int)a.M0) pf_nb = load_here(a.adj0 + (size_t)c2 * a.M0 + lane);
    const uint64_t fmask = __ballot(fresh);
    const uint32_t nfresh = __builtin_popcountll(fmask);
    if (fresh) {
      const uint32_t slot = (uint32_t)__builtin_popcountll(fmask & ((1ull << lane) - 1ull));
      ids_l[slot] = nb;
      if (n_logged + slot < a.vislog_cap) vlog[n_logged + slot] = nb;
    }
    n_logged += nfresh;
    wave_lds_sync();
    ctr.n_dist += nfresh;
    prof.mark(1);
    // distances: lane p (< nfresh) owns fresh neighbour p; a NaN distance keeps +inf and never enters R, so only the
    // nin keys below +inf are merged (they rank 0..nin-1 among the fresh keys)
    uint64_t mykey = kKeyInf;
    if (nfresh) {
      // canonical distances of rows ids_l[0..nfresh): one 4-lane group per row reading the search copy
      const float d = wave_group_dists<METRIC01>(L.qs, a.Xs, a.ld, a.dims, ids_l, nfresh, lane, a.xscale);
      if ((uint32_t)lane < nfresh && d == d) mykey = ((uint64_t)f32_to_ordered(d) << 32) | ((uint64_t)ids_l[lane] << 1);
    }
    const uint32_t nin = (uint32_t)__builtin_popcountll(__ballot(mykey != kKeyInf));
    scan_from = idx2 != kNoNode ? idx2 : nR;  // entries before idx2 are all expanded now (positions only grow)
#ifdef EHX_GRAPH_PROFILE
    if (__any(mykey == 1ull)) prof.t[7] += 1;  // keeps the distances live: the timer below waits for them
#endif
    prof.mark(2);
    // Does any fresh key enter R?  If so rank the fresh keys among themselves by counting (keys are
    // distinct: the id is part of the key); the key of rank 0 is the closest fresh neighbour.
    const bool do_merge = nin != 0 && (nR < ef || __any(mykey < R[ef - 1]));
    uint64_t minkey = kKeyInf;
    uint32_t rank = 0;
    if (do_merge) {
      batch[lane] = mykey;
      wave_lds_sync();
      rank = rank_by_counting(batch, nfresh, mykey);  // (batch[nfresh..64) = +inf never counts)
      const uint64_t first = __ballot(mykey != kKeyInf && rank == 0);
      minkey = readlane64(mykey, (int)__builtin_ctzll(first));
    }
    prof.mark(3);
    // The node expanded next is known NOW, before the merge: the closer of the closest fresh neighbour
    // and the second unexpanded entry c2 (a fresh key below R[idx2] is always inserted; one above it
    // leaves R[idx2] where it is).  Its adjacency row / visited words fly while R is merged.
    const uint64_t k2 = kidx2;  // key of the second unexpanded entry (+inf if there is none)
    bool pf_have_word;
    if (minkey < k2) {
      pf_node = (uint32_t)(minkey & 0xFFFFFFFFull) >> 1;
      pf_nb = kNoNode;
      if (lane < (int)a.M0) pf_nb = load_here(a.adj0 + (size_t)pf_node * a.M0 + lane);
      pf_have_word = false;
    } else {
      // c2 it is, and its adjacency row has landed (requested before the row fetches): its visited words, loaded
      // after this expansion's atomicOrs in program order
      pf_word = 0;
      if (pf_nb != kNoNode) pf_word = __hip_atomic_load(&vis[pf_nb >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      pf_have_word = true;
      ctr.n_pf_hit += 1;
    }
    prof.mark(4);
    if (do_merge) merge_sorted_into_R<5, 6>(L, ef, mykey, mykey != kKeyInf, rank, nin, nR, scan_from, lane, prof);
    if (!pf_have_word) {
      // the adjacency row of the fresh node expanded next landed during the merge
      pf_word = 0;
      if (pf_nb != kNoNode) pf_word = __hip_atomic_load(&vis[pf_nb >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    prof.mark(7);
  }

  finish_query<false>(a, R, nR, qi, lane, vis, vlog, n_logged, ctr, prof);
}

hipError_t launch_graph_search_wide(const GraphArgs& a, hipStream_t st);  // k_graphw.hip

hipError_t launch_graph_search(const GraphArgs& a, hipStream_t st) {
  // the wide walk serves lists of up to 32 ids (M <= 16: one half wave per expanded node)
  if (a.width > 1 && a.M0 <= 32) return launch_graph_search_wide(a, st);
  const size_t lds = graph_lds_bytes(a.ld, a.ef_cap, 1);
  static DynLdsAttr attr;
  static const GraphKernel kStrict[2] = {graph_search_kernel<0>, graph_search_kernel<1>};  // [metric != L2]
  if (hipError_t e = attr.ensure(kStrict, 2, lds); e != hipSuccess) return e;
  hipLaunchKernelGGL(kStrict[a.metric != 0], dim3(a.nq), dim3(64), lds, st, a);
  return hipGetLastError();
}

}  // namespace ehx
