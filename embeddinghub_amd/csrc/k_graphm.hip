// Graph-mode search under a row bitmap (ehx_graph_knn_masked*), or under one bitmap PER QUERY out of a table
// (ehx_graph_knn_masked_multi*): the strict walk of k_graph.hip, one wavefront per query, with ONE deviation — hnswlib >= 0.7's rule for a filter (isIdAllowed: every node is a candidate and is walked through,
// only allowed nodes enter the results and set the bound) plus a bound on the list a GPU needs.  Stated as a model in
// tests/filtered_walk_model.py; in the one-list form of k_graph.hip's header:
//   * upper levels: the greedy descent, the filter ignored;
//   * level 0: ONE sorted list R of (distance, id, allowed, expanded) keys.  A step expands the closest unexpanded entry,
//     allowed or not, and merges its unvisited neighbours (NaN distances dropped) into R.  Then the TRIM: once R holds ef
//     allowed entries everything behind the ef-th allowed one is deleted (those entries lie above hnswlib's lowerBound:
//     never expanded, never returned), and nothing is kept behind position cap (a.ef_cap >= ef: the LDS the list may take;
//     an unfiltered walk has cap = ef).  The search ends when R has no unexpanded entry;
//   * the answer: the first k allowed entries of R (a NaN seed is never returned), possibly fewer than k.
// With every row allowed the trim is R <- the ef smallest and this is k_graph.hip's walk, bit for bit.
//
// The key carries the allowed bit beside the expanded bit: (ordered distance << 32) | (id << 2) | (allowed << 1) | expanded
// — ids below 2^30, the order of keys is still (distance, id) because ids are distinct.  What differs from k_graph.hip:
//   * the allowed test of a fresh id: one load of the bitmap word (shared by the whole batch: it lives in the caches),
//     requested with the row fetches;
//   * fresh keys that the trim would delete at once (behind R's last entry while R is trimmed or at cap) are dropped
//     before the merge, so the merge (merge_sorted_into_R with cap for ef) runs only when R changes;
//   * the trim: a ballot and a prefix popcount per 64 slots of R up to the ef-th allowed entry — skipped while R cannot hold
//     ef allowed entries yet, and when R is trimmed already and no fresh allowed key went in;
//   * the epilogue compacts the first k allowed entries.
// The adjacency / visited prefetch of k_graph.hip is kept: the node it requested may be trimmed away before it is picked,
// then the pick does not match and the lists are loaded on the spot.  Everything else — LDS layout, query prologue,
// descent, ranking, merge, the visited bitmap's log and clear — is k_graph_common.h's.
// The walk is written once (k_graphm_walk.h, the body of both kernel templates below); the kernels of a table differ in
// the two places a bit is tested: the word is allow[allow_of[qi] + (id >> 5)].
#include "k_graph_common.h"

namespace ehx {

namespace {

constexpr uint64_t kKeyExpanded = 1ull, kKeyAllowed = 2ull;
__device__ __forceinline__ uint32_t mkey_id(uint64_t key) { return (uint32_t)(key & 0xFFFFFFFFull) >> 2; }

// the kernel's argument block where it lies in memory (scalar loads at the point of use; the empty asm keeps them there)
typedef const GraphArgs __attribute__((address_space(4)))* KernArgs;
__device__ __forceinline__ KernArgs late_args() {
  KernArgs p = (KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}
// query qi's entry of a [nq] argument array the host wrote before the launch: wave-uniform and constant while the kernel
// runs, so it is read with a scalar load (no vector-memory round trip in front of the load that depends on it)
typedef const uint32_t __attribute__((address_space(4)))* ConstWords;
__device__ __forceinline__ uint32_t uniform_word(const uint32_t* p, uint32_t qi) { return ((ConstWords)p)[qi]; }

}  // namespace

// ONE bitmap for the batch
template <int METRIC01>
__global__ __launch_bounds__(64) void graph_search_masked_kernel(const GraphArgs a) {
  constexpr int TABLE = 0;
#include "k_graphm_walk.h"
}

// a bitmap per query (a.allow_of)
template <int METRIC01>
__global__ __launch_bounds__(64) void graph_search_tabled_kernel(const GraphArgs a) {
  constexpr int TABLE = 1;
#include "k_graphm_walk.h"
}

hipError_t launch_graph_search_masked(const GraphArgs& a, hipStream_t st) {
  if (a.n > (1u << 30) || a.ef_cap < a.ef || a.M0 > 64 || !a.cap_hits || (a.allow_bits && !a.allow) || a.q_raw)
    return hipErrorInvalidValue;
  const size_t lds = graph_lds_bytes(a.ld, a.ef_cap, 1);
  static DynLdsAttr attr;
  static const GraphKernel kMasked[4] = {graph_search_masked_kernel<0>, graph_search_masked_kernel<1>,   // [metric != L2]
                                         graph_search_tabled_kernel<0>, graph_search_tabled_kernel<1>};  // 2 + [metric != L2]
  if (hipError_t e = attr.ensure(kMasked, 4, lds); e != hipSuccess) return e;
  hipLaunchKernelGGL(kMasked[(a.allow_of ? 2 : 0) + (a.metric != 0)], dim3(a.nq), dim3(64), lds, st, a);
  return hipGetLastError();
}

}  // namespace ehx
