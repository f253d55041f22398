// Graph-mode search under an exclusion list PER QUERY (ehx_graph_knn_except*, ehx_graphx.cpp): "the k nearest rows this
// user has not seen", walked.  The walk is k_graphm.hip's, statement for statement (k_graphm_walk.h with TABLE = 2; its
// model is tests/filtered_walk_model.py with allowed = the complement of the list): every node is a candidate and is walked
// through, only allowed nodes enter the results and set the bound, the list R is trimmed at its ef-th allowed entry and
// never grows beyond a.ef_cap.  What differs is where a row's allowed bit comes from.  A bitmap per query costs n / 8 bytes
// of device memory per query and the table holds 64 of them; a user's list of seen rows is a few hundred to a few thousand
// ids.  So the list itself is what the wave keeps:
//   * launch_except_lists (k_except.hip) has made every list of the device batch ascending, unique, 32 bits wide and cut at
//     the row count, once, before this launch;
//   * the wave copies its query's list into LDS behind the walk's own carve (graph_list_lds_offset) in its prologue,
//     16 bytes a lane, four loads in flight;
//   * the entry node and every fresh neighbour are looked up in it: lane p searches ITS neighbour, all lanes in the same
//     ceil(log2 len) halvings plus one compare (lds_list_holds) — LDS reads and selects, no divergence, no global memory;
//     an empty list reads nothing, and the walk is then the bitmap walk under an all-ones bitmap without the bitmap's loads.
// The list region is dynamic LDS sized by the launch's LONGEST list rounded up to 64 entries (a.excl_lds, from the host,
// which has validated the offsets): a batch of short lists does not pay 16 KiB per wave in occupancy for the longest list
// the interface admits.  One wavefront per query, no matrix instructions: the work is a pointer chase, a 64-lane distance
// per neighbour row (wave_group_dists) and the integer bookkeeping of R.
#include "k_graphm_keys.h"

namespace ehx {

template <int METRIC01>
__global__ __launch_bounds__(64) void graph_search_except_kernel(const GraphArgs a) {
  constexpr int TABLE = 2;
#include "k_graphm_walk.h"
}

hipError_t launch_graph_search_except(const GraphArgs& a, hipStream_t st) {
  if (a.n > (1u << 30) || a.ef_cap < a.ef || a.M0 > 64 || !a.cap_hits || !a.excl || !a.excl_cnt || (a.excl_lds & 63u) ||
      a.excl_lds > kExceptMaxList || a.q_raw)
    return hipErrorInvalidValue;
  const size_t lds = graph_list_lds_offset(a.ld, a.ef_cap) + (size_t)a.excl_lds * sizeof(uint32_t);
  if (lds > kMaxLds) return hipErrorInvalidValue;
  static DynLdsAttr attr;
  static const GraphKernel kExcept[2] = {graph_search_except_kernel<0>, graph_search_except_kernel<1>};   // [metric != L2]
  if (hipError_t e = attr.ensure(kExcept, 2, lds); e != hipSuccess) return e;
  hipLaunchKernelGGL(kExcept[a.metric != 0], dim3(a.nq), dim3(64), lds, st, a);
  return hipGetLastError();
}

}  // namespace ehx
