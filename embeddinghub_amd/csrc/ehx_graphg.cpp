// Grouped graph search: ehx_graph_knn_grouped (host pointers) and ehx_graph_knn_grouped_device — the graph walk with a cap
// per group label (include/ehx.h has the contract, DESIGN §e.35 the design, k_graphg.hip the kernel, tests/grouped_walk_model.py
// the rule in plain Python).  Labels are ehx_knn_grouped's: group_of[r] for r < n_eff = min(the call's ONE snapshot of the row
// count, n_labels); rows at or above n_eff are walked through and never returned.
// Routes.  EHX_WALK_GRAPH and EHX_WALK_AUTO on a graph space: every query is walked (there is no selectivity to decide on),
// per device batch of kSideChunk queries ONE launch through knn_graph_locked — the masked walk's hold, wait, clock and
// refusals; nothing is read back, so the call does not wait.  EHX_WALK_EXACT, and every flat space: grouped_locked, the
// exact grouped search's own body, under the same snapshot.
// The walk counts where the masked walk counts: ehx_graph_counters, ehx_stats' queries, and the queries whose list reached
// its cap behind ehx_test_graph_masked_counters.
#include "ehx_internal.h"

namespace {

constexpr const char* kGraphgWhy = "grouped graph search over shards is not built yet";

// in this order: the grouped searches' head (the NULL space, the device, k, per_group, the pointers), then the route
int graphg_check(const ehx_space* s, size_t nq, uint32_t k, uint32_t per_group, const void* q, const void* group_of,
                 uint64_t n_labels, uint32_t route, const void* o_ids, const void* o_dist, const void* o_cnt) {
  if (int rc = grouped_check_head(s, nq, k, per_group, q, group_of, n_labels, o_ids, o_dist, o_cnt)) return rc;
  if (int rc = check_route(route)) return rc;
  return check_batch_size(nq);
}

// an unsharded space, locked shared, scratch_mu held, its device current; everything is enqueued on `st`.  n_pub: the call's
// ONE read of the row count; d_group_of: at least min(n_pub, n_labels) labels on the device
int graphg_locked(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const float* d_queries, uint32_t k,
                  uint32_t per_group, const uint32_t* d_group_of, uint64_t n_labels, uint32_t route, const ResultBlock& out) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  if (s->params.mode != EHX_MODE_GRAPH || route == EHX_WALK_EXACT) {   // (a flat space has no graph)
    s->graphm_ctr[1] += nq;
    s->graphm_ctr[2] += 1;
    return grouped_locked(s, st, n_pub, nq, d_queries, k, per_group, d_group_of, n_labels, out);
  }
  if ((rc = s->masked.dCapHits.ensure(1, true))) return rc;
  s->graphm_ctr[2] += 1;
  GraphMask gm = {nullptr, std::min(n_pub, n_labels), s->masked.dCapHits.p, nullptr};
  gm.group_of = d_group_of;
  gm.per_group = per_group;
  for (size_t q0 = 0; q0 < nq; q0 += kSideChunk) {
    const size_t m = std::min(kSideChunk, nq - q0);
    const ResultBlock o = out.from(q0, m);
    if ((rc = knn_graph_locked(s, st, m, d_queries + q0 * s->dims, k, o.ids, o.dist, o.cnt, nullptr, &gm))) return rc;
    s->graphm_ctr[0] += m;
  }
  return EHX_OK;
}

}  // namespace

extern "C" {

int ehx_graph_knn_grouped_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                 uint32_t per_group, const uint32_t* d_group_of, uint64_t n_labels, uint32_t route,
                                 uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count) {
  if (int rc = graphg_check(s, n_queries, k, per_group, d_queries, d_group_of, n_labels, route, d_out_ids, d_out_dist, d_out_count))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_graph_knn_grouped_device", kGraphgWhy, n_queries, &st, [&] {
    return graphg_locked(s, st, s->n.load(std::memory_order_acquire), n_queries, d_queries, k, per_group, d_group_of, n_labels,
                         route, ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

// host pointers in, host pointers out, on the space's stream: the labels of the prefix staged in grouped.dLabels, as
// ehx_knn_grouped stages them
int ehx_graph_knn_grouped(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint32_t per_group,
                          const uint32_t* group_of, uint64_t n_labels, uint32_t route, uint64_t* out_ids, float* out_dist,
                          uint32_t* out_count) {
  if (int rc = graphg_check(s, n_queries, k, per_group, queries, group_of, n_labels, route, out_ids, out_dist, out_count)) return rc;
  return search_on_device(s, "ehx_graph_knn_grouped", kGraphgWhy, n_queries, nullptr, [&]() -> int {
    ehx_space::Grouped& w = s->grouped;
    const uint64_t n_pub = s->n.load(std::memory_order_acquire);   // the ONE read of the row count
    const uint64_t n_eff = std::min(n_pub, n_labels);
    int rc;
    if ((rc = w.dLabels.ensure(std::max<uint64_t>(n_eff, 1))) || (rc = w.host.up(s->stream, queries, n_queries, s->dims, k, false)))
      return rc;
    // (earlier calls' launches on other streams may still read the labels)
    if ((rc = wait_searches_in_flight(s, s->stream))) return rc;
    // (pageable host memory: the runtime stages it before the call returns)
    if (n_eff) HIP_TRY(hipMemcpyAsync(w.dLabels.p, group_of, n_eff * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
    if ((rc = graphg_locked(s, s->stream, n_pub, n_queries, w.host.q, k, per_group, w.dLabels.p, n_eff, route, w.host.out)))
      return rc;
    return w.host.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
  });
}

}  // extern "C"
