// Graph walk under per-query exclusion lists: ehx_graph_knn_except (host pointers), ehx_graph_knn_except_device and
// ehx_graph_knn_except_keys (the lists given as stored keys).  Query i is answered as ehx_graph_knn_masked_multi_device answers
// it alone under the complement bitmap of its list — n_bits the call's ONE snapshot of the row count, bit r clear iff r occurs
// in the list — with the same `route`, byte for byte (include/ehx.h has the contract, DESIGN §e.34 the design, k_graphx.hip the
// kernel).  The lists are ehx_knn_except's: CSR, 64-bit ids, unsorted, repeats allowed, ids at or beyond the row count
// exclude nothing, at most EHX_EXCEPT_MAX_LIST entries per query.
// Per device batch of kSideChunk queries:
//   1  launch_except_lists sorts every list once into except.dSorted (ascending, unique, cut at the row count) — what the walk
//      kernel copies into LDS and what the exact route's re-rank searches;
//   2  the routes.  EHX_WALK_GRAPH: every query is walked.  EHX_WALK_EXACT, and every flat space: ehx_knn_except's own answer
//      (except_locked_at — the int8 scan where it serves, else the exact route).  EHX_WALK_AUTO: the masked graph search's rule
//      per QUERY — walked iff its allowed rows * EHX_WALK_LIST_FACTOR >= the rows (the share cut is carried over, not measured
//      again; a list of at most 4096 ids can take a query below it only on a space of fewer than 4469 rows, so the lengths
//      are read back, one wait, only there);
//   3  ONE walk launch for the batch's walked queries (knn_graph_locked: the masked walk's hold, wait, clock and refusals), its
//      LDS list region sized by the longest list of the batch — the host knows the offsets, which it has checked — rounded up
//      to 64 entries; the others go to the exact route with their lists still sorted in the scratch.  A mixed batch is
//      gathered and scattered back part by part (except.split); the gather's index array names each query's list.
// The walk counts where the masked walk counts: ehx_graph_counters, and queries walked / answered exactly / calls / cap hits
// behind ehx_test_graph_masked_counters.
#include "ehx_internal.h"

namespace {

constexpr const char* kGraphxWhy = "graph search with exclusion lists over shards is not built yet";
constexpr const char* kGraphxInstead = "ehx_graph_knn_masked_multi";

// in this order: the NULL space, the device, then what ehx_knn_except checks of k and the pointers, then the route
int graphx_check(const ehx_space* s, size_t nq, uint32_t k, bool ptrs_ok, uint32_t route) {
  if (!s) return fail(EHX_EINVAL, "space is NULL");
  if (int rc = ehx_init(nullptr, 0)) return rc;   // (no device: EHX_ENODEVICE, whatever else is wrong with the call)
  if (int rc = except_check(s, nq, k, ptrs_ok)) return rc;
  return check_route(route);
}

// an unsharded space, locked shared, scratch_mu held, its device current; everything is enqueued on `st`.  The lists are on
// the device; off: their offsets in host memory, checked (except_check_off).
int graphx_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, const uint64_t* d_excl_ids,
                  const uint64_t* d_excl_off, const uint64_t* off, uint32_t route, const ResultBlock& out) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  ehx_space::Except& w = s->except;
  s->graphm_ctr[2] += 1;
  const uint64_t n_pub = s->n.load(std::memory_order_acquire);   // the ONE read of the row count
  if (s->params.mode != EHX_MODE_GRAPH) route = EHX_WALK_EXACT;   // (a flat space has no graph)
  if (route == EHX_WALK_EXACT) {
    if ((rc = except_check_ld(s))) return rc;   // (before anything is enqueued)
    s->graphm_ctr[1] += nq;
    return except_locked_at(s, st, n_pub, nq, d_queries, k, d_excl_ids, d_excl_off, out);
  }
  const size_t cap = std::min(kSideChunk, nq);
  if ((rc = w.dSorted.ensure(cap * kExceptMaxList)) || (rc = w.dSortedCnt.ensure(cap)) ||
      (rc = s->masked.dCapHits.ensure(1, true)))
    return rc;
  std::vector<uint32_t> cnt, iw, ix;
  for (size_t q0 = 0; q0 < nq; q0 += kSideChunk) {
    const size_t m = std::min(kSideChunk, nq - q0);
    const float* q = d_queries + q0 * s->dims;
    const ResultBlock o = out.from(q0, m);
    uint64_t longest = 0;
    for (size_t i = 0; i < m; ++i) longest = std::max(longest, off[q0 + i + 1] - off[q0 + i]);
    // (searches on other streams may still read the sorted lists of an earlier call)
    if ((rc = wait_searches_in_flight(s, st))) return rc;
    HIP_TRY(launch_except_lists(d_excl_ids, d_excl_off + q0, (uint32_t)m, n_pub, w.dSorted.p, w.dSortedCnt.p, st));
    // the route of every query.  (A list takes out at most `longest` rows: where even that leaves the share, nothing is read)
    iw.clear();
    ix.clear();
    if (route == EHX_WALK_AUTO && (n_pub - std::min(n_pub, longest)) * EHX_WALK_LIST_FACTOR < n_pub) {
      cnt.resize(m);
      HIP_TRY(hipMemcpyAsync(cnt.data(), w.dSortedCnt.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      for (size_t i = 0; i < m; ++i) ((n_pub - cnt[i]) * EHX_WALK_LIST_FACTOR >= n_pub ? iw : ix).push_back((uint32_t)i);
    }
    const size_t n_exact = ix.size(), n_walk = m - n_exact;
    if (n_exact && (rc = except_check_ld(s))) return rc;   // (EHX_WALK_AUTO: known only now)
    // n queries, query j under list of[j] (nullptr: list j), walked in ONE launch
    auto walk = [&](size_t n, const float* wq, const uint32_t* of, uint64_t* ids, float* dist, uint32_t* c) -> int {
      GraphMask gm = {nullptr, n_pub, s->masked.dCapHits.p, nullptr};
      gm.excl = w.dSorted.p;
      gm.excl_cnt = w.dSortedCnt.p;
      gm.excl_of = of;
      gm.excl_lds = (uint32_t)((longest + 63) & ~(uint64_t)63);
      if (int r = knn_graph_locked(s, st, n, wq, k, ids, dist, c, nullptr, &gm)) return r;
      s->graphm_ctr[0] += n;
      return EHX_OK;
    };
    auto exact = [&](size_t n, const float* xq, const uint32_t* of, uint64_t* ids, float* dist, uint32_t* c) -> int {
      s->graphm_ctr[1] += n;
      return except_exact(s, st, n_pub, n, xq, k, nullptr, nullptr, of, ids, dist, c, true);
    };
    if (n_exact == 0) {
      if ((rc = walk(m, q, nullptr, o.ids, o.dist, o.cnt))) return rc;
    } else if (n_walk == 0) {
      if ((rc = exact(m, q, nullptr, o.ids, o.dist, o.cnt))) return rc;
    } else {
      // a mixed batch — the walk first (what it refuses, it refuses before a row is written); the index array of each
      // gather is on the device while its answer runs and names the queries' lists
      if ((rc = w.split.rerun(
               s, st, q, iw, k,
               [&](size_t n, const float* sq, uint64_t* i2, float* d2, uint32_t* c2) { return walk(n, sq, w.split.dFbIdx.p, i2, d2, c2); },
               o.ids, o.dist, o.cnt)))
        return rc;
      if ((rc = w.split.rerun(
               s, st, q, ix, k,
               [&](size_t n, const float* sq, uint64_t* i2, float* d2, uint32_t* c2) { return exact(n, sq, w.split.dFbIdx.p, i2, d2, c2); },
               o.ids, o.dist, o.cnt)))
        return rc;
    }
  }
  return EHX_OK;
}

// host pointers in, host pointers out, on the space's stream (on_device): ids | offsets staged in except.dLists
int graphx_host_locked(ehx_space* s, size_t nq, const float* queries, uint32_t k, const uint64_t* excl_ids,
                       const uint64_t* excl_off, size_t n_excl, uint32_t route, uint64_t* out_ids, float* out_dist,
                       uint32_t* out_count) {
  ehx_space::Except& w = s->except;
  int rc;
  if ((rc = w.dLists.ensure(n_excl + nq + 1)) || (rc = w.host.up(s->stream, queries, nq, s->dims, k, false))) return rc;
  // (earlier calls' launches on other streams may still read the lists)
  if ((rc = wait_searches_in_flight(s, s->stream))) return rc;
  uint64_t* d_ids = w.dLists.p;
  uint64_t* d_off = d_ids + n_excl;
  // (pageable host memory: the runtime stages it before the call returns)
  if (n_excl) HIP_TRY(hipMemcpyAsync(d_ids, excl_ids, n_excl * sizeof(uint64_t), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(d_off, excl_off, (nq + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s->stream));
  if ((rc = graphx_locked(s, s->stream, nq, w.host.q, k, d_ids, d_off, excl_off, route, w.host.out))) return rc;
  return w.host.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
}

}  // namespace

extern "C" {

int ehx_graph_knn_except_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                const uint64_t* d_excl_ids, const uint64_t* d_excl_off, size_t n_excl, uint32_t route,
                                uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count) {
  if (int rc = graphx_check(s, n_queries, k,
                            d_out_ids && d_out_dist && d_out_count && (!n_queries || (d_queries && d_excl_off)) &&
                                (!n_excl || d_excl_ids),
                            route))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_graph_knn_except_device", kGraphxWhy, n_queries, &st, [&]() -> int {
    // the kernels trust the offsets: they are read back and checked before anything reads a list
    std::vector<uint64_t> off(n_queries + 1);
    HIP_TRY(hipMemcpyAsync(off.data(), d_excl_off, off.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (int rc = except_check_off(off.data(), n_queries, n_excl, "d_excl_off", "n_excl", kGraphxInstead)) return rc;
    return graphx_locked(s, st, n_queries, d_queries, k, d_excl_ids, d_excl_off, off.data(), route,
                         ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_graph_knn_except(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const uint64_t* excl_ids,
                         const uint64_t* excl_off, size_t n_excl, uint32_t route, uint64_t* out_ids, float* out_dist,
                         uint32_t* out_count) {
  if (int rc = graphx_check(s, n_queries, k,
                            out_ids && out_dist && out_count && (!n_queries || (queries && excl_off)) && (!n_excl || excl_ids),
                            route))
    return rc;
  if (n_queries)
    if (int rc = except_check_off(excl_off, n_queries, n_excl, "excl_off", "n_excl", kGraphxInstead)) return rc;
  return search_on_device(s, "ehx_graph_knn_except", kGraphxWhy, n_queries, nullptr, [&] {
    return graphx_host_locked(s, n_queries, queries, k, excl_ids, excl_off, n_excl, route, out_ids, out_dist, out_count);
  });
}

int ehx_graph_knn_except_keys(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const char* const* keys,
                              const size_t* klens, const uint64_t* key_off, size_t n_keys, uint32_t route, uint64_t* out_ids,
                              float* out_dist, uint32_t* out_count) {
  if (int rc = graphx_check(s, n_queries, k,
                            out_ids && out_dist && out_count && (!n_queries || (queries && key_off)) && (!n_keys || (keys && klens)),
                            route))
    return rc;
  if (n_queries)
    if (int rc = except_check_off(key_off, n_queries, n_keys, "key_off", "n_keys", kGraphxInstead)) return rc;
  // ONE shared hold for key lookup and search: the answer describes one state of the space
  return search_shared(s, "ehx_graph_knn_except_keys", kGraphxWhy, [&]() -> int {
    std::vector<uint64_t> ids;
    if (int rc = except_key_ids(s, keys, klens, n_keys, &ids)) return rc;
    return on_device(s, n_queries, s->stream, [&] {
      return graphx_host_locked(s, n_queries, queries, k, ids.data(), key_off, n_keys, route, out_ids, out_dist, out_count);
    });
  });
}

}  // extern "C"
