// Exact kNN restricted to a caller's lists of row ids: ehx_knn_among (host pointers), ehx_knn_among_device, and
// ehx_knn_among_keys (one shared list given as stored keys).  The listed rows are scanned exhaustively in the oracle's
// arithmetic (k_among.hip), whatever the space's mode: a graph space answers from its stored rows, its graph is not walked.
// Entry scaffold, host staging and the row-length gate are ehx_call.cpp's (search_shared / on_device, HostStage).
#include "ehx_internal.h"

namespace {

constexpr uint32_t kAmongGridTarget = 4096;   // workgroups a launch aims for (16 per CU): chosen, not measured
constexpr uint32_t kAmongMaxBlocks = 1024;    // ... and at most this many key lists per query for the merge

// the checks every entry point starts with, and why the gate behind the space's lock refuses a row-sharded space
int among_check(const ehx_space* s, size_t nq, uint32_t k, const void* q, const void* o_ids, const void* o_dist, const void* o_cnt) {
  return check_batch_call(s, nq, k, "k", false, o_ids && o_dist && o_cnt && (!nq || q));
}
constexpr const char* kAmongWhy = "filtered search over shards is not built yet";

}  // namespace

// an unsharded space, locked shared, scratch_mu held, its device current; everything is enqueued on `st`.
// d_off == nullptr: every query shares d_ids[0, n_cand).  max_list: an upper bound of one list's length (0: n_cand) — it
// sizes the grid only.  d_end (with d_off; ehx_labeled.cpp): query q's list is d_ids[d_off[q], d_end[q]), so queries may share
// a list inside ONE per-query launch; end_pairs: the lengths of those lists together (n_dist takes it; n_cand is then the
// length of the id array the lists lie in).
int ehx_impl::among_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k,
                           const uint64_t* d_ids, const uint64_t* d_off, size_t n_cand, size_t max_list, uint64_t* d_out_ids, float* d_out_dist,
                           uint32_t* d_out_count, bool count_queries, const uint64_t* d_end, uint64_t end_pairs) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  if ((rc = check_rows_fit_lds(s, "filtered search"))) return rc;   // (before anything is enqueued)
  // the ONE read of the row count: every page's range check answers for the same prefix
  const uint64_t n_pub = s->n.load(std::memory_order_acquire);
  AmongArgs a = {};
  a.rows = rows_view(s, n_pub);
  a.cand_ids = d_ids;
  a.cand_off = d_off;
  a.cand_end = d_off ? d_end : nullptr;
  a.n_cand = n_cand;
  a.nq = (uint32_t)nq;
  const uint64_t longest = std::max<uint64_t>(1, max_list && max_list < n_cand ? max_list : n_cand);
  const uint32_t step = among_step_rows(a);
  const uint64_t units = among_tiled(a) ? (nq + kAmongTileQ - 1) / kAmongTileQ : nq;
  a.n_blocks = (uint32_t)std::min<uint64_t>(
      std::min<uint64_t>((longest + step - 1) / step, kAmongMaxBlocks), std::max<uint64_t>(1, kAmongGridTarget / units));
  const uint32_t pages = (k + 63) / 64;
  if ((rc = s->scr.dQ.ensure(nq * s->ld))) return rc;
  if ((rc = s->scr.dPart.ensure(nq * a.n_blocks * 64))) return rc;
  if ((rc = s->scr.dMerged.ensure(nq * 64))) return rc;
  if (pages > 1 && (rc = s->scr.dGthr.ensure(nq + 8))) return rc;
  // (searches on other streams have read and written this scratch; this call's fence, below, makes a Set that rewrites
  // rows in place wait for it in turn)
  if ((rc = wait_searches_in_flight(s, st))) return rc;
  if ((rc = s->clock.begin(st, BatchClock::kOutOfRing))) return rc;
  HIP_TRY(launch_prep_queries(d_queries, (uint32_t)nq, s->dims, s->ld, (uint32_t)nq, s->metric, s->scr.dQ.p, st));
  a.Q = s->scr.dQ.p;
  a.out = s->scr.dPart.p;
  if ((rc = s->clock.scan_begin(st))) return rc;
  for (uint32_t pg = 0; pg < pages; ++pg) {
    a.floor = pg ? s->scr.dGthr.p : nullptr;
    HIP_TRY(launch_among(a, st));
    HIP_TRY(launch_flat_merge(s->scr.dPart.p, (uint32_t)nq, a.n_blocks, 64, s->scr.dMerged.p, st, a.n_blocks));
    if (pg + 1 < pages) HIP_TRY(launch_set_floor(s->scr.dMerged.p, (uint32_t)nq, s->scr.dGthr.p, st));
    // (the merged keys ARE the canonical distances: a page is written from them — launch_rerank would recompute them from
    // rows in the plain layout, which a single-copy graph space does not have)
    HIP_TRY(launch_among_emit(s->scr.dMerged.p, (uint32_t)nq, std::min<uint32_t>(64, k - pg * 64), k, pg * 64, d_out_ids,
                              d_out_dist, d_out_count, st));
  }
  if ((rc = s->clock.scan_end(st)) || (rc = s->clock.finish(st))) return rc;
  if (count_queries) s->n_queries += nq;
  s->n_dist += a.cand_end ? end_pairs : d_off ? (uint64_t)n_cand : (uint64_t)nq * n_cand;
  return EHX_OK;
}

namespace {

// host pointers in, host pointers out, on the space's stream (on_device): ids [| offsets] staged in among.dLists
int among_host_locked(ehx_space* s, size_t nq, const float* queries, uint32_t k, const uint64_t* cand_ids,
                      const uint64_t* cand_off, size_t n_cand, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  const size_t n_off = cand_off ? nq + 1 : 0;
  int rc;
  HostStage& h = s->among.host;
  if ((rc = s->among.dLists.ensure(n_cand + n_off + 1)) || (rc = h.up(s->stream, queries, nq, s->dims, k, false))) return rc;
  uint64_t* d_ids = s->among.dLists.p;
  uint64_t* d_off = cand_off ? d_ids + n_cand : nullptr;
  if (n_cand) HIP_TRY(hipMemcpyAsync(d_ids, cand_ids, n_cand * sizeof(uint64_t), hipMemcpyHostToDevice, s->stream));
  if (d_off) HIP_TRY(hipMemcpyAsync(d_off, cand_off, n_off * sizeof(uint64_t), hipMemcpyHostToDevice, s->stream));
  size_t longest = n_cand;
  if (cand_off) {
    longest = 0;
    for (size_t i = 0; i < nq; ++i) longest = std::max<size_t>(longest, cand_off[i + 1] - cand_off[i]);
  }
  if ((rc = among_locked(s, s->stream, nq, h.q, k, d_ids, d_off, n_cand, longest, h.out.ids, h.out.dist, h.out.cnt))) return rc;
  return h.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
}

}  // namespace

extern "C" {

int ehx_knn_among(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const uint64_t* cand_ids,
                  const uint64_t* cand_off, size_t n_cand, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (int rc = among_check(s, n_queries, k, queries, out_ids, out_dist, out_count)) return rc;
  if (n_cand && !cand_ids) return fail(EHX_EINVAL, "NULL argument");
  if (cand_off) {
    if (cand_off[0] > cand_off[n_queries]) return fail(EHX_EINVAL, "cand_off is not non-decreasing");
    for (size_t i = 0; i < n_queries; ++i)
      if (cand_off[i] > cand_off[i + 1]) return fail(EHX_EINVAL, "cand_off is not non-decreasing at query %zu", i);
    if (cand_off[n_queries] != n_cand)
      return fail(EHX_EINVAL, "cand_off ends at %llu, not at n_cand = %zu", (unsigned long long)cand_off[n_queries], n_cand);
  }
  return search_on_device(s, "ehx_knn_among", kAmongWhy, n_queries, nullptr, [&] {
    return among_host_locked(s, n_queries, queries, k, cand_ids, cand_off, n_cand, out_ids, out_dist, out_count);
  });
}

int ehx_knn_among_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                         const uint64_t* d_cand_ids, const uint64_t* d_cand_off, size_t n_cand, size_t max_list_hint,
                         uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count) {
  if (int rc = among_check(s, n_queries, k, d_queries, d_out_ids, d_out_dist, d_out_count)) return rc;
  if (n_cand && !d_cand_ids) return fail(EHX_EINVAL, "NULL device pointer");
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_knn_among_device", kAmongWhy, n_queries, &st, [&] {
    return among_locked(s, st, n_queries, d_queries, k, d_cand_ids, d_cand_off, n_cand, max_list_hint,
                        d_out_ids, d_out_dist, d_out_count);
  });
}

int ehx_knn_among_keys(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, size_t n_allowed,
                       const char* const* keys, const size_t* klens, uint64_t* out_ids, float* out_dist,
                       uint32_t* out_count, size_t* bad_index) {
  if (int rc = among_check(s, n_queries, k, queries, out_ids, out_dist, out_count)) return rc;
  if (n_allowed && (!keys || !klens)) return fail(EHX_EINVAL, "NULL argument");
  // ONE shared hold for key lookup and search: the answer describes one state of the space
  return search_shared(s, "ehx_knn_among_keys", kAmongWhy, [&]() -> int {
    std::vector<uint64_t> ids;
    if (int rc2 = lookup_keys(s, n_allowed, keys, klens, &ids, bad_index)) return rc2;
    return on_device(s, n_queries, s->stream, [&] {
      return among_host_locked(s, n_queries, queries, k, ids.data(), nullptr, n_allowed, out_ids, out_dist, out_count);
    });
  });
}

}  // extern "C"
