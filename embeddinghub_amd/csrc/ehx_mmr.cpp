// MMR search: ehx_mmr_select_device (candidate lists already on the device, re-ranked), ehx_knn_mmr_device and ehx_knn_mmr
// (the space's own kNN at fetch_k, then the selection).  include/ehx.h has the contract, k_mmr.hip the kernel.
//   select   ONE launch, a workgroup per query, on the call's snapshot of the row count.  It is a batch of the space's clock,
//            like a list-route batch of the grouped kNN: a Set that rewrites rows in place, and the next call that writes
//            the candidate block from another stream, wait for it (wait_searches_in_flight).
//   knn_mmr  knn_device_locked at k = fetch_k into the space's candidate block (ehx_space::Mmr), whatever route serves it —
//            the engine chain, the large-k route for 48 < fetch_k <= 256, a graph space's walk — then select, under the one
//            shared hold of search_on_device.  A flat space's two steps answer for ONE snapshot of the row count; a graph
//            space's walk takes its own, so the selection's is read behind it: never smaller, every id the walk returned is
//            a row of it.
// Entry scaffold and host staging are ehx_call.cpp's (search_on_device, HostStage).
#include "ehx_internal.h"

namespace {

constexpr const char* kMmrWhy = "MMR search over shards is not built yet";

static_assert(EHX_MMR_MAX_FETCH == kMmrMaxFetch, "the kernel gives every candidate a thread");
static_assert(EHX_MMR_MAX_FETCH <= kLargeKScanMax, "fetch_k is a k the large-k route serves at batch rate");

// what is decided before the device is looked for, with its codes and in this order (s is not read)
int mmr_check(const ehx_space* s, size_t nq, uint32_t k, uint32_t fetch_k, float lambda, bool ptrs_ok) {
  if (!s) return fail(EHX_EINVAL, "space is NULL");
  if (k == 0) return fail(EHX_EINVAL, "k is 0");
  if (k > fetch_k) return fail(EHX_EINVAL, "k=%u exceeds fetch_k=%u", k, fetch_k);
  if (!(lambda >= 0.0f && lambda <= 1.0f)) return fail(EHX_EINVAL, "lambda=%g is not in [0, 1]", (double)lambda);
  if (!ptrs_ok) return fail(EHX_EINVAL, "NULL argument");
  int rc = ehx_init(nullptr, 0);
  if (rc) return rc;
  if (fetch_k > EHX_MMR_MAX_FETCH) return fail(EHX_EUNSUPPORTED, "fetch_k=%u exceeds %u", fetch_k, EHX_MMR_MAX_FETCH);
  return check_batch_size(nq);
}

// an unsharded space, locked shared, its device current: the selection over the prefix of n_pub rows, enqueued on `st`
int mmr_select_locked(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, uint32_t fetch_k, const uint64_t* d_cand_ids,
                      const float* d_cand_dist, const uint32_t* d_cand_count, uint32_t k, float lambda, const ResultBlock& out) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  if (s->ld > mmr_max_ld())
    return fail(EHX_EUNSUPPORTED, "MMR search keeps a prepared pivot in LDS: rows of %u floats exceed %u", s->ld, mmr_max_ld());
  MmrArgs a = {};
  a.rows = rows_view(s, n_pub);
  a.cand_ids = d_cand_ids;
  a.cand_dist = d_cand_dist;
  a.cand_count = d_cand_count;
  a.out_ids = out.ids;
  a.out_dist = out.dist;
  a.out_count = out.cnt;
  a.nq = (uint32_t)nq;
  a.fetch_k = fetch_k;
  a.k = k;
  a.lambda = lambda;
  if ((rc = s->clock.begin(st, BatchClock::kOutOfRing)) || (rc = s->clock.scan_begin(st))) return rc;
  HIP_TRY(launch_mmr_select(a, st));
  if ((rc = s->clock.scan_end(st))) return rc;
  return s->clock.finish(st);
}

// ... scratch_mu held: the candidates of d_queries at fetch_k into the space's block, then the selection
int knn_mmr_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, uint32_t fetch_k, float lambda,
                   const ResultBlock& out) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  if ((rc = s->mmr.dCand.ensure(ResultBlock::bytes(nq, fetch_k, false)))) return rc;
  const ResultBlock cand = ResultBlock::at(s->mmr.dCand.p, nq, fetch_k, false);
  // (the last call's selection, on whatever stream it was given, may still read the block)
  if ((rc = wait_searches_in_flight(s, st))) return rc;
  uint64_t n_pub = s->n.load(std::memory_order_acquire);   // the ONE read of the row count of a flat space's call
  if (n_pub == 0) {   // (an empty space: no candidates; the selection writes the counts and the sentinels)
    HIP_TRY(hipMemsetAsync(cand.cnt, 0, nq * sizeof(uint32_t), st));
  } else {
    if ((rc = knn_device_locked(s, st, nq, d_queries, fetch_k, cand.ids, cand.dist, cand.cnt, n_pub))) return rc;
    if (s->params.mode == EHX_MODE_GRAPH) n_pub = s->n.load(std::memory_order_acquire);   // (behind the walk's own)
  }
  return mmr_select_locked(s, st, n_pub, nq, fetch_k, cand.ids, cand.dist, cand.cnt, k, lambda, out);
}

}  // namespace

extern "C" {

int ehx_mmr_select_device(ehx_space* s, void* stream, size_t n_queries, uint32_t fetch_k, const uint64_t* d_cand_ids,
                          const float* d_cand_dist, const uint32_t* d_cand_count, uint32_t k, float lambda,
                          uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count) {
  if (int rc = mmr_check(s, n_queries, k, fetch_k, lambda,
                         d_out_ids && d_out_dist && d_out_count && (!n_queries || (d_cand_ids && d_cand_dist && d_cand_count))))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_mmr_select_device", kMmrWhy, n_queries, &st, [&] {
    return mmr_select_locked(s, st, s->n.load(std::memory_order_acquire), n_queries, fetch_k, d_cand_ids, d_cand_dist,
                             d_cand_count, k, lambda, ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_knn_mmr_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k, uint32_t fetch_k,
                       float lambda, uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count) {
  if (int rc = mmr_check(s, n_queries, k, fetch_k, lambda, d_out_ids && d_out_dist && d_out_count && (!n_queries || d_queries)))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_knn_mmr_device", kMmrWhy, n_queries, &st, [&] {
    return knn_mmr_locked(s, st, n_queries, d_queries, k, fetch_k, lambda,
                          ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_knn_mmr(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint32_t fetch_k, float lambda,
                uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (int rc = mmr_check(s, n_queries, k, fetch_k, lambda, out_ids && out_dist && out_count && (!n_queries || queries)))
    return rc;
  return search_on_device(s, "ehx_knn_mmr", kMmrWhy, n_queries, nullptr, [&]() -> int {
    HostStage& h = s->mmr.host;
    int rc;
    if ((rc = h.up(s->stream, queries, n_queries, s->dims, k, false))) return rc;
    if ((rc = knn_mmr_locked(s, s->stream, n_queries, h.q, k, fetch_k, lambda, h.out))) return rc;
    return h.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
  });
}

}  // extern "C"
