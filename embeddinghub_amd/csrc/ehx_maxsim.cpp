// MaxSim search: ehx_maxsim_select_device (candidate entities already on the device, scored), ehx_knn_maxsim_device and
// ehx_knn_maxsim (the candidates from the space's own grouped search, then the scoring).  include/ehx.h has the contract,
// k_maxsim.hip the kernels.
//   open        what both forms start with, under the ONE hold of search_on_device: the checks that read the space, `st`
//               ordered behind the searches in flight (they may still read the scratch, and the index), the ONE snapshot of
//               the row count and the entity column's index for it — rebuilt here if an append or a write left it stale
//               (colindex_ensure, as a search under a stored label column does).
//   select      the query vectors prepared (n_queries * n_tokens of them, as any query is), then ONE launch, a workgroup per
//               query.  A batch of the space's clock, like the MMR selection: a Set that rewrites rows in place, and the next
//               call that writes the scratch from another stream, wait for it.
//   knn_maxsim  the live query vectors — the first T_i of every query — compacted where a count is short (the counts of the
//               device form are read back: the call's one wait besides the grouped search's own), the grouped search's body
//               (grouped_locked, ehx_grouped.cpp) over them at k = fetch_k, per_group = 1 with the stored column read where
//               it lies, its rows turned into labels (maxsim_labels_kernel), then select — on the same snapshot.
// Entry scaffold and host staging are ehx_call.cpp's (search_on_device, HostStage).
#include "ehx_internal.h"

namespace {

constexpr const char* kMaxsimWhy = "MaxSim search over shards is not built yet";

static_assert(EHX_MAXSIM_MAX_TOKENS == kMaxsimMaxTokens && EHX_MAXSIM_MAX_CAND == kMaxsimMaxCand, "the kernel's tables");

// what is decided before the device is looked for, with its codes and in this order (s is not read).  fetch_k: of the kNN
// forms, whose candidate block holds n_cand = n_tokens * fetch_k labels per query; 0: the select form
int maxsim_check(const ehx_space* s, size_t nq, uint32_t n_tokens, uint32_t entity_col, uint64_t n_cand, uint32_t k,
                 uint32_t fetch_k, bool knn, bool ptrs_ok) {
  if (!s) return fail(EHX_EINVAL, "space is NULL");
  if (k == 0) return fail(EHX_EINVAL, "k is 0");
  if (n_tokens == 0) return fail(EHX_EINVAL, "n_tokens is 0");
  if (knn && fetch_k == 0) return fail(EHX_EINVAL, "fetch_k is 0");
  if (!ptrs_ok) return fail(EHX_EINVAL, "NULL argument");
  if (int rc = check_group_col(entity_col)) return rc;
  if (n_tokens > EHX_MAXSIM_MAX_TOKENS) return fail(EHX_EUNSUPPORTED, "n_tokens=%u exceeds %u", n_tokens, EHX_MAXSIM_MAX_TOKENS);
  if (n_cand > EHX_MAXSIM_MAX_CAND)
    return knn ? fail(EHX_EUNSUPPORTED, "n_tokens * fetch_k = %u * %u exceeds %u", n_tokens, fetch_k, EHX_MAXSIM_MAX_CAND)
               : fail(EHX_EUNSUPPORTED, "n_cand=%llu exceeds %u", (unsigned long long)n_cand, EHX_MAXSIM_MAX_CAND);
  if (fetch_k > EHX_MAX_K_GROUPED) return fail(EHX_EUNSUPPORTED, "fetch_k=%u exceeds %u", fetch_k, (unsigned)EHX_MAX_K_GROUPED);
  if (k > EHX_MAXSIM_MAX_CAND) return fail(EHX_EUNSUPPORTED, "k=%u exceeds %u", k, EHX_MAXSIM_MAX_CAND);
  int rc = ehx_init(nullptr, 0);
  if (rc) return rc;
  return check_batch_size(nq * n_tokens);
}

// an unsharded space, locked shared, scratch_mu held, its device current: *n_pub = the call's ONE read of the row count,
// *ix = the index of `col` for it (nullptr: an empty space)
int maxsim_open(ehx_space* s, hipStream_t st, uint32_t col, uint64_t* n_pub, const ehx_space::ColIndex** ix) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  if (s->ld > maxsim_max_ld())
    return fail(EHX_EUNSUPPORTED, "MaxSim search keeps a block of prepared query vectors in LDS: rows of %u floats exceed %u", s->ld,
                maxsim_max_ld());
  s->maxsim.calls += 1;
  if ((rc = s->maxsim.dWork.ensure_zeroed_once(2))) return rc;
  if ((rc = wait_searches_in_flight(s, st))) return rc;
  *n_pub = s->n.load(std::memory_order_acquire);
  *ix = nullptr;
  if (*n_pub == 0) return EHX_OK;
  const uint64_t before = s->colidx[col].builds;
  if ((rc = colindex_ensure(s, st, col, *n_pub, ix))) return rc;
  s->maxsim.rebuilds += s->colidx[col].builds - before;
  return EHX_OK;
}

// ... behind maxsim_open: the scoring of the candidate blocks, enqueued on `st`
int maxsim_select_locked(ehx_space* s, hipStream_t st, uint64_t n_pub, const ehx_space::ColIndex* ix, size_t nq, uint32_t n_tokens,
                         const float* d_tokens, const uint32_t* d_token_count, uint32_t n_cand, const uint32_t* d_cand,
                         const uint32_t* d_cand_count, uint32_t k, const ResultBlock& out) {
  int rc;
  const size_t nv = nq * n_tokens;
  if ((rc = s->maxsim.dQ.ensure(nv * s->ld))) return rc;
  HIP_TRY(launch_prep_queries(d_tokens, (uint32_t)nv, s->dims, s->ld, (uint32_t)nv, s->metric, s->maxsim.dQ.p, st));
  MaxsimArgs a = {};
  a.rows = rows_view(s, n_pub);
  a.Q = s->maxsim.dQ.p;
  a.token_count = d_token_count;
  a.cand = d_cand;
  a.cand_count = d_cand_count;
  if (ix) {
    a.labels = ix->dLabels.p;
    a.start = ix->dStart.p;
    a.perm = ix->dPerm.p;
    a.n_labels = (uint32_t)ix->labels.size();
  }
  a.out_ids = out.ids;
  a.out_score = out.dist;
  a.out_count = out.cnt;
  a.work = s->maxsim.dWork.p;
  a.nq = (uint32_t)nq;
  a.n_tokens = n_tokens;
  a.n_cand = n_cand;
  a.k = k;
  if ((rc = s->clock.begin(st, BatchClock::kOutOfRing)) || (rc = s->clock.scan_begin(st))) return rc;
  HIP_TRY(launch_maxsim_score(a, st));
  if ((rc = s->clock.scan_end(st))) return rc;
  return s->clock.finish(st);
}

// ... scratch_mu held.  h_count: the token counts in host memory where the caller has them there (d_token_count then holds
// the same on the device); both nullptr: every query has n_tokens vectors
int knn_maxsim_locked(ehx_space* s, hipStream_t st, size_t nq, uint32_t n_tokens, const float* d_tokens,
                      const uint32_t* h_count, const uint32_t* d_token_count, uint32_t col, uint32_t k, uint32_t fetch_k,
                      const ResultBlock& out) {
  int rc;
  uint64_t n_pub;
  const ehx_space::ColIndex* ix;
  if ((rc = grouped_check_ld(s))) return rc;   // (before anything is enqueued)
  if ((rc = maxsim_open(s, st, col, &n_pub, &ix))) return rc;
  ehx_space::Maxsim& w = s->maxsim;
  std::vector<uint32_t> count_read;
  if (d_token_count && !h_count) {
    count_read.resize(nq);
    HIP_TRY(hipMemcpyAsync(count_read.data(), d_token_count, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    h_count = count_read.data();
  }
  // the live vectors: the first T_i of query i, in query order; compacted only where some count is short
  size_t m = nq * n_tokens;
  const float* d_live = d_tokens;
  const uint32_t* d_base = nullptr;
  if (h_count) {
    std::vector<uint32_t> idx, base(nq);
    for (size_t i = 0; i < nq; ++i) {
      base[i] = (uint32_t)idx.size();
      for (uint32_t t = 0; t < std::min(h_count[i], n_tokens); ++t) idx.push_back((uint32_t)(i * n_tokens + t));
    }
    if (idx.size() < m) {
      m = idx.size();
      if ((rc = w.dIdx.ensure(m + nq)) || (rc = w.dLive.ensure(std::max<size_t>(m, 1) * s->dims))) return rc;
      // (pageable host memory: the runtime stages it before the call returns)
      if (m) HIP_TRY(hipMemcpyAsync(w.dIdx.p, idx.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(w.dIdx.p + m, base.data(), nq * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      if (m) HIP_TRY(launch_gather_queries(d_tokens, w.dIdx.p, (uint32_t)m, s->dims, w.dLive.p, st));
      d_live = w.dLive.p;
      d_base = w.dIdx.p + m;
    }
  }
  const uint32_t n_cand = n_tokens * fetch_k;
  if ((rc = w.dFetch.ensure(ResultBlock::bytes(std::max<size_t>(m, 1), fetch_k, false))) || (rc = w.dCand.ensure(nq * n_cand + nq)))
    return rc;
  const ResultBlock got = ResultBlock::at(w.dFetch.p, std::max<size_t>(m, 1), fetch_k, false);
  const uint32_t* d_col = nullptr;
  const bool searched = n_pub && m;
  if (searched) {
    if ((rc = column_as_groups(s, st, col, n_pub, &d_col))) return rc;
    if ((rc = grouped_locked(s, st, n_pub, m, d_live, fetch_k, 1, d_col, n_pub, got))) return rc;
  }
  uint32_t* d_cand = w.dCand.p;
  uint32_t* d_cand_count = d_cand + nq * n_cand;
  HIP_TRY(launch_maxsim_labels(got.ids, searched ? got.cnt : nullptr, d_col, n_pub, d_base, d_token_count, (uint32_t)nq, n_tokens,
                               fetch_k, d_cand, d_cand_count, st));
  return maxsim_select_locked(s, st, n_pub, ix, nq, n_tokens, d_tokens, d_token_count, n_cand, d_cand, d_cand_count, k, out);
}

}  // namespace

extern "C" {

int ehx_maxsim_select_device(ehx_space* s, void* stream, size_t n_queries, uint32_t n_tokens, const float* d_tokens,
                             const uint32_t* d_token_count, uint32_t entity_col, uint32_t n_cand, const uint32_t* d_cand,
                             const uint32_t* d_cand_count, uint32_t k, uint64_t* d_out_ids, float* d_out_score,
                             uint32_t* d_out_count) {
  if (int rc = maxsim_check(s, n_queries, n_tokens, entity_col, n_cand, k, 0, false,
                            d_out_ids && d_out_score && d_out_count && (!n_queries || (d_tokens && d_cand && d_cand_count))))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_maxsim_select_device", kMaxsimWhy, n_queries, &st, [&]() -> int {
    uint64_t n_pub;
    const ehx_space::ColIndex* ix;
    if (int rc = maxsim_open(s, st, entity_col, &n_pub, &ix)) return rc;
    return maxsim_select_locked(s, st, n_pub, ix, n_queries, n_tokens, d_tokens, d_token_count, n_cand, d_cand, d_cand_count, k,
                                ResultBlock{d_out_ids, d_out_score, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_knn_maxsim_device(ehx_space* s, void* stream, size_t n_queries, uint32_t n_tokens, const float* d_tokens,
                          const uint32_t* d_token_count, uint32_t entity_col, uint32_t k, uint32_t fetch_k, uint64_t* d_out_ids,
                          float* d_out_score, uint32_t* d_out_count) {
  if (int rc = maxsim_check(s, n_queries, n_tokens, entity_col, (uint64_t)n_tokens * fetch_k, k, fetch_k, true,
                            d_out_ids && d_out_score && d_out_count && (!n_queries || d_tokens)))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_knn_maxsim_device", kMaxsimWhy, n_queries, &st, [&] {
    return knn_maxsim_locked(s, st, n_queries, n_tokens, d_tokens, nullptr, d_token_count, entity_col, k, fetch_k,
                             ResultBlock{d_out_ids, d_out_score, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_knn_maxsim(ehx_space* s, size_t n_queries, uint32_t n_tokens, const float* tokens, const uint32_t* token_count,
                   uint32_t entity_col, uint32_t k, uint32_t fetch_k, uint64_t* out_ids, float* out_score, uint32_t* out_count) {
  if (int rc = maxsim_check(s, n_queries, n_tokens, entity_col, (uint64_t)n_tokens * fetch_k, k, fetch_k, true,
                            out_ids && out_score && out_count && (!n_queries || tokens)))
    return rc;
  return search_on_device(s, "ehx_knn_maxsim", kMaxsimWhy, n_queries, nullptr, [&]() -> int {
    HostStage& h = s->maxsim.host;
    int rc;
    // (a query's vectors are one staged "query" of n_tokens * dims floats: the same bytes)
    if ((rc = h.up(s->stream, tokens, n_queries, n_tokens * s->dims, k, false))) return rc;
    const uint32_t* d_count = nullptr;
    if (token_count) {
      if ((rc = s->maxsim.dTok.ensure(n_queries))) return rc;
      // (the last call's kernels, on whatever stream, may still read the counts; pageable host memory: staged before the
      // call returns)
      if ((rc = wait_searches_in_flight(s, s->stream))) return rc;
      HIP_TRY(hipMemcpyAsync(s->maxsim.dTok.p, token_count, n_queries * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
      d_count = s->maxsim.dTok.p;
    }
    if ((rc = knn_maxsim_locked(s, s->stream, n_queries, n_tokens, h.q, token_count, d_count, entity_col, k, fetch_k, h.out)))
      return rc;
    return h.out.copy_out(s->stream, out_ids, out_score, out_count, nullptr);
  });
}

}  // extern "C"
