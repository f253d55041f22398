// What the batched entry points (ehx_knn_among*, ehx_range*, ehx_knn_masked*, ehx_knn_by_keys / _by_ids_device) and the flat
// chain share around their kernels: argument checks, the poisoned / dropped / sharded / row-length gates (the entry scaffold
// that runs them, search_shared / on_device, is ehx_internal.h's), key lookup, where the rows are, the result block and the
// staging of a host call, the re-run of a sub-batch by another path, the int8 scan's arguments, the int8 radius scan that
// serves the range search (one pass), and the falling-radius kNN on it (radius_knn: several passes) that serves the bitmap
// search and the large-k route.
#include "ehx_internal.h"

namespace ehx_impl {

int check_not_poisoned(const ehx_space* s) {   // (only a single-copy graph space, x_perm, is ever poisoned: ehx_write.cpp)
  if (s->poisoned.load())
    return fail(EHX_EINTERNAL, "graph space: an in-place overwrite failed half way (rows left in raw order); drop and rebuild it");
  return EHX_OK;
}

int check_space_and_k(const ehx_space* s, uint32_t k, const char* k_name, bool zero_k_ok) {
  if (!s) return fail(EHX_EINVAL, "space is NULL");
  if (k == 0 && !zero_k_ok) return fail(EHX_EINVAL, "%s is 0", k_name);
  if (k > EHX_MAX_K_PAGED) return fail(EHX_EUNSUPPORTED, "%s=%u exceeds %u", k_name, k, EHX_MAX_K_PAGED);
  return EHX_OK;
}

int check_batch_size(size_t nq) {
  if (nq > (1u << 24)) return fail(EHX_EINVAL, "too many queries in one call: %zu", nq);
  return EHX_OK;
}

int check_batch_call(const ehx_space* s, size_t nq, uint32_t k, const char* k_name, bool zero_k_ok, bool ptrs_ok,
                     const char* null_text) {
  int rc = check_space_and_k(s, k, k_name, zero_k_ok);
  if (rc) return rc;
  if (!ptrs_ok) return fail(EHX_EINVAL, "%s", null_text);
  return check_batch_size(nq);
}

int check_unsharded(const ehx_space* s, const char* what, const char* why) {
  if (s->dropped) return fail(EHX_ENOTFOUND, "Not found");
  if (is_parent(s)) return fail(EHX_EUNSUPPORTED, "%s: space '%s' is row-sharded (%s)", what, s->name.c_str(), why);
  return EHX_OK;
}

int check_rows_fit_lds(const ehx_space* s, const char* subject) {
  if (s->ld <= among_max_ld()) return EHX_OK;
  return fail(EHX_EUNSUPPORTED, "%s keeps a prepared query in LDS: rows of %u floats exceed %u", subject, s->ld, among_max_ld());
}

int lookup_keys(ehx_space* s, size_t n, const char* const* keys, const size_t* klens, std::vector<uint64_t>* ids,
                size_t* bad_index) {
  ids->resize(n);
  std::shared_lock<std::shared_mutex> kl(s->kmu);
  for (size_t i = 0; i < n; ++i) {
    if (!keys[i]) return fail(EHX_EINVAL, "NULL argument");
    if (implicit_id(s, keys[i], klens[i], &(*ids)[i])) continue;
    auto it = s->key_to_id.find(std::string(keys[i], klens[i]));
    if (it == s->key_to_id.end()) {
      if (bad_index) *bad_index = i;
      return fail(EHX_ENOTFOUND, "Not found");
    }
    (*ids)[i] = it->second;
  }
  return EHX_OK;
}

RowsView rows_view(const ehx_space* s, uint64_t n_pub) {
  RowsView v;
  v.X = s->rows.dX.p;
  v.inv_norm = s->rows.dInv.p;
  v.n_rows = n_pub;
  v.dims = s->dims;
  v.ld = s->ld;
  v.x_half = (uint32_t)s->x_half;
  v.x_perm = s->x_perm ? 1u : 0u;
  v.metric = s->metric;
  return v;
}

}  // namespace ehx_impl

size_t ResultBlock::bytes(size_t nq, uint32_t k, bool with_total) {
  return nq * k * (sizeof(uint64_t) + sizeof(float)) + nq * sizeof(uint32_t) + (with_total ? nq * sizeof(uint64_t) : 0);
}

ResultBlock ResultBlock::at(unsigned char* p, size_t nq, uint32_t k, bool with_total) {
  const size_t ids_b = nq * k * sizeof(uint64_t), tot_b = with_total ? nq * sizeof(uint64_t) : 0, dist_b = nq * k * sizeof(float);
  return {(uint64_t*)p, (float*)(p + ids_b + tot_b), (uint32_t*)(p + ids_b + tot_b + dist_b),
          with_total ? (uint64_t*)(p + ids_b) : nullptr, nq, k};
}

int ResultBlock::copy_out(hipStream_t st, uint64_t* h_ids, float* h_dist, uint32_t* h_cnt, uint64_t* h_total) const {
  HIP_TRY(hipMemcpyAsync(h_ids, ids, nq * k * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h_dist, dist, nq * k * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h_cnt, cnt, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (h_total && total) HIP_TRY(hipMemcpyAsync(h_total, total, nq * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return EHX_OK;
}

int ResultBlock::copy_block_out(hipStream_t st, void* h_pin) const {
  HIP_TRY(hipMemcpyAsync(h_pin, ids, bytes(nq, k, false), hipMemcpyDeviceToHost, st));
  return EHX_OK;
}

void ResultBlock::unpack(const void* h_pin, uint64_t* h_ids, float* h_dist, uint32_t* h_cnt) const {
  const char* h = (const char*)h_pin;   // (laid out as the device block is; any alignment)
  memcpy(h_ids, h, nq * k * sizeof(uint64_t));
  memcpy(h_dist, h + ((const char*)dist - (const char*)ids), nq * k * sizeof(float));
  memcpy(h_cnt, h + ((const char*)cnt - (const char*)ids), nq * sizeof(uint32_t));
}

int HostStage::up(hipStream_t st, const float* queries, size_t nq, uint32_t dims, uint32_t k, bool with_total, size_t n_tail) {
  int rc;
  if ((rc = dQraw.ensure(nq * dims + n_tail)) || (rc = dOut.ensure(ResultBlock::bytes(nq, k, with_total)))) return rc;
  q = dQraw.p;
  out = ResultBlock::at(dOut.p, nq, k, with_total);
  // (pageable host memory: the runtime stages it before the call returns; the staging buffers are their path's alone and
  // the path's stream orders their reuse)
  HIP_TRY(hipMemcpyAsync(q, queries, nq * dims * sizeof(float), hipMemcpyHostToDevice, st));
  return EHX_OK;
}

int SubsetBufs::rerun(ehx_space* s, hipStream_t st, const float* d_queries, const std::vector<uint32_t>& idx, uint32_t k,
                      const Answer& answer, uint64_t* d_ids, float* d_dist, uint32_t* d_count) {
  const size_t m = idx.size();
  int rc;
  if ((rc = dFbQ.ensure(m * s->dims)) || (rc = dFbIds.ensure(m * k)) || (rc = dFbDist.ensure(m * k)) ||
      (rc = dFbCnt.ensure(m)) || (rc = dFbIdx.ensure(m)))
    return rc;
  // (the index list comes from pageable host memory: the runtime stages it before the call returns)
  HIP_TRY(hipMemcpyAsync(dFbIdx.p, idx.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HIP_TRY(launch_gather_queries(d_queries, dFbIdx.p, (uint32_t)m, s->dims, dFbQ.p, st));
  if ((rc = answer(m, dFbQ.p, dFbIds.p, dFbDist.p, dFbCnt.p))) return rc;
  HIP_TRY(launch_scatter_results(dFbIds.p, dFbDist.p, dFbCnt.p, dFbIdx.p, (uint32_t)m, k, d_ids, d_dist, d_count, st));
  return s->clock.extend(st);
}

namespace ehx_impl {

int i8_scan_args(ehx_space* s, ehx_space::I8Set::Buffers& b, const ScanPlan& p, uint64_t n_pub, ScanArgsI8* a) {
  int rc;
  if ((rc = b.dQ.ensure((size_t)p.q_rows * s->ld))) return rc;
  if ((rc = b.dQ8.ensure(scanq8_bytes(p.q_rows, s->ld8)))) return rc;
  if ((rc = b.dQp8.ensure(p.q_rows))) return rc;
  if ((rc = b.dQuv.ensure(p.q_rows))) return rc;
  if ((rc = b.dThr8.ensure(p.q_rows))) return rc;
  if ((rc = b.dCnt.ensure(8, true))) return rc;   // (the set's own: a batch may run outside the pipeline lock)
  if ((rc = b.dPool.ensure((size_t)p.q_rows * kPoolCap))) return rc;
  if ((rc = b.dI8Ctl.ensure((size_t)p.q_rows * 2 + kSyncWordsI8))) return rc;
  *a = ScanArgsI8();
  a->Q = b.dQ8.p;
  a->X = s->i8.dX8.p;
  a->rowp = s->i8.dRowp8.p;
  a->tilep = s->i8.dTilep8.p;
  a->tileg = s->i8.dTileg8.p;
  a->perm = s->i8.dPerm8.p;
  a->qparams = b.dQp8.p;
  a->thr = b.dThr8.p;
  a->cand = b.dCnt.p;
  a->pool = b.dPool.p;
  a->pool_cnt = b.dI8Ctl.p;
  a->ovf = b.dI8Ctl.p + p.q_rows;
  a->pool_cap = kPoolCap;
  a->n = (uint32_t)n_pub;
  a->ld = s->ld8;
  a->q_tiles = p.q_tiles;
  a->skew = env().i8_skew;
  // (cosine / inner product: B_r is one constant, every margin 0; L2^2 on normalised rows: no tile has a margin worth the
  // epilogue's extra permute and multiply-add per query block — 6.25 M x 128: 1.02 -> 1.07 ms per batch with them)
  a->group_b = s->metric == EHX_METRIC_L2SQ && s->h_margin8.load(std::memory_order_relaxed) > 0 && env().i8_groupb ? 1u : 0u;
  return EHX_OK;
}

int i8_radius_scan(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const float* d_queries, const float* d_radius,
                   const RadiusScan& c, RadiusScanOut* out) {
  const std::vector<TileRange>& passes = *c.passes;
  ehx_space::I8Set& sc = s->i8set[s->i8_next_set.fetch_add(1, std::memory_order_relaxed) & 1u];
  std::lock_guard<std::mutex> l(sc.mu);
  std::vector<ScanPlan> plans;
  for (auto& ps : passes) {
    plans.push_back(plan_scan((uint32_t)nq, ps.second, 1, engine().n_cus));
    if (plans.back().n_chunks > 256) return fail(EHX_EINTERNAL, "scan plan with %u chunks", plans.back().n_chunks);
  }
  const ScanPlan& p = plans.back();   // (q_tiles, q_rows are the same for every pass)
  int rc;
  ScanArgsI8 a;
  if ((rc = i8_scan_args(s, sc.buf, p, n_pub, &a))) return rc;
  a.allow = c.allow;
  a.allow_bits = c.allow_bits;
  a.allow_per_query = c.allow_per_query ? 1u : 0u;
  a.allow_label = c.allow_label ? 1u : 0u;
  {
    std::lock_guard<std::mutex> ql(s->i8_enqueue_mu);   // (this batch's launches go onto the stream as one block)
    if ((rc = wait_searches_in_flight(s, st))) return rc;
    if ((rc = sc.clock.begin(st, BatchClock::kOutOfRing))) return rc;   // (timed, but not a kNN batch: outside the ring)
    // thr[q] = +inf, control words zero; every pass then maps the radius as it stands to its threshold (and its marks)
    HIP_TRY(launch_prep_queries_i8(d_queries, (uint32_t)nq, s->dims, s->ld, s->ld8, p.q_rows, s->metric, sc.buf.dQ.p,
                                   sc.buf.dQ8.p, sc.buf.dQp8.p, sc.buf.dQuv.p, sc.buf.dThr8.p, sc.buf.dI8Ctl.p, st));
    if (c.seed) {   // (the first radii: part of the timed scan phase, which then opens here)
      if ((rc = sc.clock.scan_begin(st)) || (rc = c.seed(a, sc))) return rc;
    }
    for (size_t i = 0; i < passes.size(); ++i) {
      if (i == 0 && c.time_thr && !c.seed && (rc = sc.clock.scan_begin(st))) return rc;
      HIP_TRY(launch_range_thr(d_radius, sc.buf.dQuv.p, s->rows.dMaxSumsq.p, (uint32_t)nq, s->dims, s->metric, sc.buf.dThr8.p,
                               a.ovf, st));
      set_scan_pass(a, plans[i], passes[i].first);
      if (i == 0 && !c.time_thr && !c.seed && (rc = sc.clock.scan_begin(st))) return rc;
      HIP_TRY(launch_flat_scan_i8(a, st));
      if ((rc = c.rerank(i, i + 1 == passes.size(), a, sc))) return rc;
    }
    if ((rc = sc.clock.finish(st))) return rc;
  }
  // the verdict: pool counts, overflow flags and marks, and the caller's words (read once per batch, one wait)
  out->ctl.resize(2 * (size_t)p.q_rows);
  out->word.resize(nq);
  out->pool_cnt = out->ctl.data();
  out->flag = out->ctl.data() + p.q_rows;
  HIP_TRY(hipMemcpyAsync(out->ctl.data(), sc.buf.dI8Ctl.p, out->ctl.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(out->word.data(), c.d_word, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return EHX_OK;
}

int radius_knn(ehx_space* s, hipStream_t st, RadiusKnnBufs& w, uint64_t n_pub, const float* d_queries, const RadiusKnn& c,
               RadiusKnnTally* t) {
  const size_t nq = c.out.nq, cap = std::min(kSideChunk, nq);
  const uint32_t k = c.out.k;
  int rc;
  if ((rc = w.dTop.ensure(cap * kLargeKMax)) || (rc = w.dTopCnt.ensure(cap)) || (rc = w.dRadius.ensure(cap)) ||
      (rc = w.dWork.ensure(cap)))
    return rc;
  size_t q0 = 0, m = 0;    // the batch in hand: its first query, its queries and its rows of the output
  ResultBlock o{};
  auto rerank = [&](uint32_t mode, const ScanArgsI8& a, ehx_space::I8Set& sc) -> int {
    RadiusRerankArgs r = {};
    r.Q = sc.buf.dQ.p;
    r.rows = rows_view(s, n_pub);
    r.radius = w.dRadius.p;
    r.pool = sc.buf.dPool.p;
    r.pool_cnt = a.pool_cnt;
    r.ovf = a.ovf;
    r.top = w.dTop.p;
    r.top_cnt = w.dTopCnt.p;
    r.work = w.dWork.p;
    r.out_ids = o.ids;
    r.out_dist = o.dist;
    r.out_count = o.cnt;
    r.nq = (uint32_t)m;
    r.k = k;
    r.mode = mode;
    HIP_TRY(c.rerank ? c.rerank(r, st) : launch_radius_rerank(r, st));
    return EHX_OK;
  };
  RadiusScan scan;
  scan.passes = &c.passes;
  scan.allow = c.allow;
  scan.allow_bits = c.allow_bits;
  scan.allow_per_query = c.allow_per_query;
  scan.allow_label = c.allow_label;
  scan.time_thr = true;
  scan.d_word = w.dWork.p;   // the rows re-ranked (the seed's sample included)
  if (!c.first_radius) {
    scan.seed = [&](const ScanArgsI8& a, ehx_space::I8Set& sc) -> int {
      // (the control words are zero, the prepared queries in place): the sample -> the first radii, nothing carried
      if (c.fill_pool) {
        if (int r = c.fill_pool(q0, m, sc.buf.dPool.p, a.pool_cnt)) return r;
      } else {
        HIP_TRY(launch_radius_seed(sc.buf.dPool.p, a.pool_cnt, (uint32_t)m, n_pub, c.seed_stride, c.n_sample, st));
      }
      return rerank(kRadiusSeed, a, sc);
    };
  }
  scan.rerank = [&](size_t, bool last, const ScanArgsI8& a, ehx_space::I8Set& sc) -> int {
    if (int r = rerank(last ? kRadiusLast : kRadiusPass, a, sc)) return r;
    return last ? sc.clock.scan_end(st) : (int)EHX_OK;   // (the timed scan phase: the seed and every pass with its re-rank)
  };
  std::vector<uint32_t> todo;
  for (q0 = 0; q0 < nq; q0 += kSideChunk) {
    m = std::min(kSideChunk, nq - q0);
    o = c.out.from(q0, m);
    const float* q = d_queries + q0 * s->dims;
    if (c.first_radius) {   // (and what the seed-mode re-rank does besides: nothing carried, nothing re-ranked yet)
      if ((rc = c.first_radius(m, q, o, w.dRadius.p))) return rc;
      HIP_TRY(hipMemsetAsync(w.dTopCnt.p, 0, m * sizeof(uint32_t), st));
      HIP_TRY(hipMemsetAsync(w.dWork.p, 0, m * sizeof(uint32_t), st));
    }
    RadiusScanOut v;
    if ((rc = i8_radius_scan(s, st, n_pub, m, q, w.dRadius.p, scan, &v))) return rc;
    todo.clear();
    uint64_t n_pairs = 0;
    for (size_t j = 0; j < m; ++j) {
      n_pairs += v.word[j];
      if (v.flag[j]) {
        todo.push_back((uint32_t)j);
        t->overflowed += v.flag[j] == 1u;
      }
    }
    s->n_dist += n_pairs;
    t->batches += 1;
    t->queries += m;
    t->handed += todo.size();
    if (todo.empty()) continue;
    if (c.handed) {
      if ((rc = c.handed(q0, todo, q, o))) return rc;
      continue;
    }
    if ((rc = w.sub.rerun(s, st, q, todo, k, c.exact, o.ids, o.dist, o.cnt))) return rc;
  }
  return EHX_OK;
}

}  // namespace ehx_impl
