// Exact range search: ehx_range (host pointers), ehx_range_keys, ehx_range_device.  Every row whose canonical distance is
// <= the query's radius, ordered by (distance, id), the first max_results written, all of them counted (k_range.hip).
//   int8 path   flat spaces whose first engine is the int8 filter: ONE pass of flat_scan_i8_kernel over all tiles under a
//               threshold mapped from the radius (no sample pass, no cascade), the survivors re-ranked in the oracle's
//               arithmetic and cut at the radius; queries the bound does not serve or whose pool overflowed go on to
//   exact path  every space: the canonical distance of every row (a graph space answers from its stored rows, its graph is
//               not walked); a query with more than kPoolCap members is answered by the exact kNN pipeline at k = max_results.
#include "ehx_internal.h"

namespace {

constexpr size_t kRangeChunk = 2048;          // queries per device batch: their pools are 64 MiB
constexpr uint32_t kRangeGridTarget = 4096;   // workgroups the exact kernel's launch aims for (16 per CU): chosen, not measured

typedef ResultBlock RangeOut;   // the caller's arrays, or a host call's staging block; total may be nullptr

int range_check(const ehx_space* s, size_t nq, uint32_t max_results, const void* q, const void* radius, const void* o_ids,
                const void* o_dist, const void* o_cnt) {
  int rc = ehx_init(nullptr, 0);   // (no device: EHX_ENODEVICE, whatever else is wrong with the call)
  if (rc) return rc;
  return check_batch_call(s, nq, max_results, "max_results", false, o_ids && o_dist && o_cnt && (!nq || (q && radius)));
}
int range_unsharded(const ehx_space* s, const char* what) {
  return check_unsharded(s, what, "range search over shards is not built yet");
}

// Queries whose pool overflowed (idx: their indices in the batch) have more than kPoolCap >= max_results members: their
// answer is the top max_results of the whole space, from the exact kNN pipeline (a graph space: the exact kNN among ALL
// its row ids, its graph is not walked).  The totals are already written.
int range_overflow(ehx_space* s, hipStream_t st, uint64_t n_pub, const float* d_queries, const std::vector<uint32_t>& idx,
                   uint32_t k, const RangeOut& o) {
  SubsetBufs& sub = s->range.sub;   // (its own: knn_device_locked's stages use the engine chain's)
  int rc;
  if ((rc = sub.gather(d_queries, idx, s->dims, k, st))) return rc;
  if (s->params.mode == EHX_MODE_GRAPH) {
    if ((rc = s->range.dIota.ensure(n_pub))) return rc;
    HIP_TRY(launch_range_iota(s->range.dIota.p, n_pub, st));
    rc = among_locked(s, st, sub.m, sub.dFbQ.p, k, s->range.dIota.p, nullptr, n_pub, 0, sub.dFbIds.p, sub.dFbDist.p, sub.dFbCnt.p);
  } else {
    rc = knn_device_locked(s, st, sub.m, sub.dFbQ.p, k, sub.dFbIds.p, sub.dFbDist.p, sub.dFbCnt.p, n_pub);
  }
  if (rc) return rc;
  if ((rc = sub.scatter(o.ids, o.dist, o.cnt, st))) return rc;
  return s->clock.extend(st);   // (the scatter belongs to the last batch: writers wait for it too)
}

// The exact path for the queries sel[0, m) of a batch of nq (sel == nullptr: all of them); counted[j] != 0: query sel[j]'s
// overflow is in the counters already.
int range_exact_stage(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const float* d_queries, const float* d_radius,
                      const std::vector<uint32_t>* sel, const std::vector<uint8_t>* counted, uint32_t max_results,
                      const RangeOut& o) {
  const size_t m = sel ? sel->size() : nq;
  int rc;
  if ((rc = s->scr.dQ.ensure(nq * s->ld))) return rc;
  if ((rc = s->range.dPool.ensure(m * kPoolCap))) return rc;
  if ((rc = s->range.dCtl.ensure(m))) return rc;
  if (sel && (rc = s->range.dSel.ensure(m))) return rc;
  // (searches on other streams have read and written this scratch; this batch's fence makes a Set that rewrites rows in
  // place wait for it in turn)
  if ((rc = wait_searches_in_flight(s, st))) return rc;
  if ((rc = s->clock.begin(st, BatchClock::kOutOfRing))) return rc;
  HIP_TRY(hipMemsetAsync(s->range.dCtl.p, 0, m * sizeof(uint32_t), st));
  if (sel) HIP_TRY(hipMemcpyAsync(s->range.dSel.p, sel->data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HIP_TRY(launch_prep_queries(d_queries, (uint32_t)nq, s->dims, s->ld, (uint32_t)nq, s->metric, s->scr.dQ.p, st));
  RangeArgs a = {};
  a.Q = s->scr.dQ.p;
  a.rows = rows_view(s, n_pub);
  a.radius = d_radius;
  a.sel = sel ? s->range.dSel.p : nullptr;
  a.pool = s->range.dPool.p;
  a.pool_cnt = s->range.dCtl.p;
  const uint32_t step = range_step_rows(a);
  a.n_blocks = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, (n_pub + step - 1) / step),
                                            std::max<uint64_t>(1, kRangeGridTarget / m));
  if ((rc = s->clock.scan_begin(st))) return rc;
  HIP_TRY(launch_range_exact(a, (uint32_t)m, st));
  HIP_TRY(launch_range_emit(s->range.dPool.p, s->range.dCtl.p, a.sel, (uint32_t)m, max_results, o.ids, o.dist, o.cnt, o.total,
                            st));
  if ((rc = s->clock.scan_end(st)) || (rc = s->clock.finish(st))) return rc;
  // the verdict: which pools overflowed (one copy, one wait)
  std::vector<uint32_t> cnt(m);
  HIP_TRY(hipMemcpyAsync(cnt.data(), s->range.dCtl.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  s->n_dist += (uint64_t)m * n_pub;
  std::vector<uint32_t> over;
  uint64_t n_trunc = 0, n_over_new = 0;
  for (size_t j = 0; j < m; ++j) {
    n_trunc += cnt[j] > max_results;
    if (cnt[j] > kPoolCap) {
      over.push_back(sel ? (*sel)[j] : (uint32_t)j);
      n_over_new += !(counted && (*counted)[j]);
    }
  }
  s->range_ctr[1] += m;
  s->range_ctr[2] += n_over_new;
  s->range_ctr[3] += n_trunc;
  s->n_queries += m - over.size();   // (the kNN pipeline counts the queries it answers)
  if (over.empty()) return EHX_OK;
  return range_overflow(s, st, n_pub, d_queries, over, max_results, o);
}

// The int8 path for a batch of nq queries, in one of the space's int8 scratch sets: *todo = the queries it leaves to the
// exact path (the bound does not serve them, or their pool overflowed: (*counted)[j] = 1 for the latter).
int range_i8_stage(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const float* d_queries, const float* d_radius,
                   uint32_t max_results, const RangeOut& o, std::vector<uint32_t>* todo, std::vector<uint8_t>* counted) {
  Engine& E = engine();
  const int set = (int)(s->i8_next_set.fetch_add(1, std::memory_order_relaxed) & 1u);
  ehx_space::I8Set& sc = s->i8set[set];
  std::lock_guard<std::mutex> l(sc.mu);
  const uint32_t n_tiles = (uint32_t)((n_pub + kTileRows16 - 1) / kTileRows16);
  const ScanPlan p = plan_scan((uint32_t)nq, n_tiles, 1, E.n_cus);   // ONE pass over all tiles
  if (p.n_chunks > 256) return fail(EHX_EINTERNAL, "scan plan with %u chunks", p.n_chunks);
  int rc;
  ScanArgsI8 a;
  if ((rc = i8_scan_args(s, sc.buf, p, n_pub, &a))) return rc;
  if ((rc = s->range.dCtl.ensure(p.q_rows))) return rc;
  {
    std::lock_guard<std::mutex> ql(s->i8_enqueue_mu);   // (this batch's launches go onto the stream as one block)
    if ((rc = wait_searches_in_flight(s, st))) return rc;
    if ((rc = sc.clock.begin(st, BatchClock::kOutOfRing))) return rc;   // (timed, but not a kNN batch: outside the ring)
    // thr[q] = +inf, control words zero ...
    HIP_TRY(launch_prep_queries_i8(d_queries, (uint32_t)nq, s->dims, s->ld, s->ld8, p.q_rows, s->metric, sc.buf.dQ.p,
                                   sc.buf.dQ8.p, sc.buf.dQp8.p, sc.buf.dQuv.p, sc.buf.dThr8.p, sc.buf.dI8Ctl.p, st));
    // ... then the radius' threshold, and the marks of the queries the bound does not serve
    HIP_TRY(launch_range_thr(d_radius, sc.buf.dQuv.p, s->rows.dMaxSumsq.p, (uint32_t)nq, s->dims, s->metric, sc.buf.dThr8.p, a.ovf,
                             st));
    set_scan_pass(a, p, 0);   // ONE pass over all tiles
    if ((rc = sc.clock.scan_begin(st))) return rc;
    HIP_TRY(launch_flat_scan_i8(a, st));
    if ((rc = sc.clock.scan_end(st))) return rc;
    RangeRerankArgs r = {};
    r.Q = sc.buf.dQ.p;
    r.rows = rows_view(s, n_pub);
    r.radius = d_radius;
    r.pool = sc.buf.dPool.p;
    r.pool_cnt = a.pool_cnt;
    r.ovf = a.ovf;
    r.kept = s->range.dCtl.p;
    r.out_ids = o.ids;
    r.out_dist = o.dist;
    r.out_count = o.cnt;
    r.out_total = o.total;
    r.nq = (uint32_t)nq;
    r.max_results = max_results;
    HIP_TRY(launch_range_rerank(r, st));
    if ((rc = sc.clock.finish(st))) return rc;
  }
  // the verdict: overflow flags, marks and what the re-rank kept (read once per batch, one wait)
  std::vector<uint32_t> ctl(2 * (size_t)p.q_rows), kept(nq);
  HIP_TRY(hipMemcpyAsync(ctl.data(), sc.buf.dI8Ctl.p, ctl.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(kept.data(), s->range.dCtl.p, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  todo->clear();
  counted->clear();
  uint64_t n_pairs = 0, n_trunc = 0, n_over = 0;
  for (size_t q = 0; q < nq; ++q) {
    const uint32_t flag = ctl[p.q_rows + q];
    if (flag) {
      todo->push_back((uint32_t)q);
      counted->push_back(flag == 1u);
      n_over += flag == 1u;
    } else {
      n_pairs += ctl[q];
      n_trunc += kept[q] > max_results;
    }
  }
  s->n_dist += n_pairs;
  s->n_queries += nq - todo->size();
  s->range_ctr[0] += nq - todo->size();
  s->range_ctr[2] += n_over;
  s->range_ctr[3] += n_trunc;
  return EHX_OK;
}

// an unsharded space, locked shared, scratch_mu held, its device current; everything is enqueued on `st`
int range_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, const float* d_radius, uint32_t max_results,
                 const RangeOut& out) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  if (s->ld > among_max_ld())   // (before anything is enqueued)
    return fail(EHX_EUNSUPPORTED, "range search keeps a prepared query in LDS: rows of %u floats exceed %u", s->ld,
                among_max_ld());
  // the ONE read of the row count: every stage of the call answers for the same prefix
  const uint64_t n_pub = s->n.load(std::memory_order_acquire);
  const bool i8 = resolve_engine(s, n_pub) == EHX_ENGINE_I8 && s->ld <= range_rerank_max_ld();
  std::vector<uint32_t> todo;
  std::vector<uint8_t> counted;
  for (size_t q0 = 0; q0 < nq; q0 += kRangeChunk) {
    const size_t m = std::min(kRangeChunk, nq - q0);
    const float* q = d_queries + q0 * s->dims;
    const float* r = d_radius + q0;
    const RangeOut o = out.from(q0, m);
    if (i8) {
      if ((rc = range_i8_stage(s, st, n_pub, m, q, r, max_results, o, &todo, &counted))) return rc;
      if (todo.empty()) continue;
      if ((rc = range_exact_stage(s, st, n_pub, m, q, r, &todo, &counted, max_results, o))) return rc;
    } else if ((rc = range_exact_stage(s, st, n_pub, m, q, r, nullptr, nullptr, max_results, o))) {
      return rc;
    }
  }
  return EHX_OK;
}

// host pointers in, host pointers out, on the space's stream (scratch_mu held): queries | radii staged in range.dQraw
int range_host_locked(ehx_space* s, size_t nq, const float* queries, const float* radius, uint32_t k, uint64_t* out_ids,
                      float* out_dist, uint32_t* out_count, uint64_t* out_total) {
  int rc;
  HIP_TRY(hipSetDevice(s->device));
  if ((rc = s->range.dQraw.ensure(nq * s->dims + nq))) return rc;
  if ((rc = s->range.dOut.ensure(ResultBlock::bytes(nq, k, true)))) return rc;
  float* d_q = s->range.dQraw.p;
  float* d_r = d_q + nq * s->dims;
  const RangeOut o = ResultBlock::at(s->range.dOut.p, nq, k, true);
  DrainUnlessOk drain{s->stream};
  // (pageable host memory: the runtime stages it before the call returns; the staging buffers are this path's alone and
  // the space's stream orders their reuse)
  HIP_TRY(hipMemcpyAsync(d_q, queries, nq * s->dims * sizeof(float), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(d_r, radius, nq * sizeof(float), hipMemcpyHostToDevice, s->stream));
  if ((rc = range_locked(s, s->stream, nq, d_q, d_r, k, o))) return rc;
  return drain.done(o.copy_out(s->stream, out_ids, out_dist, out_count, out_total));
}

}  // namespace

extern "C" {

int ehx_range(ehx_space* s, size_t n_queries, const float* queries, const float* radius, uint32_t max_results,
              uint64_t* out_ids, float* out_dist, uint32_t* out_count, uint64_t* out_total) {
  int rc = range_check(s, n_queries, max_results, queries, radius, out_ids, out_dist, out_count);
  if (rc) return rc;
  yield_to_writer(s);
  std::shared_lock<std::shared_mutex> rl(s->mu);
  if ((rc = range_unsharded(s, "ehx_range"))) return rc;
  if (n_queries == 0) return EHX_OK;
  std::lock_guard<std::mutex> sl(s->scratch_mu);
  return range_host_locked(s, n_queries, queries, radius, max_results, out_ids, out_dist, out_count, out_total);
}

int ehx_range_keys(ehx_space* s, size_t n_queries, const float* queries, const float* radius, uint32_t max_results,
                   uint64_t* out_ids, float* out_dist, uint32_t* out_count, uint64_t* out_total, char* key_arena,
                   size_t arena_cap, uint64_t* key_off) {
  int rc = range_check(s, n_queries, max_results, queries, radius, out_ids, out_dist, out_count);
  if (rc) return rc;
  if (!key_off || (!key_arena && arena_cap)) return fail(EHX_EINVAL, "NULL argument");
  yield_to_writer(s);
  // ONE shared hold for the search and the key lookup: the keys are those of the rows the search saw
  std::shared_lock<std::shared_mutex> rl(s->mu);
  if ((rc = range_unsharded(s, "ehx_range_keys"))) return rc;
  if (n_queries) {
    std::lock_guard<std::mutex> sl(s->scratch_mu);
    if ((rc = range_host_locked(s, n_queries, queries, radius, max_results, out_ids, out_dist, out_count, out_total)))
      return rc;
  }
  return fill_key_arena(s, n_queries, max_results, out_ids, out_count, key_arena, arena_cap, key_off);
}

int ehx_range_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, const float* d_radius,
                     uint32_t max_results, uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count,
                     uint64_t* d_out_total) {
  int rc = range_check(s, n_queries, max_results, d_queries, d_radius, d_out_ids, d_out_dist, d_out_count);
  if (rc) return rc;
  yield_to_writer(s);
  std::shared_lock<std::shared_mutex> rl(s->mu);
  if ((rc = range_unsharded(s, "ehx_range_device"))) return rc;
  if (n_queries == 0) return EHX_OK;
  std::lock_guard<std::mutex> sl(s->scratch_mu);
  HIP_TRY(hipSetDevice(s->device));
  DrainUnlessOk drain{(hipStream_t)stream};
  return drain.done(range_locked(s, (hipStream_t)stream, n_queries, d_queries, d_radius, max_results,
                                 RangeOut{d_out_ids, d_out_dist, d_out_count, d_out_total, n_queries, max_results}));
}

// test hook, not part of the ABI: queries answered by the int8 path, by the exact path, pool overflows, truncated answers
void ehx_test_range_counters(ehx_space* s, uint64_t out[4]) {
  for (int i = 0; i < 4; ++i) out[i] = s ? s->range_ctr[i].load(std::memory_order_relaxed) : 0;
}

}  // extern "C"
