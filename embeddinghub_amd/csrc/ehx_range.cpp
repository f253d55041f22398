// Exact range search: ehx_range (host pointers), ehx_range_keys, ehx_range_device.  Every row whose canonical distance is
// <= the query's radius, ordered by (distance, id), the first max_results written, all of them counted (k_range.hip).
//   int8 path   flat spaces whose first engine is the int8 filter: the radius scan (i8_radius_scan, ehx_call.cpp) with ONE
//               pass over all tiles under a threshold mapped from the radius (no sample pass, no cascade), the survivors
//               re-ranked in the oracle's arithmetic and cut at the radius; queries the bound does not serve or whose pool
//               overflowed go on to
//   exact path  every space: the canonical distance of every row (a graph space answers from its stored rows, its graph is
//               not walked); a query with more than kPoolCap members is answered by the exact kNN pipeline at k = max_results.
// The int8 path's stage (range_i8_stage) also serves the range search under row bitmaps (ehx_rangem.cpp), which hands it the
// bitmaps for the scan's flush.
// Entry scaffold, host staging, sub-batch re-runs: ehx_call.cpp's (search_shared / on_device, HostStage, SubsetBufs::rerun).
#include "ehx_internal.h"

namespace {

int range_check(const ehx_space* s, size_t nq, uint32_t max_results, const void* q, const void* radius, const void* o_ids,
                const void* o_dist, const void* o_cnt) {
  int rc = ehx_init(nullptr, 0);   // (no device: EHX_ENODEVICE, whatever else is wrong with the call)
  if (rc) return rc;
  return check_batch_call(s, nq, max_results, "max_results", false, o_ids && o_dist && o_cnt && (!nq || (q && radius)));
}
constexpr const char* kRangeWhy = "range search over shards is not built yet";

// Queries whose pool overflowed (idx: their indices in the batch) have more than kPoolCap >= max_results members: their
// answer is the top max_results of the whole space, from the exact kNN pipeline (a graph space: the exact kNN among ALL
// its row ids, its graph is not walked).  The totals are already written.
int range_overflow(ehx_space* s, hipStream_t st, uint64_t n_pub, const float* d_queries, const std::vector<uint32_t>& idx,
                   uint32_t k, const ResultBlock& o) {
  // (its own sub-batch: knn_device_locked's stages use the engine chain's)
  return s->range.sub.rerun(s, st, d_queries, idx, k, [&](size_t m, const float* q, uint64_t* ids, float* dist, uint32_t* cnt) -> int {
    if (s->params.mode != EHX_MODE_GRAPH) return knn_device_locked(s, st, m, q, k, ids, dist, cnt, n_pub);
    int rc = s->range.dIota.ensure(n_pub);
    if (rc) return rc;
    HIP_TRY(launch_range_iota(s->range.dIota.p, n_pub, st));
    return among_locked(s, st, m, q, k, s->range.dIota.p, nullptr, n_pub, 0, ids, dist, cnt);
  }, o.ids, o.dist, o.cnt);
}

// The exact path for the queries sel[0, m) of a batch of nq (sel == nullptr: all of them); counted[j] != 0: query sel[j]'s
// overflow is in the counters already.
int range_exact_stage(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const float* d_queries, const float* d_radius,
                      const std::vector<uint32_t>* sel, const std::vector<uint8_t>* counted, uint32_t max_results,
                      const ResultBlock& o) {
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

}  // namespace

namespace ehx_impl {

// The int8 path for a batch of nq queries — ONE pass of the radius scan over all tiles, the radius fixed: out->todo = the
// queries it leaves to the exact path (the bound does not serve them, or their pool overflowed: out->counted[j] = 1 for the
// latter).  allow (the filtered range search, ehx_rangem.cpp): the bitmaps of the scan's flush, and the tiles below their
// n_bits — the only ones that hold a member.  The caller adds the verdict's figures to its own counters.
int range_i8_stage(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const float* d_queries, const float* d_radius,
                   uint32_t max_results, const ResultBlock& o, const RangeAllow* allow, RangeI8Verdict* out) {
  int rc;
  if ((rc = s->range.dCtl.ensure(nq))) return rc;
  const std::vector<TileRange> all = {{0u, allow ? allow->n_tiles : (uint32_t)((n_pub + kTileRows16 - 1) / kTileRows16)}};
  RadiusScan scan;
  scan.passes = &all;
  if (allow) {
    scan.allow = allow->allow;
    scan.allow_bits = allow->allow_bits;
    scan.allow_per_query = allow->per_query;
  }
  scan.d_word = s->range.dCtl.p;   // what the re-rank kept
  scan.rerank = [&](size_t, bool, const ScanArgsI8& a, ehx_space::I8Set& sc) {
    if (int rc2 = sc.clock.scan_end(st)) return rc2;   // (the timed scan phase is the scan alone)
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
    return (int)EHX_OK;
  };
  RadiusScanOut v;
  if ((rc = i8_radius_scan(s, st, n_pub, nq, d_queries, d_radius, scan, &v))) return rc;
  *out = RangeI8Verdict();
  for (size_t q = 0; q < nq; ++q) {
    if (const uint32_t flag = v.flag[q]) {
      out->todo.push_back((uint32_t)q);
      out->counted.push_back(flag == 1u);
      out->n_over += flag == 1u;
    } else {
      out->n_pairs += v.pool_cnt[q];
      out->n_trunc += v.word[q] > max_results;
    }
  }
  return EHX_OK;
}

}  // namespace ehx_impl

namespace {

// an unsharded space, locked shared, scratch_mu held, its device current; everything is enqueued on `st`
int range_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, const float* d_radius, uint32_t max_results,
                 const ResultBlock& out) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  if ((rc = check_rows_fit_lds(s, "range search"))) return rc;   // (before anything is enqueued)
  // the ONE read of the row count: every stage of the call answers for the same prefix
  const uint64_t n_pub = s->n.load(std::memory_order_acquire);
  const bool i8 = i8_serves_radius(s, n_pub);
  RangeI8Verdict v;
  for (size_t q0 = 0; q0 < nq; q0 += kSideChunk) {
    const size_t m = std::min(kSideChunk, nq - q0);
    const float* q = d_queries + q0 * s->dims;
    const float* r = d_radius + q0;
    const ResultBlock o = out.from(q0, m);
    if (i8) {
      if ((rc = range_i8_stage(s, st, n_pub, m, q, r, max_results, o, nullptr, &v))) return rc;
      s->n_dist += v.n_pairs;
      s->n_queries += m - v.todo.size();
      s->range_ctr[0] += m - v.todo.size();
      s->range_ctr[2] += v.n_over;
      s->range_ctr[3] += v.n_trunc;
      if (v.todo.empty()) continue;
      if ((rc = range_exact_stage(s, st, n_pub, m, q, r, &v.todo, &v.counted, max_results, o))) return rc;
    } else if ((rc = range_exact_stage(s, st, n_pub, m, q, r, nullptr, nullptr, max_results, o))) {
      return rc;
    }
  }
  return EHX_OK;
}

// host pointers in, host pointers out, on the space's stream (on_device): queries | radii staged in range.host
int range_host_locked(ehx_space* s, size_t nq, const float* queries, const float* radius, uint32_t k, uint64_t* out_ids,
                      float* out_dist, uint32_t* out_count, uint64_t* out_total) {
  int rc;
  HostStage& h = s->range.host;
  if ((rc = h.up(s->stream, queries, nq, s->dims, k, true, nq))) return rc;
  float* d_r = h.q + nq * s->dims;
  HIP_TRY(hipMemcpyAsync(d_r, radius, nq * sizeof(float), hipMemcpyHostToDevice, s->stream));
  if ((rc = range_locked(s, s->stream, nq, h.q, d_r, k, h.out))) return rc;
  return h.out.copy_out(s->stream, out_ids, out_dist, out_count, out_total);
}

}  // namespace

extern "C" {

int ehx_range(ehx_space* s, size_t n_queries, const float* queries, const float* radius, uint32_t max_results,
              uint64_t* out_ids, float* out_dist, uint32_t* out_count, uint64_t* out_total) {
  if (int rc = range_check(s, n_queries, max_results, queries, radius, out_ids, out_dist, out_count)) return rc;
  return search_on_device(s, "ehx_range", kRangeWhy, n_queries, nullptr, [&] {
    return range_host_locked(s, n_queries, queries, radius, max_results, out_ids, out_dist, out_count, out_total);
  });
}

int ehx_range_keys(ehx_space* s, size_t n_queries, const float* queries, const float* radius, uint32_t max_results,
                   uint64_t* out_ids, float* out_dist, uint32_t* out_count, uint64_t* out_total, char* key_arena,
                   size_t arena_cap, uint64_t* key_off) {
  if (int rc = range_check(s, n_queries, max_results, queries, radius, out_ids, out_dist, out_count)) return rc;
  if (!key_off || (!key_arena && arena_cap)) return fail(EHX_EINVAL, "NULL argument");
  // ONE shared hold for the search and the key lookup: the keys are those of the rows the search saw
  return search_shared(s, "ehx_range_keys", kRangeWhy, [&]() -> int {
    const int rc2 = on_device(s, n_queries, s->stream, [&] {
      return range_host_locked(s, n_queries, queries, radius, max_results, out_ids, out_dist, out_count, out_total);
    });
    return rc2 ? rc2 : fill_key_arena(s, n_queries, max_results, out_ids, out_count, key_arena, arena_cap, key_off);
  });
}

int ehx_range_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, const float* d_radius,
                     uint32_t max_results, uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count,
                     uint64_t* d_out_total) {
  if (int rc = range_check(s, n_queries, max_results, d_queries, d_radius, d_out_ids, d_out_dist, d_out_count)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_range_device", kRangeWhy, n_queries, &st, [&] {
    return range_locked(s, st, n_queries, d_queries, d_radius, max_results,
                        ResultBlock{d_out_ids, d_out_dist, d_out_count, d_out_total, n_queries, max_results});
  });
}

// test hook, not part of the ABI: queries answered by the int8 path, by the exact path, pool overflows, truncated answers
void ehx_test_range_counters(ehx_space* s, uint64_t out[4]) {
  for (int i = 0; i < 4; ++i) out[i] = s ? s->range_ctr[i].load(std::memory_order_relaxed) : 0;
}

}  // extern "C"
