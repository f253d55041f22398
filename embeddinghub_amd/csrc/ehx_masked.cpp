// kNN under a row bitmap.  Exact: ehx_knn_masked (host pointers) and ehx_knn_masked_device; on the graph path:
// ehx_graph_knn_masked* (the section at the end).  Row r is allowed iff r < n_bits,
// r is below the call's ONE snapshot of the row count and bit r & 31 of word r >> 5 is set; the answer is ehx_knn_among's
// with the ascending list of allowed rows, byte for byte (k_radius.hip's header has the argument).
//   compaction   the bitmap -> allowed rows before every 256-row tile (read back once: the host plans the passes from
//                them) and the ascending list of allowed ids
//   exact route  among_locked over that list: spaces the range search's int8 path does not serve, k > 48, lists of at
//                most max(1024, rows / 128) rows
//   scan route   the falling-radius kNN (radius_knn, ehx_call.cpp; k_radius.hip's header has the kernels and the argument)
//                with the bitmap in the int8 scan's flush: the first radius is the exact k-th distance of a sample of <= 256
//                allowed rows, taken by the list scan (its tiles share the sample's rows between queries), the passes are cut
//                by ALLOWED rows seen (4096, 65536, ...: sound wherever the bitmap's rows cluster), and the queries it
//                hands on — pool overflow, or the bound does not serve them — take the exact route
// Entry scaffold and host staging are ehx_call.cpp's (search_shared / on_device, HostStage).
#include "ehx_internal.h"

// (the constants of the routes are ehx_internal.h's: ehx_maskedq.cpp routes every query of a table of bitmaps by them)
// At most this many allowed rows: the exact route.  max(1024, rows / 128), MEASURED (scripts/bench_masked.py, 1 M x 768
// cosine, batch 1024, k = 10: the list scan costs what the scan route costs at 7 697 allowed rows, 0.77 % of the space;
// profiles/masked_bench.jsonl).
uint64_t ehx_impl::masked_exact_cut(uint64_t n_pub) { return std::max<uint64_t>(1024, n_pub / 128); }

int ehx_impl::masked_check(const ehx_space* s, size_t nq, uint32_t k, const void* q, const void* mask, uint64_t n_bits,
                           const void* o_ids, const void* o_dist, const void* o_cnt) {
  int rc = ehx_init(nullptr, 0);   // (no device: EHX_ENODEVICE, whatever else is wrong with the call)
  if (rc) return rc;
  if ((rc = check_batch_call(s, nq, k, "k", false, o_ids && o_dist && o_cnt && (!nq || q)))) return rc;
  if (n_bits && !mask) return fail(EHX_EINVAL, "NULL mask with n_bits = %llu", (unsigned long long)n_bits);
  return EHX_OK;
}

// tile ranges of the scan passes: pass j (j = 1, 2, ...; the sample is stage 0) ends at the first tile where the allowed
// rows seen reach kMaskedSample * 16^j, the last pass takes the rest.  cum[t] = allowed rows in tiles [0, t).
std::vector<TileRange> ehx_impl::masked_passes(const std::vector<uint32_t>& cum, uint32_t n_tiles) {
  std::vector<TileRange> out;
  uint32_t t0 = 0;
  for (uint64_t want = kMaskedSample * kMaskedPassGrowth; t0 < n_tiles; want *= kMaskedPassGrowth) {
    // (cum is non-decreasing: the first t with cum[t] >= want)
    uint32_t t1 = (uint32_t)(std::lower_bound(cum.begin() + t0 + 1, cum.begin() + n_tiles + 1, want,
                                              [](uint32_t c, uint64_t w) { return (uint64_t)c < w; }) - cum.begin());
    if (t1 > n_tiles || cum[n_tiles] <= want) t1 = n_tiles;
    out.push_back({t0, t1 - t0});
    t0 = t1;
  }
  return out;
}

namespace {

// The bitmap of one call, compacted: the call's ONE read of the row count, the rows the bitmap covers below it, the allowed
// rows before every tile (read back) and, in masked.dList, the ascending list of allowed ids.
struct MaskedList {
  uint64_t n_pub = 0, n_eff = 0, n_allowed = 0;
  uint32_t n_tiles = 0;
  std::vector<uint32_t> cum;
};
int masked_compact_locked(ehx_space* s, hipStream_t st, const uint32_t* d_mask, uint64_t n_bits, MaskedList* m) {
  int rc;
  // the ONE read of the row count: the list names rows below it only, and every later stage sees at least this prefix
  m->n_pub = s->n.load(std::memory_order_acquire);
  m->n_eff = std::min<uint64_t>(n_bits, m->n_pub);   // (row ids are 32 bits wide: n_pub < 2^32)
  m->n_tiles = (uint32_t)((m->n_eff + kTileRows16 - 1) / kTileRows16);
  const uint32_t n_tiles = m->n_tiles;
  if ((rc = s->masked.dCum.ensure((size_t)n_tiles + 1)) || (rc = s->masked.dList.ensure(std::max<uint64_t>(m->n_eff, 1))) ||
      (rc = s->masked.dSample.ensure(kMaskedSample)))
    return rc;
  m->cum.assign((size_t)n_tiles + 1, 0u);
  if (n_tiles) {
    // (earlier calls' launches on other streams may still read the list and the sample)
    if ((rc = wait_searches_in_flight(s, st))) return rc;
    HIP_TRY(launch_masked_compact(d_mask, m->n_eff, n_tiles, s->masked.dCum.p, s->masked.dList.p, st));
    HIP_TRY(hipMemcpyAsync(m->cum.data(), s->masked.dCum.p, m->cum.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  m->n_allowed = m->cum[n_tiles];
  return EHX_OK;
}

// the exact answer over a compacted bitmap: the scan route where it serves, else the list scan
int masked_answer_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, const uint32_t* d_mask,
                         const MaskedList& m, const ResultBlock& out) {
  int rc;
  const uint64_t n_pub = m.n_pub, n_eff = m.n_eff, n_allowed = m.n_allowed;
  const uint32_t n_tiles = m.n_tiles;
  const std::vector<uint32_t>& cum = m.cum;
  const bool scan = n_allowed > masked_exact_cut(n_pub) && k <= kMaskedScanMaxK && i8_serves_radius(s, n_pub);
  if (!scan) {
    s->masked_ctr[1] += nq;
    return among_locked(s, st, nq, d_queries, k, s->masked.dList.p, nullptr, n_allowed, 0, out.ids, out.dist, out.cnt);
  }
  const uint64_t stride = (n_allowed + kMaskedSample - 1) / kMaskedSample;
  RadiusKnn c;
  c.passes = masked_passes(cum, n_tiles);
  c.allow = d_mask;
  c.allow_bits = (uint32_t)n_eff;
  c.out = out;
  // stage 0: the exact k nearest of the sample, by the list scan, into the caller's arrays (every query's row is written
  // again, by the last pass or by the exact route; its queries are not counted there: the verdict counts every query once);
  // their k-th distance is the first radius, +Inf while the sample gives fewer than k
  const uint64_t n_sample = (n_allowed + stride - 1) / stride;
  c.first_radius = [&](size_t m, const float* q, const ResultBlock& o, float* d_radius) -> int {
    if (int r = among_locked(s, st, m, q, k, s->masked.dSample.p, nullptr, n_sample, 0, o.ids, o.dist, o.cnt, false)) return r;
    HIP_TRY(launch_masked_radius(o.dist, o.cnt, (uint32_t)m, k, d_radius, st));
    return EHX_OK;
  };
  c.exact = [&](size_t n, const float* sq, uint64_t* ids, float* dist, uint32_t* cnt) {
    return among_locked(s, st, n, sq, k, s->masked.dList.p, nullptr, n_allowed, 0, ids, dist, cnt);
  };
  HIP_TRY(launch_masked_sample(s->masked.dList.p, n_allowed, stride, s->masked.dSample.p, st));
  RadiusKnnTally t;
  rc = radius_knn(s, st, s->masked.scan, n_pub, d_queries, c, &t);
  s->n_queries += t.queries - t.handed;   // (among_locked counts the rest)
  s->masked_ctr[0] += t.queries - t.handed;
  s->masked_ctr[1] += t.handed;
  s->masked_ctr[2] += t.overflowed;
  s->masked_ctr[3] += t.batches * c.passes.size();
  return rc;
}

// an unsharded space, locked shared, scratch_mu held, its device current; everything is enqueued on `st`
int masked_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, const uint32_t* d_mask,
                  uint64_t n_bits, const ResultBlock& out) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  if ((rc = check_rows_fit_lds(s, "filtered search"))) return rc;   // (before anything is enqueued)
  s->masked_ctr[4] += 1;
  MaskedList m;
  if ((rc = masked_compact_locked(s, st, d_mask, n_bits, &m))) return rc;
  return masked_answer_locked(s, st, nq, d_queries, k, d_mask, m, out);
}

// what a host form stages in front of its device form: the queries, room for the results (h) and the bitmap's words below
// the row count (masked.dMaskRaw); *n_eff = the bits that may be looked at
int masked_stage_host(ehx_space* s, HostStage& h, size_t nq, const float* queries, uint32_t k, const uint32_t* mask,
                      uint64_t n_bits, uint64_t* n_eff) {
  // (bits at or above the row count are never looked at: only the words below it are staged.  This load of the row count
  // is the call's snapshot: the device form's own, later, load can only be larger, and the bits it may look at end at n_eff)
  *n_eff = std::min<uint64_t>(n_bits, s->n.load(std::memory_order_acquire));
  const size_t n_words = (size_t)((*n_eff + 31) / 32);
  int rc;
  if ((rc = s->masked.dMaskRaw.ensure(std::max<size_t>(n_words, 1)))) return rc;
  if ((rc = h.up(s->stream, queries, nq, s->dims, k, false))) return rc;
  if (n_words) HIP_TRY(hipMemcpyAsync(s->masked.dMaskRaw.p, mask, n_words * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
  return EHX_OK;
}

// host pointers in, host pointers out, on the space's stream (on_device): the bitmap staged in masked.dMaskRaw
int masked_host_locked(ehx_space* s, size_t nq, const float* queries, uint32_t k, const uint32_t* mask, uint64_t n_bits,
                       uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  int rc;
  uint64_t n_eff;
  HostStage& h = s->masked.host;
  if ((rc = masked_stage_host(s, h, nq, queries, k, mask, n_bits, &n_eff))) return rc;
  if ((rc = masked_locked(s, s->stream, nq, h.q, k, s->masked.dMaskRaw.p, n_eff, h.out))) return rc;
  return h.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
}

// ---- the graph walk under the bitmap (ehx_graph_knn_masked*; k_graphm.hip has the walk, tests/filtered_walk_model.py its
// model).  Routes: the walk — knn_graph_locked with the bitmap: the same arguments, wait, clock and refusals as an
// unfiltered graph search; or the exact answer above, byte for byte ehx_knn_masked_device's.  EHX_WALK_AUTO compacts the
// bitmap first (one wait) and walks iff allowed rows * EHX_WALK_LIST_FACTOR >= the rows the bitmap covers: below that share
// a list of cap = FACTOR * ef entries cannot hold ef allowed ones and the walk degenerates (MEASURED: the exact route
// overtakes the walk between shares 1 / 11 and 1 / 14, scripts/bench_graph_masked.py, profiles/graph_masked_bench.jsonl;
// include/ehx.h has the figures beside the constant).  A flat space has no graph: the exact route. ----
int graphm_check(const ehx_space* s, size_t nq, uint32_t k, const void* q, const void* mask, uint64_t n_bits, uint32_t route,
                 const void* o_ids, const void* o_dist, const void* o_cnt) {
  if (int rc = masked_check(s, nq, k, q, mask, n_bits, o_ids, o_dist, o_cnt)) return rc;
  if (route != EHX_WALK_AUTO && route != EHX_WALK_GRAPH && route != EHX_WALK_EXACT)
    return fail(EHX_EINVAL, "route %u is none of EHX_WALK_AUTO, EHX_WALK_GRAPH, EHX_WALK_EXACT", route);
  return EHX_OK;
}

int graphm_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, const uint32_t* d_mask,
                  uint64_t n_bits, uint32_t route, const ResultBlock& out) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  s->graphm_ctr[2] += 1;
  if (s->params.mode != EHX_MODE_GRAPH) route = EHX_WALK_EXACT;
  MaskedList m;
  if (route != EHX_WALK_GRAPH) {
    if (route == EHX_WALK_EXACT && (rc = check_rows_fit_lds(s, "filtered search"))) return rc;   // (before anything is enqueued)
    if ((rc = masked_compact_locked(s, st, d_mask, n_bits, &m))) return rc;
    if (route == EHX_WALK_AUTO) route = m.n_allowed * EHX_WALK_LIST_FACTOR >= m.n_eff ? EHX_WALK_GRAPH : EHX_WALK_EXACT;
  }
  if (route == EHX_WALK_EXACT) {
    if ((rc = check_rows_fit_lds(s, "filtered search"))) return rc;   // (EHX_WALK_AUTO: known only now)
    s->graphm_ctr[1] += nq;
    return masked_answer_locked(s, st, nq, d_queries, k, d_mask, m, out);
  }
  if ((rc = s->masked.dCapHits.ensure(1, true))) return rc;
  // (the walk takes its own snapshot of the row count behind the refusal g_n != n; a bitmap cut at an earlier, smaller
  // count only allows fewer rows)
  const GraphMask gm = {d_mask, std::min<uint64_t>(n_bits, s->n.load(std::memory_order_acquire)), s->masked.dCapHits.p};
  if ((rc = knn_graph_locked(s, st, nq, d_queries, k, out.ids, out.dist, out.cnt, nullptr, &gm))) return rc;
  s->graphm_ctr[0] += nq;
  return EHX_OK;
}

int graphm_host_locked(ehx_space* s, size_t nq, const float* queries, uint32_t k, const uint32_t* mask, uint64_t n_bits,
                       uint32_t route, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  int rc;
  uint64_t n_eff;
  HostStage& h = s->masked.host;
  if ((rc = masked_stage_host(s, h, nq, queries, k, mask, n_bits, &n_eff))) return rc;
  if ((rc = graphm_locked(s, s->stream, nq, h.q, k, s->masked.dMaskRaw.p, n_eff, route, h.out))) return rc;
  return h.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
}

}  // namespace

extern "C" {

int ehx_knn_masked_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                          const uint32_t* d_mask, uint64_t n_bits, uint64_t* d_out_ids, float* d_out_dist,
                          uint32_t* d_out_count) {
  if (int rc = masked_check(s, n_queries, k, d_queries, d_mask, n_bits, d_out_ids, d_out_dist, d_out_count)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_knn_masked_device", kMaskedWhy, n_queries, &st, [&] {
    return masked_locked(s, st, n_queries, d_queries, k, d_mask, n_bits,
                         ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_knn_masked(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const uint32_t* mask, uint64_t n_bits,
                   uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (int rc = masked_check(s, n_queries, k, queries, mask, n_bits, out_ids, out_dist, out_count)) return rc;
  return search_on_device(s, "ehx_knn_masked", kMaskedWhy, n_queries, nullptr, [&] {
    return masked_host_locked(s, n_queries, queries, k, mask, n_bits, out_ids, out_dist, out_count);
  });
}

int ehx_graph_knn_masked_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                const uint32_t* d_mask, uint64_t n_bits, uint32_t route, uint64_t* d_out_ids,
                                float* d_out_dist, uint32_t* d_out_count) {
  if (int rc = graphm_check(s, n_queries, k, d_queries, d_mask, n_bits, route, d_out_ids, d_out_dist, d_out_count)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_graph_knn_masked_device", kMaskedWhy, n_queries, &st, [&] {
    return graphm_locked(s, st, n_queries, d_queries, k, d_mask, n_bits, route,
                         ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_graph_knn_masked(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const uint32_t* mask,
                         uint64_t n_bits, uint32_t route, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (int rc = graphm_check(s, n_queries, k, queries, mask, n_bits, route, out_ids, out_dist, out_count)) return rc;
  return search_on_device(s, "ehx_graph_knn_masked", kMaskedWhy, n_queries, nullptr, [&] {
    return graphm_host_locked(s, n_queries, queries, k, mask, n_bits, route, out_ids, out_dist, out_count);
  });
}

// test hook, not part of the ABI: queries walked, queries answered exactly, calls, walked queries whose list reached its
// cap (read from the device behind whatever is queued)
int ehx_test_graph_masked_counters(ehx_space* s, uint64_t out[4]) {
  for (int i = 0; i < 3; ++i) out[i] = s ? s->graphm_ctr[i].load(std::memory_order_relaxed) : 0;
  out[3] = 0;
  if (!s || !s->masked.dCapHits.p) return EHX_OK;
  unsigned long long hits = 0;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(&hits, s->masked.dCapHits.p, sizeof(hits), hipMemcpyDeviceToHost));
  out[3] = hits;
  return EHX_OK;
}

// test hook, not part of the ABI: queries answered on the scan route, on the exact route, queries that overflowed, scan
// passes launched, calls
void ehx_test_masked_counters(ehx_space* s, uint64_t out[5]) {
  for (int i = 0; i < 5; ++i) out[i] = s ? s->masked_ctr[i].load(std::memory_order_relaxed) : 0;
}

}  // extern "C"
