// Exact kNN under a row bitmap: ehx_knn_masked (host pointers) and ehx_knn_masked_device.  Row r is allowed iff r < n_bits,
// r is below the call's ONE snapshot of the row count and bit r & 31 of word r >> 5 is set; the answer is ehx_knn_among's
// with the ascending list of allowed rows, byte for byte (k_masked.hip's header has the argument).
//   compaction   the bitmap -> allowed rows before every 256-row tile (read back once: the host plans the passes from
//                them) and the ascending list of allowed ids
//   exact route  among_locked over that list: spaces the range search's int8 path does not serve, k > 48, lists of at
//                most max(1024, rows / 128) rows
//   scan route   in one int8 scratch set: the exact k-th distance of a sample of <= 256 allowed rows is the first radius;
//                passes of flat_scan_i8_kernel over disjoint tile ranges, cut by ALLOWED rows seen (4096, 65536, ...: sound
//                wherever the bitmap's rows cluster), each under the threshold of the radius so far with the bitmap in its
//                flush, each followed by masked_rerank_kernel; no host wait between passes.  Queries whose pool overflowed
//                or which the bound does not serve take the exact route afterwards.
#include "ehx_internal.h"

namespace {

constexpr size_t kMaskedChunk = 2048;       // queries per device batch of the scan route: their pools are 64 MiB
constexpr uint32_t kMaskedScanMaxK = 48;    // the scan route carries <= k keys per query between passes: the certified engines' k
constexpr uint64_t kMaskedSample = 256;     // allowed rows in the sample, at most
constexpr uint64_t kMaskedPassGrowth = 16;  // pass j ends where kMaskedSample * 16^j allowed rows have been seen
// At most this many allowed rows: the exact route.  max(1024, rows / 128), MEASURED (scripts/bench_masked.py, 1 M x 768
// cosine, batch 1024, k = 10: the list scan costs what the scan route costs at 7 697 allowed rows, 0.77 % of the space;
// profiles/masked_bench.jsonl).
uint64_t masked_exact_cut(uint64_t n_pub) { return std::max<uint64_t>(1024, n_pub / 128); }

int masked_check(const ehx_space* s, size_t nq, uint32_t k, const void* q, const void* mask, uint64_t n_bits, const void* o_ids,
                 const void* o_dist, const void* o_cnt) {
  int rc = ehx_init(nullptr, 0);   // (no device: EHX_ENODEVICE, whatever else is wrong with the call)
  if (rc) return rc;
  if ((rc = check_batch_call(s, nq, k, "k", false, o_ids && o_dist && o_cnt && (!nq || q)))) return rc;
  if (n_bits && !mask) return fail(EHX_EINVAL, "NULL mask with n_bits = %llu", (unsigned long long)n_bits);
  return EHX_OK;
}
int masked_unsharded(const ehx_space* s, const char* what) {
  return check_unsharded(s, what, "filtered search over shards is not built yet");
}

// tile ranges of the scan passes: pass j (j = 1, 2, ...; the sample is stage 0) ends at the first tile where the allowed
// rows seen reach kMaskedSample * 16^j, the last pass takes the rest.  cum[t] = allowed rows in tiles [0, t).
std::vector<std::pair<uint32_t, uint32_t>> masked_passes(const std::vector<uint32_t>& cum, uint32_t n_tiles) {
  std::vector<std::pair<uint32_t, uint32_t>> out;
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

// The scan route for a batch of nq <= kMaskedChunk queries; *todo = the queries it leaves to the exact route.
int masked_scan_stage(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const float* d_queries, uint32_t k,
                      const uint32_t* d_mask, uint64_t n_eff, uint64_t n_sample,
                      const std::vector<std::pair<uint32_t, uint32_t>>& passes, const ResultBlock& o,
                      std::vector<uint32_t>* todo) {
  Engine& E = engine();
  int rc;
  if ((rc = s->masked.dRadius.ensure(nq)) || (rc = s->masked.dWork.ensure(nq))) return rc;
  // stage 0: the exact k nearest of the sample, into the caller's arrays (every query's row is written again below, by the
  // last pass or by the exact route); their k-th distance is the first radius
  // (its queries are not counted there: the stage's verdict counts every query once)
  if ((rc = among_locked(s, st, nq, d_queries, k, s->masked.dSample.p, nullptr, n_sample, 0, o.ids, o.dist, o.cnt, false)))
    return rc;
  HIP_TRY(launch_masked_radius(o.dist, o.cnt, (uint32_t)nq, k, s->masked.dRadius.p, st));
  HIP_TRY(hipMemsetAsync(s->masked.dWork.p, 0, nq * sizeof(uint32_t), st));

  const int set = (int)(s->i8_next_set.fetch_add(1, std::memory_order_relaxed) & 1u);
  ehx_space::I8Set& sc = s->i8set[set];
  std::lock_guard<std::mutex> l(sc.mu);
  std::vector<ScanPlan> plans;
  for (auto& ps : passes) {
    plans.push_back(plan_scan((uint32_t)nq, ps.second, 1, E.n_cus));
    if (plans.back().n_chunks > 256) return fail(EHX_EINTERNAL, "scan plan with %u chunks", plans.back().n_chunks);
  }
  const ScanPlan& p = plans.back();   // (q_tiles, q_rows are the same for every pass)
  ScanArgsI8 a;
  if ((rc = i8_scan_args(s, sc.buf, p, n_pub, &a))) return rc;
  a.allow = d_mask;
  a.allow_bits = (uint32_t)n_eff;
  {
    std::lock_guard<std::mutex> ql(s->i8_enqueue_mu);   // (this batch's launches go onto the stream as one block)
    if ((rc = wait_searches_in_flight(s, st))) return rc;
    if ((rc = sc.clock.begin(st, BatchClock::kOutOfRing))) return rc;   // (timed, but not a kNN batch: outside the ring)
    // thr[q] = +inf, control words zero; every pass then maps the radius so far to its threshold
    HIP_TRY(launch_prep_queries_i8(d_queries, (uint32_t)nq, s->dims, s->ld, s->ld8, p.q_rows, s->metric, sc.buf.dQ.p,
                                   sc.buf.dQ8.p, sc.buf.dQp8.p, sc.buf.dQuv.p, sc.buf.dThr8.p, sc.buf.dI8Ctl.p, st));
    MaskedRerankArgs r = {};
    r.Q = sc.buf.dQ.p;
    r.rows = rows_view(s, n_pub);
    r.radius = s->masked.dRadius.p;
    r.pool = sc.buf.dPool.p;
    r.pool_cnt = a.pool_cnt;
    r.ovf = a.ovf;
    r.work = s->masked.dWork.p;
    r.out_ids = o.ids;
    r.out_dist = o.dist;
    r.out_count = o.cnt;
    r.nq = (uint32_t)nq;
    r.k = k;
    if ((rc = sc.clock.scan_begin(st))) return rc;
    for (size_t i = 0; i < passes.size(); ++i) {
      HIP_TRY(launch_range_thr(s->masked.dRadius.p, sc.buf.dQuv.p, s->rows.dMaxSumsq.p, (uint32_t)nq, s->dims, s->metric,
                               sc.buf.dThr8.p, a.ovf, st));
      set_scan_pass(a, plans[i], passes[i].first);
      HIP_TRY(launch_flat_scan_i8(a, st));
      r.last = i + 1 == passes.size() ? 1u : 0u;
      HIP_TRY(launch_masked_rerank(r, st));
    }
    if ((rc = sc.clock.scan_end(st)) || (rc = sc.clock.finish(st))) return rc;
  }
  // the verdict: overflow flags, marks and the rows re-ranked (read once per batch, one wait)
  std::vector<uint32_t> flags(nq), work(nq);
  HIP_TRY(hipMemcpyAsync(flags.data(), sc.buf.dI8Ctl.p + p.q_rows, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(work.data(), s->masked.dWork.p, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  todo->clear();
  uint64_t n_pairs = 0, n_over = 0;
  for (size_t q = 0; q < nq; ++q) {
    n_pairs += work[q];
    if (flags[q]) {
      todo->push_back((uint32_t)q);
      n_over += flags[q] == 1u;
    }
  }
  s->n_dist += n_pairs;
  s->n_queries += nq - todo->size();
  s->masked_ctr[0] += nq - todo->size();
  s->masked_ctr[2] += n_over;
  s->masked_ctr[3] += passes.size();
  return EHX_OK;
}

// an unsharded space, locked shared, scratch_mu held, its device current; everything is enqueued on `st`
int masked_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, const uint32_t* d_mask,
                  uint64_t n_bits, const ResultBlock& out) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  if (s->ld > among_max_ld())   // (before anything is enqueued)
    return fail(EHX_EUNSUPPORTED, "filtered search keeps a prepared query in LDS: rows of %u floats exceed %u", s->ld,
                among_max_ld());
  s->masked_ctr[4] += 1;
  // the ONE read of the row count: the list names rows below it only, and every later stage sees at least this prefix
  const uint64_t n_pub = s->n.load(std::memory_order_acquire);
  const uint64_t n_eff = std::min<uint64_t>(n_bits, n_pub);   // (row ids are 32 bits wide: n_pub < 2^32)
  const uint32_t n_tiles = (uint32_t)((n_eff + kTileRows16 - 1) / kTileRows16);
  if ((rc = s->masked.dCum.ensure((size_t)n_tiles + 1)) || (rc = s->masked.dList.ensure(std::max<uint64_t>(n_eff, 1))) ||
      (rc = s->masked.dSample.ensure(kMaskedSample)))
    return rc;
  std::vector<uint32_t> cum((size_t)n_tiles + 1, 0u);
  if (n_tiles) {
    // (earlier calls' launches on other streams may still read the list and the sample)
    if ((rc = wait_searches_in_flight(s, st))) return rc;
    HIP_TRY(launch_masked_compact(d_mask, n_eff, n_tiles, s->masked.dCum.p, s->masked.dList.p, st));
    HIP_TRY(hipMemcpyAsync(cum.data(), s->masked.dCum.p, cum.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  const uint64_t n_allowed = cum[n_tiles];
  const bool scan = n_allowed > masked_exact_cut(n_pub) && k <= kMaskedScanMaxK && resolve_engine(s, n_pub) == EHX_ENGINE_I8 &&
                    s->ld <= range_rerank_max_ld();
  if (!scan) {
    s->masked_ctr[1] += nq;
    return among_locked(s, st, nq, d_queries, k, s->masked.dList.p, nullptr, n_allowed, 0, out.ids, out.dist, out.cnt);
  }
  const uint64_t stride = (n_allowed + kMaskedSample - 1) / kMaskedSample;
  const uint64_t n_sample = (n_allowed + stride - 1) / stride;
  HIP_TRY(launch_masked_sample(s->masked.dList.p, n_allowed, stride, s->masked.dSample.p, st));
  const std::vector<std::pair<uint32_t, uint32_t>> passes = masked_passes(cum, n_tiles);
  std::vector<uint32_t> todo;
  for (size_t q0 = 0; q0 < nq; q0 += kMaskedChunk) {
    const size_t m = std::min(kMaskedChunk, nq - q0);
    const float* q = d_queries + q0 * s->dims;
    const ResultBlock o = out.from(q0, m);
    if ((rc = masked_scan_stage(s, st, n_pub, m, q, k, d_mask, n_eff, n_sample, passes, o, &todo))) return rc;
    if (todo.empty()) continue;
    // flagged queries: gathered, answered by the exact kNN among the whole list, scattered back
    SubsetBufs& sub = s->masked.sub;
    if ((rc = sub.gather(q, todo, s->dims, k, st))) return rc;
    if ((rc = among_locked(s, st, sub.m, sub.dFbQ.p, k, s->masked.dList.p, nullptr, n_allowed, 0, sub.dFbIds.p, sub.dFbDist.p,
                           sub.dFbCnt.p)))
      return rc;
    if ((rc = sub.scatter(o.ids, o.dist, o.cnt, st))) return rc;
    if ((rc = s->clock.extend(st))) return rc;   // (the scatter belongs to the last batch: writers wait for it too)
    s->masked_ctr[1] += todo.size();
  }
  return EHX_OK;
}

}  // namespace

extern "C" {

int ehx_knn_masked_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                          const uint32_t* d_mask, uint64_t n_bits, uint64_t* d_out_ids, float* d_out_dist,
                          uint32_t* d_out_count) {
  int rc = masked_check(s, n_queries, k, d_queries, d_mask, n_bits, d_out_ids, d_out_dist, d_out_count);
  if (rc) return rc;
  yield_to_writer(s);
  std::shared_lock<std::shared_mutex> rl(s->mu);
  if ((rc = masked_unsharded(s, "ehx_knn_masked_device"))) return rc;
  if (n_queries == 0) return EHX_OK;
  std::lock_guard<std::mutex> sl(s->scratch_mu);
  HIP_TRY(hipSetDevice(s->device));
  DrainUnlessOk drain{(hipStream_t)stream};
  return drain.done(masked_locked(s, (hipStream_t)stream, n_queries, d_queries, k, d_mask, n_bits,
                                  ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k}));
}

int ehx_knn_masked(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const uint32_t* mask, uint64_t n_bits,
                   uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  int rc = masked_check(s, n_queries, k, queries, mask, n_bits, out_ids, out_dist, out_count);
  if (rc) return rc;
  yield_to_writer(s);
  std::shared_lock<std::shared_mutex> rl(s->mu);
  if ((rc = masked_unsharded(s, "ehx_knn_masked"))) return rc;
  if (n_queries == 0) return EHX_OK;
  std::lock_guard<std::mutex> sl(s->scratch_mu);
  HIP_TRY(hipSetDevice(s->device));
  // (bits at or above the row count are never looked at: only the words below it are staged.  This load of the row count
  // is the call's snapshot: masked_locked's own, later, load can only be larger, and the bits it may look at end at n_eff)
  const uint64_t n_eff = std::min<uint64_t>(n_bits, s->n.load(std::memory_order_acquire));
  const size_t n_words = (size_t)((n_eff + 31) / 32);
  if ((rc = s->masked.dMaskRaw.ensure(std::max<size_t>(n_words, 1)))) return rc;
  if ((rc = s->masked.dQraw.ensure(n_queries * s->dims))) return rc;
  if ((rc = s->masked.dOut.ensure(ResultBlock::bytes(n_queries, k, false)))) return rc;
  const ResultBlock o = ResultBlock::at(s->masked.dOut.p, n_queries, k, false);
  DrainUnlessOk drain{s->stream};
  // (pageable host memory: the runtime stages it before the call returns; the staging buffers are this path's alone and
  // the space's stream orders their reuse)
  if (n_words) HIP_TRY(hipMemcpyAsync(s->masked.dMaskRaw.p, mask, n_words * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(s->masked.dQraw.p, queries, n_queries * s->dims * sizeof(float), hipMemcpyHostToDevice, s->stream));
  if ((rc = masked_locked(s, s->stream, n_queries, s->masked.dQraw.p, k, s->masked.dMaskRaw.p, n_eff, o))) return rc;
  return drain.done(o.copy_out(s->stream, out_ids, out_dist, out_count, nullptr));
}

// test hook, not part of the ABI: queries answered on the scan route, on the exact route, queries that overflowed, scan
// passes launched, calls
void ehx_test_masked_counters(ehx_space* s, uint64_t out[5]) {
  for (int i = 0; i < 5; ++i) out[i] = s ? s->masked_ctr[i].load(std::memory_order_relaxed) : 0;
}

}  // extern "C"
