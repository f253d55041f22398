// Boosted kNN: ehx_knn_boosted / _device (the penalties a caller's float array) and ehx_knn_decay / _device (the penalties the
// linear decay of a stored column).  Row i of the answer: the first k rows of the prefix — ONE snapshot of the row count, cut
// at n_penalty in the array form — in (score, id) order, score = fl(D + fl(w p)) (include/ehx.h has the contract, k_boost.hip's
// header the kernels, the map from the score radius to the distance radius and why the answer is exact).  Nothing is stored
// with the rows for it, and the int8 scan kernel does not know of the penalties.
//   scan route    flat spaces whose int8 scan serves a radius on the prefix (i8_serves_radius), plain rows (no x_perm), device
//                 batches of at least kLargeKMinQueries queries, EVERY k <= 256.  The falling-radius kNN (radius_knn,
//                 ehx_call.cpp) as the large-k route plans it (largek_passes, the strided seed — growth and sample size are that
//                 route's defaults, carried over, not tuned for loose radii), with boost_rerank_kernel as its re-rank; the
//                 array form runs boost_floor_kernel once per call in front of the first device batch, and a call whose floor
//                 flag is set (a penalty of -Inf, or no finite penalty) goes whole to the exact route.  The queries the scan
//                 hands on — pool overflow, a distance radius the bound does not serve or that is not finite — go, each with
//                 its own weight, to the
//   exact route   everything else (graph spaces, which answer from their stored rows; small spaces; SCAN_F32 / SCAN_F16; small
//                 batches): consecutive slabs of kPoolCap rows of the whole prefix (launch_grouped_range_slab with the
//                 identity list) through the same re-rank in pass mode, the score radius falling from +Inf, the last slab in
//                 last mode.  Every row's canonical distance is computed at most once, for any k <= 256.
// Entry scaffold, host staging, sub-batch re-runs: ehx_call.cpp's (search_on_device, HostStage, SubsetBufs::rerun).
#include "ehx_internal.h"

namespace {

constexpr const char* kBoostWhy = "boosted search over shards is not built yet";

static_assert(EHX_MAX_K_GROUPED == kLargeKMax, "the re-rank carries one key per thread");

// where a call's penalties come from (BoostRerankArgs' fields of the same names)
struct BoostSource {
  int form;
  const float* penalty;
  const uint32_t* col;
  uint32_t origin, span;
};

// what is decided before the device is looked for, with its codes and in this order (s is not read)
int boost_check(const ehx_space* s, size_t nq, uint32_t k, bool ptrs_ok) {
  if (!s) return fail(EHX_EINVAL, "space is NULL");
  if (k == 0) return fail(EHX_EINVAL, "k is 0");
  if (k > EHX_MAX_K_GROUPED) return fail(EHX_EUNSUPPORTED, "k=%u exceeds %u", k, EHX_MAX_K_GROUPED);
  if (!ptrs_ok) return fail(EHX_EINVAL, "NULL argument");
  return check_batch_size(nq);
}

int boost_check_col(uint32_t col) {
  return col < EHX_MAX_COLUMNS ? (int)EHX_OK : fail(EHX_EINVAL, "col = %u: a space has %u columns", col, (unsigned)EHX_MAX_COLUMNS);
}

int boost_check_ld(const ehx_space* s) {
  if (int rc = check_rows_fit_lds(s, "boosted search")) return rc;
  if (s->ld > boost_rerank_max_ld())
    return fail(EHX_EUNSUPPORTED, "boosted search keeps a pool and a prepared query in LDS: rows of %u floats exceed %u", s->ld,
                boost_rerank_max_ld());
  return EHX_OK;
}

// the weights of a call, host memory: finite and not negative (the distance radius rests on w >= 0)
int boost_check_weights(const float* w, size_t nq, const char* name) {
  for (size_t i = 0; i < nq; ++i)
    if (!(w[i] >= 0.0f) || std::isinf(w[i]))
      return fail(EHX_EINVAL, "%s[%zu] = %g: a weight is finite and not negative", name, i, (double)w[i]);
  return EHX_OK;
}

// the re-rank's arguments around a falling-radius re-rank's: query j of r weighs d_weight[weight_of ? weight_of[j] : j]
BoostRerankArgs boost_args(const RadiusRerankArgs& r, uint64_t n_eff, const BoostSource& src, const float* d_weight,
                           const uint32_t* weight_of, float* score_r, const float* floor, uint32_t* flag) {
  BoostRerankArgs e = {};
  e.r = r;
  e.n_penalty = n_eff;
  e.penalty = src.penalty;
  e.col = src.col;
  e.origin = src.origin;
  e.span = src.span;
  e.weight = d_weight;
  e.weight_of = weight_of;
  e.score_r = score_r;
  e.floor = floor;
  e.flag = flag;
  e.form = src.form;
  return e;
}

// The exact route for nq queries over the prefix of n_eff rows, enqueued on `st`.  Query j weighs d_weight[weight_of ?
// weight_of[j] : j] (d_weight == nullptr: 1; nq <= kSideChunk with weight_of).
int boost_exact(ehx_space* s, hipStream_t st, uint64_t n_eff, size_t nq, const float* d_queries, uint32_t k, const BoostSource& src,
                const float* d_weight, const uint32_t* weight_of, uint64_t* d_ids, float* d_score, uint32_t* d_count,
                bool count_queries) {
  ehx_space::Boost& w = s->boost;
  const size_t cap = std::min(kSideChunk, nq);
  int rc;
  if ((rc = s->scr.dQ.ensure(cap * s->ld)) || (rc = w.dPool.ensure(cap * kPoolCap)) || (rc = w.dCtl.ensure(2 * cap)) ||
      (rc = w.exact.dTop.ensure(cap * kLargeKMax)) || (rc = w.exact.dTopCnt.ensure(cap)) || (rc = w.exact.dRadius.ensure(cap)) ||
      (rc = w.exact.dWork.ensure(cap)) || (rc = w.dRange.ensure(2 * cap)) || (rc = w.dScoreExact.ensure(cap)))
    return rc;
  std::vector<uint64_t> up(2 * cap, 0);   // a device batch's [m] starts | [m] ends: every query walks the whole prefix
  const uint64_t n_slabs = std::max<uint64_t>(1, (n_eff + kPoolCap - 1) / kPoolCap);   // (no row: one empty slab writes the page)
  for (size_t q0 = 0; q0 < nq; q0 += kSideChunk) {
    const size_t m = std::min(kSideChunk, nq - q0);
    std::fill(up.begin() + m, up.begin() + 2 * m, n_eff);
    // (searches on other streams have read and written this scratch; this batch's fence makes a Set that rewrites rows in
    // place wait for it in turn)
    if ((rc = wait_searches_in_flight(s, st))) return rc;
    if ((rc = s->clock.begin(st, BatchClock::kOutOfRing))) return rc;
    HIP_TRY(hipMemsetAsync(w.dCtl.p, 0, 2 * m * sizeof(uint32_t), st));
    // (pageable host memory: the runtime stages it before the call returns)
    HIP_TRY(hipMemcpyAsync(w.dRange.p, up.data(), 2 * m * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(launch_prep_queries(d_queries + q0 * s->dims, (uint32_t)m, s->dims, s->ld, (uint32_t)m, s->metric, s->scr.dQ.p, st));
    RadiusRerankArgs r = {};
    r.Q = s->scr.dQ.p;
    r.rows = rows_view(s, n_eff);
    r.radius = w.exact.dRadius.p;   // (no scan reads a distance radius here, and none is written: flag == nullptr)
    r.pool = w.dPool.p;
    r.pool_cnt = w.dCtl.p;
    r.ovf = w.dCtl.p + m;
    r.top = w.exact.dTop.p;
    r.top_cnt = w.exact.dTopCnt.p;
    r.work = w.exact.dWork.p;
    r.out_ids = d_ids + q0 * k;
    r.out_dist = d_score + q0 * k;
    r.out_count = d_count + q0;
    r.nq = (uint32_t)m;
    r.k = k;
    if ((rc = s->clock.scan_begin(st))) return rc;
    for (uint64_t b = 0; b < n_slabs; ++b) {
      // (the first slab's state: the SCORE radius +Inf, nothing carried)
      HIP_TRY(launch_grouped_range_slab(nullptr, w.dRange.p, w.dRange.p + m, b, b == 0, w.dPool.p, w.dCtl.p, w.dScoreExact.p,
                                        r.top_cnt, r.work, (uint32_t)m, st));
      r.mode = b + 1 == n_slabs ? kRadiusLast : kRadiusPass;
      HIP_TRY(launch_boost_rerank(boost_args(r, n_eff, src, d_weight ? d_weight + (weight_of ? 0 : q0) : nullptr, weight_of,
                                             w.dScoreExact.p, nullptr, nullptr),
                                  st));
    }
    if ((rc = s->clock.scan_end(st)) || (rc = s->clock.finish(st))) return rc;
  }
  if (count_queries) s->n_queries += nq;
  s->n_dist += (uint64_t)nq * n_eff;
  return EHX_OK;
}

// an unsharded space, locked shared, scratch_mu held, its device current; everything is enqueued on `st`.  The weights are on
// the device and checked (boost_check_weights).  n_penalty: the rows that have a penalty (the column form: every row).
int boost_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, BoostSource src, uint32_t col,
                 uint64_t n_penalty, const float* d_weight, const ResultBlock& out) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  if ((rc = boost_check_ld(s))) return rc;   // (before anything is enqueued)
  ehx_space::Boost& w = s->boost;
  const uint64_t n_pub = s->n.load(std::memory_order_acquire);   // the ONE read of the row count
  const uint64_t n_eff = std::min(n_pub, n_penalty);             // rows without a penalty are not searched
  if (src.form == kBoostColumn && (rc = column_as_groups(s, st, col, n_pub, &src.col))) return rc;
  s->boost_ctr[4] += 1;
  // The scan is told the SNAPSHOT: its flush cuts by position, and a tile's rows are stored permuted, so the last tile of a
  // shorter prefix would lose rows.  The passes cover the tiles that hold the rows with a penalty; what that last tile holds
  // beyond them takes pool slots and is dropped by the re-rank before it is read.
  const bool scans = s->params.mode != EHX_MODE_GRAPH && !s->x_perm && n_eff > 0 && i8_serves_radius(s, n_pub);
  // (a last device batch below the gate goes with the exact route's queries)
  const size_t tail = nq % kSideChunk;
  size_t n_scan = !scans ? 0 : (tail && tail < kLargeKMinQueries ? nq - tail : nq);
  const float* d_floor = nullptr;   // (the column form: p >= 0, p_min = 0 without a look at the column)
  if (n_scan && src.form == kBoostArray) {
    // p_min, once per call, and the flag that sends the call to the exact route (one small copy and a wait)
    if ((rc = w.dFloor.ensure(kBoostFloorWords))) return rc;
    if ((rc = wait_searches_in_flight(s, st))) return rc;   // (an earlier call's re-ranks on another stream read the floor)
    const uint32_t init[kBoostFloorWords] = {0xFFFFFFFFu, 0u, 0u, 0u};
    uint32_t flag = 0;
    // (pageable host memory: the runtime stages it before the call returns)
    HIP_TRY(hipMemcpyAsync(w.dFloor.p, init, sizeof(init), hipMemcpyHostToDevice, st));
    HIP_TRY(launch_boost_floor(src.penalty, n_eff, w.dFloor.p, engine().n_cus, st));
    HIP_TRY(hipMemcpyAsync(&flag, w.dFloor.p + 2, sizeof(flag), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (flag) n_scan = 0;
    d_floor = (const float*)(w.dFloor.p + 3);
  }
  if (n_scan) {
    const size_t cap = std::min(kSideChunk, n_scan);
    if ((rc = w.dScoreScan.ensure(cap))) return rc;
    RadiusKnn c;
    c.passes = largek_passes(n_eff, env().largek_growth);
    c.seed_stride = (n_eff + kLargeKSample - 1) / kLargeKSample;
    c.n_sample = (uint32_t)((n_eff + c.seed_stride - 1) / c.seed_stride);
    c.out = ResultBlock{out.ids, out.dist, out.cnt, nullptr, n_scan, k};
    size_t batch0 = 0;   // the call's first query of the device batch in hand (radius_knn takes them in order)
    c.fill_pool = [&](size_t q0, size_t m, uint64_t* pool, uint32_t* pool_cnt) -> int {
      batch0 = q0;
      HIP_TRY(launch_radius_seed(pool, pool_cnt, (uint32_t)m, n_eff, c.seed_stride, c.n_sample, st));
      return EHX_OK;
    };
    c.rerank = [&](const RadiusRerankArgs& r, hipStream_t on) {
      // (r.ovf is the scan's own flag array, which its kernels write: the re-rank marks a query there as range_thr_kernel does)
      return launch_boost_rerank(boost_args(r, n_eff, src, d_weight ? d_weight + batch0 : nullptr, nullptr, w.dScoreScan.p,
                                            d_floor, const_cast<uint32_t*>(r.ovf)),
                                 on);
    };
    // the flagged queries of a device batch, each with its own weight: ONE sub-batch on the exact route (the gather's index
    // array, still on the device when the answer runs, names their weights)
    c.handed = [&](size_t q0, const std::vector<uint32_t>& todo, const float* q, const ResultBlock& o) -> int {
      return w.scan.sub.rerun(
          s, st, q, todo, k,
          [&](size_t n, const float* sq, uint64_t* i2, float* d2, uint32_t* c2) {
            return boost_exact(s, st, n_eff, n, sq, k, src, d_weight ? d_weight + q0 : nullptr, w.scan.sub.dFbIdx.p, i2, d2, c2, false);
          },
          o.ids, o.dist, o.cnt);
    };
    test_pause();
    RadiusKnnTally t;
    const int r = radius_knn(s, st, w.scan, n_pub, d_queries, c, &t);
    for (uint64_t b = 0; b < t.batches; ++b)   // (the int8 scan copy: every query of a batch against every row once)
      count_scan_batch(s, (size_t)std::min<uint64_t>(kSideChunk, t.queries - b * kSideChunk), n_eff, k, 1);
    s->n_i8_queries += t.queries;
    s->n_i8_fallback += t.handed;
    s->n_exhaustive += t.handed;
    s->boost_ctr[0] += t.queries - t.handed;
    s->boost_ctr[1] += t.handed;
    s->boost_ctr[2] += t.overflowed;
    s->boost_ctr[3] += t.batches * c.passes.size();
    if (r) return r;
  }
  if (n_scan == nq) return EHX_OK;
  s->boost_ctr[1] += nq - n_scan;
  return boost_exact(s, st, n_eff, nq - n_scan, d_queries + n_scan * s->dims, k, src, d_weight ? d_weight + n_scan : nullptr, nullptr,
                     out.ids + n_scan * k, out.dist + n_scan * k, out.cnt + n_scan, true);
}

// the device forms: the weights are read back and checked before anything is enqueued
int boost_device(ehx_space* s, const char* what, void* stream, size_t nq, const float* d_queries, uint32_t k, const BoostSource& src,
                 uint32_t col, uint64_t n_penalty, const float* d_weight, uint64_t* d_ids, float* d_score, uint32_t* d_count) {
  if (int rc = ehx_init(nullptr, 0)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, what, kBoostWhy, nq, &st, [&]() -> int {
    if (d_weight) {
      std::vector<float> wt(nq);
      HIP_TRY(hipMemcpyAsync(wt.data(), d_weight, nq * sizeof(float), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (int rc = boost_check_weights(wt.data(), nq, "d_weight")) return rc;
    }
    return boost_locked(s, st, nq, d_queries, k, src, col, n_penalty, d_weight, ResultBlock{d_ids, d_score, d_count, nullptr, nq, k});
  });
}

// the host forms, on the space's stream: queries and results staged in boost.host, penalties | weights in boost.dStage
int boost_host(ehx_space* s, const char* what, size_t nq, const float* queries, uint32_t k, BoostSource src, uint32_t col,
               uint64_t n_penalty, const float* weight, uint64_t* out_ids, float* out_score, uint32_t* out_count) {
  if (weight && nq)
    if (int rc = boost_check_weights(weight, nq, "weight")) return rc;
  if (int rc = ehx_init(nullptr, 0)) return rc;
  return search_on_device(s, what, kBoostWhy, nq, nullptr, [&]() -> int {
    ehx_space::Boost& w = s->boost;
    const size_t n_pen = src.form == kBoostArray ? (size_t)n_penalty : 0;
    int rc;
    if ((rc = w.dStage.ensure(std::max<size_t>(n_pen + (weight ? nq : 0), 1))) || (rc = w.host.up(s->stream, queries, nq, s->dims, k, false)))
      return rc;
    // (earlier calls' launches on other streams may still read the staged penalties)
    if ((rc = wait_searches_in_flight(s, s->stream))) return rc;
    // (pageable host memory: the runtime stages it before the call returns)
    if (n_pen) HIP_TRY(hipMemcpyAsync(w.dStage.p, src.penalty, n_pen * sizeof(float), hipMemcpyHostToDevice, s->stream));
    if (weight) HIP_TRY(hipMemcpyAsync(w.dStage.p + n_pen, weight, nq * sizeof(float), hipMemcpyHostToDevice, s->stream));
    src.penalty = w.dStage.p;
    if ((rc = boost_locked(s, s->stream, nq, w.host.q, k, src, col, n_penalty, weight ? w.dStage.p + n_pen : nullptr, w.host.out)))
      return rc;
    return w.host.out.copy_out(s->stream, out_ids, out_score, out_count, nullptr);
  });
}

}  // namespace

extern "C" {

int ehx_knn_boosted_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k, const float* d_penalty,
                           uint64_t n_penalty, const float* d_weight, uint64_t* d_out_ids, float* d_out_score,
                           uint32_t* d_out_count) {
  if (int rc = boost_check(s, n_queries, k, d_out_ids && d_out_score && d_out_count && (!n_queries || d_queries) && (!n_penalty || d_penalty)))
    return rc;
  return boost_device(s, "ehx_knn_boosted_device", stream, n_queries, d_queries, k, BoostSource{kBoostArray, d_penalty, nullptr, 0, 0}, 0,
                      n_penalty, d_weight, d_out_ids, d_out_score, d_out_count);
}

int ehx_knn_boosted(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const float* penalty, uint64_t n_penalty,
                    const float* weight, uint64_t* out_ids, float* out_score, uint32_t* out_count) {
  if (int rc = boost_check(s, n_queries, k, out_ids && out_score && out_count && (!n_queries || queries) && (!n_penalty || penalty)))
    return rc;
  return boost_host(s, "ehx_knn_boosted", n_queries, queries, k, BoostSource{kBoostArray, penalty, nullptr, 0, 0}, 0, n_penalty, weight,
                    out_ids, out_score, out_count);
}

int ehx_knn_decay_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k, uint32_t col,
                         uint32_t origin, uint32_t span, const float* d_weight, uint64_t* d_out_ids, float* d_out_score,
                         uint32_t* d_out_count) {
  if (int rc = boost_check(s, n_queries, k, d_out_ids && d_out_score && d_out_count && (!n_queries || d_queries))) return rc;
  if (int rc = boost_check_col(col)) return rc;
  return boost_device(s, "ehx_knn_decay_device", stream, n_queries, d_queries, k, BoostSource{kBoostColumn, nullptr, nullptr, origin, span},
                      col, ~0ull, d_weight, d_out_ids, d_out_score, d_out_count);
}

int ehx_knn_decay(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint32_t col, uint32_t origin, uint32_t span,
                  const float* weight, uint64_t* out_ids, float* out_score, uint32_t* out_count) {
  if (int rc = boost_check(s, n_queries, k, out_ids && out_score && out_count && (!n_queries || queries))) return rc;
  if (int rc = boost_check_col(col)) return rc;
  return boost_host(s, "ehx_knn_decay", n_queries, queries, k, BoostSource{kBoostColumn, nullptr, nullptr, origin, span}, col, ~0ull,
                    weight, out_ids, out_score, out_count);
}

}  // extern "C"
