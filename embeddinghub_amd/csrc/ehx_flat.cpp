// The exact flat chain: scan plans, the fp32 / fp16 / int8 matrix-core pipelines with their certified re-rank, the
// exhaustive canonical pass, and the engine fall-through of one device batch (knn_device_locked).
#include "ehx_internal.h"

namespace ehx_impl {

// plan one scan pass over `n_tiles` row tiles
ScanPlan plan_scan(uint32_t nq, uint32_t n_tiles, uint32_t k, int n_cus) {
  ScanPlan p;
  p.q_tiles = (nq + kTileQ - 1) / kTileQ;
  p.q_rows = p.q_tiles * kTileQ;
  p.n_tiles = n_tiles;
  p.kprime = k + 8;  // EHX_MAX_K + 8 = 56 < kCandSlots: a compacted candidate list always has free slots
  // one persistent workgroup per CU: grid ~= n_cus, split as q_tiles x n_chunks
  uint32_t chunks = (uint32_t)n_cus / p.q_tiles;
  if (chunks < 1) chunks = 1;
  if (chunks >= 8) chunks &= ~7u;
  if (chunks > p.n_tiles) chunks = p.n_tiles ? p.n_tiles : 1;
  p.n_chunks = chunks;
  p.tiles_per_chunk = p.n_tiles ? (p.n_tiles + chunks - 1) / chunks : 0;
  p.grid = p.q_tiles * p.n_chunks;
  p.xcd_map = (p.n_chunks % 8 == 0) ? 1u : 0u;
  return p;
}

std::vector<ScanPass> plan_cascade(uint32_t nq, uint32_t n_tiles, uint32_t k, int n_cus, uint64_t first_tiles, uint64_t growth) {
  std::vector<ScanPass> passes;
  uint64_t done = 0;
  for (uint64_t cum = first_tiles; cum * 2 < n_tiles; cum *= growth) {
    passes.push_back({(uint32_t)done, plan_scan(nq, (uint32_t)(cum - done), k, n_cus)});
    done = cum;
  }
  passes.push_back({(uint32_t)done, plan_scan(nq, (uint32_t)(n_tiles - done), k, n_cus)});
  return passes;
}

// one flat pipeline: prepared queries -> scan -> merge -> canonical re-rank.
//   f16 = false: the fp32 MFMA scan (k_flat8.hip), exact on its own.
//   f16 = true : the fp16 MFMA filter scan (k_flat16.hip); per-query certification flags land in
//                s->scr.verdict and the caller re-runs the flagged remainder through the fp32 scan.
static int flat_pass(ehx_space* s, uint64_t n_pub, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, uint64_t* d_ids,
                     float* d_dist, uint32_t* d_count, bool f16) {
  Engine& E = engine();
  // A cascade of scan passes over growing row ranges (one tile per workgroup, then x8 per pass): after
  // every pass the per-workgroup candidate lists are merged into the query's running best-64 and its
  // k'-th best key — an upper bound of the final k'-th best — becomes the threshold the next pass starts
  // from.  A pass over 8x the rows seen so far appends only ~7 k' candidates per query, so nearly every
  // tile epilogue stays on its branch-free fast path; a single pass would have every workgroup warm its
  // thresholds up from +inf (~k' ln(rows/k') appends per list).
  const uint32_t tile_rows = f16 ? kTileRows16 : kTileRows;
  const uint32_t n_tiles = (uint32_t)((n_pub + tile_rows - 1) / tile_rows);
  constexpr uint32_t lpc = kScanListsPerChunk;
  // Filter scan: a SAMPLE pass first — the first 8 tiles (2048 rows) are scanned in dump mode (all scores to
  // HBM, no candidate lists) and sample_select turns them into the k'-th best score per query, so not even
  // the first real pass has to warm its lists up from +inf (which costs ~3 list compactions per list).
  constexpr uint32_t kSampleTiles = 8;
  const bool sample = f16 && n_tiles >= 256;
  // the filter scan gets its first thresholds from the sample pass below, so its cascade can start wide (128 tiles) and
  // grow x16: three scan launches at 10 M rows; without one, pass 0 is one tile per workgroup and the passes grow x8, on
  // spaces of at least 16 such passes; everything smaller is one pass
  const uint32_t whole_chunks = plan_scan((uint32_t)nq, n_tiles, k, E.n_cus).n_chunks;
  const bool x8 = !sample && n_tiles >= 16 * whole_chunks;
  std::vector<ScanPass> passes =
      plan_cascade((uint32_t)nq, n_tiles, k, E.n_cus, sample ? 128 : x8 ? whole_chunks : n_tiles, sample ? 16 : 8);
  ScanPlan p = passes.back().plan;  // (q_tiles, q_rows, kprime are the same for every pass)
  test_pause();
  if (f16) {
    // the filter keeps k' = k + 22 candidates (<= 56): the certification needs the k'-th lower bound to
    // clear the k-th exact distance by the fp16 error bound, so it wants more slack than the fp32 scan
    const uint32_t kp = k + 22 > 56 ? (k + 8 > 56 ? k + 8 : 56) : k + 22;
    for (auto& ps : passes) ps.plan.kprime = kp;
    p.kprime = kp;
  } else if (s->dims > 1024) {
    // fp32 scan at large d: the certification margin grows like d * 2^-24 (cert_margin) while the gap between the
    // k-th and the k'-th best of isotropic data shrinks like ln(k'/k) / sqrt(d): widen k' (up to the 56 a
    // 64-slot list allows) so that typical data still certifies instead of falling to the exhaustive pass
    const double grow = std::exp(std::min(4.0, 5.3e-7 * std::pow((double)s->dims, 1.5)));
    uint32_t kp = (uint32_t)std::ceil((double)k * grow);
    kp = std::min<uint32_t>(56, std::max<uint32_t>(k + 8, kp));
    for (auto& ps : passes) ps.plan.kprime = kp;
    p.kprime = kp;
  }
  uint32_t lists_total = 0, grid_max = 0;  // every pass reuses the same list slots
  for (auto& ps : passes) {
    lists_total = std::max(lists_total, ps.plan.n_chunks * lpc);
    grid_max = std::max(grid_max, ps.plan.grid);
  }
  int rc;
  if ((rc = s->scr.dQ.ensure((size_t)p.q_rows * s->ld))) return rc;
  if ((rc = s->scr.dCand.ensure((size_t)grid_max * 512 * kCandSlots))) return rc;
  if ((rc = s->scr.dPart.ensure((size_t)p.q_rows * lists_total * p.kprime))) return rc;
  if ((rc = s->scr.dMerged.ensure((size_t)p.q_rows * 64))) return rc;
  if ((rc = s->scr.dGthr.ensure((size_t)p.q_rows + 8))) return rc;  // +8: instrumentation slots of profiling builds
  if ((rc = s->scr.dScanErr.ensure_zeroed_once(1))) return rc;
  if ((rc = s->scr.verdict.ensure(p.q_rows))) return rc;
  if (f16) {
    if ((rc = s->scr.dQ16.ensure(scanq16_halves(p.q_rows, s->ld16)))) return rc;
    if ((rc = s->scr.dQgamma.ensure(p.q_rows))) return rc;
    if ((rc = s->scr.dQuv.ensure(p.q_rows))) return rc;
    if (sample && (rc = s->scr.dSample.ensure((size_t)kSampleTiles * kTileRows16 * p.q_rows))) return rc;
  }
  // scratch buffers are shared by all callers: order this pipeline after the previous one even
  // when it was enqueued on a different stream
  {
    int rcw = wait_searches_in_flight(s, st);
    if (rcw) return rcw;
  }
  BatchClock& clock = s->clock;   // (every batch timed and in the ring; an empty space's outside it)
  if ((rc = clock.begin(st, n_pub ? 1u : BatchClock::kOutOfRing))) return rc;
  HIP_TRY(launch_prep_queries(d_queries, (uint32_t)nq, s->dims, s->ld, p.q_rows, s->metric, s->scr.dQ.p, st));
  if (f16)
    HIP_TRY(launch_prep_queries16(d_queries, (uint32_t)nq, s->dims, s->ld16, p.q_rows, s->metric, s->scr.dQ16.p,
                                  s->scr.dQgamma.p, s->scr.dQuv.p, st));
  if (n_pub == 0) {
    // empty space: every query returns count 0
    HIP_TRY(hipMemsetAsync(s->scr.dMerged.p, 0xFF, (size_t)p.q_rows * 64 * sizeof(uint64_t), st));
    if ((rc = clock.scan_begin(st)) || (rc = clock.scan_end(st))) return rc;
  } else {
    // the cascade's passes through the engine's kernel, each followed by its merge
    auto cascade = [&](auto& a, auto launch) -> int {
      for (size_t i = 0; i < passes.size(); ++i) {
        const bool last = i + 1 == passes.size();
        set_scan_pass(a, passes[i].plan, passes[i].tile0);
        HIP_TRY(launch(a, st));
        if (last && (rc = clock.scan_end(st))) return rc;   // (the final merge is outside the timed scan phase)
        HIP_TRY(launch_flat_merge(s->scr.dPart.p, (uint32_t)nq, passes[i].plan.n_chunks * lpc, p.kprime, s->scr.dMerged.p, st,
                                  lists_total, i > 0, last ? nullptr : (unsigned long long*)s->scr.dGthr.p));
      }
      return EHX_OK;
    };
    HIP_TRY(hipMemsetAsync(s->scr.dGthr.p, 0xFF, (size_t)p.q_rows * sizeof(uint64_t), st));
    if ((rc = clock.scan_begin(st))) return rc;
    if (f16) {
      ScanArgs16 h;
      scan_args_shared(h, s->scr.dCand.p, s->scr.dPart.p, s->scr.dScanErr.p, s->scr.dGthr.p, p, lists_total, n_pub);
      h.Q = s->scr.dQ16.p;
      h.X = s->f16.dX16.p;
      h.rowp = s->f16.dRowp16.p;
      h.qgamma = s->scr.dQgamma.p;
      h.eps = scan16_eps(s->dims);
      h.cos = s->metric == EHX_METRIC_COSINE;
      h.ld = s->ld16;
      if (sample) {
        ScanPlan sp = plan_scan((uint32_t)nq, kSampleTiles, k, E.n_cus);
        set_scan_pass(h, sp, 0);
        h.dump = s->scr.dSample.p;
        HIP_TRY(launch_flat_scan16(h, st));
        h.dump = nullptr;
        HIP_TRY(launch_sample_select(s->scr.dSample.p, kSampleTiles * kTileRows16, p.q_rows, (uint32_t)nq, p.kprime,
                                     (unsigned long long*)s->scr.dGthr.p, st));
      }
      if ((rc = cascade(h, launch_flat_scan16))) return rc;
    } else {
      ScanArgs a;
      scan_args_shared(a, s->scr.dCand.p, s->scr.dPart.p, s->scr.dScanErr.p, s->scr.dGthr.p, p, lists_total, n_pub);
      a.Q = s->scr.dQ.p;
      a.X = s->rows.dX.p;
      a.x_half = (uint32_t)s->x_half;
      a.rowp = s->rows.dRowp.p;
      a.ld = s->ld;
      if ((rc = cascade(a, launch_flat_scan8))) return rc;
    }
  }
  RerankArgs r;
  r.Q = s->scr.dQ.p;
  r.rows = rows_view(s, n_pub);
  r.merged = s->scr.dMerged.p;
  r.out_ids = d_ids;
  r.out_dist = d_dist;
  r.out_count = d_count;
  r.n_uncertified = s->scr.verdict.count.p;  // (the caller reads and clears it)
  r.nq = (uint32_t)nq;
  r.k = k;
  r.kprime = p.kprime;
  if (f16) r.quv = s->scr.dQuv.p;
  r.max_sumsq = s->rows.dMaxSumsq.p;
  r.uncert_flags = s->scr.verdict.flags.p;
  HIP_TRY(launch_rerank(r, st));
  if ((rc = clock.finish(st))) return rc;
  s->n_rerank += (uint64_t)nq * p.kprime;
  return EHX_OK;
}

// which scan engine answers first on this space right now: EHX_ENGINE_* (include/ehx.h)
// for the prefix of n_pub rows (the caller's snapshot: the unsafe-row counts are read after it, see ehx_space::h_unsafe)
int resolve_engine(const ehx_space* s, uint64_t n_pub) {
  if (s->params.mode != EHX_MODE_FLAT || s->scan_sel == EHX_SCAN_F32 || n_pub == 0) return EHX_ENGINE_F32;
  if (s->scan_sel == EHX_SCAN_AUTO && s->has8 && s->h_unsafe8.load(std::memory_order_relaxed) == 0 && n_pub >= s->i8_min_rows)
    return EHX_ENGINE_I8;
  if (s->has16 && s->h_unsafe.load(std::memory_order_relaxed) == 0) return EHX_ENGINE_F16;
  return EHX_ENGINE_F32;
}

// EHX_I8_COUNT / EHX_I8_DEBUG, diagnosis only: the scan's epilogue counters of this batch (builds with -DEHX_I8_COUNT=1) and
// what its uncertified queries look like, on stderr.  Waits for the stream.
static int i8_diagnose(ehx_space::I8Set::Buffers& b, hipStream_t st, size_t nq, uint32_t k, uint32_t width,
                       const uint32_t* d_ovf, const float* d_dist) {
  HIP_TRY(hipStreamSynchronize(st));
  if (env().i8_count) {
    unsigned long long c[8] = {0};
    HIP_TRY(hipMemcpy(c, b.dCnt.p, sizeof(c), hipMemcpyDeviceToHost));
    fprintf(stderr, "[i8 count] tests %llu alarms %llu row-block alarms %llu trips %llu (cumulative)\n", c[0], c[1], c[2], c[3]);
  }
  if (env().i8_debug) {
    std::vector<uint32_t> fl(nq), ov(nq);
    std::vector<float4> qp(nq);
    std::vector<float2> uv(nq);
    std::vector<uint64_t> mg(nq * width);
    std::vector<float> od(nq * k);
    HIP_TRY(hipMemcpy(fl.data(), b.verdict.flags.p, nq * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ov.data(), d_ovf, nq * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(qp.data(), b.dQp8.p, nq * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(uv.data(), b.dQuv.p, nq * sizeof(float2), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(mg.data(), b.dMerged8.p, nq * width * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(od.data(), d_dist, nq * k * 4, hipMemcpyDeviceToHost));
    int shown = 0;
    for (size_t q = 0; q < nq && shown < 6; ++q) {
      if (!fl[q]) continue;
      ++shown;
      auto S = [&](int i) { return mg[q * width + i] == ~0ull ? INFINITY : ordered_to_f32((uint32_t)(mg[q * width + i] >> 32)); };
      fprintf(stderr, "[i8 debug] q=%zu ovf=%u tmin=%g S[0]=%g S[63]=%g S[127]=%g S[255]=%g kth_dist=%g u=%g v=%g\n", q, ov[q],
              qp[q].w, S(0), S(63), S(127), S(255), od[q * k + k - 1], uv[q].x, uv[q].y);
    }
  }
  return EHX_OK;
}

// The int8 filter pipeline (k_flati8.hip, k_select.hip): prepared queries -> sample pass (first thresholds) ->
// cascade of collect passes, x4 in rows, each followed by select256 (running best 256 + the next threshold) ->
// rerank256 (canonical distances of the k' = 128 best lower bounds, top-k, certificate).  Per-query verdicts land in
// the set's own Verdict, like those of flat_pass in the space's.
// `set`: which of the space's two scratch sets (ehx_space::I8Set) this batch runs in; the caller holds that set's mutex.
// *kprime_used: the logical length of the candidate list the batch ran with.
static int flat_pass8(ehx_space* s, uint64_t n_pub, int set, hipStream_t st, size_t nq, const float* d_queries, uint32_t k,
                      uint64_t* d_ids, float* d_dist, uint32_t* d_count, uint32_t* kprime_used) {
  Engine& E = engine();
  ehx_space::I8Set& sc = s->i8set[set];
  const uint32_t n_tiles = (uint32_t)((n_pub + kTileRows16 - 1) / kTileRows16);
  // The cascade's shape.  Shards of at least 2048 tiles (524 288 rows): a first pass of 128 tiles that aims for 64 keys
  // per query, then x8 in rows per pass; smaller ones: 512 tiles, min(512, 2 k') keys, x4 (one or two passes).  Round 5,
  // same box, 60 batches each (profiles/r05_i_ab_cascade.jsonl): 1.25 M x 768 1.190 -> 1.146 ms per batch, 10 M x 768
  // 6.64 -> 6.58, 6.25 M x 128 1.154 -> 1.139 (256 / x8 / 64: 12.5 M x 1536 fp16 18.7 -> 18.4); at 200 000 x 768 the
  // second pass the small first pass brings costs more than its tighter threshold saves (scan phase 0.248 -> 0.274).
  // A loose first pass is the expensive one: its threshold comes from a 2048-row sample and every key it lets through
  // is a trip through the epilogue's slow path.  EHX_I8_FIRST_TILES / EHX_I8_GROWTH / EHX_I8_FIRST_KEYS override.
  const bool big = n_tiles >= 2048;
  const uint32_t growth = env().i8_growth ? env().i8_growth : (big ? 8u : 4u);
  const double safety = [] {
    // rank of the next pass's threshold = 256 x (share of the rows seen) x safety.  2: the last pass of a 10 M-row batch
    // runs under the 138th best of the first 27 % (about 510 rows below it overall: the list still fills to 256, the
    // certificate's floor is unchanged) instead of the 256th (950 rows): fewer alarms, fewer keys — 7.64 -> 7.46 ms per
    // batch, 0 fallbacks over 25 batches; 1.5: 7.44; 1: a query falls to the next engine (profiles/r03_e_i8_safety_sweep.jsonl)
    return env().i8_safety;  // (EHX_I8_SAFETY; 1e9: always the 256th best)
  }();
  // EHX_I8_SYNC = N > 0: lock-step by tile of the query-tile workgroups that stream one row chunk, tolerance N tiles
  // (k_flati8.hip); 0 / unset: off.
  const int sync_mode = env().i8_sync;
  const bool use_sync = sync_mode > 0;
  constexpr uint32_t kSampleTiles = 8;
  // The int8 bound leaves ~60-75 rows per query ON AVERAGE that it cannot exclude from the top-10 at 10 M rows
  // (scripts/studies/int8_filter_bound.py), with a heavy tail — a query whose 10th neighbour is unusually far has
  // several times as many — and a query whose list is too short costs a whole scan by the next engine.  So the
  // threshold rank is the full width of the running list; the re-rank reads only as many candidates as it needs.
  // The list is 256 keys wide to begin with.  Longer rows leave more survivors (the bound is ~0.02 in dot units whatever
  // the dimension, while the spread of the dot products shrinks like 1/sqrt(d)): at 12.5 M x 1536 a fifth of the
  // queries needed more than 256 candidates and went to the next engine, which doubled the batch time.  A space whose
  // batches keep losing queries that way doubles its list (i8_adapt), up to kMerged8Max.
  const uint32_t width = s->i8_width.load(std::memory_order_relaxed);  // (read once: another batch may widen it meanwhile)
  const long kprime_env = env().i8_kprime;
  // How many candidates a query keeps is what the scan's epilogue pays for (every key collected is a trip through its
  // slow path, and the waves of a workgroup wait for each other at every stage: 1.25 M x 768 collected 470 keys per
  // query, 70 % of the epilogue's tests alarmed).  The rows a query cannot exclude grow with the index (60-75 on average
  // at 10 M x 768, fewer on a shard of 1 M), so the list's LOGICAL length k' follows the row count — 128 below 4 M rows,
  // else the full width (64 was tried: no query lost at 1 - 1.25 M x 768 in 50 batches, 3 of 256 at 100 k x 768); rows
  // of 1024 dims and more always get the full width (the bound is ~1.3e-2 in dot units whatever d while the scores'
  // spread shrinks like 1/sqrt(d): 18 000 x 2048 needs its 256) — and, like the width, doubles when queries lose their
  // certificate because the list was too short (i8_adapt).
  // Short rows need fewer still: the bound is a smaller share of the scores' spread (0.15 sigma at d = 128 against 0.36
  // at d = 768), and on short rows the hit path is what a tile's time is made of (two stages of matrix work per tile at
  // d = 128).  Measured, 46 000 queries each, 0 fallbacks (profiles/r04_p_kprime_short_rows.jsonl): 6.25 M x 128 k' 256 /
  // 128 / 64 = 1.380 / 1.277 / 1.238 ms per batch, 1 M x 128 0.447 (128) / 0.414 (64); 4 M x 384 and 10 M x 256 are fine
  // with 128 (1.762 against 1.825, 2.620 against 2.722 ms) and lose queries by the hundred with 64.
  uint32_t kp_auto = n_pub >= 4000000 ? 256u : 128u;
  if (s->dims <= 128) kp_auto = 64u;
  else if (s->dims < 512) kp_auto = 128u;
  if (s->dims >= 1024) kp_auto = width;
  const uint32_t kp_want = std::max(kp_auto, s->i8_kprime_min.load(std::memory_order_relaxed));
  const uint32_t kprime = kprime_env >= 64 ? (uint32_t)std::min<long>(kprime_env, (long)width) : std::min(kp_want, width);
  s->i8_kprime_last.store(kprime, std::memory_order_relaxed);
  *kprime_used = kprime;
  // First pass: up to 512 tiles (131 072 rows) under a threshold taken from the sample at a LOW rank, chosen so that
  // the pass collects ~1000 keys per query (any threshold is sound, see sample_select256_kernel); then x4 in rows per
  // pass under the 256th best so far.
  const uint32_t kFirstTiles = env().i8_first_tiles ? env().i8_first_tiles : (big ? 128u : 512u);
  const std::vector<ScanPass> passes = plan_cascade((uint32_t)nq, n_tiles, k, E.n_cus, kFirstTiles, growth);
  // rank of the threshold the select after pass i publishes for pass i + 1: the kprime-th best is always valid; while
  // only a share f of the rows has been seen, the final kprime-th best is expected near rank kprime * f of the prefix, so
  // rank kprime * f * safety (>= 16) is a much tighter threshold that is still above it — fewer keys collected, fewer
  // epilogue alarms in the middle passes.  Sound whatever happens (the certificate uses the smallest threshold ever
  // applied, qparams.w).
  auto rank_after = [&](size_t i) -> uint32_t {
    if (i + 1 >= passes.size()) return kprime;
    const double f = (double)((uint64_t)(passes[i + 1].tile0) * kTileRows16) / (double)n_pub;
    return (uint32_t)std::min<double>(kprime, std::max<double>(16.0, std::ceil(kprime * f * safety)));
  };
  // The first pass runs under a threshold taken from the sample at a LOW rank, chosen for the number of keys the pass
  // should collect: a single pass has to fill the list with room to spare (2 x its logical length — every key collected
  // is a trip through the epilogue's slow path, and on a 20 000-row space 4 x meant a hit in 2.6 % of all pairs); with more
  // passes to come it only has to deliver the next threshold's rank (twice over, at least min(512, 2 k') keys: round 2
  // collected 1024 and spent more than half of the first pass in the epilogue's slow path).
  const uint64_t first_rows = (uint64_t)passes.front().plan.n_tiles * kTileRows16;
  const uint64_t first_keys_env = env().i8_first_keys;  // (EHX_I8_FIRST_KEYS: keys per query the first pass aims for)
  const uint64_t first_floor = first_keys_env ? first_keys_env : (big ? 64ull : std::min<uint64_t>(512, 2ull * kprime));
  const uint64_t first_keys = std::min<uint64_t>(
      2048, passes.size() == 1 ? 2ull * kprime : std::max<uint64_t>(first_floor, 2ull * rank_after(0)));
  const uint32_t sample_rank =
      (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(8, first_keys * kSampleTiles * kTileRows16 / first_rows));
  const ScanPlan p = passes.back().plan;  // (q_tiles, q_rows are the same for every pass)
  test_pause();
  uint32_t grid_max = 0, chunks_max = 0;
  for (auto& ps : passes) {
    grid_max = std::max(grid_max, ps.plan.grid);
    chunks_max = std::max(chunks_max, ps.plan.n_chunks);
  }
  if (chunks_max > 256) return fail(EHX_EINTERNAL, "scan plan with %u chunks", chunks_max);
  int rc;
  ScanArgsI8 a;
  if ((rc = i8_scan_args(s, sc.buf, p, n_pub, &a))) return rc;
  if ((rc = sc.buf.dSample8.ensure((size_t)kSampleTiles * kTileRows16 * p.q_rows))) return rc;
  if ((rc = sc.buf.dMerged8.ensure((size_t)p.q_rows * width))) return rc;
  if ((rc = sc.buf.verdict.ensure(p.q_rows, ehx_space::I8Set::kStampWords))) return rc;
  // The LONG passes (the compile-time-slot loop, chunks of at least 64 tiles, mapped to XCDs; at 10 M x 768: pass 3 and the
  // last) are stamped — every workgroup's start and finish, riding home behind the verdict's count — and read their tile
  // ranges from the share planner's table (ehx_balance.h): a power-limited pass ends with its slowest XCD, so the XCDs get
  // shares in proportion to the rates the stamps of earlier batches showed.  EHX_I8_BALANCE=0: stamps only, uniform split.
  constexpr uint32_t kTable = kBalanceMaxChunks + 1;
  std::vector<int> stamp_slot(passes.size(), -1);
  sc.n_stamped = 0;
  // (the shards of a row-sharded space keep the plain passes: G devices, G sets of XCDs, not measured)
  if (s->ld8 % 256u == 0u && !s->keyless) {
    const uint32_t min_tpc = s->i8_balance_min_tpc.load(std::memory_order_relaxed);
    uint32_t off = 0;
    for (size_t i = passes.size(); i-- > 0 && sc.n_stamped < ehx_space::I8Set::kStampedPasses;) {
      const ScanPlan& pl = passes[i].plan;
      if (!pl.xcd_map || pl.tiles_per_chunk < min_tpc || pl.grid > ehx_space::I8Set::kStampGrid || pl.n_chunks > kBalanceMaxChunks)
        continue;
      ehx_space::I8Set::StampedPass& sp = sc.stamped[sc.n_stamped];
      sp.key = BalanceState::key_of(pl.q_tiles, pl.n_chunks, pl.tiles_per_chunk);
      sp.grid = pl.grid;
      sp.q_tiles = pl.q_tiles;
      sp.n_tiles = pl.n_tiles;
      sp.n_chunks = pl.n_chunks;
      sp.tile0 = passes[i].tile0;
      sp.stamp_off = off;
      off += 2 * pl.grid;
      double f[kXcds];
      s->i8_balance.factors(sp.key, f);
      // (a table the planner could not validate is not used: the kernel's own arithmetic, which sp.bounds then restates)
      sp.table = env().i8_balance && balance_bounds(f, pl.n_tiles, pl.n_chunks, sp.bounds);
      if (!sp.table) balance_uniform(pl.n_tiles, pl.n_chunks, sp.bounds);
      stamp_slot[i] = (int)sc.n_stamped++;
    }
    if (sc.n_stamped &&
        (rc = sc.buf.hBounds.ensure((size_t)ehx_space::I8Set::kStampedPasses * kTable, hipHostMallocCoherent | hipHostMallocMapped, true)))
      return rc;
    sc.buf.verdict.riding = off;
  } else {
    sc.buf.verdict.riding = 0;
  }
  uint32_t* const pool_cnt = a.pool_cnt;
  uint32_t* const ovf = a.ovf;
  uint32_t* sync = sc.buf.dI8Ctl.p + 2 * (size_t)p.q_rows;
  // (a caller's stream other than the space's own: searches already in flight there and here finish first)
  if ((rc = wait_searches_in_flight(s, st))) return rc;
  if ((rc = sc.clock.begin(st, env().stats_every))) return rc;
  HIP_TRY(launch_prep_queries_i8(d_queries, (uint32_t)nq, s->dims, s->ld, s->ld8, p.q_rows, s->metric, sc.buf.dQ.p,
                                 sc.buf.dQ8.p, sc.buf.dQp8.p, sc.buf.dQuv.p, sc.buf.dThr8.p, sc.buf.dI8Ctl.p, st));
  auto scan = [&](const ScanPlan& pl, uint32_t tile0) -> hipError_t {
    set_scan_pass(a, pl, tile0);
    return launch_flat_scan_i8(a, st);
  };
  if ((rc = sc.clock.scan_begin(st))) return rc;
  {  // sample pass: lower bounds of the first 2048 rows -> thr[q] = the k'-th best of them
    ScanPlan sp = plan_scan((uint32_t)nq, kSampleTiles, k, E.n_cus);
    a.dump = sc.buf.dSample8.p;
    a.sync = nullptr;
    HIP_TRY(scan(sp, 0));
    a.dump = nullptr;
    HIP_TRY(launch_sample_select256(sc.buf.dSample8.p, kSampleTiles * kTileRows16, p.q_rows, (uint32_t)nq, sample_rank,
                                    sc.buf.dThr8.p, st));
  }
  for (size_t i = 0; i < passes.size(); ++i) {
    const bool last = i + 1 == passes.size();
    a.sync = nullptr;
    if (use_sync && passes[i].plan.xcd_map && p.q_tiles > 1 && passes[i].plan.tiles_per_chunk >= 4 &&
        passes[i].plan.n_chunks * 4u <= kSyncWordsI8) {   // (four progress words per chunk: ADVICE r05)
      a.sync = sync;
      a.sync_tol = (uint32_t)sync_mode;
      if (i > 0) HIP_TRY(hipMemsetAsync(sync, 0, kSyncWordsI8 * sizeof(uint32_t), st));
    }
    a.bounds = nullptr;
    a.stamps = nullptr;
    if (stamp_slot[i] >= 0) {
      const ehx_space::I8Set::StampedPass& sp = sc.stamped[stamp_slot[i]];
      a.stamps = (uint64_t*)sc.buf.verdict.extra_dev() + sp.stamp_off;
      if (sp.table) {   // (the set's batch before this one has long read its tables: the set's mutex, enqueue to outcome)
        uint32_t* const tab = sc.buf.hBounds.p + (size_t)stamp_slot[i] * kTable;
        std::copy(sp.bounds, sp.bounds + sp.n_chunks + 1, tab);
        a.bounds = tab;
      }
    }
    HIP_TRY(scan(passes[i].plan, passes[i].tile0));
    // (the last select and the re-rank are outside the timed scan phase, like flat_pass's final merge)
    if (last && (rc = sc.clock.scan_end(st))) return rc;
    HIP_TRY(launch_select256(sc.buf.dPool.p, pool_cnt, kPoolCap, (uint32_t)nq, rank_after(i), sc.buf.dMerged8.p, width, i > 0,
                             sc.buf.dThr8.p, sc.buf.dQp8.p, st));
  }
  Rerank256Args r;
  r.Q = sc.buf.dQ.p;
  r.X = s->rows.dX.p;
  r.x_half = (uint32_t)s->x_half;
  r.inv_norm = s->rows.dInv.p;
  r.merged = sc.buf.dMerged8.p;
  r.width = width;
  r.ovf = ovf;
  r.quv = sc.buf.dQuv.p;
  r.qparams = sc.buf.dQp8.p;
  r.max_sumsq = s->rows.dMaxSumsq.p;
  r.out_ids = d_ids;
  r.out_dist = d_dist;
  r.out_count = d_count;
  r.n_uncertified = sc.buf.verdict.count.p;
  r.uncert_flags = sc.buf.verdict.flags.p;
  r.nq = (uint32_t)nq;
  r.k = k;
  r.kprime = kprime;
  r.n = (uint32_t)n_pub;
  r.dims = s->dims;
  r.ld = s->ld;
  r.metric = s->metric;
  HIP_TRY(launch_rerank256(r, st));
  if ((env().i8_count || env().i8_debug) && (rc = i8_diagnose(sc.buf, st, nq, k, width, ovf, d_dist))) return rc;
  if ((rc = sc.clock.finish(st))) return rc;
  s->n_rerank += (uint64_t)nq * kprime;
  return EHX_OK;
}

// Exhaustive canonical pass: the canonical distance of every row for `nq` queries (k_flat.hip:
// exhaustive_kernel), merged and emitted through the re-rank with the certification switched off (the keys
// are exact).  Serves (a) queries no matrix-core scan can certify and (b) requests with k > EHX_MAX_K, which
// it answers in pages of 64 results (each page keeps the keys strictly above the previous page's last).
int exhaustive_pass(ehx_space* s, uint64_t n_pub, hipStream_t st, size_t nq, const float* d_queries, uint32_t k,
                    uint64_t* d_ids, float* d_dist, uint32_t* d_count) {
  // rows per workgroup: 8192 when there are queries enough to fill the chip; fewer queries get smaller blocks (down to
  // one 64-row step) so that about 2048 workgroups share the shard — the keys are exact whatever the partition
  const uint32_t kRowsPerBlock =
      (uint32_t)std::min<uint64_t>(8192, std::max<uint64_t>(64, ((uint64_t)n_pub * nq / 2048 + 63) / 64 * 64));
  const uint32_t n_blocks = (uint32_t)((n_pub + kRowsPerBlock - 1) / kRowsPerBlock);
  const uint32_t pages = (k + 63) / 64;
  const RowsView rows = rows_view(s, n_pub);
  int rc;
  if ((rc = s->scr.dQ.ensure(nq * s->ld))) return rc;
  if ((rc = s->scr.dPart.ensure(nq * n_blocks * 64))) return rc;
  if ((rc = s->scr.dMerged.ensure(nq * 64))) return rc;
  if ((rc = s->scr.verdict.ensure(nq))) return rc;
  if (pages > 1 && (rc = s->scr.dGthr.ensure(nq + 8))) return rc;
  {
    int rcw = wait_searches_in_flight(s, st);
    if (rcw) return rcw;
  }
  if ((rc = s->clock.begin(st, BatchClock::kOutOfRing))) return rc;
  HIP_TRY(launch_prep_queries(d_queries, (uint32_t)nq, s->dims, s->ld, (uint32_t)nq, s->metric, s->scr.dQ.p, st));
  if ((rc = s->clock.scan_begin(st))) return rc;
  for (uint32_t pg = 0; pg < pages; ++pg) {
    if (pg) test_pause();
    const uint64_t* floor = pg ? s->scr.dGthr.p : nullptr;
    HIP_TRY(launch_exhaustive(s->scr.dQ.p, rows, kRowsPerBlock, n_blocks, (uint32_t)nq, floor, s->scr.dPart.p, st));
    HIP_TRY(launch_flat_merge(s->scr.dPart.p, (uint32_t)nq, n_blocks, 64, s->scr.dMerged.p, st, n_blocks));
    if (pg + 1 < pages) HIP_TRY(launch_set_floor(s->scr.dMerged.p, (uint32_t)nq, s->scr.dGthr.p, st));
    RerankArgs r;
    r.Q = s->scr.dQ.p;
    r.rows = rows;
    r.merged = s->scr.dMerged.p;
    r.out_ids = d_ids;
    r.out_dist = d_dist;
    r.out_count = d_count;
    r.n_uncertified = s->scr.verdict.count.p;   // (never raised: exact keys are never flagged)
    r.nq = (uint32_t)nq;
    r.k = std::min<uint32_t>(64, k - pg * 64);
    r.kprime = 64;
    r.uncert_flags = s->scr.verdict.flags.p;
    r.exact_keys = 1;
    r.out_stride = k;
    r.out_offset = pg * 64;
    HIP_TRY(launch_rerank(r, st));
  }
  if ((rc = s->clock.scan_end(st)) || (rc = s->clock.finish(st))) return rc;
  s->n_dist += (uint64_t)nq * n_pub * pages;
  return EHX_OK;
}

// Adaptation of the int8 list after a batch of `nq` queries that ran with logical length `kprime`, lost `n_failed`
// queries to the next engine, `n_short` of them because their candidate LIST was too short.  Called for EVERY int8
// batch, clean ones included, whichever path ran it (i8_stage_outcome; the pipelined path once skipped it for clean
// batches: its score never decayed, and two losing batches any distance apart widened the list).
// The list is too short for this data when batches keep losing queries to the next engine — which re-reads every
// row for them, nearly a batch's worth of time however few they are (12.5 M x 1536: 13 queries in 10 batches cost
// 45 % of the run).  Only queries whose LIST was the failing part count (the re-rank flags them 2: a pool overflow,
// exact ties at the threshold or lost candidates are not cured by width, and a width, once raised, stays).  A batch of
// at least 64 queries that loses more than 2 % of them that way widens the list at once; otherwise every losing
// batch adds 4 to a score that decays by 1 per clean batch, and 8 widens (two losing batches close together).
static void i8_adapt(ehx_space* s, size_t nq, size_t n_failed, size_t n_short, uint32_t kprime) {
  std::lock_guard<std::mutex> l(s->i8_adapt_mu);
  if (n_short == 0) s->i8_fb_score = s->i8_fb_score ? s->i8_fb_score - 1 : 0;
  else s->i8_fb_score += 4;
  const uint32_t width = s->i8_width.load(std::memory_order_relaxed);
  if (!((nq >= 64 && n_short * 50 > nq) || s->i8_fb_score >= 8)) return;
  // (a batch that ran with an older, shorter list than the space has by now says nothing about the present one)
  if (kprime < std::min(width, std::max(s->i8_kprime_min.load(std::memory_order_relaxed), kprime))) {
    s->i8_fb_score = 0;
    return;
  }
  if (!(width < kMerged8Max || kprime < width)) return;
  if (kprime < width) s->i8_kprime_min.store(std::min(width, 2 * kprime), std::memory_order_relaxed);  // k' first
  else {
    s->i8_width.store(width * 2, std::memory_order_relaxed);
    s->i8_kprime_min.store(width * 2, std::memory_order_relaxed);
  }
  s->i8_fb_score = 0;
  if (env().i8_trace)
    fprintf(stderr, "[ehx i8] %zu of %zu queries uncertified (%zu by a short list): candidate list now %u of %u\n", n_failed,
            nq, n_short, std::max(s->i8_kprime_min.load(), kprime), s->i8_width.load());
}

void count_scan_batch(ehx_space* s, size_t nq, uint64_t n_pub, uint32_t k, uint64_t elem_bytes) {
  s->n_queries += nq;
  s->n_dist += (uint64_t)nq * n_pub;
  // SURVEY §8d brute force bytes per batch: N*d*s + B*d*4 + B*k*12 (s = bytes per element the scan reads)
  s->bytes_algo += n_pub * s->dims * elem_bytes + (uint64_t)nq * s->dims * 4ull + (uint64_t)nq * k * 12ull;
}

int i8_stage_enqueue(ehx_space* s, uint64_t n_pub, int set, hipStream_t st, hipEvent_t after, bool pipelined, size_t nq,
                     const float* d_queries, uint32_t k, uint64_t* d_ids, float* d_dist, uint32_t* d_count, I8Outcome* o) {
  // (this batch's launches go onto the stream as one block: per-batch scan windows stay clean)
  std::lock_guard<std::mutex> ql(s->i8_enqueue_mu);
  if (after) HIP_TRY(hipStreamWaitEvent(st, after, 0));
  int rc = flat_pass8(s, n_pub, set, st, nq, d_queries, k, d_ids, d_dist, d_count, &o->kprime);
  if (rc) return rc;
  Verdict& v = s->i8set[set].buf.verdict;
  return pipelined ? v.post_and_record(st) : v.post(st);
}

// The stamps of the batch's long passes have landed with its verdict: every pass's relative XCD rates go into the space's
// factors for its shape (the next batch planned uses them), and the final pass is kept for the test hooks.
static void i8_balance_outcome(ehx_space* s, ehx_space::I8Set& sc) {
  const uint64_t* const words = (const uint64_t*)sc.buf.verdict.extra_landed();
  for (uint32_t j = sc.n_stamped; j-- > 0;) {   // (in the cascade's order: slot 0 is its final pass)
    const ehx_space::I8Set::StampedPass& sp = sc.stamped[j];
    const uint64_t* const stamps = words + sp.stamp_off;
    uint32_t tiles[kXcds];
    double rate[kXcds];
    balance_xcd_tiles(sp.bounds, sp.n_chunks, tiles);
    const bool ok = balance_rates(stamps, sp.grid, tiles, rate);
    if (ok) s->i8_balance.update(sp.key, rate);
    if (j == 0) {
      ehx_space::I8BalanceLast& l = s->i8_balance_last;
      std::lock_guard<std::mutex> g(l.mu);
      ++l.batches;
      l.grid = sp.grid;
      l.q_tiles = sp.q_tiles;
      l.n_tiles = sp.n_tiles;
      l.n_chunks = sp.n_chunks;
      l.tile0 = sp.tile0;
      l.table = sp.table ? 1u : 0u;
      std::copy(sp.bounds, sp.bounds + sp.n_chunks + 1, l.bounds);
      l.stamps.assign(stamps, stamps + 2 * (size_t)sp.grid);
      s->i8_balance.factors(sp.key, l.factors);
      std::copy(rate, rate + kXcds, l.rate);
    }
  }
  sc.n_stamped = 0;
}

int i8_stage_outcome(ehx_space* s, uint64_t n_pub, int set, hipStream_t st, size_t nq, uint32_t k, I8Outcome* o) {
  Verdict& v = s->i8set[set].buf.verdict;
  o->failed.clear();
  o->n_short = 0;
  i8_balance_outcome(s, s->i8set[set]);
  int rc;
  if (v.read() && (rc = v.collect(st, nq, nullptr, &o->failed, &o->n_short))) return rc;
  count_scan_batch(s, nq, n_pub, k, 1);   // (the int8 scan copy)
  s->n_i8_queries += nq;
  s->n_i8_fallback += o->failed.size();
  i8_adapt(s, nq, o->failed.size(), o->n_short, o->kprime);
  return EHX_OK;
}

// Device pipeline of a flat space: up to three stages, each run only for the queries the previous one
// could not certify, so the answer is always the exhaustive fp32 answer in the oracle's arithmetic:
//   0. int8 matrix-core filter scan + certified re-rank      (all queries; spaces with the int8 scan copy, >= i8_min_rows)
//   1. fp16 matrix-core filter scan + certified re-rank      (what stage 0 could not certify / spaces without it)
//   2. fp32 matrix-core scan + certified re-rank              (what stage 1 could not certify / fp32-only spaces)
//   3. canonical distance of every row                        (what stage 2 could not certify: near-ties finer
//                                                              than the certification margin; kMaxExhaustive
//                                                              queries per launch group, as many groups as needed)
// One host round trip (8 bytes) per stage to read its verdict (Verdict, ehx_own.h).
// knn_device_locked: the gates in front of the chain and stage 0; flat_chain_rest: stages 1 to 3.
int knn_device_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k,
                      uint64_t* d_ids, float* d_dist, uint32_t* d_count, uint64_t n_pub) {
  if (k == 0 || nq == 0) return EHX_OK;
  if (nq > (1u << 24)) return fail(EHX_EINVAL, "too many queries in one call: %zu", nq);
  if (s->params.mode == EHX_MODE_GRAPH) {
    // searchKnn(q, k) keeps max(ef, k) results and returns the k best (index.cc:41): any k the result list holds
    if (k > EHX_MAX_K_PAGED) return fail(EHX_EUNSUPPORTED, "graph mode: k=%u exceeds %u", k, EHX_MAX_K_PAGED);
    return knn_graph_locked(s, st, nq, d_queries, k, d_ids, d_dist, d_count);
  }
  // the ONE read of the row count in this search (a caller that has a snapshot already passes it)
  if (n_pub == kNoSnapshot) n_pub = s->n.load(std::memory_order_acquire);
  if (k > EHX_MAX_K) {
    // beyond the candidate capacity of one scan pass: a batch of k <= kLargeKScanMax on an int8 space takes the large-k scan
    // route (ehx_largek.cpp); everything else the exhaustive canonical pass, paged (exact, HBM-bound — the whole shard is
    // read once per page of 64 results and per query)
    if (k > EHX_MAX_K_PAGED) return fail(EHX_EUNSUPPORTED, "k=%u exceeds EHX_MAX_K_PAGED=%u", k, EHX_MAX_K_PAGED);
    if (n_pub == 0) {
      HIP_TRY(hipMemsetAsync(d_count, 0, nq * sizeof(uint32_t), st));
      return EHX_OK;
    }
    // (no int8 scratch set is held here: stage 0's lock is taken further down, the route takes its own)
    if (largek_serves(s, nq, k, n_pub)) return largek_locked(s, st, n_pub, nq, d_queries, k, d_ids, d_dist, d_count);
    int rc2 = exhaustive_pass(s, n_pub, st, nq, d_queries, k, d_ids, d_dist, d_count);
    if (rc2) return rc2;
    s->n_queries += nq;
    s->n_exhaustive += nq;
    HIP_TRY(hipStreamSynchronize(st));   // (callers rely on it)
    return EHX_OK;
  }
  // ONE query against a small shard — the reference's own usage: one NearestNeighbor RPC, one query (server.cc:172-210;
  // BASELINE configs[0]: 10 k x 128).  The matrix-core engines are built for batches: their dozen launches (sample pass,
  // cascade, selects, re-rank) take ~0.55 ms for a single query on 10 k rows, where the exhaustive canonical pass — the
  // oracle's arithmetic over every row, exact by construction, three launches — reads the rows once.  Concurrent single
  // queries never get here alone: ehx_knn coalesces them into device batches.  (EHX_SMALL_EXACT_BYTES=0 switches it off.)
  const uint64_t small_bytes = env().small_exact_bytes;
  if (nq == 1 && s->scan_sel == EHX_SCAN_AUTO && n_pub > 0 && n_pub * s->ld * s->esz <= small_bytes) {
    int rc2 = exhaustive_pass(s, n_pub, st, nq, d_queries, k, d_ids, d_dist, d_count);
    if (rc2) return rc2;
    s->n_queries += nq;
    s->n_exhaustive += nq;
    return EHX_OK;   // (no wait here: the caller's copy-back or stream order is the wait)
  }
  const int eng = resolve_engine(s, n_pub);
  test_pause();
  if (eng != EHX_ENGINE_I8) return flat_chain_rest(s, st, n_pub, nq, d_queries, k, d_ids, d_dist, d_count, eng, nullptr);
  I8Outcome o;
  {
    // (scratch set 0, held for the stage and its verdict: host batches may be using both sets through knn_host_direct's
    // pipelined path at the same time)
    std::lock_guard<std::mutex> set_lock(s->i8set[0].mu);
    int rc = i8_stage_enqueue(s, n_pub, 0, st, nullptr, false, nq, d_queries, k, d_ids, d_dist, d_count, &o);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = i8_stage_outcome(s, n_pub, 0, st, nq, k, &o))) return rc;
  }
  if (o.failed.empty()) return EHX_OK;
  return flat_chain_rest(s, st, n_pub, nq, d_queries, k, d_ids, d_dist, d_count, eng, &o);
}

int flat_chain_rest(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const float* d_queries, uint32_t k,
                    uint64_t* d_ids, float* d_dist, uint32_t* d_count, int eng, const I8Outcome* i8) {
  constexpr size_t kMaxExhaustive = 32;
  enum { kFilter, kF32, kExhaustive };
  int rc;
  Verdict& v = s->scr.verdict;
  // run one stage on `subset` (nullptr = every query); *unc = global indices it could not certify
  auto stage = [&](int kind, const std::vector<uint32_t>* subset, std::vector<uint32_t>* unc) -> int {
    const size_t m = subset ? subset->size() : nq;
    auto pass = [&](size_t n, const float* q, uint64_t* oi, float* od, uint32_t* oc) {
      return kind == kExhaustive ? exhaustive_pass(s, n_pub, st, n, q, k, oi, od, oc)
                                 : flat_pass(s, n_pub, st, n, q, k, oi, od, oc, kind == kFilter);
    };
    rc = subset ? s->scr.sub.rerun(s, st, d_queries, *subset, k, pass, d_ids, d_dist, d_count)
                : pass(nq, d_queries, d_ids, d_dist, d_count);
    if (rc) return rc;
    unc->clear();
    if ((rc = v.post(st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    size_t n_short;   // (only the int8 list adapts to it)
    return v.read() ? v.collect(st, m, subset, unc, &n_short) : EHX_OK;
  };

  std::vector<uint32_t> todo, next;
  bool all = true;  // `todo` = every query
  const bool filter = (eng == EHX_ENGINE_I8 || eng == EHX_ENGINE_F16) && s->has16 && s->h_unsafe.load(std::memory_order_relaxed) == 0;
  if (i8) {
    todo = i8->failed;
    all = todo.size() * 2 > nq;
  } else {  // (a batch's work counters are those of its first engine)
    count_scan_batch(s, nq, n_pub, k, filter ? 2 : s->esz);
  }
  if (filter) {
    const size_t m = all ? nq : todo.size();
    if ((rc = stage(kFilter, all ? nullptr : &todo, &next))) return rc;
    s->n_filter_queries += m;
    s->n_filter_fallback += next.size();
    if (next.empty()) return EHX_OK;
    todo.swap(next);
    all = todo.size() * 2 > nq;  // most of the batch: just run it all through the fp32 scan
  }
  if ((rc = stage(kF32, all ? nullptr : &todo, &next))) return rc;
  if (next.empty()) return EHX_OK;
  todo.swap(next);
  // Whatever the matrix-core scans could not certify is answered by the exhaustive canonical pass, kMaxExhaustive
  // queries at a time (bounded scratch): an EHX_OK result is always the certified exhaustive top-k.
  std::vector<uint32_t> chunk;
  for (size_t i0 = 0; i0 < todo.size(); i0 += kMaxExhaustive) {
    chunk.assign(todo.begin() + i0, todo.begin() + std::min(todo.size(), i0 + kMaxExhaustive));
    if ((rc = stage(kExhaustive, &chunk, &next))) return rc;
    s->n_exhaustive += chunk.size();
    if (!next.empty()) {  // cannot happen: exact keys are never flagged
      s->n_uncertified_final += next.size();
      return fail(EHX_EINTERNAL, "%zu queries left uncertified by the exhaustive canonical pass", next.size());
    }
  }
  return EHX_OK;
}

}  // namespace ehx_impl
