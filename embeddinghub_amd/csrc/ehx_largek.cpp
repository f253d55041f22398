// The large-k scan route of the flat chain: exact kNN for EHX_MAX_K < k <= kLargeKScanMax and batches of at least
// kLargeKMinQueries queries on a space whose int8 scan serves a radius.  knn_device_locked alone decides the route; the
// answer is the exhaustive pass's, byte for byte (k_largek.hip's header has the argument).
//   seed     a strided sample of <= kLargeKSample rows in every query's pool (the stride, not the first rows: data ordered
//            by id still gives a representative radius); the re-rank in seed mode makes its exact k-th distance the first
//            radius and carries nothing
//   passes   the radius scan (i8_radius_scan, ehx_call.cpp) over disjoint tile ranges cut at kLargeKSample * g^j rows, no
//            bitmap, each under the threshold of the radius so far, each followed by largek_rerank_kernel, which merges the
//            pass's hits into the query's carried exact keys and lowers the radius; no host wait between passes
//   verdict  ONE read of flags and work counts behind the last pass; queries whose pool overflowed or which the bound does
//            not serve are gathered, answered by the exhaustive pass at k and scattered back (SubsetBufs::rerun)
// Growth g = 4 (EHX_LARGEK_GROWTH): a pass's hits number about k g plus what the bound cannot exclude — 1024 at k = 256,
// a quarter of a pool — and the passes log_g(rows / kLargeKSample); reasoning, A/B'd by scripts/bench_largek.py.
#include "ehx_internal.h"

namespace ehx_impl {

std::vector<TileRange> largek_passes(uint64_t n_rows, uint32_t growth) {
  std::vector<TileRange> out;
  const uint64_t n_tiles = (n_rows + kTileRows16 - 1) / kTileRows16;
  const uint64_t g = std::min<uint64_t>(16, std::max<uint64_t>(2, growth));
  uint64_t t0 = 0;
  for (uint64_t want = kLargeKSample * g; t0 < n_tiles; want *= g) {
    // (want < 2^32 * 16 while the loop runs: row ids are 32 bits wide)
    uint64_t t1 = (want + kTileRows16 - 1) / kTileRows16;
    if (want >= n_rows) t1 = n_tiles;
    out.push_back({(uint32_t)t0, (uint32_t)(t1 - t0)});
    t0 = t1;
  }
  return out;
}

bool largek_serves(const ehx_space* s, size_t nq, uint32_t k, uint64_t n_pub) {
  // (x_perm: the re-rank walks plain rows, as masked_rerank does — only single-copy graph spaces store them otherwise)
  const size_t min_q = env().largek_min_queries ? env().largek_min_queries : kLargeKMinQueries;   // (the knob: A/B only)
  return env().largek && k > EHX_MAX_K && k <= kLargeKScanMax && nq >= min_q && !s->x_perm && i8_serves_radius(s, n_pub);
}

namespace {

// The route for a batch of nq <= kSideChunk queries; *todo = the queries it leaves to the exhaustive pass.
int largek_stage(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const float* d_queries, uint32_t k,
                 const std::vector<TileRange>& passes, uint64_t stride, uint32_t n_sample, uint64_t* d_ids, float* d_dist,
                 uint32_t* d_count, std::vector<uint32_t>* todo) {
  ehx_space::LargeK& w = s->largek;
  int rc;
  if ((rc = w.dTop.ensure(nq * kLargeKMax)) || (rc = w.dTopCnt.ensure(nq)) || (rc = w.dRadius.ensure(nq)) ||
      (rc = w.dWork.ensure(nq)))
    return rc;
  auto rerank = [&](uint32_t mode, const ScanArgsI8& a, ehx_space::I8Set& sc) -> int {
    LargeKRerankArgs r = {};
    r.Q = sc.buf.dQ.p;
    r.rows = rows_view(s, n_pub);
    r.radius = w.dRadius.p;
    r.pool = sc.buf.dPool.p;
    r.pool_cnt = a.pool_cnt;
    r.ovf = a.ovf;
    r.top = w.dTop.p;
    r.top_cnt = w.dTopCnt.p;
    r.work = w.dWork.p;
    r.out_ids = d_ids;
    r.out_dist = d_dist;
    r.out_count = d_count;
    r.nq = (uint32_t)nq;
    r.k = k;
    r.mode = mode;
    HIP_TRY(launch_largek_rerank(r, st));
    return EHX_OK;
  };
  RadiusScanOut v;   // word[q]: the rows re-ranked, the sample's included
  rc = i8_radius_scan(s, st, n_pub, nq, d_queries, w.dRadius.p, passes, nullptr, 0, true,
                      [&](size_t, bool last, const ScanArgsI8& a, ehx_space::I8Set& sc) {
    if (int r = rerank(last ? kLargeKLast : kLargeKPass, a, sc)) return r;
    return last ? sc.clock.scan_end(st) : (int)EHX_OK;   // (the timed scan phase is the seed and every pass with its re-rank)
  }, w.dWork.p, &v, [&](const ScanArgsI8& a, ehx_space::I8Set& sc) {
    // stage 0 (the control words are zero, the prepared queries in place): the sample -> the first radii
    HIP_TRY(launch_largek_seed(sc.buf.dPool.p, a.pool_cnt, (uint32_t)nq, n_pub, stride, n_sample, st));
    return rerank(kLargeKSeed, a, sc);
  });
  if (rc) return rc;
  todo->clear();
  uint64_t n_pairs = 0, n_over = 0;
  for (size_t q = 0; q < nq; ++q) {
    n_pairs += v.word[q];
    if (v.flag[q]) {
      todo->push_back((uint32_t)q);
      n_over += v.flag[q] == 1u;
    }
  }
  count_scan_batch(s, nq, n_pub, k, 1);   // (the int8 scan copy: every query against every row once)
  s->n_dist += n_pairs;
  s->n_i8_queries += nq;
  s->n_i8_fallback += todo->size();
  s->largek_ctr[0] += nq - todo->size();
  s->largek_ctr[1] += todo->size();
  s->largek_ctr[2] += n_over;
  s->largek_ctr[3] += passes.size();
  return EHX_OK;
}

}  // namespace

int largek_locked(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const float* d_queries, uint32_t k,
                  uint64_t* d_ids, float* d_dist, uint32_t* d_count) {
  s->largek_ctr[4] += 1;
  const std::vector<TileRange> passes = largek_passes(n_pub, env().largek_growth);
  const uint64_t stride = (n_pub + kLargeKSample - 1) / kLargeKSample;
  const uint32_t n_sample = (uint32_t)((n_pub + stride - 1) / stride);
  test_pause();
  int rc;
  std::vector<uint32_t> todo;
  for (size_t q0 = 0; q0 < nq; q0 += kSideChunk) {
    const size_t m = std::min(kSideChunk, nq - q0);
    const float* q = d_queries + q0 * s->dims;
    uint64_t* ids = d_ids + q0 * k;
    float* dist = d_dist + q0 * k;
    uint32_t* cnt = d_count + q0;
    if ((rc = largek_stage(s, st, n_pub, m, q, k, passes, stride, n_sample, ids, dist, cnt, &todo))) return rc;
    if (todo.empty()) continue;
    // flagged queries: gathered, answered by the exhaustive pass at k, scattered back
    rc = s->largek.sub.rerun(s, st, q, todo, k, [&](size_t n, const float* sq, uint64_t* oi, float* od, uint32_t* oc) {
      return exhaustive_pass(s, n_pub, st, n, sq, k, oi, od, oc);
    }, ids, dist, cnt);
    if (rc) return rc;
    s->n_exhaustive += todo.size();
  }
  HIP_TRY(hipStreamSynchronize(st));   // (callers rely on it, as on the paged pass's)
  return EHX_OK;
}

}  // namespace ehx_impl
