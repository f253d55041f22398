// The large-k scan route of the flat chain: exact kNN for EHX_MAX_K < k <= kLargeKScanMax and batches of at least
// kLargeKMinQueries queries on a space whose int8 scan serves a radius.  knn_device_locked alone decides the route; the
// answer is the exhaustive pass's, byte for byte.  The route is the falling-radius kNN (radius_knn, ehx_call.cpp;
// k_radius.hip's header has the kernels and the argument) with no bitmap; this file holds what is the route's own:
//   seed     a strided sample of <= kLargeKSample rows (the stride, not the first rows: data ordered by id still gives a
//            representative radius)
//   passes   disjoint tile ranges cut at kLargeKSample * g^j rows
//   exact    the queries the route hands on are answered by the exhaustive pass at k
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
  // (x_perm: the re-rank walks plain rows, as the bitmap search's does — only single-copy graph spaces store them otherwise)
  const size_t min_q = env().largek_min_queries ? env().largek_min_queries : kLargeKMinQueries;   // (the knob: A/B only)
  return env().largek && k > EHX_MAX_K && k <= kLargeKScanMax && nq >= min_q && !s->x_perm && i8_serves_radius(s, n_pub);
}

int largek_locked(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const float* d_queries, uint32_t k,
                  uint64_t* d_ids, float* d_dist, uint32_t* d_count) {
  s->largek_ctr[4] += 1;
  RadiusKnn c;
  c.passes = largek_passes(n_pub, env().largek_growth);
  c.seed_stride = (n_pub + kLargeKSample - 1) / kLargeKSample;
  c.n_sample = (uint32_t)((n_pub + c.seed_stride - 1) / c.seed_stride);
  c.out = ResultBlock{d_ids, d_dist, d_count, nullptr, nq, k};
  c.exact = [&](size_t n, const float* sq, uint64_t* oi, float* od, uint32_t* oc) {
    return exhaustive_pass(s, n_pub, st, n, sq, k, oi, od, oc);
  };
  test_pause();
  RadiusKnnTally t;
  const int rc = radius_knn(s, st, s->largek, n_pub, d_queries, c, &t);
  for (uint64_t b = 0; b < t.batches; ++b)   // (the int8 scan copy: every query of a batch against every row once)
    count_scan_batch(s, (size_t)std::min<uint64_t>(kSideChunk, t.queries - b * kSideChunk), n_pub, k, 1);
  s->n_i8_queries += t.queries;
  s->n_i8_fallback += t.handed;
  s->n_exhaustive += t.handed;
  s->largek_ctr[0] += t.queries - t.handed;
  s->largek_ctr[1] += t.handed;
  s->largek_ctr[2] += t.overflowed;
  s->largek_ctr[3] += t.batches * c.passes.size();
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(st));   // (callers rely on it, as on the paged pass's)
  return EHX_OK;
}

}  // namespace ehx_impl
