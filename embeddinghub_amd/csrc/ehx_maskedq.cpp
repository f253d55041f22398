// kNN under a TABLE of row bitmaps, one per query: ehx_knn_masked_multi (host pointers) and ehx_knn_masked_multi_device.
// Query i is searched under bitmap mask_of[i]; row i of the answer is ehx_knn_masked_device's for that query alone under
// that bitmap, byte for byte — allowed rows, the ONE snapshot of the row count, order, sentinels as ehx_masked.cpp states
// them.  What a serving process needs when one micro-batch carries requests of several tenants: the scan passes run once
// per batch, not once per filter.
//   compaction   every bitmap of the table in one set of launches (k_maskedq.hip): allowed rows before every tile per mask,
//                read back ONCE together with mask_of (device form), then the ascending lists, back to back, and a sample
//                of <= 256 ids per mask
//   routing      per query through its mask, by ehx_masked.cpp's rules unchanged: the exact route for spaces the int8 radius
//                scan does not serve, k > 48, and masks of at most max(1024, rows / 128) allowed rows; the scan route else
//   grouping     the queries are ordered scan route first, then by mask (SubsetBufs: gathered, answered, scattered back;
//                skipped when they come in that order), so the queries of one mask are ONE range of the batch: the exact
//                route and the first radius are one shared-list among_locked per mask over its range
//   scan route   radius_knn with a bitmap per query in the int8 scan's flush (kMaskPerQuery, k_flati8.hip): ONE block, the
//                word offset of every query's bitmap followed by the bitmaps.  First radius: the exact k-th distance over
//                the sample of the query's OWN mask — k_radius.hip's argument holds per query.  ONE pass plan: pass j ends
//                at the first tile where some scanned mask has seen 256 * 16^j allowed rows (the pointwise maximum of the
//                scanned masks' counts), so no mask sees more allowed rows in a pass than it would alone.  Flagged queries
//                (pool overflow, or the bound does not serve them) take the exact route under their own mask.
// n_masks <= kMaskedqMaxMasks = 64: a choice (include/ehx.h says why), not a knob.
#include "ehx_internal.h"

namespace {

static_assert(kSideChunk % 256 == 0, "the offset table covers the padded query rows of one device batch");
constexpr size_t kTabWords = kSideChunk;   // word offsets in front of the bitmaps

int maskedq_check(const ehx_space* s, size_t nq, uint32_t k, const void* q, const void* masks, uint32_t n_masks, uint64_t n_bits,
                  const void* mask_of, const void* o_ids, const void* o_dist, const void* o_cnt) {
  if (!s) return fail(EHX_EINVAL, "space is NULL");
  if (int rc = masked_check(s, nq, k, q, masks, n_bits, o_ids, o_dist, o_cnt)) return rc;
  if (nq == 0) return EHX_OK;
  if (n_masks == 0) return fail(EHX_EINVAL, "n_masks is 0 with %zu queries", nq);
  if (n_masks > kMaskedqMaxMasks) return fail(EHX_EUNSUPPORTED, "n_masks=%u exceeds %u", n_masks, kMaskedqMaxMasks);
  if (!mask_of) return fail(EHX_EINVAL, "NULL mask_of");
  return EHX_OK;
}

int check_mask_of(const uint32_t* mask_of, size_t nq, uint32_t n_masks) {
  for (size_t i = 0; i < nq; ++i)
    if (mask_of[i] >= n_masks) return fail(EHX_EINVAL, "mask_of[%zu] = %u is not below n_masks = %u", i, mask_of[i], n_masks);
  return EHX_OK;
}

// Where the table comes from: n_masks bitmaps of `stride` words each, in host or device memory.
struct MaskTable {
  const uint32_t* p;
  uint64_t stride;
  bool host;
};

// an unsharded space, locked shared, scratch_mu held, its device current; everything is enqueued on `st`.  mask_of: in host
// memory and checked (host form), or nullptr: d_mask_of is read back with the allowed counts and checked then.
int maskedq_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, const MaskTable& tab,
                   uint32_t n_masks, uint64_t n_bits, const uint32_t* mask_of, const uint32_t* d_mask_of, const ResultBlock& out) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  if ((rc = check_rows_fit_lds(s, "filtered search"))) return rc;   // (before anything is enqueued)
  s->masked_ctr[4] += 1;
  ehx_space::MaskedMulti& w = s->maskedq;
  // the ONE read of the row count: the lists name rows below it only, and every later stage sees at least this prefix
  const uint64_t n_pub = s->n.load(std::memory_order_acquire);
  const uint64_t n_eff = std::min<uint64_t>(n_bits, n_pub);   // (row ids are 32 bits wide: n_pub < 2^32)
  const uint64_t words = (n_eff + 31) / 32;
  const uint32_t n_tiles = (uint32_t)((n_eff + kTileRows16 - 1) / kTileRows16);
  const size_t cum_row = (size_t)n_tiles + 1;
  if (kTabWords + (uint64_t)n_masks * words > 0xFFFFFFFFull)
    return fail(EHX_EUNSUPPORTED, "%u bitmaps of %llu rows exceed the 2^32 words of one table", n_masks, (unsigned long long)n_eff);
  if ((rc = w.dBlock.ensure(kTabWords + std::max<size_t>((size_t)n_masks * words, 1))) ||
      (rc = w.dCum.ensure((size_t)n_masks * cum_row)) || (rc = w.dSample.ensure((size_t)n_masks * kMaskedSample)))
    return rc;
  uint32_t* d_maps = w.dBlock.p + kTabWords;
  std::vector<uint32_t> cum((size_t)n_masks * cum_row, 0u), h_mask_of;
  // (earlier calls' launches on other streams may still read the block, the lists and the samples)
  if ((rc = wait_searches_in_flight(s, st))) return rc;
  if (words) {
    // the words below the row count of every bitmap, dense.  (Host words are pageable memory: the runtime stages them
    // before the call returns.)
    for (uint32_t m = 0; m < n_masks; ++m)
      HIP_TRY(hipMemcpyAsync(d_maps + (size_t)m * words, tab.p + (size_t)m * tab.stride, words * sizeof(uint32_t),
                             tab.host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
    HIP_TRY(launch_maskedq_count(d_maps, n_masks, n_eff, n_tiles, w.dCum.p, st));
    HIP_TRY(hipMemcpyAsync(cum.data(), w.dCum.p, cum.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  }
  if (!mask_of) {   // the device form: mask_of comes back with the counts — the ONE wait of the compaction
    h_mask_of.resize(nq);
    HIP_TRY(hipMemcpyAsync(h_mask_of.data(), d_mask_of, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    mask_of = h_mask_of.data();
  }
  if (words || !h_mask_of.empty()) HIP_TRY(hipStreamSynchronize(st));
  if (!h_mask_of.empty() && (rc = check_mask_of(mask_of, nq, n_masks))) return rc;   // (the outputs are unwritten)

  // the lists, back to back, and the samples
  MaskedqOffsets off = {};
  std::vector<uint64_t> n_allowed(n_masks);
  uint64_t total = 0;
  for (uint32_t m = 0; m < n_masks; ++m) {
    off.off[m] = total;
    n_allowed[m] = cum[(size_t)m * cum_row + n_tiles];
    total += n_allowed[m];
  }
  if ((rc = w.dList.ensure(std::max<uint64_t>(total, 1)))) return rc;
  HIP_TRY(launch_maskedq_fill(d_maps, n_masks, n_eff, n_tiles, w.dCum.p, off, w.dList.p, w.dSample.p, st));

  // routing, and the order the queries are answered in: the scan route's first, then by mask
  const bool scan_serves = k <= kMaskedScanMaxK && i8_serves_radius(s, n_pub);
  std::vector<char> scans(n_masks);
  for (uint32_t m = 0; m < n_masks; ++m) scans[m] = scan_serves && n_allowed[m] > masked_exact_cut(n_pub);
  std::vector<uint32_t> idx(nq);
  for (size_t i = 0; i < nq; ++i) idx[i] = (uint32_t)i;
  auto place = [&](uint32_t i) { return (scans[mask_of[i]] ? 0u : kMaskedqMaxMasks) + mask_of[i]; };
  std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return place(a) < place(b); });
  bool in_order = true;
  for (size_t i = 0; i < nq && in_order; ++i) in_order = idx[i] == i;
  std::vector<uint32_t> gm(nq);   // the mask of every query in that order
  size_t n_scan = 0;
  for (size_t i = 0; i < nq; ++i) {
    gm[i] = mask_of[idx[i]];
    n_scan += scans[gm[i]];
  }
  // [b, e): the next run of queries of one mask in [b, end)
  auto run_end = [&](size_t b, size_t end) {
    size_t e = b + 1;
    while (e < end && gm[e] == gm[b]) ++e;
    return e;
  };
  auto exact = [&](uint32_t m, size_t n, const float* q, uint64_t* ids, float* dist, uint32_t* cnt) {
    return among_locked(s, st, n, q, k, w.dList.p + off.off[m], nullptr, n_allowed[m], 0, ids, dist, cnt);
  };

  auto answer = [&](size_t, const float* gq, uint64_t* ids, float* dist, uint32_t* cnt) -> int {
    if (n_scan) {
      // ONE pass plan: the allowed rows seen are, tile by tile, those of whichever scanned mask has seen most
      std::vector<uint32_t> seen(cum_row, 0u);
      for (size_t b = 0; b < n_scan; b = run_end(b, n_scan)) {
        const uint32_t* c = cum.data() + (size_t)gm[b] * cum_row;
        for (size_t t = 0; t < cum_row; ++t) seen[t] = std::max(seen[t], c[t]);
      }
      RadiusKnn c;
      c.passes = masked_passes(seen, n_tiles);
      c.allow = w.dBlock.p;
      c.allow_bits = (uint32_t)n_eff;
      c.allow_per_query = true;
      c.out = ResultBlock{ids, dist, cnt, nullptr, n_scan, k};
      std::vector<uint32_t> offs(kTabWords);
      // stage 0 of a device batch [q0, q0 + m): its queries' word offsets into the block, and per mask the exact k nearest
      // of the mask's sample by the list scan, into the batch's rows of the output (written again behind it; not counted
      // as queries): their k-th distance is the first radius, +Inf while the sample gives fewer than k
      c.first_radius = [&](size_t m, const float* q, const ResultBlock& o, float* d_radius) -> int {
        const size_t q0 = (size_t)(q - gq) / s->dims;
        for (size_t j = 0; j < kTabWords; ++j)   // (padding queries: any bitmap, they collect nothing)
          offs[j] = (uint32_t)(kTabWords + (uint64_t)gm[q0 + std::min(j, m - 1)] * words);
        HIP_TRY(hipMemcpyAsync(w.dBlock.p, offs.data(), kTabWords * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        for (size_t b = q0; b < q0 + m;) {
          const size_t e = run_end(b, q0 + m), j = b - q0;
          const uint64_t a = n_allowed[gm[b]], stride = (a + kMaskedSample - 1) / kMaskedSample;
          if (int r = among_locked(s, st, e - b, q + j * s->dims, k, w.dSample.p + (size_t)gm[b] * kMaskedSample, nullptr,
                                   (size_t)((a + stride - 1) / stride), 0, o.ids + j * k, o.dist + j * k, o.cnt + j, false))
            return r;
          b = e;
        }
        HIP_TRY(launch_masked_radius(o.dist, o.cnt, (uint32_t)m, k, d_radius, st));
        return EHX_OK;
      };
      // the flagged queries of a device batch, mask by mask
      c.handed = [&](size_t q0, const std::vector<uint32_t>& todo, const float* q, const ResultBlock& o) -> int {
        for (size_t b = 0; b < todo.size();) {
          const uint32_t m = gm[q0 + todo[b]];
          size_t e = b + 1;
          while (e < todo.size() && gm[q0 + todo[e]] == m) ++e;
          const std::vector<uint32_t> part(todo.begin() + b, todo.begin() + e);
          if (int r = w.scan.sub.rerun(
                  s, st, q, part, k,
                  [&](size_t n, const float* sq, uint64_t* i2, float* d2, uint32_t* c2) { return exact(m, n, sq, i2, d2, c2); },
                  o.ids, o.dist, o.cnt))
            return r;
          b = e;
        }
        return EHX_OK;
      };
      RadiusKnnTally t;
      const int r = radius_knn(s, st, w.scan, n_pub, gq, c, &t);
      s->n_queries += t.queries - t.handed;   // (among_locked counts the rest)
      s->masked_ctr[0] += t.queries - t.handed;
      s->masked_ctr[1] += t.handed;
      s->masked_ctr[2] += t.overflowed;
      s->masked_ctr[3] += t.batches * c.passes.size();
      if (r) return r;
    }
    for (size_t b = n_scan; b < nq;) {   // the exact route: one shared list per mask
      const size_t e = run_end(b, nq);
      s->masked_ctr[1] += e - b;
      if (int r = exact(gm[b], e - b, gq + b * s->dims, ids + b * k, dist + b * k, cnt + b)) return r;
      b = e;
    }
    return EHX_OK;
  };
  if (in_order) return answer(nq, d_queries, out.ids, out.dist, out.cnt);
  return w.group.rerun(s, st, d_queries, idx, k, answer, out.ids, out.dist, out.cnt);
}

// host pointers in, host pointers out, on the space's stream (on_device)
int maskedq_host_locked(ehx_space* s, size_t nq, const float* queries, uint32_t k, const uint32_t* masks, uint32_t n_masks,
                        uint64_t n_bits, const uint32_t* mask_of, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  int rc;
  HostStage& h = s->maskedq.host;
  if ((rc = h.up(s->stream, queries, nq, s->dims, k, false))) return rc;
  const MaskTable tab = {masks, (n_bits + 31) / 32, true};
  if ((rc = maskedq_locked(s, s->stream, nq, h.q, k, tab, n_masks, n_bits, mask_of, nullptr, h.out))) return rc;
  return h.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
}

}  // namespace

extern "C" {

int ehx_knn_masked_multi_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                const uint32_t* d_masks, uint32_t n_masks, uint64_t n_bits, const uint32_t* d_mask_of,
                                uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count) {
  if (int rc = maskedq_check(s, n_queries, k, d_queries, d_masks, n_masks, n_bits, d_mask_of, d_out_ids, d_out_dist, d_out_count))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_knn_masked_multi_device", kMaskedWhy, n_queries, &st, [&] {
    const MaskTable tab = {d_masks, (n_bits + 31) / 32, false};
    return maskedq_locked(s, st, n_queries, d_queries, k, tab, n_masks, n_bits, nullptr, d_mask_of,
                          ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_knn_masked_multi(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const uint32_t* masks,
                         uint32_t n_masks, uint64_t n_bits, const uint32_t* mask_of, uint64_t* out_ids, float* out_dist,
                         uint32_t* out_count) {
  if (int rc = maskedq_check(s, n_queries, k, queries, masks, n_masks, n_bits, mask_of, out_ids, out_dist, out_count)) return rc;
  if (int rc = check_mask_of(mask_of, n_queries, n_masks)) return rc;   // (before anything is enqueued)
  return search_on_device(s, "ehx_knn_masked_multi", kMaskedWhy, n_queries, nullptr, [&] {
    return maskedq_host_locked(s, n_queries, queries, k, masks, n_masks, n_bits, mask_of, out_ids, out_dist, out_count);
  });
}

}  // extern "C"
