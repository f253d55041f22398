// kNN under row bitmaps.  Exact: ehx_knn_masked (host pointers) and ehx_knn_masked_device under ONE bitmap,
// ehx_knn_masked_multi and ehx_knn_masked_multi_device under a TABLE of bitmaps, query i under bitmap mask_of[i]; on the
// graph path: ehx_graph_knn_masked* and ehx_graph_knn_masked_multi* (the section at the end).  Row r is allowed iff r < n_bits, r is below the call's ONE
// snapshot of the row count and bit r & 31 of word r >> 5 is set; the answer is ehx_knn_among's with the ascending list of
// allowed rows, byte for byte (k_radius.hip's header has the argument), and row i of a table's answer is the one-bitmap
// answer for query i alone under its bitmap.  One bitmap is a table of one: ONE plan (masked_plan) and ONE answer over it
// (masked_answer) serve every entry point, the graph walk's exact route included.  The answer itself is filtered_answer over
// a FilterView — "which row test in the flush, which compacted table" — which the search under a label column
// (ehx_labeled.cpp) shares: masked_answer only states the bitmaps' view.
//   compaction   every bitmap in one set of launches (k_masked.hip): allowed rows before every 256-row tile per mask, read
//                back ONCE (the host plans the passes from them) together with mask_of (a table's device form), and the
//                ascending lists, back to back (one mask: filled in front of that wait; several: behind it, placed by
//                the counts); where a mask takes the scan route, a sample of <= 256 ids per mask
//   routing      per query through its mask: the exact route for spaces the range search's int8 path does not serve,
//                k > 48, and masks of at most max(1024, rows / 128) allowed rows; the scan route else
//   grouping     the queries are ordered scan route first, then by mask (SubsetBufs: gathered, answered, scattered back;
//                skipped when they come in that order, as one mask always does), so the queries of one mask are ONE range
//                of the batch: the exact route and the first radius are one shared-list among_locked per mask over its range
//   exact route  among_locked over the mask's list
//   scan route   the falling-radius kNN (radius_knn, ehx_call.cpp; k_radius.hip's header has the kernels and the argument)
//                with the bitmap in the int8 scan's flush — the batch's one bitmap, or with several a bitmap per query
//                (kMaskPerQuery, k_flati8.hip): ONE block, the word offset of every query's bitmap followed by the bitmaps.
//                First radius: the exact k-th distance over the sample of the query's OWN mask, taken by the list scan (its
//                tiles share the sample's rows between queries).  ONE pass plan, cut by ALLOWED rows seen (4096, 65536,
//                ...: sound wherever the bitmap's rows cluster): pass j ends at the first tile where some scanned mask has
//                seen 256 * 16^j allowed rows (the pointwise maximum of the scanned masks' counts), so no mask sees more
//                allowed rows in a pass than it would alone.  The queries it hands on — pool overflow, or the bound does
//                not serve them — take the exact route under their own mask.
// The plan, the cut between the routes and the check of mask_of are declared in ehx_internal.h: the range search under row
// bitmaps (ehx_rangem.cpp) compacts its table with the same masked_plan.  So are THE routing rule of every filtered
// search (filter_routes_cut / _gate) and the view over a plan of bitmaps (masked_view: ehx_groupedm.cpp's too).
// n_masks <= kMaskedMaxMasks = 64: a choice (include/ehx.h says why), not a knob.
// Entry scaffold and host staging are ehx_call.cpp's (search_shared / on_device, HostStage).
#include "ehx_internal.h"

namespace {

constexpr uint32_t kMaskedScanMaxK = 48;    // the scan route carries <= k keys per query between passes: the certified engines' k
constexpr uint64_t kMaskedSample = 256;     // allowed rows in the sample, at most (sample_stride, ehx_kernels.h)
constexpr uint64_t kMaskedPassGrowth = 16;  // pass j ends where kMaskedSample * 16^j allowed rows have been seen
constexpr const char* kMaskedWhy = "filtered search over shards is not built yet";
static_assert(kSideChunk % 256 == 0, "the offset table covers the padded query rows of one device batch");

int masked_check(const ehx_space* s, size_t nq, uint32_t k, const void* q, const void* mask, uint64_t n_bits,
                 const void* o_ids, const void* o_dist, const void* o_cnt) {
  int rc = ehx_init(nullptr, 0);   // (no device: EHX_ENODEVICE, whatever else is wrong with the call)
  if (rc) return rc;
  if ((rc = check_batch_call(s, nq, k, "k", false, o_ids && o_dist && o_cnt && (!nq || q)))) return rc;
  if (n_bits && !mask) return fail(EHX_EINVAL, "NULL mask with n_bits = %llu", (unsigned long long)n_bits);
  return EHX_OK;
}

// tile ranges of the scan passes: pass j (j = 1, 2, ...; the sample is stage 0) ends at the first tile where the allowed
// rows seen reach kMaskedSample * 16^j, the last pass takes the rest.  cum[t] = allowed rows in tiles [0, t), non-decreasing.
std::vector<TileRange> masked_passes(const std::vector<uint32_t>& cum, uint32_t n_tiles) {
  std::vector<TileRange> out;
  uint32_t t0 = 0;
  for (uint64_t want = kMaskedSample * kMaskedPassGrowth; t0 < n_tiles; want *= kMaskedPassGrowth) {
    // (the first t with cum[t] >= want)
    uint32_t t1 = (uint32_t)(std::lower_bound(cum.begin() + t0 + 1, cum.begin() + n_tiles + 1, want,
                                              [](uint32_t c, uint64_t w) { return (uint64_t)c < w; }) - cum.begin());
    if (t1 > n_tiles || cum[n_tiles] <= want) t1 = n_tiles;
    out.push_back({t0, t1 - t0});
    t0 = t1;
  }
  return out;
}

// The bitmaps of a call on the device, bitmap m at *d_maps + m * words (words: those of the n_eff rows below the row count):
// ONE device bitmap where it lies; host words and every table dense in masked.dBlock behind the offset words — copied there,
// or written there by the table's builder (MaskTable::build).  (Host words are pageable memory: the runtime stages them
// before the call returns.)
int masked_maps(ehx_space* s, hipStream_t st, const MaskTable& tab, uint64_t n_eff, const uint32_t** d_maps) {
  int rc;
  const bool in_place = tab.n_masks == 1 && !tab.host && !tab.build;
  const uint64_t words = (n_eff + 31) / 32;
  if (kTabWords + (uint64_t)tab.n_masks * words > 0xFFFFFFFFull)
    return fail(EHX_EUNSUPPORTED, "%u bitmaps of %llu rows exceed the 2^32 words of one table", tab.n_masks,
                (unsigned long long)n_eff);
  ehx_space::Masked& w = s->masked;
  if (!in_place && (rc = w.dBlock.ensure(kTabWords + std::max<size_t>((size_t)tab.n_masks * words, 1)))) return rc;
  // (earlier calls' launches on other streams may still read the block, the lists and the samples)
  if ((rc = wait_searches_in_flight(s, st))) return rc;
  *d_maps = in_place ? tab.p : w.dBlock.p + kTabWords;
  if (tab.build) return words ? tab.build(n_eff, words, w.dBlock.p + kTabWords, st) : (int)EHX_OK;
  for (uint32_t m = 0; !in_place && words && m < tab.n_masks; ++m)
    HIP_TRY(hipMemcpyAsync(w.dBlock.p + kTabWords + (size_t)m * words, tab.p + (size_t)m * tab.stride, words * sizeof(uint32_t),
                           tab.host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
  return EHX_OK;
}

}  // namespace

namespace ehx_impl {

int masked_table_check(const ehx_space* s, size_t nq, uint32_t k, const void* q, const void* masks, uint32_t n_masks,
                       uint64_t n_bits, const void* mask_of, const void* o_ids, const void* o_dist, const void* o_cnt) {
  if (!s) return fail(EHX_EINVAL, "space is NULL");
  if (int rc = masked_check(s, nq, k, q, masks, n_bits, o_ids, o_dist, o_cnt)) return rc;
  if (nq == 0) return EHX_OK;
  if (n_masks == 0) return fail(EHX_EINVAL, "n_masks is 0 with %zu queries", nq);
  if (n_masks > kMaskedMaxMasks) return fail(EHX_EUNSUPPORTED, "n_masks=%u exceeds %u", n_masks, kMaskedMaxMasks);
  if (!mask_of) return fail(EHX_EINVAL, "NULL mask_of");
  return EHX_OK;
}

// At most this many allowed rows: the exact route.  max(1024, rows / 128), MEASURED (scripts/bench_masked.py, 1 M x 768
// cosine, batch 1024, k = 10: the list scan costs what the scan route costs at 7 697 allowed rows, 0.77 % of the space;
// profiles/masked_bench.jsonl).
uint64_t masked_exact_cut(uint64_t n_pub) { return std::max<uint64_t>(1024, n_pub / 128); }

int check_mask_of(const uint32_t* mask_of, size_t nq, uint32_t n_masks) {
  for (size_t i = 0; i < nq; ++i)
    if (mask_of[i] >= n_masks) return fail(EHX_EINVAL, "mask_of[%zu] = %u is not below n_masks = %u", i, mask_of[i], n_masks);
  return EHX_OK;
}

// an unsharded space, locked shared, scratch_mu held, its device current; everything is enqueued on `st`.  mask_of: in host
// memory and checked; or d_mask_of (a table's device form): read back with the allowed counts — the ONE wait of the
// compaction — and checked then, the outputs unwritten; or neither: every query is mask 0 and nothing is read back for it.
int masked_plan(ehx_space* s, hipStream_t st, const MaskTable& tab, uint64_t n_bits, size_t nq, const uint32_t* mask_of,
                const uint32_t* d_mask_of, MaskedPlan* p) {
  int rc;
  ehx_space::Masked& w = s->masked;
  // the ONE read of the row count: the lists name rows below it only, and every later stage sees at least this prefix
  p->n_pub = s->n.load(std::memory_order_acquire);
  p->n_eff = std::min<uint64_t>(n_bits, p->n_pub);   // (row ids are 32 bits wide: n_pub < 2^32)
  p->words = (p->n_eff + 31) / 32;
  p->n_tiles = (uint32_t)((p->n_eff + kTileRows16 - 1) / kTileRows16);
  p->n_masks = tab.n_masks;
  p->mask_of = mask_of;
  const uint32_t n_masks = tab.n_masks, n_tiles = p->n_tiles;
  if ((rc = masked_maps(s, st, tab, p->n_eff, &p->d_maps))) return rc;
  if ((rc = w.dCum.ensure((size_t)n_masks * (n_tiles + 1)))) return rc;
  p->cum.assign((size_t)n_masks * (n_tiles + 1), 0u);
  // the lists (list_rows: what they hold together, at most), behind the counts
  auto fill = [&](uint64_t list_rows) -> int {
    if (int r = w.dList.ensure(std::max<uint64_t>(list_rows, 1))) return r;
    HIP_TRY(launch_masked_fill(p->d_maps, p->words, n_masks, p->n_eff, n_tiles, w.dCum.p, p->off, w.dList.p, st));
    return EHX_OK;
  };
  // Several masks: the lists' offsets come from the counts, so they are filled behind the wait.  ONE mask: its list starts
  // at 0 and holds at most n_eff ids — both known now — so it is filled in front of the wait, the order the one-bitmap call
  // had before it was folded into this function.  HOISTED AFTER A MEASUREMENT (profiles/masked_unify_ab.jsonl, DESIGN §e.16
  // "One masked path"; 1 M x 768 cosine, batch 1024, k = 10, the one-bitmap call on the exact route at density 0.005,
  // median of three medians against the range of the library before the fold): count, wait, fill for every n_masks
  // 1.3844 ms against 1.3772..1.3793; hoisted 1.3765 in 1.3688..1.3781 and, a session later, 1.3780 against
  // 1.3699..1.3767.  Code the fold did not touch (the graph walk) missed its own range by as much in those sessions: the
  // figures allow the parent's order, they do not prove it the faster one.
  const bool fill_early = n_masks == 1;
  if (n_tiles) {
    HIP_TRY(launch_masked_count(p->d_maps, p->words, n_masks, p->n_eff, n_tiles, w.dCum.p, st));
    if (fill_early && (rc = fill(p->n_eff))) return rc;
    HIP_TRY(hipMemcpyAsync(p->cum.data(), w.dCum.p, p->cum.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  }
  if (d_mask_of) {
    p->mask_of_read.resize(nq);
    HIP_TRY(hipMemcpyAsync(p->mask_of_read.data(), d_mask_of, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    p->mask_of = p->mask_of_read.data();
  }
  if (n_tiles || d_mask_of) HIP_TRY(hipStreamSynchronize(st));
  if (d_mask_of && (rc = check_mask_of(p->mask_of, nq, n_masks))) return rc;
  // where the lists start, back to back
  p->n_allowed.resize(n_masks);
  uint64_t total = 0;
  for (uint32_t m = 0; m < n_masks; ++m) {
    p->off.off[m] = total;
    p->n_allowed[m] = p->cum_of(m)[n_tiles];
    total += p->n_allowed[m];
  }
  return fill_early && n_tiles ? (int)EHX_OK : fill(total);   // (no tile: nothing is launched, the list is one spare entry)
}

}  // namespace ehx_impl

namespace ehx_impl {

bool filter_scan_serves(const ehx_space* s, uint32_t k, uint64_t n_pub) {
  return k <= kMaskedScanMaxK && i8_serves_radius(s, n_pub);
}

void filter_routes_cut(bool scan_serves, uint64_t cut, const uint64_t* n_allowed, uint32_t n_filters, char* scans) {
  for (uint32_t f = 0; f < n_filters; ++f) scans[f] = scan_serves && n_allowed[f] > cut;
}

void filter_routes_gate(const uint32_t* filter_of, size_t nq, size_t min_scan_queries, uint32_t n_filters, char* scans) {
  if (!min_scan_queries || !n_filters) return;
  size_t naming = 0;
  for (size_t i = 0; i < nq; ++i) naming += scans[filter_of ? filter_of[i] : 0u] != 0;
  if (naming < min_scan_queries) std::fill(scans, scans + n_filters, (char)0);
}

FilterView masked_view(ehx_space* s, hipStream_t st, const MaskedPlan& p, const char* scans, uint32_t* head_of) {
  ehx_space::Masked& w = s->masked;
  const bool per_query = p.n_masks > 1;   // one mask: the batch's ONE bitmap in the flush, nothing grouped, no offsets
  for (uint32_t m = 0; m < p.n_masks; ++m) head_of[m] = (uint32_t)(kTabWords + (uint64_t)m * p.words);
  FilterView v;
  v.n_pub = p.n_pub;
  v.n_eff = p.n_eff;
  v.n_tiles = p.n_tiles;
  v.n_filters = p.n_masks;
  v.n_allowed = p.n_allowed.data();
  v.off = p.off.off;
  v.filter_of = p.mask_of;
  v.scans = scans;
  v.cum = p.cum.data();
  v.d_list = w.dList.p;
  v.sample = &w.dSample;
  v.allow = per_query ? w.dBlock.p : p.d_maps;
  v.allow_per_query = per_query;
  v.d_head = per_query ? w.dBlock.p : nullptr;
  v.head_of = head_of;
  v.samples = [s, st, &p]() -> int {
    ehx_space::Masked& m = s->masked;
    if (int r = m.dSample.ensure((size_t)p.n_masks * kMaskedSample)) return r;
    HIP_TRY(launch_masked_samples(m.dList.p, p.off, m.dCum.p, p.n_masks, p.n_tiles, m.dSample.p, st));
    return EHX_OK;
  };
  return v;
}

// The exact answer over compacted row filters — bitmaps (masked_answer, below) or the labels of a column (ehx_labeled.cpp):
// per filter the scan route where v.scans says so, else the list scan.  Only the row test in the scan's flush (v.allow*), the
// table the compaction filled and the counters differ between the two.
int filtered_answer(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, const FilterView& v,
                    const ResultBlock& out) {
  ehx_space::Masked& w = s->masked;
  const uint32_t n_filters = v.n_filters, n_tiles = v.n_tiles;
  auto filter_at = [&](size_t i) { return v.filter_of ? v.filter_of[i] : 0u; };
  auto row_of = [&](uint32_t f) { return (size_t)(v.scan_of ? v.scan_of[f] : f); };   // of cum and of the samples
  // routing, and the order the queries are answered in: the scan route's first, then by filter — with v.shared_min > 1 the
  // list route's filters that fewer queries name behind the others: they take ONE per-query launch together
  std::vector<uint32_t> named(v.shared_min > 1 ? n_filters : 0, 0u);
  for (size_t i = 0; i < nq && !named.empty(); ++i) named[filter_at(i)] += 1;
  auto tier = [&](uint32_t f) { return v.scans[f] ? 0u : (named.empty() || named[f] >= v.shared_min) ? 1u : 2u; };
  auto place = [&](uint32_t i) {
    const uint32_t f = filter_at(i);
    return (uint64_t)tier(f) * n_filters + f;
  };
  std::vector<uint32_t> idx(nq), gm(nq);   // gm: the filter of every query in that order
  for (size_t i = 0; i < nq; ++i) idx[i] = (uint32_t)i;
  auto before = [&](uint32_t a, uint32_t b) { return place(a) < place(b); };
  const bool in_order = std::is_sorted(idx.begin(), idx.end(), before);   // (one filter: always)
  if (!in_order) std::stable_sort(idx.begin(), idx.end(), before);
  size_t n_scan = 0, n_shared = 0;
  for (size_t i = 0; i < nq; ++i) {
    gm[i] = filter_at(idx[i]);
    n_scan += tier(gm[i]) == 0u;
    n_shared += tier(gm[i]) == 1u;
  }
  // [b, e): the next run of queries of one filter in [b, end)
  auto run_end = [&](size_t b, size_t end) {
    size_t e = b + 1;
    while (e < end && gm[e] == gm[b]) ++e;
    return e;
  };
  auto exact = [&](uint32_t f, size_t n, const float* q, uint64_t* ids, float* dist, uint32_t* cnt) {
    return among_locked(s, st, n, q, k, v.d_list + v.off[f], nullptr, v.n_allowed[f], 0, ids, dist, cnt);
  };

  auto answer = [&](size_t, const float* gq, uint64_t* ids, float* dist, uint32_t* cnt) -> int {
    if (n_scan) {
      // ONE pass plan: the allowed rows seen are, tile by tile, those of whichever scanned filter has seen most
      std::vector<uint32_t> seen((size_t)n_tiles + 1, 0u);
      for (size_t b = 0; b < n_scan; b = run_end(b, n_scan)) {
        const uint32_t* c = v.cum + row_of(gm[b]) * ((size_t)n_tiles + 1);
        for (size_t t = 0; t <= n_tiles; ++t) seen[t] = std::max(seen[t], c[t]);
      }
      RadiusKnn c;
      c.passes = masked_passes(seen, n_tiles);
      c.allow = v.allow;
      c.allow_bits = (uint32_t)v.n_eff;
      c.allow_per_query = v.allow_per_query;
      c.allow_label = v.allow_label;
      c.out = ResultBlock{ids, dist, cnt, nullptr, n_scan, k};
      std::vector<uint32_t> head(v.d_head ? kTabWords : 0);
      // stage 0 of a device batch [q0, q0 + m): where the flush tests per query, the head of its block — every query's word
      // (its bitmap's offset, or its wanted label); per filter the exact k nearest of the filter's sample by the list scan,
      // into the batch's rows of the output (every query's row is written again, by the last pass or by the exact route; its
      // queries are not counted there: the verdict counts every query once): their k-th distance is the first radius, +Inf
      // while the sample gives fewer than k
      c.first_radius = [&](size_t m, const float* q, const ResultBlock& o, float* d_radius) -> int {
        const size_t q0 = (size_t)(q - gq) / s->dims;
        if (v.d_head) {
          for (size_t j = 0; j < kTabWords; ++j)   // (padding queries: any word, they collect nothing)
            head[j] = v.head_of[gm[q0 + std::min(j, m - 1)]];
          HIP_TRY(hipMemcpyAsync(v.d_head, head.data(), kTabWords * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        }
        for (size_t b = q0; b < q0 + m;) {
          const size_t e = run_end(b, q0 + m), j = b - q0;
          const uint64_t a = v.n_allowed[gm[b]], stride = sample_stride(a);
          if (int r = among_locked(s, st, e - b, q + j * s->dims, k, v.sample->p + row_of(gm[b]) * kMaskedSample, nullptr,
                                   (size_t)((a + stride - 1) / stride), 0, o.ids + j * k, o.dist + j * k, o.cnt + j, false))
            return r;
          b = e;
        }
        HIP_TRY(launch_masked_radius(o.dist, o.cnt, (uint32_t)m, k, d_radius, st));
        return EHX_OK;
      };
      // the flagged queries of a device batch, filter by filter
      c.handed = [&](size_t q0, const std::vector<uint32_t>& todo, const float* q, const ResultBlock& o) -> int {
        for (size_t b = 0; b < todo.size();) {
          const uint32_t f = gm[q0 + todo[b]];
          size_t e = b + 1;
          while (e < todo.size() && gm[q0 + todo[e]] == f) ++e;
          const std::vector<uint32_t> part(todo.begin() + b, todo.begin() + e);
          if (int r = w.scan.sub.rerun(
                  s, st, q, part, k,
                  [&](size_t n, const float* sq, uint64_t* i2, float* d2, uint32_t* c2) { return exact(f, n, sq, i2, d2, c2); },
                  o.ids, o.dist, o.cnt))
            return r;
          b = e;
        }
        return EHX_OK;
      };
      // (the filters' samples: stage 0 of the scan route alone, so the exact route does not pay for them)
      if (int r = v.samples()) return r;
      RadiusKnnTally t;
      const int r = radius_knn(s, st, w.scan, v.n_pub, gq, c, &t);
      s->n_queries += t.queries - t.handed;   // (among_locked counts the rest)
      v.ctr[0] += t.queries - t.handed;
      v.ctr[1] += t.handed;
      v.ctr[2] += t.overflowed;
      v.ctr[3] += t.batches * c.passes.size();
      if (r) return r;
    }
    for (size_t b = n_scan; b < n_scan + n_shared;) {   // the exact route: one shared list per filter
      const size_t e = run_end(b, n_scan + n_shared);
      v.ctr[1] += e - b;
      if (int r = exact(gm[b], e - b, gq + b * s->dims, ids + b * k, dist + b * k, cnt + b)) return r;
      b = e;
    }
    // ... and the filters that few queries name: ONE launch, a list per query, queries of one filter naming the same list
    if (const size_t b = n_scan + n_shared; b < nq) {
      const size_t n = nq - b;
      std::vector<uint64_t> range(2 * n);   // [n] where every query's list starts | [n] where it ends
      uint64_t pairs = 0, longest = 0;
      for (size_t j = 0; j < n; ++j) {
        const uint32_t f = gm[b + j];
        range[j] = v.off[f];
        range[n + j] = v.off[f] + v.n_allowed[f];
        pairs += v.n_allowed[f];
        longest = std::max(longest, v.n_allowed[f]);
      }
      if (int r = v.d_range->ensure(2 * n)) return r;
      // (pageable host memory: the runtime stages it before the call returns)
      HIP_TRY(hipMemcpyAsync(v.d_range->p, range.data(), range.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
      v.ctr[1] += n;
      if (int r = among_locked(s, st, n, gq + b * s->dims, k, v.d_list, v.d_range->p, (size_t)v.list_rows, (size_t)longest,
                               ids + b * k, dist + b * k, cnt + b, true, v.d_range->p + n, pairs))
        return r;
    }
    return EHX_OK;
  };
  if (in_order) return answer(nq, d_queries, out.ids, out.dist, out.cnt);
  return w.group.rerun(s, st, d_queries, idx, k, answer, out.ids, out.dist, out.cnt);
}

}  // namespace ehx_impl

namespace {

// the exact answer over a plan of bitmaps: filtered_answer with the bitmap — the batch's ONE, or one per query — in the flush
int masked_answer(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, const MaskedPlan& p,
                  const ResultBlock& out) {
  char scans[kMaskedMaxMasks];
  uint32_t head_of[kMaskedMaxMasks];
  filter_routes_cut(filter_scan_serves(s, k, p.n_pub), masked_exact_cut(p.n_pub), p.n_allowed.data(), p.n_masks, scans);
  FilterView v = masked_view(s, st, p, scans, head_of);
  v.ctr = s->masked_ctr;
  return filtered_answer(s, st, nq, d_queries, k, v, out);
}

}  // namespace

namespace ehx_impl {

// an unsharded space, locked shared, scratch_mu held, its device current; everything is enqueued on `st` (mask_of /
// d_mask_of: masked_plan's)
int masked_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, const MaskTable& tab,
                  uint64_t n_bits, const uint32_t* mask_of, const uint32_t* d_mask_of, const ResultBlock& out) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  if ((rc = check_rows_fit_lds(s, "filtered search"))) return rc;   // (before anything is enqueued)
  s->masked_ctr[4] += 1;
  MaskedPlan p;
  if ((rc = masked_plan(s, st, tab, n_bits, nq, mask_of, d_mask_of, &p))) return rc;
  return masked_answer(s, st, nq, d_queries, k, p, out);
}

}  // namespace ehx_impl

namespace {

// host pointers in, host pointers out, on the space's stream (on_device)
int masked_host_locked(ehx_space* s, size_t nq, const float* queries, uint32_t k, const uint32_t* masks, uint32_t n_masks,
                       uint64_t n_bits, const uint32_t* mask_of, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  int rc;
  HostStage& h = s->masked.host;
  if ((rc = h.up(s->stream, queries, nq, s->dims, k, false))) return rc;
  const MaskTable tab = {masks, (n_bits + 31) / 32, n_masks, true};
  if ((rc = masked_locked(s, s->stream, nq, h.q, k, tab, n_bits, mask_of, nullptr, h.out))) return rc;
  return h.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
}

// ---- the graph walk under bitmaps (ehx_graph_knn_masked*: ONE bitmap; ehx_graph_knn_masked_multi*: a table, query i under
// bitmap mask_of[i]; k_graphm.hip has the walk, tests/filtered_walk_model.py its model).  One bitmap is a table of one: ONE
// function (graphm_locked) serves both.  Routes: the walk — knn_graph_locked with the bitmaps: the same arguments, wait,
// clock and refusals as an unfiltered graph search; or the exact answer above, byte for byte ehx_knn_masked_multi_device's.
// EHX_WALK_AUTO compacts the bitmaps first (one wait) and decides PER MASK: its queries are walked iff its allowed rows *
// EHX_WALK_LIST_FACTOR >= the rows the bitmaps cover: below that share a list of cap = FACTOR * ef entries cannot hold ef
// allowed ones and the walk degenerates (MEASURED: the exact route overtakes the walk between shares 1 / 11 and 1 / 14,
// scripts/bench_graph_masked.py, profiles/graph_masked_bench.jsonl; include/ehx.h has the figures beside the constant).
// A batch of a table may therefore be mixed: its walked queries take ONE walk launch, the others ONE masked_answer over the
// same plan, each part gathered and scattered back (masked.split); a batch that is all walk or all exact is answered in
// place.  A flat space has no graph: the exact route. ----
int check_route(uint32_t route) {
  if (route != EHX_WALK_AUTO && route != EHX_WALK_GRAPH && route != EHX_WALK_EXACT)
    return fail(EHX_EINVAL, "route %u is none of EHX_WALK_AUTO, EHX_WALK_GRAPH, EHX_WALK_EXACT", route);
  return EHX_OK;
}

int graphm_check(const ehx_space* s, size_t nq, uint32_t k, const void* q, const void* mask, uint64_t n_bits, uint32_t route,
                 const void* o_ids, const void* o_dist, const void* o_cnt) {
  if (int rc = masked_check(s, nq, k, q, mask, n_bits, o_ids, o_dist, o_cnt)) return rc;
  return check_route(route);
}

}  // namespace

namespace ehx_impl {

int graphm_table_check(const ehx_space* s, size_t nq, uint32_t k, const void* q, const void* masks, uint32_t n_masks,
                       uint64_t n_bits, const void* mask_of, uint32_t route, const void* o_ids, const void* o_dist,
                       const void* o_cnt) {
  if (int rc = masked_table_check(s, nq, k, q, masks, n_masks, n_bits, mask_of, o_ids, o_dist, o_cnt)) return rc;
  return check_route(route);
}

// an unsharded space, locked shared, scratch_mu held, its device current; everything is enqueued on `st`.  mask_of /
// d_mask_of: masked_plan's; neither: ONE bitmap (tab.n_masks == 1), every query under it.
int graphm_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, const MaskTable& tab,
                  uint64_t n_bits, const uint32_t* mask_of, const uint32_t* d_mask_of, uint32_t route, const ResultBlock& out) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  ehx_space::Masked& w = s->masked;
  s->graphm_ctr[2] += 1;
  if (s->params.mode != EHX_MODE_GRAPH) route = EHX_WALK_EXACT;
  MaskedPlan p;
  if (route != EHX_WALK_GRAPH) {
    if (route == EHX_WALK_EXACT && (rc = check_rows_fit_lds(s, "filtered search"))) return rc;   // (before anything is enqueued)
    if ((rc = masked_plan(s, st, tab, n_bits, nq, mask_of, d_mask_of, &p))) return rc;
  } else {
    // every query is walked: nothing is compacted.  The plan is the call's snapshot of the row count (the walk takes its own
    // behind the refusal g_n != n; bitmaps cut at an earlier, smaller count only allow fewer rows), the bitmaps where the
    // kernel reads them (ONE device bitmap: where it lies) and a table's mask_of on the host, checked
    p.n_pub = s->n.load(std::memory_order_acquire);
    p.n_eff = std::min<uint64_t>(n_bits, p.n_pub);
    p.words = (p.n_eff + 31) / 32;
    p.n_masks = tab.n_masks;
    p.mask_of = mask_of;
    p.d_maps = tab.p;
    // (a table that is BUILT has no words anywhere yet, whatever its size: masked_maps has them written)
    if ((tab.host || tab.build || tab.n_masks > 1) && (rc = masked_maps(s, st, tab, p.n_eff, &p.d_maps))) return rc;
    if (d_mask_of) {
      p.mask_of_read.resize(nq);
      HIP_TRY(hipMemcpyAsync(p.mask_of_read.data(), d_mask_of, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      p.mask_of = p.mask_of_read.data();
      if ((rc = check_mask_of(p.mask_of, nq, tab.n_masks))) return rc;
    }
  }
  // the route of every mask, and of every query through its mask
  bool walks[kMaskedMaxMasks];
  for (uint32_t m = 0; m < tab.n_masks; ++m)
    walks[m] = route == EHX_WALK_GRAPH || (route == EHX_WALK_AUTO && p.n_allowed[m] * EHX_WALK_LIST_FACTOR >= p.n_eff);
  size_t n_walk = p.mask_of ? 0 : (walks[0] ? nq : 0);   // (one bitmap: nothing per query on the host's clock)
  for (size_t i = 0; p.mask_of && i < nq; ++i) n_walk += walks[p.mask_of[i]];
  if (n_walk < nq && (rc = check_rows_fit_lds(s, "filtered search"))) return rc;   // (EHX_WALK_AUTO: known only now)

  // n queries under the masks of[0, n) (nullptr: mask 0), walked in ONE launch
  auto walk = [&](size_t n, const float* q, const uint32_t* of, uint64_t* ids, float* dist, uint32_t* cnt) -> int {
    if (int r = w.dCapHits.ensure(1, true)) return r;
    const uint32_t* d_of = nullptr;
    if (tab.n_masks > 1) {   // (one bitmap: the kernel that reads no offsets)
      std::vector<uint32_t> offs(n);
      for (size_t i = 0; i < n; ++i) offs[i] = (uint32_t)((uint64_t)of[i] * p.words);   // (masked_maps: below 2^32)
      if (int r = w.dWalkOf.ensure(n)) return r;
      // (pageable host memory: the runtime stages it before the call returns; masked_maps has ordered `st` behind the
      // earlier calls that may still read the buffer)
      HIP_TRY(hipMemcpyAsync(w.dWalkOf.p, offs.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      d_of = w.dWalkOf.p;
    }
    const GraphMask gm = {p.d_maps, p.n_eff, w.dCapHits.p, d_of};
    if (int r = knn_graph_locked(s, st, n, q, k, ids, dist, cnt, nullptr, &gm)) return r;
    s->graphm_ctr[0] += n;
    return EHX_OK;
  };
  // n queries under p.mask_of[0, n), answered exactly
  auto exact = [&](size_t n, const float* q, uint64_t* ids, float* dist, uint32_t* cnt) -> int {
    s->graphm_ctr[1] += n;
    return masked_answer(s, st, n, q, k, p, ResultBlock{ids, dist, cnt, nullptr, n, k});
  };
  if (n_walk == nq) return walk(nq, d_queries, p.mask_of, out.ids, out.dist, out.cnt);
  if (n_walk == 0) return exact(nq, d_queries, out.ids, out.dist, out.cnt);
  // a mixed batch: each part gathered with its slice of mask_of, answered, scattered into its own rows — the walk first
  // (what it refuses, it refuses before a row is written)
  std::vector<uint32_t> iw, ix, mw, mx;   // the walked queries and the others, and their masks
  for (size_t i = 0; i < nq; ++i) {
    const bool wk = walks[p.mask_of[i]];
    (wk ? iw : ix).push_back((uint32_t)i);
    (wk ? mw : mx).push_back(p.mask_of[i]);
  }
  if ((rc = w.split.rerun(
           s, st, d_queries, iw, k,
           [&](size_t n, const float* q, uint64_t* ids, float* dist, uint32_t* cnt) { return walk(n, q, mw.data(), ids, dist, cnt); },
           out.ids, out.dist, out.cnt)))
    return rc;
  p.mask_of = mx.data();
  return w.split.rerun(s, st, d_queries, ix, k, exact, out.ids, out.dist, out.cnt);
}

}  // namespace ehx_impl

namespace {

// host pointers in, host pointers out, on the space's stream: the bitmaps' words below the row count are staged by whichever
// route is taken (bits at or above the call's snapshot of the row count are never looked at: they are not even copied)
int graphm_host_locked(ehx_space* s, size_t nq, const float* queries, uint32_t k, const uint32_t* masks, uint32_t n_masks,
                       uint64_t n_bits, const uint32_t* mask_of, uint32_t route, uint64_t* out_ids, float* out_dist,
                       uint32_t* out_count) {
  int rc;
  HostStage& h = s->masked.host;
  if ((rc = h.up(s->stream, queries, nq, s->dims, k, false))) return rc;
  const MaskTable tab = {masks, (n_bits + 31) / 32, n_masks, true};
  if ((rc = graphm_locked(s, s->stream, nq, h.q, k, tab, n_bits, mask_of, nullptr, route, h.out))) return rc;
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
    const MaskTable tab = {d_mask, (n_bits + 31) / 32, 1, false};
    return masked_locked(s, st, n_queries, d_queries, k, tab, n_bits, nullptr, nullptr,
                         ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_knn_masked(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const uint32_t* mask, uint64_t n_bits,
                   uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (int rc = masked_check(s, n_queries, k, queries, mask, n_bits, out_ids, out_dist, out_count)) return rc;
  return search_on_device(s, "ehx_knn_masked", kMaskedWhy, n_queries, nullptr, [&] {
    return masked_host_locked(s, n_queries, queries, k, mask, 1, n_bits, nullptr, out_ids, out_dist, out_count);
  });
}

int ehx_knn_masked_multi_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                const uint32_t* d_masks, uint32_t n_masks, uint64_t n_bits, const uint32_t* d_mask_of,
                                uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count) {
  if (int rc = masked_table_check(s, n_queries, k, d_queries, d_masks, n_masks, n_bits, d_mask_of, d_out_ids, d_out_dist,
                                  d_out_count))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_knn_masked_multi_device", kMaskedWhy, n_queries, &st, [&] {
    const MaskTable tab = {d_masks, (n_bits + 31) / 32, n_masks, false};
    return masked_locked(s, st, n_queries, d_queries, k, tab, n_bits, nullptr, d_mask_of,
                         ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_knn_masked_multi(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const uint32_t* masks,
                         uint32_t n_masks, uint64_t n_bits, const uint32_t* mask_of, uint64_t* out_ids, float* out_dist,
                         uint32_t* out_count) {
  if (int rc = masked_table_check(s, n_queries, k, queries, masks, n_masks, n_bits, mask_of, out_ids, out_dist, out_count))
    return rc;
  if (int rc = check_mask_of(mask_of, n_queries, n_masks)) return rc;   // (before anything is enqueued)
  return search_on_device(s, "ehx_knn_masked_multi", kMaskedWhy, n_queries, nullptr, [&] {
    return masked_host_locked(s, n_queries, queries, k, masks, n_masks, n_bits, mask_of, out_ids, out_dist, out_count);
  });
}

int ehx_graph_knn_masked_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                const uint32_t* d_mask, uint64_t n_bits, uint32_t route, uint64_t* d_out_ids,
                                float* d_out_dist, uint32_t* d_out_count) {
  if (int rc = graphm_check(s, n_queries, k, d_queries, d_mask, n_bits, route, d_out_ids, d_out_dist, d_out_count)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_graph_knn_masked_device", kMaskedWhy, n_queries, &st, [&] {
    const MaskTable tab = {d_mask, (n_bits + 31) / 32, 1, false};
    return graphm_locked(s, st, n_queries, d_queries, k, tab, n_bits, nullptr, nullptr, route,
                         ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_graph_knn_masked(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const uint32_t* mask,
                         uint64_t n_bits, uint32_t route, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (int rc = graphm_check(s, n_queries, k, queries, mask, n_bits, route, out_ids, out_dist, out_count)) return rc;
  return search_on_device(s, "ehx_graph_knn_masked", kMaskedWhy, n_queries, nullptr, [&] {
    return graphm_host_locked(s, n_queries, queries, k, mask, 1, n_bits, nullptr, route, out_ids, out_dist, out_count);
  });
}

int ehx_graph_knn_masked_multi_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                      const uint32_t* d_masks, uint32_t n_masks, uint64_t n_bits, const uint32_t* d_mask_of,
                                      uint32_t route, uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count) {
  if (int rc = graphm_table_check(s, n_queries, k, d_queries, d_masks, n_masks, n_bits, d_mask_of, route, d_out_ids, d_out_dist,
                                  d_out_count))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_graph_knn_masked_multi_device", kMaskedWhy, n_queries, &st, [&] {
    const MaskTable tab = {d_masks, (n_bits + 31) / 32, n_masks, false};
    return graphm_locked(s, st, n_queries, d_queries, k, tab, n_bits, nullptr, d_mask_of, route,
                         ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_graph_knn_masked_multi(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const uint32_t* masks,
                               uint32_t n_masks, uint64_t n_bits, const uint32_t* mask_of, uint32_t route, uint64_t* out_ids,
                               float* out_dist, uint32_t* out_count) {
  if (int rc = graphm_table_check(s, n_queries, k, queries, masks, n_masks, n_bits, mask_of, route, out_ids, out_dist, out_count))
    return rc;
  if (int rc = check_mask_of(mask_of, n_queries, n_masks)) return rc;   // (before anything is enqueued)
  return search_on_device(s, "ehx_graph_knn_masked_multi", kMaskedWhy, n_queries, nullptr, [&] {
    return graphm_host_locked(s, n_queries, queries, k, masks, n_masks, n_bits, mask_of, route, out_ids, out_dist, out_count);
  });
}

// test hook, not part of the ABI: queries walked, queries answered exactly, calls, walked queries whose list reached its
// cap (read from the device behind whatever is queued); ehx_graph_knn_masked* and ehx_graph_knn_masked_multi* both count here
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
// passes launched, calls (ehx_knn_masked* and ehx_knn_masked_multi* both count here)
void ehx_test_masked_counters(ehx_space* s, uint64_t out[5]) {
  for (int i = 0; i < 5; ++i) out[i] = s ? s->masked_ctr[i].load(std::memory_order_relaxed) : 0;
}

}  // extern "C"
