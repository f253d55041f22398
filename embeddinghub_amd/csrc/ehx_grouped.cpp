// Grouped kNN: ehx_knn_grouped (host pointers) and ehx_knn_grouped_device, and the ONE answer the three grouped searches
// share (grouped_answer; its other callers: ehx_groupedm.cpp under row bitmaps, ehx_groupedl.cpp under a label column).  The
// first k ELIGIBLE rows of the prefix n_eff = min(the call's ONE snapshot of the row count, n_labels) in (canonical distance,
// id) order; a row is eligible iff its label is EHX_GROUP_NONE or fewer than per_group rows of its label precede it in that
// order (include/ehx.h has the contract, k_grouped.hip's header the kernels and why the answer is exact).  The labels travel
// with the call, as a bitmap does: nothing is stored with the rows.
//
// grouped_answer takes a FilterView (ehx_internal.h): per filter the rows it allows as a range of a list, and whether it
// scans.  A caller keeps only what names its rows — here: ONE filter that allows the prefix, the identity list (d_list ==
// nullptr), no row test in the flush.
//   scan route   the filters whose `scans` is set — the caller's gate: flat spaces whose int8 scan serves a radius on the
//                prefix (i8_serves_radius), plain rows (no x_perm), at least kLargeKMinQueries such queries, any k <= 256, and
//                for a filtered form more than masked_exact_cut(rows) allowed rows: the falling-radius kNN (radius_knn,
//                ehx_call.cpp) with the view's row test in the int8 scan's flush and grouped_rerank_kernel as its re-rank.
//                Seed: every query's pool takes a strided-by-rank sample of at most kLargeKSample entries of ITS OWN range
//                (grouped_range_seed_kernel; the identity list: the large-k route's rows 0, stride, 2 stride, ...).  Passes:
//                largek_passes(n_eff, growth) for every form: a filtered pass never lets more hits through than the
//                unfiltered search would under the same radius.  (Passes cut by allowed rows seen, as the bitmap kNN's: a
//                follow-up.)  The queries it hands on — pool overflow, or a radius the bound does not serve: a sample that
//                cannot reach k groups leaves the radius at +Inf — take, each under its own range, the
//   list route   everything else (graph spaces, which answer from their stored rows; small spaces; SCAN_F32 / SCAN_F16;
//                small batches; filters at or below the cut): grouped_list — grouped_range_slab_kernel and
//                grouped_rerank_kernel in pass mode over consecutive slabs of kPoolCap entries of every query's range, the
//                radius falling from +Inf, the last slab in last mode; the loop runs the slabs of the longest range of the
//                device batch, ONE launch per slab whatever number of ranges it names.  Every listed row's canonical distance
//                is computed once, plus one sort of a slab per query.
// Entry scaffold, host staging, sub-batch re-runs: ehx_call.cpp's (search_on_device, HostStage, SubsetBufs::rerun).
#include "ehx_internal.h"

namespace {

constexpr const char* kGroupedWhy = "grouped search over shards is not built yet";

static_assert(EHX_MAX_K_GROUPED == kLargeKMax, "the re-rank carries one key per thread");
static_assert(EHX_GROUP_NONE == kGroupNone, "the header's label of a row that is a group of its own");

}  // namespace

namespace ehx_impl {

int grouped_check_head(const ehx_space* s, size_t nq, uint32_t k, uint32_t per_group, const void* q, const void* group_of,
                       uint64_t n_labels, const void* o_ids, const void* o_dist, const void* o_cnt) {
  if (!s) return fail(EHX_EINVAL, "space is NULL");   // (before the device is looked for)
  int rc = ehx_init(nullptr, 0);   // (no device: EHX_ENODEVICE, whatever else is wrong with the call)
  if (rc) return rc;
  if (k == 0) return fail(EHX_EINVAL, "k is 0");
  if (per_group == 0) return fail(EHX_EINVAL, "per_group is 0");
  if (k > EHX_MAX_K_GROUPED) return fail(EHX_EUNSUPPORTED, "k=%u exceeds %u", k, EHX_MAX_K_GROUPED);
  if (!(o_ids && o_dist && o_cnt && (!nq || q))) return fail(EHX_EINVAL, "NULL argument");
  if (n_labels && !group_of) return fail(EHX_EINVAL, "NULL group_of with n_labels = %llu", (unsigned long long)n_labels);
  return EHX_OK;
}

int grouped_check_ld(const ehx_space* s) {
  if (s->ld > grouped_rerank_max_ld())
    return fail(EHX_EUNSUPPORTED, "grouped search keeps a prepared query in LDS: rows of %u floats exceed %u", s->ld,
                grouped_rerank_max_ld());
  return EHX_OK;
}

bool grouped_scan_serves(const ehx_space* s, uint64_t n_eff) {
  return s->params.mode != EHX_MODE_GRAPH && !s->x_perm && n_eff > 0 && i8_serves_radius(s, n_eff);
}

int grouped_list(ehx_space* s, hipStream_t st, uint64_t n_eff, const uint64_t* d_list, const uint64_t* range, size_t nq,
                 const float* d_queries, uint32_t k, uint32_t per_group, const uint32_t* d_group_of, uint64_t* d_ids,
                 float* d_dist, uint32_t* d_count, bool count_queries) {
  ehx_space::Grouped& w = s->grouped;
  const size_t cap = std::min(kSideChunk, nq);
  int rc;
  if ((rc = s->scr.dQ.ensure(cap * s->ld)) || (rc = w.dPool.ensure(cap * kPoolCap)) || (rc = w.dCtl.ensure(2 * cap)) ||
      (rc = w.exact.dTop.ensure(cap * kLargeKMax)) || (rc = w.exact.dTopCnt.ensure(cap)) || (rc = w.exact.dRadius.ensure(cap)) ||
      (rc = w.exact.dWork.ensure(cap)) || (rc = w.dRange.ensure(2 * cap)))
    return rc;
  std::vector<uint64_t> up(2 * cap);   // a device batch's [m] starts | [m] ends
  uint64_t n_listed = 0;
  for (size_t q0 = 0; q0 < nq; q0 += kSideChunk) {
    const size_t m = std::min(kSideChunk, nq - q0);
    uint64_t longest = 0;
    for (size_t j = 0; j < m; ++j) {
      up[j] = range[q0 + j];
      up[m + j] = range[nq + q0 + j];
      longest = std::max(longest, up[m + j] - up[j]);
      n_listed += up[m + j] - up[j];
    }
    const uint64_t n_slabs = std::max<uint64_t>(1, (longest + kPoolCap - 1) / kPoolCap);   // (no row: one empty slab writes the page)
    // (searches on other streams have read and written this scratch; this batch's fence makes a Set that rewrites rows in
    // place wait for it in turn)
    if ((rc = wait_searches_in_flight(s, st))) return rc;
    if ((rc = s->clock.begin(st, BatchClock::kOutOfRing))) return rc;
    HIP_TRY(hipMemsetAsync(w.dCtl.p, 0, 2 * m * sizeof(uint32_t), st));
    // (pageable host memory: the runtime stages it before the call returns)
    HIP_TRY(hipMemcpyAsync(w.dRange.p, up.data(), 2 * m * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(launch_prep_queries(d_queries + q0 * s->dims, (uint32_t)m, s->dims, s->ld, (uint32_t)m, s->metric, s->scr.dQ.p, st));
    GroupedRerankArgs g = {};
    g.group_of = d_group_of;
    g.per_group = per_group;
    RadiusRerankArgs& r = g.r;
    r.Q = s->scr.dQ.p;
    r.rows = rows_view(s, n_eff);
    r.radius = w.exact.dRadius.p;
    r.pool = w.dPool.p;
    r.pool_cnt = w.dCtl.p;
    r.ovf = w.dCtl.p + m;
    r.top = w.exact.dTop.p;
    r.top_cnt = w.exact.dTopCnt.p;
    r.work = w.exact.dWork.p;
    r.out_ids = d_ids + q0 * k;
    r.out_dist = d_dist + q0 * k;
    r.out_count = d_count + q0;
    r.nq = (uint32_t)m;
    r.k = k;
    if ((rc = s->clock.scan_begin(st))) return rc;
    for (uint64_t b = 0; b < n_slabs; ++b) {
      HIP_TRY(launch_grouped_range_slab(d_list, w.dRange.p, w.dRange.p + m, b, b == 0, w.dPool.p, w.dCtl.p, r.radius, r.top_cnt,
                                        r.work, (uint32_t)m, st));
      r.mode = b + 1 == n_slabs ? kRadiusLast : kRadiusPass;
      HIP_TRY(launch_grouped_rerank(g, st));
    }
    if ((rc = s->clock.scan_end(st)) || (rc = s->clock.finish(st))) return rc;
  }
  if (count_queries) s->n_queries += nq;
  s->n_dist += n_listed;
  return EHX_OK;
}

// The order the queries are answered in: the scan route's first; where the flush reads a bitmap per query
// (v.allow_per_query) further by filter, which keeps one bitmap's queries in the same query tiles of the flush; otherwise as
// they came.  A batch that is already in that order is answered in place, any other gathered, answered and scattered back
// (SubsetBufs::rerun).
int grouped_answer(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, uint32_t per_group,
                   const uint32_t* d_group_of, const FilterView& v, const ResultBlock& out) {
  ehx_space::Grouped& w = s->grouped;
  const uint64_t n_eff = v.n_eff;
  auto filter_at = [&](size_t i) { return v.filter_of ? v.filter_of[i] : 0u; };
  auto place = [&](uint32_t i) {
    const uint32_t f = filter_at(i);
    return (uint64_t)(v.scans[f] ? 0u : 1u) * v.n_filters + (v.allow_per_query ? f : 0u);
  };
  std::vector<uint32_t> idx(nq), gm(nq);   // gm: the filter of every query in that order
  for (size_t i = 0; i < nq; ++i) idx[i] = (uint32_t)i;
  auto before = [&](uint32_t a, uint32_t b) { return place(a) < place(b); };
  const bool in_order = std::is_sorted(idx.begin(), idx.end(), before);   // (one filter: always)
  if (!in_order) std::stable_sort(idx.begin(), idx.end(), before);
  size_t n_scan = 0;
  for (size_t i = 0; i < nq; ++i) {
    gm[i] = filter_at(idx[i]);
    n_scan += v.scans[gm[i]] != 0;
  }
  int rc;
  if ((rc = w.dRange.ensure(2 * std::min(kSideChunk, nq)))) return rc;   // (sized once: both routes upload into it)
  // [n] where the list of every one of the queries `of` (positions in that order, behind `base`) starts | [n] where it ends
  auto ranges_of = [&](const uint32_t* of, size_t base, size_t n) {
    std::vector<uint64_t> range(2 * n);
    for (size_t j = 0; j < n; ++j) {
      const uint32_t f = gm[of ? base + of[j] : base + j];
      range[j] = v.off[f];
      range[n + j] = v.off[f] + v.n_allowed[f];
    }
    return range;
  };
  auto list = [&](const std::vector<uint64_t>& range, size_t n, const float* q, uint64_t* ids, float* dist, uint32_t* cnt, bool count) {
    return grouped_list(s, st, n_eff, v.d_list, range.data(), n, q, k, per_group, d_group_of, ids, dist, cnt, count);
  };
  auto answer = [&](size_t, const float* gq, uint64_t* ids, float* dist, uint32_t* cnt) -> int {
    if (n_scan) {
      RadiusKnn c;
      c.passes = largek_passes(n_eff, env().largek_growth);
      c.allow = v.allow;
      c.allow_bits = v.allow ? (uint32_t)n_eff : 0u;
      c.allow_per_query = v.allow_per_query;
      c.allow_label = v.allow_label;
      c.out = ResultBlock{ids, dist, cnt, nullptr, n_scan, k};
      std::vector<uint32_t> head(v.d_head ? kTabWords : 0);
      // stage 0 of a device batch [q0, q0 + m): where the flush tests per query, the head of its block — every query's word
      // (its bitmap's offset, or its wanted label); every query's range, and from it the sample in the query's pool
      c.fill_pool = [&](size_t q0, size_t m, uint64_t* pool, uint32_t* pool_cnt) -> int {
        if (v.d_head) {
          for (size_t j = 0; j < kTabWords; ++j)   // (padding queries repeat the last: they collect nothing)
            head[j] = v.head_of[gm[q0 + std::min(j, m - 1)]];
          // (pageable host memory: the runtime stages it before the call returns)
          HIP_TRY(hipMemcpyAsync(v.d_head, head.data(), kTabWords * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        }
        const std::vector<uint64_t> range = ranges_of(nullptr, q0, m);
        HIP_TRY(hipMemcpyAsync(w.dRange.p, range.data(), 2 * m * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        HIP_TRY(launch_grouped_range_seed(v.d_list, w.dRange.p, w.dRange.p + m, pool, pool_cnt, (uint32_t)m, st));
        return EHX_OK;
      };
      // The scan runs on the snapshot's rows — a row's place inside its tile of the scan copy is not its id's, so the copy
      // cannot be cut at a row count of its own — over the tiles that hold the prefix; the flush drops every row at or above
      // n_eff with the rows the filter excludes, and the re-rank reads no row (and no label) at or above it
      c.rerank = [&](const RadiusRerankArgs& r, hipStream_t on) {
        GroupedRerankArgs g = {r, d_group_of, per_group};
        g.r.rows.n_rows = n_eff;
        return launch_grouped_rerank(g, on);
      };
      // the flagged queries of a device batch, each under its own range: ONE sub-batch on the list route
      c.handed = [&](size_t q0, const std::vector<uint32_t>& todo, const float* q, const ResultBlock& o) -> int {
        const std::vector<uint64_t> range = ranges_of(todo.data(), q0, todo.size());
        return w.scan.sub.rerun(
            s, st, q, todo, k,
            [&](size_t n, const float* sq, uint64_t* i2, float* d2, uint32_t* c2) {
              return list(range, n, sq, i2, d2, c2, false);   // (the scan batch counted them)
            },
            o.ids, o.dist, o.cnt);
      };
      RadiusKnnTally t;
      const int r = radius_knn(s, st, w.scan, v.n_pub, gq, c, &t);
      for (uint64_t b = 0; b < t.batches; ++b)   // (the int8 scan copy: every query of a batch against every prefix row once)
        count_scan_batch(s, (size_t)std::min<uint64_t>(kSideChunk, t.queries - b * kSideChunk), n_eff, k, 1);
      s->n_i8_queries += t.queries;
      s->n_i8_fallback += t.handed;
      v.ctr[0] += t.queries - t.handed;
      v.ctr[1] += t.handed;
      v.ctr[2] += t.overflowed;
      v.ctr[3] += t.batches * c.passes.size();
      if (r) return r;
    }
    if (n_scan == nq) return EHX_OK;
    v.ctr[1] += nq - n_scan;
    return list(ranges_of(nullptr, n_scan, nq - n_scan), nq - n_scan, gq + n_scan * s->dims, ids + n_scan * k, dist + n_scan * k,
                cnt + n_scan, true);
  };
  if (in_order) return answer(nq, d_queries, out.ids, out.dist, out.cnt);
  return w.group.rerun(s, st, d_queries, idx, k, answer, out.ids, out.dist, out.cnt);
}

}  // namespace ehx_impl

namespace {

// an unsharded space, locked shared, scratch_mu held, its device current; everything is enqueued on `st`.  n_pub: the call's
// ONE read of the row count; d_group_of: at least min(n_pub, n_labels) labels on the device
int grouped_locked(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const float* d_queries, uint32_t k,
                   uint32_t per_group, const uint32_t* d_group_of, uint64_t n_labels, const ResultBlock& out) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  if ((rc = grouped_check_ld(s))) return rc;   // (before anything is enqueued)
  s->grouped_ctr[4] += 1;
  // ONE filter that allows the prefix: rows [0, n_eff) of the identity list, nothing tested in the flush
  const uint64_t n_eff = std::min(n_pub, n_labels), off = 0;
  const char scans = nq >= kLargeKMinQueries && grouped_scan_serves(s, n_eff);
  FilterView v;
  v.n_pub = n_pub;
  v.n_eff = n_eff;
  v.n_filters = 1;
  v.n_allowed = &n_eff;
  v.off = &off;
  v.scans = &scans;
  v.ctr = s->grouped_ctr;
  return grouped_answer(s, st, nq, d_queries, k, per_group, d_group_of, v, out);
}

// host pointers in, host pointers out, on the space's stream (on_device): the labels of the prefix staged in grouped.dLabels
int grouped_host_locked(ehx_space* s, size_t nq, const float* queries, uint32_t k, uint32_t per_group, const uint32_t* group_of,
                        uint64_t n_labels, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  int rc;
  ehx_space::Grouped& w = s->grouped;
  const uint64_t n_pub = s->n.load(std::memory_order_acquire);   // the ONE read of the row count
  const uint64_t n_eff = std::min(n_pub, n_labels);
  if ((rc = w.dLabels.ensure(std::max<uint64_t>(n_eff, 1))) || (rc = w.host.up(s->stream, queries, nq, s->dims, k, false))) return rc;
  // (earlier calls' launches on other streams may still read the labels)
  if ((rc = wait_searches_in_flight(s, s->stream))) return rc;
  // (pageable host memory: the runtime stages it before the call returns)
  if (n_eff) HIP_TRY(hipMemcpyAsync(w.dLabels.p, group_of, n_eff * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
  if ((rc = grouped_locked(s, s->stream, n_pub, nq, w.host.q, k, per_group, w.dLabels.p, n_eff, w.host.out))) return rc;
  return w.host.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
}

int grouped_check(const ehx_space* s, size_t nq, uint32_t k, uint32_t per_group, const void* q, const void* group_of,
                  uint64_t n_labels, const void* o_ids, const void* o_dist, const void* o_cnt) {
  if (int rc = grouped_check_head(s, nq, k, per_group, q, group_of, n_labels, o_ids, o_dist, o_cnt)) return rc;
  return check_batch_size(nq);
}

}  // namespace

extern "C" {

int ehx_knn_grouped_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k, uint32_t per_group,
                           const uint32_t* d_group_of, uint64_t n_labels, uint64_t* d_out_ids, float* d_out_dist,
                           uint32_t* d_out_count) {
  if (int rc = grouped_check(s, n_queries, k, per_group, d_queries, d_group_of, n_labels, d_out_ids, d_out_dist, d_out_count))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_knn_grouped_device", kGroupedWhy, n_queries, &st, [&] {
    return grouped_locked(s, st, s->n.load(std::memory_order_acquire), n_queries, d_queries, k, per_group, d_group_of, n_labels,
                          ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_knn_grouped(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint32_t per_group,
                    const uint32_t* group_of, uint64_t n_labels, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (int rc = grouped_check(s, n_queries, k, per_group, queries, group_of, n_labels, out_ids, out_dist, out_count)) return rc;
  return search_on_device(s, "ehx_knn_grouped", kGroupedWhy, n_queries, nullptr, [&] {
    return grouped_host_locked(s, n_queries, queries, k, per_group, group_of, n_labels, out_ids, out_dist, out_count);
  });
}

// test hook, not part of the ABI: queries answered on the scan route, handed to the list route (by the gate or by the scan
// route), of those the ones whose pool overflowed, scan passes launched, calls
void ehx_test_grouped_counters(ehx_space* s, uint64_t out[5]) {
  for (int i = 0; i < 5; ++i) out[i] = s ? s->grouped_ctr[i].load(std::memory_order_relaxed) : 0;
}

}  // extern "C"
