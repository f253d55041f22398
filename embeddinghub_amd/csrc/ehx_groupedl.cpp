// Grouped kNN under a label column: ehx_knn_grouped_labeled (host pointers) and ehx_knn_grouped_labeled_device.  Two columns
// under one length: group_of[r] the entity a row belongs to (EHX_GROUP_NONE: a group of its own), label_of[r] the partition —
// tenant, namespace, collection — it lies in; want[i] the partition query i is confined to.  FILTER FIRST, THEN CAP: the
// first k ELIGIBLE rows among the rows r < n_eff = min(the call's ONE snapshot of the row count, n_labels) with label_of[r] ==
// want[i], in (canonical distance, id) order; such a row is eligible iff its group is EHX_GROUP_NONE or fewer than per_group
// rows OF THE SAME PARTITION and group precede it.  Row i of the answer is, byte for byte, ehx_knn_grouped_masked_device's
// for query i alone under the bitmap of its partition (include/ehx.h has the contract, k_groupedl.hip's header why the answer
// is exact).  The number of distinct wanted labels is not limited: a call is served in device batches of kSideChunk queries,
// and per batch
//   compaction   the label search's (labeled_plan, ehx_labeled.cpp): the batch's distinct wanted labels ("slots"), per slot
//                its rows and its list in masked.dList, for the slots that scan an ascending list and the column's copy behind
//                the head of labeled.dBlock
//   routing      the grouped search's under bitmaps, decided BEFORE the lists are filled: a slot scans iff the space is flat
//                with plain rows, its int8 scan serves a radius on the prefix, the slot has more than masked_exact_cut(rows)
//                rows and at least kLargeKMinQueries queries of the batch name such slots — otherwise none scans, and the
//                batch pays for no tile prefix, no column copy and no second wait.  Any k <= 256 scans.  At most 127 slots
//                can (ehx_labeled.cpp's argument).  The cut is CARRIED OVER from the bitmap search, not measured for this call.
//   scan route   the falling-radius kNN (radius_knn, ehx_call.cpp) with "the row's label is the query's" in the int8 scan's
//                flush (allow_label: the head of the block is every query's wanted label) and grouped_rerank_kernel as its
//                re-rank.  Seed: every query's pool takes a strided-by-rank sample of at most kLargeKSample ids of ITS OWN
//                slot's list (grouped_range_seed_kernel).  Passes: largek_passes(n_eff, growth), the unfiltered grouped
//                search's: a pass never lets more hits through than that search would under the same radius.
//   list route   everything else — graph spaces (from their stored rows), small spaces, SCAN_F32 / SCAN_F16, small batches,
//                slots at or below the cut — and the queries the scan hands on, each under its own slot: the grouped search's
//                loop over slabs with each slab drawn from the query's range of masked.dList (grouped_range_slab_kernel).  The
//                loop runs the slabs of the longest list of the batch, ONE launch per slab whatever number of slots it names.
// Waits: the device form reads d_want back (one wait for the whole call, the outputs unwritten until then), then per device
// batch the compaction's — once for the counts, a second time only where some slot scans — and radius_knn's one verdict.
// Entry scaffold, host staging, sub-batch re-runs: ehx_call.cpp's (search_on_device, HostStage, SubsetBufs::rerun).
#include "ehx_internal.h"

namespace {

constexpr const char* kGroupedLabeledWhy = "filtered grouped search over shards is not built yet";
static_assert(kTabWords == kLabelHead, "the head of the label block holds a word per query of a device batch");

// the union of ehx_knn_grouped_masked's and ehx_knn_labeled's checks, with their codes and in their order
int groupedl_check(const ehx_space* s, size_t nq, uint32_t k, uint32_t per_group, const void* q, const void* group_of,
                   const void* label_of, uint64_t n_labels, const void* want, const void* o_ids, const void* o_dist,
                   const void* o_cnt) {
  if (!s) return fail(EHX_EINVAL, "space is NULL");   // (before the device is looked for)
  int rc = ehx_init(nullptr, 0);   // (no device: EHX_ENODEVICE, whatever else is wrong with the call)
  if (rc) return rc;
  if (k == 0) return fail(EHX_EINVAL, "k is 0");
  if (per_group == 0) return fail(EHX_EINVAL, "per_group is 0");
  if (k > EHX_MAX_K_GROUPED) return fail(EHX_EUNSUPPORTED, "k=%u exceeds %u", k, EHX_MAX_K_GROUPED);
  if (!(o_ids && o_dist && o_cnt && (!nq || q))) return fail(EHX_EINVAL, "NULL argument");
  if (n_labels && !group_of) return fail(EHX_EINVAL, "NULL group_of with n_labels = %llu", (unsigned long long)n_labels);
  if (n_labels && !label_of) return fail(EHX_EINVAL, "NULL label_of with n_labels = %llu", (unsigned long long)n_labels);
  if (!want) return fail(EHX_EINVAL, "NULL want");
  return check_batch_size(nq);
}

// ehx_knn_grouped_by_label*: the same checks with their codes and in their order (the columns are the space's: no pointers,
// no length), then the column numbers
int grouped_by_label_check(const ehx_space* s, size_t nq, uint32_t k, uint32_t per_group, const void* q, uint32_t group_col,
                           uint32_t label_col, const void* want, const void* o_ids, const void* o_dist, const void* o_cnt) {
  if (int rc = groupedl_check(s, nq, k, per_group, q, nullptr, nullptr, 0, want, o_ids, o_dist, o_cnt)) return rc;
  if (group_col >= EHX_MAX_COLUMNS || label_col >= EHX_MAX_COLUMNS)
    return fail(EHX_EINVAL, "group_col = %u, label_col = %u: a space has %u columns", group_col, label_col, (unsigned)EHX_MAX_COLUMNS);
  return EHX_OK;
}

// The list route for nq <= kSideChunk queries, query j over masked.dList[start[j], end[j]) (range: [nq] starts | [nq] ends,
// host memory; d_list: masked.dList, or a stored column's permutation): any space kind.  count_queries: its queries are not
// in n_queries yet.
int groupedl_list(ehx_space* s, hipStream_t st, uint64_t n_eff, const uint64_t* d_list, const std::vector<uint64_t>& range, size_t nq,
                  const float* d_queries, uint32_t k, uint32_t per_group, const uint32_t* d_group_of, uint64_t* d_ids,
                  float* d_dist, uint32_t* d_count, bool count_queries) {
  ehx_space::Grouped& w = s->grouped;
  ehx_space::GroupedLabeled& gw = s->groupedl;
  int rc;
  if ((rc = s->scr.dQ.ensure(nq * s->ld)) || (rc = w.dPool.ensure(nq * kPoolCap)) || (rc = w.dCtl.ensure(2 * nq)) ||
      (rc = w.exact.dTop.ensure(nq * kLargeKMax)) || (rc = w.exact.dTopCnt.ensure(nq)) || (rc = w.exact.dRadius.ensure(nq)) ||
      (rc = w.exact.dWork.ensure(nq)) || (rc = gw.dRange.ensure(2 * nq)))
    return rc;
  uint64_t n_listed = 0, longest = 0;
  for (size_t j = 0; j < nq; ++j) {
    const uint64_t len = range[nq + j] - range[j];
    longest = std::max(longest, len);
    n_listed += len;
  }
  const uint64_t n_slabs = std::max<uint64_t>(1, (longest + kPoolCap - 1) / kPoolCap);   // (no row: one empty slab writes the page)
  // (searches on other streams have read and written this scratch; this batch's fence makes a Set that rewrites rows in
  // place wait for it in turn)
  if ((rc = wait_searches_in_flight(s, st))) return rc;
  if ((rc = s->clock.begin(st, BatchClock::kOutOfRing))) return rc;
  HIP_TRY(hipMemsetAsync(w.dCtl.p, 0, 2 * nq * sizeof(uint32_t), st));
  // (pageable host memory: the runtime stages it before the call returns)
  HIP_TRY(hipMemcpyAsync(gw.dRange.p, range.data(), 2 * nq * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  HIP_TRY(launch_prep_queries(d_queries, (uint32_t)nq, s->dims, s->ld, (uint32_t)nq, s->metric, s->scr.dQ.p, st));
  GroupedRerankArgs g = {};
  g.group_of = d_group_of;
  g.per_group = per_group;
  RadiusRerankArgs& r = g.r;
  r.Q = s->scr.dQ.p;
  r.rows = rows_view(s, n_eff);
  r.radius = w.exact.dRadius.p;
  r.pool = w.dPool.p;
  r.pool_cnt = w.dCtl.p;
  r.ovf = w.dCtl.p + nq;
  r.top = w.exact.dTop.p;
  r.top_cnt = w.exact.dTopCnt.p;
  r.work = w.exact.dWork.p;
  r.out_ids = d_ids;
  r.out_dist = d_dist;
  r.out_count = d_count;
  r.nq = (uint32_t)nq;
  r.k = k;
  if ((rc = s->clock.scan_begin(st))) return rc;
  for (uint64_t b = 0; b < n_slabs; ++b) {
    HIP_TRY(launch_grouped_range_slab(d_list, gw.dRange.p, gw.dRange.p + nq, b, b == 0, w.dPool.p, w.dCtl.p, r.radius,
                                      r.top_cnt, r.work, (uint32_t)nq, st));
    r.mode = b + 1 == n_slabs ? kRadiusLast : kRadiusPass;
    HIP_TRY(launch_grouped_rerank(g, st));
  }
  if ((rc = s->clock.scan_end(st)) || (rc = s->clock.finish(st))) return rc;
  if (count_queries) s->n_queries += nq;
  s->n_dist += n_listed;
  return EHX_OK;
}

// One device batch of m <= kSideChunk queries under want[0, m) (host memory) over the prefix of n_eff rows of both columns.
// *col_copied: the flush's copy of the label column is in place (made once per call, and only where some slot scans).
// ix: the label column is a stored one — the plan is read from its fresh index (colindex_plan: no launch, no wait), the
// lists are runs of its permutation and the flush's block is the index's.
int groupedl_batch(ehx_space* s, hipStream_t st, uint64_t n_pub, uint64_t n_eff, size_t m, const float* d_queries, uint32_t k,
                   uint32_t per_group, const uint32_t* d_group_of, const uint32_t* d_label_of, const ehx_space::ColIndex* ix,
                   const uint32_t* want, bool* col_copied, const ResultBlock& out) {
  int rc;
  ehx_space::GroupedLabeled& w = s->groupedl;
  // routing: the grouped search's under bitmaps (ehx_groupedm.cpp), applied by the plan before it fills the lists
  const bool scan_serves = s->params.mode != EHX_MODE_GRAPH && !s->x_perm && n_eff > 0 && i8_serves_radius(s, n_eff);
  LabeledPlan p;
  if (ix) colindex_plan(*ix, m, want, scan_serves, masked_exact_cut(n_pub), kLargeKMinQueries, &p);
  else if ((rc = labeled_plan(s, st, n_eff, m, d_label_of, want, scan_serves, masked_exact_cut(n_pub), kLargeKMinQueries, col_copied, &p)))
    return rc;
  const uint64_t* d_list = ix ? ix->dPerm.p : s->masked.dList.p;
  uint32_t* d_block = ix ? ix->dBlock.p : s->labeled.dBlock.p;
  if ((rc = w.dRange.ensure(2 * m))) return rc;   // (sized once per batch: the seed and the list route upload into it)
  // the order the queries are answered in: the scan route's first (SubsetBufs: gathered, answered, scattered back; skipped
  // when they come in that order — always where no slot scans)
  auto scans_at = [&](size_t i) { return p.scans[p.slot_of[i]] != 0; };
  std::vector<uint32_t> idx(m), gs(m);   // gs: the slot of every query in that order
  for (size_t i = 0; i < m; ++i) idx[i] = (uint32_t)i;
  auto before = [&](uint32_t a, uint32_t b) { return scans_at(a) && !scans_at(b); };
  const bool in_order = std::is_sorted(idx.begin(), idx.end(), before);
  if (!in_order) std::stable_sort(idx.begin(), idx.end(), before);
  size_t n_scan = 0;
  for (size_t i = 0; i < m; ++i) {
    gs[i] = p.slot_of[idx[i]];
    n_scan += p.scans[gs[i]] != 0;
  }
  // [n] where the list of every one of the queries `of` (positions in that order) starts | [n] where it ends
  auto ranges_of = [&](const uint32_t* of, size_t base, size_t n) {
    std::vector<uint64_t> range(2 * n);
    for (size_t j = 0; j < n; ++j) {
      const uint32_t f = gs[of ? base + of[j] : base + j];
      range[j] = p.off[f];
      range[n + j] = p.off[f] + p.n_allowed[f];
    }
    return range;
  };
  auto list = [&](const std::vector<uint64_t>& range, size_t n, const float* q, uint64_t* ids, float* dist, uint32_t* cnt, bool count) {
    return groupedl_list(s, st, n_eff, d_list, range, n, q, k, per_group, d_group_of, ids, dist, cnt, count);
  };
  auto answer = [&](size_t, const float* gq, uint64_t* ids, float* dist, uint32_t* cnt) -> int {
    if (n_scan) {
      RadiusKnn c;
      c.passes = largek_passes(n_eff, env().largek_growth);
      c.allow = d_block;
      c.allow_label = true;
      c.allow_bits = (uint32_t)n_eff;
      c.out = ResultBlock{ids, dist, cnt, nullptr, n_scan, k};
      std::vector<uint32_t> head(kLabelHead);
      // stage 0 of a device batch [q0, q0 + mm) of the scanning queries (ONE: n_scan <= kSideChunk): the head of the label
      // block — every query's wanted label, in batch order — every query's range, and from it the sample in the query's pool
      c.fill_pool = [&](size_t q0, size_t mm, uint64_t* pool, uint32_t* pool_cnt) -> int {
        for (size_t j = 0; j < kLabelHead; ++j)   // (padding queries repeat the last: they collect nothing)
          head[j] = p.table[gs[q0 + std::min(j, mm - 1)]];
        // (pageable host memory: the runtime stages it before the call returns)
        HIP_TRY(hipMemcpyAsync(d_block, head.data(), kLabelHead * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        const std::vector<uint64_t> range = ranges_of(nullptr, q0, mm);
        HIP_TRY(hipMemcpyAsync(w.dRange.p, range.data(), 2 * mm * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        HIP_TRY(launch_grouped_range_seed(d_list, w.dRange.p, w.dRange.p + mm, pool, pool_cnt, (uint32_t)mm, st));
        return EHX_OK;
      };
      // The scan runs over the tiles that hold the prefix; the flush drops every row at or above n_eff with the rows of
      // other labels, and the re-rank reads no row (and no group label) at or above it
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
      const int r = radius_knn(s, st, w.scan, n_pub, gq, c, &t);
      for (uint64_t b = 0; b < t.batches; ++b)   // (the int8 scan copy: every query of a batch against every prefix row once)
        count_scan_batch(s, (size_t)std::min<uint64_t>(kSideChunk, t.queries - b * kSideChunk), n_eff, k, 1);
      s->n_i8_queries += t.queries;
      s->n_i8_fallback += t.handed;
      s->groupedl_ctr[0] += t.queries - t.handed;
      s->groupedl_ctr[1] += t.handed;
      s->groupedl_ctr[2] += t.overflowed;
      s->groupedl_ctr[3] += t.batches * c.passes.size();
      if (r) return r;
    }
    if (n_scan == m) return EHX_OK;
    s->groupedl_ctr[1] += m - n_scan;
    return list(ranges_of(nullptr, n_scan, m - n_scan), m - n_scan, gq + n_scan * s->dims, ids + n_scan * k, dist + n_scan * k,
                cnt + n_scan, true);
  };
  if (in_order) return answer(m, d_queries, out.ids, out.dist, out.cnt);
  return w.group.rerun(s, st, d_queries, idx, k, answer, out.ids, out.dist, out.cnt);
}

// an unsharded space, locked shared, scratch_mu held, its device current; everything is enqueued on `st`.  group_of /
// label_of: at least min(n_labels, row count) entries each, in host memory (cols_on_host: staged in grouped.dLabels and
// labeled.dCol) or on the device; want: in host memory, or d_want, read back once (the outputs unwritten until then)
int groupedl_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, uint32_t per_group,
                    const uint32_t* group_of, const uint32_t* label_of, bool cols_on_host, uint64_t n_labels,
                    const uint32_t* want, const uint32_t* d_want, const ResultBlock& out, int group_col = -1, int label_col = -1) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  if (s->ld > grouped_rerank_max_ld())   // (before anything is enqueued)
    return fail(EHX_EUNSUPPORTED, "grouped search keeps a prepared query in LDS: rows of %u floats exceed %u", s->ld,
                grouped_rerank_max_ld());
  s->groupedl_ctr[4] += 1;
  // the ONE read of the row count: the lists name rows below it only, and every later stage sees at least this prefix
  const uint64_t n_pub = s->n.load(std::memory_order_acquire);
  const bool stored = label_col >= 0;   // ehx_knn_grouped_by_label*: both columns are the space's, over the whole prefix
  const uint64_t n_eff = stored ? n_pub : std::min<uint64_t>(n_labels, n_pub);   // (row ids are 32 bits wide: n_pub < 2^32)
  if (!stored && (rc = labeled_plan_scratch(s, n_eff))) return rc;
  // (earlier calls' launches on other streams may still read the block, the lists and the staged columns)
  if ((rc = wait_searches_in_flight(s, st))) return rc;
  const uint32_t *d_group_of = group_of, *d_label_of = label_of;
  const ehx_space::ColIndex* ix = nullptr;   // the label column's index, rebuilt here if a write or an append left it stale
  if (stored && ((rc = colindex_ensure(s, st, (uint32_t)label_col, n_pub, &ix)) ||
                 (rc = column_as_groups(s, st, (uint32_t)group_col, n_pub, &d_group_of))))
    return rc;
  if (cols_on_host) {
    if ((rc = s->grouped.dLabels.ensure(std::max<uint64_t>(n_eff, 1))) || (rc = s->labeled.dCol.ensure(std::max<uint64_t>(n_eff, 1))))
      return rc;
    // (labels at or above the prefix are never looked at: they are not even copied; pageable host memory: the runtime
    // stages it before the call returns)
    if (n_eff) {
      HIP_TRY(hipMemcpyAsync(s->grouped.dLabels.p, group_of, n_eff * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(s->labeled.dCol.p, label_of, n_eff * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    d_group_of = s->grouped.dLabels.p;
    d_label_of = s->labeled.dCol.p;
  }
  std::vector<uint32_t> want_read;
  if (!want) {
    want_read.resize(nq);
    HIP_TRY(hipMemcpyAsync(want_read.data(), d_want, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    want = want_read.data();
  }
  bool col_copied = false;
  for (size_t q0 = 0; q0 < nq; q0 += kSideChunk) {
    const size_t m = std::min(kSideChunk, nq - q0);
    if ((rc = groupedl_batch(s, st, n_pub, n_eff, m, d_queries + q0 * s->dims, k, per_group, d_group_of, d_label_of, ix,
                             want + q0, &col_copied, out.from(q0, m))))
      return rc;
  }
  return EHX_OK;
}

}  // namespace

extern "C" {

int ehx_knn_grouped_labeled_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                   uint32_t per_group, const uint32_t* d_group_of, const uint32_t* d_label_of,
                                   uint64_t n_labels, const uint32_t* d_want, uint64_t* d_out_ids, float* d_out_dist,
                                   uint32_t* d_out_count) {
  if (int rc = groupedl_check(s, n_queries, k, per_group, d_queries, d_group_of, d_label_of, n_labels, d_want, d_out_ids,
                              d_out_dist, d_out_count))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_knn_grouped_labeled_device", kGroupedLabeledWhy, n_queries, &st, [&] {
    return groupedl_locked(s, st, n_queries, d_queries, k, per_group, d_group_of, d_label_of, false, n_labels, nullptr, d_want,
                           ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_knn_grouped_labeled(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint32_t per_group,
                            const uint32_t* group_of, const uint32_t* label_of, uint64_t n_labels, const uint32_t* want,
                            uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (int rc = groupedl_check(s, n_queries, k, per_group, queries, group_of, label_of, n_labels, want, out_ids, out_dist,
                              out_count))
    return rc;
  return search_on_device(s, "ehx_knn_grouped_labeled", kGroupedLabeledWhy, n_queries, nullptr, [&]() -> int {
    int rc;
    HostStage& h = s->groupedl.host;
    if ((rc = h.up(s->stream, queries, n_queries, s->dims, k, false))) return rc;
    if ((rc = groupedl_locked(s, s->stream, n_queries, h.q, k, per_group, group_of, label_of, true, n_labels, want, nullptr,
                              h.out)))
      return rc;
    return h.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
  });
}

int ehx_knn_grouped_by_label_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                    uint32_t per_group, uint32_t group_col, uint32_t label_col, const uint32_t* d_want,
                                    uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count) {
  if (int rc = grouped_by_label_check(s, n_queries, k, per_group, d_queries, group_col, label_col, d_want, d_out_ids, d_out_dist,
                                      d_out_count))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_knn_grouped_by_label_device", kGroupedLabeledWhy, n_queries, &st, [&] {
    return groupedl_locked(s, st, n_queries, d_queries, k, per_group, nullptr, nullptr, false, 0, nullptr, d_want,
                           ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k}, (int)group_col, (int)label_col);
  });
}

int ehx_knn_grouped_by_label(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint32_t per_group,
                             uint32_t group_col, uint32_t label_col, const uint32_t* want, uint64_t* out_ids, float* out_dist,
                             uint32_t* out_count) {
  if (int rc = grouped_by_label_check(s, n_queries, k, per_group, queries, group_col, label_col, want, out_ids, out_dist, out_count))
    return rc;
  return search_on_device(s, "ehx_knn_grouped_by_label", kGroupedLabeledWhy, n_queries, nullptr, [&]() -> int {
    int rc;
    HostStage& h = s->groupedl.host;   // (queries up, results down: no column travels)
    if ((rc = h.up(s->stream, queries, n_queries, s->dims, k, false))) return rc;
    if ((rc = groupedl_locked(s, s->stream, n_queries, h.q, k, per_group, nullptr, nullptr, false, 0, want, nullptr, h.out,
                              (int)group_col, (int)label_col)))
      return rc;
    return h.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
  });
}

// test hook, not part of the ABI: queries answered on the scan route, on the list route (by the gate or handed on by the
// scan route), of those the ones whose pool overflowed, scan passes launched, calls
void ehx_test_grouped_labeled_counters(ehx_space* s, uint64_t out[5]) {
  for (int i = 0; i < 5; ++i) out[i] = s ? s->groupedl_ctr[i].load(std::memory_order_relaxed) : 0;
}

}  // extern "C"
