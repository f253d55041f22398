// Exact kNN under a label column: ehx_knn_labeled (host pointers) and ehx_knn_labeled_device.  One opaque 32-bit label per
// row, one wanted label per query; row r is allowed for query i iff r < n_eff = min(the call's ONE snapshot of the row count,
// n_labels) and label_of[r] == want[i].  Row i of the answer is, byte for byte, ehx_knn_masked_device's for query i alone
// under the bitmap of those rows.  The number of distinct wanted labels is not limited: a call is served in device batches
// of kSideChunk queries, and per batch
//   slots        the host sorts and de-duplicates the batch's wanted labels: at most 2048 "slots"
//   compaction   k_labeled.hip: per-slot row counts (read back: the first wait), every slot's list of row ids back to back in
//                masked.dList, and — for the slots that scan — the rows before every 256-row tile (read back: the second wait,
//                taken only where some slot scans), an ascending list and the by-rank sample
//   answer       the bitmap search's (filtered_answer, ehx_masked.cpp): its routing rule per slot, its grouping, its ONE pass
//                plan, its first radius and its re-runs, with the row test of the int8 scan's flush "the row's label is the
//                query's" (kMaskLabel, k_flati8.hip: ONE block, every query's wanted label | a copy of the column)
// At most 127 slots can scan: a slot scans only with more than masked_exact_cut(n) = max(1024, n / 128) rows, the slots'
// rows are disjoint, and n / max(1024, n / 128) <= 128 with a strict "more than" — so the tile prefixes are a table of at
// most 127 x tiles, never slots x tiles.  The cut itself is CARRIED OVER from the bitmap search, where it was measured for a
// list shared by the whole batch (scripts/bench_masked.py); it was not measured for this call — scripts/bench_labeled.py
// leg (c) records where the two routes cross here.
// The list route: a slot that at least kLabeledSharedMin queries of the batch name takes the shared-list tile kernel over
// their range, as every mask does; all the others — in a batch of 1024 tenants, all of them — go through ONE per-query-list
// launch (AmongArgs::cand_end lets queries of one slot name the same list), not one launch per label.
// The device form waits once for d_want (the whole call's), then per device batch at most twice for the compaction — the
// counts, and the scanning slots' tile prefixes — whatever the number of labels the batch names; the scan route's verdict is
// radius_knn's one wait per device batch, as under bitmaps.
// The compaction is a plan (LabeledPlan, labeled_plan), the view over it labeled_view, and the body of a call — checks,
// scratch, waits, staging, the loop over device batches — labeled_call (all in ehx_internal.h): the grouped search under a
// label column (ehx_groupedl.cpp) shares the three and differs in what it passes (LabelCall: whether the scan route serves,
// the cut, the gate — none here) and in what answers a device batch.  A slot's route: filter_routes_cut / _gate (ehx_masked.cpp).
// Entry scaffold and host staging are ehx_call.cpp's (search_shared / on_device, HostStage).
#include "ehx_internal.h"

namespace {

constexpr const char* kLabeledWhy = "filtered search over shards is not built yet";
constexpr uint32_t kLabeledSharedMin = kAmongTileQ;   // one query tile of the shared-list kernel: a choice, not measured
static_assert(kSideChunk <= kLabeledMaxSlots, "a device batch names at most one slot per query");
static_assert(kTabWords == kLabelHead, "the head of the label block is the head filtered_answer rewrites per device batch");

int labeled_check(const ehx_space* s, size_t nq, uint32_t k, const void* q, const void* label_of, uint64_t n_labels,
                  const void* want, const void* o_ids, const void* o_dist, const void* o_cnt) {
  if (!s) return fail(EHX_EINVAL, "space is NULL");   // (before the device is looked for)
  int rc = ehx_init(nullptr, 0);
  if (rc) return rc;
  if ((rc = check_batch_call(s, nq, k, "k", false, o_ids && o_dist && o_cnt && (!nq || q)))) return rc;
  if (n_labels && !label_of) return fail(EHX_EINVAL, "NULL label_of with n_labels = %llu", (unsigned long long)n_labels);
  if (!want) return fail(EHX_EINVAL, "NULL want");
  return EHX_OK;
}

// ehx_knn_by_label*: ehx_knn_labeled*'s checks with their codes and in their order (the column is the space's: no pointer,
// no length), then the column number
int by_label_check(const ehx_space* s, size_t nq, uint32_t k, const void* q, uint32_t label_col, const void* want,
                   const void* o_ids, const void* o_dist, const void* o_cnt) {
  if (int rc = labeled_check(s, nq, k, q, nullptr, 0, want, o_ids, o_dist, o_cnt)) return rc;
  if (label_col >= EHX_MAX_COLUMNS) return fail(EHX_EINVAL, "label_col = %u: a space has %u columns", label_col, (unsigned)EHX_MAX_COLUMNS);
  return EHX_OK;
}

}  // namespace

namespace ehx_impl {

// the scratch labeled_plan fills, sized for a prefix of n_eff rows (once per call, before anything is enqueued)
static int labeled_plan_scratch(ehx_space* s, uint64_t n_eff) {
  ehx_space::Labeled& w = s->labeled;
  int rc;
  if ((rc = w.dBlock.ensure(kLabelHead + std::max<uint64_t>(n_eff, 1))) || (rc = w.dSlotOf.ensure(std::max<uint64_t>(n_eff, 1))) ||
      (rc = w.dSlots.ensure(4 * (size_t)kLabeledMaxSlots)) || (rc = w.dOff.ensure((size_t)kLabeledMaxSlots + kLabeledMaxScan + 1)))
    return rc;
  return EHX_OK;
}

// the slots: the batch's distinct wanted labels, ascending, and the slot of every query
void labeled_slots(const uint32_t* want, size_t m, LabeledPlan* p) {
  std::vector<uint32_t>& table = p->table;
  table.assign(want, want + m);
  p->slot_of.resize(m);
  std::sort(table.begin(), table.end());
  table.erase(std::unique(table.begin(), table.end()), table.end());
  p->n_slots = (uint32_t)table.size();
  for (size_t j = 0; j < m; ++j)
    p->slot_of[j] = (uint32_t)(std::lower_bound(table.begin(), table.end(), want[j]) - table.begin());
}

// The compaction of the column for one device batch (ehx_internal.h has the contract).
int labeled_plan(ehx_space* s, hipStream_t st, uint64_t n_eff, size_t m, const uint32_t* d_label_of, const uint32_t* want,
                 bool scan_serves, uint64_t cut, size_t min_scan_queries, bool* col_copied, LabeledPlan* p) {
  int rc;
  ehx_space::Labeled& w = s->labeled;
  ehx_space::Masked& mw = s->masked;
  const uint32_t n_tiles = p->n_tiles = (uint32_t)((n_eff + kTileRows16 - 1) / kTileRows16);
  labeled_slots(want, m, p);
  std::vector<uint32_t>& table = p->table;
  const uint32_t n_slots = p->n_slots;
  uint32_t* d_table = w.dSlots.p;
  uint32_t* d_count = d_table + kLabeledMaxSlots;
  uint32_t* d_scan_of = d_count + kLabeledMaxSlots;
  uint32_t* d_cursor = d_scan_of + kLabeledMaxSlots;
  // (pageable host memory, here and below: the runtime stages it before the call returns)
  HIP_TRY(hipMemcpyAsync(d_table, table.data(), n_slots * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  std::vector<uint32_t> count(n_slots, 0u);
  if (n_tiles) {
    HIP_TRY(launch_labeled_count(d_label_of, n_eff, d_table, n_slots, w.dSlotOf.p, d_count, st));
    HIP_TRY(hipMemcpyAsync(count.data(), d_count, n_slots * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // the first wait
  }
  // routing per slot (filter_routes: the bitmap search's rule; with min_scan_queries the grouped search's gate on top of it),
  // decided BEFORE the lists are filled: where the lists start, and the scanning slots' indices
  std::vector<uint64_t>& n_allowed = p->n_allowed;
  n_allowed.assign(count.begin(), count.end());
  std::vector<char>& scans = p->scans;
  scans.assign(n_slots, 0);
  filter_routes_cut(scan_serves, cut, n_allowed.data(), n_slots, scans.data());
  filter_routes_gate(p->slot_of.data(), m, min_scan_queries, n_slots, scans.data());
  std::vector<uint64_t>& off = p->off;
  std::vector<uint64_t> scan_off;
  off.assign(n_slots, 0);
  std::vector<uint32_t>& scan_of = p->scan_of;
  scan_of.assign(n_slots, kLabeledNoScan);
  uint64_t total = 0;
  for (uint32_t f = 0; f < n_slots; ++f) {
    off[f] = total;
    total += count[f];
    if (!scans[f]) continue;
    scan_of[f] = (uint32_t)scan_off.size();
    scan_off.push_back(off[f]);
  }
  p->total = total;
  const uint32_t n_scan = p->n_scan = (uint32_t)scan_off.size();
  if (n_scan > kLabeledMaxScan || total > n_eff)   // (disjoint sets of more than max(1024, n / 128) rows each: at most 127)
    return fail(EHX_EINTERNAL, "label compaction: %u scanning labels, %llu listed rows of %llu", n_scan,
                (unsigned long long)total, (unsigned long long)n_eff);
  std::vector<uint32_t>& cum = p->cum;
  cum.assign((size_t)n_scan * (n_tiles + 1), 0u);
  if ((rc = mw.dList.ensure(std::max<uint64_t>(total, 1)))) return rc;
  if (n_tiles) {
    uint64_t* d_off = w.dOff.p;
    uint64_t* d_scan_off = d_off + kLabeledMaxSlots;
    HIP_TRY(hipMemcpyAsync(d_off, off.data(), n_slots * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_scan_of, scan_of.data(), n_slots * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (n_scan) {
      if ((rc = mw.dCum.ensure(cum.size()))) return rc;
      HIP_TRY(hipMemcpyAsync(d_scan_off, scan_off.data(), n_scan * sizeof(uint64_t), hipMemcpyHostToDevice, st));
      HIP_TRY(launch_labeled_tiles(w.dSlotOf.p, n_eff, n_tiles, d_scan_of, n_scan, mw.dCum.p, st));
      HIP_TRY(hipMemcpyAsync(cum.data(), mw.dCum.p, cum.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(launch_labeled_fill(w.dSlotOf.p, n_eff, n_tiles, n_slots, d_off, d_scan_of, n_scan, mw.dCum.p, d_cursor, mw.dList.p, st));
    if (n_scan) {
      if (!*col_copied)   // the flush's copy of the column: 4 bytes per row, once per call
        HIP_TRY(hipMemcpyAsync(w.dBlock.p + kLabelHead, d_label_of, n_eff * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
      *col_copied = true;
      HIP_TRY(hipStreamSynchronize(st));   // the second wait: the host plans the passes from the tile prefixes
    }
  }
  return EHX_OK;
}

}  // namespace ehx_impl

namespace ehx_impl {

FilterView labeled_view(ehx_space* s, hipStream_t st, uint64_t n_pub, uint64_t n_eff, const LabeledPlan& p,
                        const ehx_space::ColIndex* ix) {
  ehx_space::Labeled& w = s->labeled;
  ehx_space::Masked& mw = s->masked;
  FilterView v;
  v.n_pub = n_pub;
  v.n_eff = n_eff;
  v.list_rows = p.total;
  v.n_tiles = p.n_tiles;
  v.n_filters = p.n_slots;
  v.n_allowed = p.n_allowed.data();
  v.off = p.off.data();
  v.filter_of = p.slot_of.data();
  v.scans = p.scans.data();
  v.cum = ix ? ix->cum.data() : p.cum.data();
  v.scan_of = p.scan_of.data();
  v.d_list = ix ? ix->dPerm.p : mw.dList.p;
  v.sample = ix ? &ix->dSample : &mw.dSample;
  v.samples = [s, st, &p, ix]() -> int {
    if (ix) return EHX_OK;   // (prepared when the index was built)
    ehx_space::Masked& m = s->masked;
    if (int r = m.dSample.ensure((size_t)p.n_scan * 256)) return r;
    HIP_TRY(launch_labeled_samples(m.dList.p, s->labeled.dOff.p + kLabeledMaxSlots, m.dCum.p, p.n_scan, p.n_tiles, m.dSample.p, st));
    return EHX_OK;
  };
  v.allow = v.d_head = ix ? ix->dBlock.p : w.dBlock.p;
  v.allow_label = true;
  v.head_of = p.table.data();   // (the head word of a query is its wanted label itself)
  v.shared_min = kLabeledSharedMin;
  v.d_range = &w.dRange;
  return v;
}

int labeled_call(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const LabelCall& c, const std::function<int()>& stage,
                 const std::function<int(size_t, size_t, FilterView&)>& batch) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  if ((rc = c.fits(s))) return rc;   // (before anything is enqueued)
  c.ctr[4] += 1;
  const bool stored = c.label_col >= 0;
  const uint64_t n_eff = std::min<uint64_t>(c.n_labels, n_pub);   // (row ids are 32 bits wide: n_pub < 2^32)
  if (!stored && (rc = labeled_plan_scratch(s, n_eff))) return rc;
  // (earlier calls' launches on other streams may still read the block, the lists, the samples and the staged columns)
  if ((rc = wait_searches_in_flight(s, st))) return rc;
  const ehx_space::ColIndex* ix = nullptr;   // a stored column: its index, rebuilt here if a write or an append left it stale
  if (stored && (rc = colindex_ensure(s, st, (uint32_t)c.label_col, n_pub, &ix))) return rc;
  if (stage && (rc = stage())) return rc;
  const uint32_t* d_label_of = c.label_of;
  if (c.on_host) {
    // (labels at or above the prefix are never looked at: they are not even copied; pageable host memory: the runtime stages
    // it before the call returns)
    if ((rc = s->labeled.dCol.ensure(std::max<uint64_t>(n_eff, 1)))) return rc;
    if (n_eff) HIP_TRY(hipMemcpyAsync(s->labeled.dCol.p, c.label_of, n_eff * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    d_label_of = s->labeled.dCol.p;
  }
  const uint32_t* want = c.want;
  std::vector<uint32_t> want_read;
  if (!want) {
    want_read.resize(nq);
    HIP_TRY(hipMemcpyAsync(want_read.data(), c.d_want, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    want = want_read.data();
  }
  bool col_copied = false;
  for (size_t q0 = 0; q0 < nq; q0 += kSideChunk) {
    const size_t m = std::min(kSideChunk, nq - q0);
    LabeledPlan p;
    if (ix) colindex_plan(*ix, m, want + q0, c.scan_serves, c.cut, c.min_scan_queries, &p);
    else if ((rc = labeled_plan(s, st, n_eff, m, d_label_of, want + q0, c.scan_serves, c.cut, c.min_scan_queries, &col_copied, &p)))
      return rc;
    FilterView v = labeled_view(s, st, n_pub, n_eff, p, ix);
    v.ctr = c.ctr;
    if ((rc = batch(q0, m, v))) return rc;
  }
  return EHX_OK;
}

}  // namespace ehx_impl

namespace {

// ehx_knn_labeled* and ehx_knn_by_label* over labeled_call: the kNN's routing inputs, filtered_answer per device batch
int labeled_locked(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const float* d_queries, uint32_t k, LabelCall c,
                   const ResultBlock& out) {
  const uint32_t forced = s->labeled_route.load(std::memory_order_relaxed);   // (test hook: the bench's crossover sweep)
  c.scan_serves = filter_scan_serves(s, k, n_pub);
  c.cut = forced == 1 ? 0 : forced == 2 ? ~0ull : masked_exact_cut(n_pub);
  c.fits = [](const ehx_space* sp) { return check_rows_fit_lds(sp, "filtered search"); };
  c.ctr = s->labeled_ctr;
  return labeled_call(s, st, n_pub, nq, c, nullptr, [&](size_t q0, size_t m, FilterView& v) {
    return filtered_answer(s, st, m, d_queries + q0 * s->dims, k, v, out.from(q0, m));
  });
}

}  // namespace

extern "C" {

int ehx_knn_labeled_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                           const uint32_t* d_label_of, uint64_t n_labels, const uint32_t* d_want, uint64_t* d_out_ids,
                           float* d_out_dist, uint32_t* d_out_count) {
  if (int rc = labeled_check(s, n_queries, k, d_queries, d_label_of, n_labels, d_want, d_out_ids, d_out_dist, d_out_count))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_knn_labeled_device", kLabeledWhy, n_queries, &st, [&] {
    // the ONE read of the row count: the lists name rows below it only, and every later stage sees at least this prefix
    const uint64_t n_pub = s->n.load(std::memory_order_acquire);
    return labeled_locked(s, st, n_pub, n_queries, d_queries, k, LabelCall{d_label_of, false, -1, n_labels, nullptr, d_want},
                          ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_knn_labeled(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const uint32_t* label_of,
                    uint64_t n_labels, const uint32_t* want, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (int rc = labeled_check(s, n_queries, k, queries, label_of, n_labels, want, out_ids, out_dist, out_count)) return rc;
  return search_on_device(s, "ehx_knn_labeled", kLabeledWhy, n_queries, nullptr, [&]() -> int {
    int rc;
    const uint64_t n_pub = s->n.load(std::memory_order_acquire);   // the ONE read of the row count
    HostStage& h = s->labeled.host;
    if ((rc = h.up(s->stream, queries, n_queries, s->dims, k, false))) return rc;
    // (the column is staged in labeled.dCol by the body, behind its wait for the searches in flight)
    if ((rc = labeled_locked(s, s->stream, n_pub, n_queries, h.q, k, LabelCall{label_of, true, -1, n_labels, want, nullptr}, h.out)))
      return rc;
    return h.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
  });
}

int ehx_knn_by_label_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k, uint32_t label_col,
                            const uint32_t* d_want, uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count) {
  if (int rc = by_label_check(s, n_queries, k, d_queries, label_col, d_want, d_out_ids, d_out_dist, d_out_count)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_knn_by_label_device", kLabeledWhy, n_queries, &st, [&] {
    const uint64_t n_pub = s->n.load(std::memory_order_acquire);   // the ONE read of the row count
    test_pause();   // (an append may publish here: the index and every stage describe n_pub rows all the same)
    return labeled_locked(s, st, n_pub, n_queries, d_queries, k, LabelCall{nullptr, false, (int)label_col, n_pub, nullptr, d_want},
                          ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_knn_by_label(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint32_t label_col, const uint32_t* want,
                     uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (int rc = by_label_check(s, n_queries, k, queries, label_col, want, out_ids, out_dist, out_count)) return rc;
  return search_on_device(s, "ehx_knn_by_label", kLabeledWhy, n_queries, nullptr, [&]() -> int {
    int rc;
    const uint64_t n_pub = s->n.load(std::memory_order_acquire);   // the ONE read of the row count
    test_pause();
    HostStage& h = s->labeled.host;   // (queries up, results down: no column travels)
    if ((rc = h.up(s->stream, queries, n_queries, s->dims, k, false))) return rc;
    if ((rc = labeled_locked(s, s->stream, n_pub, n_queries, h.q, k, LabelCall{nullptr, false, (int)label_col, n_pub, want, nullptr},
                             h.out)))
      return rc;
    return h.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
  });
}

// test hook, not part of the ABI: queries answered on the scan route, on the list route, queries that overflowed, scan
// passes launched, calls
void ehx_test_labeled_counters(ehx_space* s, uint64_t out[5]) {
  for (int i = 0; i < 5; ++i) out[i] = s ? s->labeled_ctr[i].load(std::memory_order_relaxed) : 0;
}

// test hook, not part of the ABI: 0 the cut decides the route (the default), 1 the scan route for every non-empty label where
// the int8 scan serves (more than 127 such labels in one batch: EHX_EINTERNAL), 2 the list route for every label — how
// scripts/bench_labeled.py finds where they cross
void ehx_test_labeled_route(ehx_space* s, uint32_t route) {
  if (s) s->labeled_route.store(route <= 2u ? route : 0u, std::memory_order_relaxed);
}

}  // extern "C"
