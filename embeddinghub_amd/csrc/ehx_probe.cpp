// Exact kNN under a per-query SET of stored labels: ehx_knn_by_labels (host pointers) and ehx_knn_by_labels_device.  Row r is
// allowed for query i iff r < n_pub (the call's ONE snapshot of the row count) and the stored column's value at r is among
// the first min(want_count[i], n_want) entries of row i of `want`; row i of the answer is, byte for byte,
// ehx_knn_masked_device's for query i alone under the bitmap of those rows.  An IVF probe over the library's own k-means
// labels, or "the groups this user belongs to".
// Always the list route, LIST-major (k_probe.hip): the column's index (colindex_ensure) holds every label's rows back to
// back, and the host — against the index's mirror, no device work — turns a device batch into a work list:
//   resolve     every wanted label binary-searched in the mirror; a label no row carries, a repeat inside a set and a slot
//               beyond the query's count name nothing (once per call; the longest list probed fixes the chunks per pair, C)
//   sort        the batch's (query, slot) pairs counting-sorted by label position: cursors in an array as long as the label
//               table, kept zero between plans, so a plan costs the pairs and the labels they touch, not the table
//   cut         a label's pairs into tiles of 8, a list longer than kProbeChunk rows into up to C chunks: an item per
//               (label, chunk, tile), the tiles of one chunk adjacent so that they meet its rows in L2
//   upload      the items planned in a pinned block, ONE async copy; two blocks taken in turn, so the host waits only for
//               the copy out of the block it is about to overwrite — the batch before the last one's
// then per device batch launch_prep_queries, the fill of the key lists, the probe kernel, launch_flat_merge over n_want * C
// lists per query and launch_among_emit per page of 64 with launch_set_floor in between — ehx_among.cpp's page scaffold.
// The device form waits once, for d_want and d_want_count.  Entry scaffold and host staging are ehx_call.cpp's.
#include "ehx_internal.h"

namespace {

constexpr const char* kProbeWhy = "filtered search over shards is not built yet";
constexpr uint32_t kNoList = ~0u;             // a (query, slot) pair that names no list
constexpr size_t kProbeMaxLists = 65536;      // key lists of a device batch (pairs x C): 32 MiB, half a side search's pools
static_assert(EHX_MAX_WANT * kProbeMaxChunks <= 1024, "launch_flat_merge's lists per query, as the among search bounds them");
static_assert(EHX_MAX_WANT <= 64 && kSideChunk <= (1u << 26), "a pair is packed as query << 6 | slot");

int probe_check(const ehx_space* s, size_t nq, uint32_t k, const void* q, uint32_t label_col, uint32_t n_want, const void* want,
                const void* o_ids, const void* o_dist, const void* o_cnt) {
  if (int rc = by_label_check(s, nq, k, q, label_col, want, o_ids, o_dist, o_cnt)) return rc;
  if (n_want == 0 || n_want > EHX_MAX_WANT) return fail(EHX_EINVAL, "n_want = %u: 1 to %u labels per query", n_want, (unsigned)EHX_MAX_WANT);
  return EHX_OK;
}

// where every (query, slot) pair's list lies in the index's label table (kNoList: nowhere); the longest list named
uint64_t probe_resolve(const ehx_space::ColIndex& ix, size_t nq, uint32_t n_want, const uint32_t* want, const uint32_t* want_count,
                       std::vector<uint32_t>* pos) {
  pos->assign(nq * n_want, kNoList);
  uint64_t longest = 0;
  for (size_t i = 0; i < nq; ++i) {
    const uint32_t* w = want + i * n_want;
    const uint32_t cnt = want_count ? std::min(want_count[i], n_want) : n_want;
    for (uint32_t j = 0; j < cnt; ++j) {
      if (std::find(w, w + j, w[j]) != w + j) continue;   // a label repeated inside a set counts once
      const auto it = std::lower_bound(ix.labels.begin(), ix.labels.end(), w[j]);
      if (it == ix.labels.end() || *it != w[j]) continue;   // no row carries the label
      const uint32_t t = (uint32_t)(it - ix.labels.begin());
      (*pos)[i * n_want + j] = t;
      longest = std::max<uint64_t>(longest, (uint64_t)ix.start[t + 1] - ix.start[t]);
    }
  }
  return longest;
}

// the work list of the device batch whose pairs' lists are pos[0, m * n_want): *items, and what it stages and evaluates
void probe_plan(const ehx_space::ColIndex& ix, std::vector<uint32_t>& head, size_t m, uint32_t n_want, uint32_t C,
                const uint32_t* pos, std::vector<ProbeItem>* items, uint64_t* rows_staged, uint64_t* pairs_done) {
  items->clear();
  head.resize(ix.labels.size(), 0u);   // (all zero here, and again on return)
  std::vector<uint32_t> touched;
  for (size_t i = 0; i < m * n_want; ++i)
    if (pos[i] != kNoList && head[pos[i]]++ == 0) touched.push_back(pos[i]);
  std::sort(touched.begin(), touched.end());
  uint32_t run = 0;
  for (uint32_t t : touched) {   // counts -> where the label's pairs begin
    const uint32_t c = head[t];
    head[t] = run;
    run += c;
  }
  std::vector<uint32_t> pairs(run);   // query << 6 | slot, by label position, ascending within a label
  for (size_t i = 0; i < m * n_want; ++i)
    if (pos[i] != kNoList) pairs[head[pos[i]]++] = (uint32_t)((i / n_want) << 6 | (i % n_want));
  uint32_t begin = 0;
  for (uint32_t t : touched) {
    const uint32_t end = head[t];   // (the cursor has run to the label's end)
    head[t] = 0;
    const uint64_t lo0 = ix.start[t], len = (uint64_t)ix.start[t + 1] - lo0;
    const uint64_t n_ch = std::min<uint64_t>(C, (len + kProbeChunk - 1) / kProbeChunk);
    const uint64_t per = round_up((len + n_ch - 1) / n_ch, 64);   // (whole batches of 64 keys)
    for (uint32_t ch = 0; ch * per < len; ++ch) {
      ProbeItem it = {};
      it.lo = (uint32_t)(lo0 + ch * per);
      it.hi = (uint32_t)(lo0 + std::min<uint64_t>(len, (ch + 1) * per));
      it.chunk = ch;
      for (uint32_t p0 = begin; p0 < end; p0 += kProbeTilePairs) {
        it.n_pairs = std::min<uint32_t>(kProbeTilePairs, end - p0);
        for (uint32_t j = 0; j < kProbeTilePairs; ++j) {
          it.q[j] = j < it.n_pairs ? pairs[p0 + j] >> 6 : 0u;
          it.slot[j] = j < it.n_pairs ? pairs[p0 + j] & 63u : 0u;
        }
        items->push_back(it);
        *rows_staged += it.hi - it.lo;
        *pairs_done += (uint64_t)(it.hi - it.lo) * it.n_pairs;
      }
    }
    begin = end;
  }
}

// the items into the pinned block whose turn it is, and from there to the device in one copy
int probe_upload(ehx_space* s, hipStream_t st, const std::vector<ProbeItem>& items) {
  ehx_space::Probe& w = s->probe;
  const uint32_t b = w.turn++ & 1u;
  int rc;
  if (w.up_pending[b]) HIP_TRY(hipEventSynchronize(w.up_ev[b]));   // (the copy of two plans ago: long done as a rule)
  w.up_pending[b] = false;
  if ((rc = w.hItems[b].ensure(round_up(items.size(), 4096))) || (rc = w.up_ev[b].ensure(hipEventDisableTiming))) return rc;
  std::copy(items.begin(), items.end(), w.hItems[b].p);
  HIP_TRY(hipMemcpyAsync(w.dItems.p, w.hItems[b].p, items.size() * sizeof(ProbeItem), hipMemcpyHostToDevice, st));
  HIP_TRY(hipEventRecord(w.up_ev[b], st));
  w.up_pending[b] = true;
  return EHX_OK;
}

// an unsharded space, locked shared, scratch_mu held, its device current; everything is enqueued on `st`.  n_pub: the call's
// ONE read of the row count.  want / want_count: host memory, or nullptr with d_want / d_want_count (read back: one wait).
int probe_locked(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const float* d_queries, uint32_t k, uint32_t label_col,
                 uint32_t n_want, const uint32_t* want, const uint32_t* want_count, const uint32_t* d_want,
                 const uint32_t* d_want_count, const ResultBlock& out) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  if (s->ld > probe_max_ld())   // (before anything is enqueued)
    return fail(EHX_EUNSUPPORTED, "the label-set search keeps 8 prepared queries and 8 rows in LDS: rows of %u floats exceed %u",
                s->ld, probe_max_ld());
  s->probe_ctr[0] += 1;
  // (earlier calls' launches on other streams may still read the index, the work list and the exhaustive pass's scratch)
  if ((rc = wait_searches_in_flight(s, st))) return rc;
  const ehx_space::ColIndex* ix = nullptr;
  if ((rc = colindex_ensure(s, st, label_col, n_pub, &ix))) return rc;
  std::vector<uint32_t> want_read;
  if (!want) {
    want_read.resize(nq * n_want + (d_want_count ? nq : 0));
    HIP_TRY(hipMemcpyAsync(want_read.data(), d_want, nq * n_want * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (d_want_count)
      HIP_TRY(hipMemcpyAsync(want_read.data() + nq * n_want, d_want_count, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // the call's one wait
    want = want_read.data();
    want_count = d_want_count ? want_read.data() + nq * n_want : nullptr;
  }
  std::vector<uint32_t> pos;
  const uint64_t longest = probe_resolve(*ix, nq, n_want, want, want_count, &pos);
  const uint32_t C = (uint32_t)std::min<uint64_t>(kProbeMaxChunks, std::max<uint64_t>(1, (longest + kProbeChunk - 1) / kProbeChunk));
  const uint32_t lists = n_want * C, pages = (k + 63) / 64;
  const size_t m_max = std::min(nq, std::max<size_t>(1, std::min(kSideChunk, kProbeMaxLists / lists)));
  if ((rc = s->scr.dQ.ensure(m_max * s->ld)) || (rc = s->scr.dPart.ensure(m_max * lists * 64)) ||
      (rc = s->scr.dMerged.ensure(m_max * 64)) || (rc = s->scr.dGthr.ensure(m_max + 8)) ||
      (rc = s->probe.dItems.ensure(m_max * lists)))   // (an item per (label, chunk, tile): at most one per pair and chunk)
    return rc;
  ProbeArgs a = {};
  a.rows = rows_view(s, n_pub);
  a.Q = s->scr.dQ.p;
  a.perm = ix->dPerm.p;
  a.n_perm = ix->n;
  a.items = s->probe.dItems.p;
  a.out = s->scr.dPart.p;
  a.n_want = n_want;
  a.n_chunks = C;
  std::vector<ProbeItem> items;
  for (size_t q0 = 0; q0 < nq; q0 += m_max) {
    const size_t m = std::min(m_max, nq - q0);
    uint64_t rows_staged = 0, pairs_done = 0;
    probe_plan(*ix, s->probe.head, m, n_want, C, pos.data() + q0 * n_want, &items, &rows_staged, &pairs_done);
    a.nq = (uint32_t)m;
    a.n_items = (uint32_t)items.size();
    const ResultBlock o = out.from(q0, m);
    if ((rc = s->clock.begin(st, BatchClock::kOutOfRing))) return rc;
    if (a.n_items && (rc = probe_upload(s, st, items))) return rc;
    HIP_TRY(launch_prep_queries(d_queries + q0 * s->dims, (uint32_t)m, s->dims, s->ld, (uint32_t)m, s->metric, s->scr.dQ.p, st));
    HIP_TRY(launch_probe_fill(a.out, m * lists * 64, st));   // (once: every page's items write the same blocks)
    if ((rc = s->clock.scan_begin(st))) return rc;
    for (uint32_t pg = 0; pg < pages; ++pg) {
      a.floor = pg ? s->scr.dGthr.p : nullptr;
      HIP_TRY(launch_probe(a, st));
      HIP_TRY(launch_flat_merge(a.out, (uint32_t)m, lists, 64, s->scr.dMerged.p, st, lists));
      if (pg + 1 < pages) HIP_TRY(launch_set_floor(s->scr.dMerged.p, (uint32_t)m, s->scr.dGthr.p, st));
      HIP_TRY(launch_among_emit(s->scr.dMerged.p, (uint32_t)m, std::min<uint32_t>(64, k - pg * 64), k, pg * 64, o.ids, o.dist,
                                o.cnt, st));
    }
    if ((rc = s->clock.scan_end(st)) || (rc = s->clock.finish(st))) return rc;
    s->n_queries += m;
    s->n_dist += pairs_done * pages;
    s->probe_ctr[1] += (uint64_t)a.n_items * pages;
    s->probe_ctr[2] += rows_staged * pages;
    s->probe_ctr[3] += pairs_done * pages;
  }
  return EHX_OK;
}

}  // namespace

extern "C" {

int ehx_knn_by_labels_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k, uint32_t label_col,
                             uint32_t n_want, const uint32_t* d_want, const uint32_t* d_want_count, uint64_t* d_out_ids,
                             float* d_out_dist, uint32_t* d_out_count) {
  if (int rc = probe_check(s, n_queries, k, d_queries, label_col, n_want, d_want, d_out_ids, d_out_dist, d_out_count)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_knn_by_labels_device", kProbeWhy, n_queries, &st, [&] {
    const uint64_t n_pub = s->n.load(std::memory_order_acquire);   // the ONE read of the row count
    test_pause();   // (an append may publish here: the index and every stage describe n_pub rows all the same)
    return probe_locked(s, st, n_pub, n_queries, d_queries, k, label_col, n_want, nullptr, nullptr, d_want, d_want_count,
                        ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_knn_by_labels(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint32_t label_col, uint32_t n_want,
                      const uint32_t* want, const uint32_t* want_count, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (int rc = probe_check(s, n_queries, k, queries, label_col, n_want, want, out_ids, out_dist, out_count)) return rc;
  return search_on_device(s, "ehx_knn_by_labels", kProbeWhy, n_queries, nullptr, [&]() -> int {
    int rc;
    const uint64_t n_pub = s->n.load(std::memory_order_acquire);   // the ONE read of the row count
    test_pause();
    HostStage& h = s->probe.host;   // (queries up, results down: the sets are planned where they lie)
    if ((rc = h.up(s->stream, queries, n_queries, s->dims, k, false))) return rc;
    if ((rc = probe_locked(s, s->stream, n_pub, n_queries, h.q, k, label_col, n_want, want, want_count, nullptr, nullptr, h.out)))
      return rc;
    return h.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
  });
}

// test hook, not part of the ABI: calls, work items launched, rows staged, (row, query) pairs evaluated
void ehx_test_probe_counters(ehx_space* s, uint64_t out[4]) {
  for (int i = 0; i < 4; ++i) out[i] = s ? s->probe_ctr[i].load(std::memory_order_relaxed) : 0;
}

}  // extern "C"
