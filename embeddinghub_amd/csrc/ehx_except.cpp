// kNN with per-query exclusion lists: ehx_knn_except (host pointers), ehx_knn_except_device and ehx_knn_except_keys (the lists
// given as stored keys).  Row i of the answer: the first k rows of the prefix — ONE snapshot of the row count — in (canonical
// distance, id) order that query i's list does not name; ehx_knn_masked's answer under the complement bitmap of the list
// (include/ehx.h has the contract, k_except.hip's header the kernels and why the answer is exact).  The lists travel with the
// call in CSR form; nothing is stored with the rows, and the int8 scan kernel does not know of them.
//   scan route    flat spaces whose int8 scan serves a radius on the prefix (i8_serves_radius), plain rows (no x_perm), device
//                 batches of at least kLargeKMinQueries queries, EVERY k <= 256 — k <= 48 too: the certified chain's k + 8
//                 candidate slots cannot absorb excluded rows.  The falling-radius kNN (radius_knn, ehx_call.cpp) as the
//                 large-k route plans it (largek_passes, the strided seed), with except_rerank_kernel as its re-rank and, in
//                 front of a device batch's seed, except_lists_kernel: the lists are sorted once, not once per pass.  The
//                 queries it hands on — pool overflow, a radius the bound does not serve (a sample with fewer than k allowed
//                 rows leaves it at +Inf) — go, each with its own list, still sorted in the scratch, to the
//   exact route   everything else (graph spaces, which answer from their stored rows; small spaces; SCAN_F32 / SCAN_F16; small
//                 batches): consecutive slabs of kPoolCap rows of the whole prefix (launch_grouped_range_slab with the
//                 identity list) through the same re-rank in pass mode, the radius falling from +Inf, the last slab in last
//                 mode — one launch pair per slab for the whole device batch.  Every row's canonical distance is computed at
//                 most once, for any k <= 256.
// Entry scaffold, host staging, sub-batch re-runs: ehx_call.cpp's (search_on_device, HostStage, SubsetBufs::rerun).
#include "ehx_internal.h"

namespace {

constexpr const char* kExceptWhy = "search with exclusion lists over shards is not built yet";

static_assert(EHX_EXCEPT_MAX_LIST == kExceptMaxList, "the header's limit is the kernel's LDS list");
static_assert(EHX_MAX_K_GROUPED == kLargeKMax, "the re-rank carries one key per thread");

}  // namespace

namespace ehx_impl {

// what is decided before the device is looked for, with its codes and in this order (s is not read)
int except_check(const ehx_space* s, size_t nq, uint32_t k, bool ptrs_ok) {
  if (!s) return fail(EHX_EINVAL, "space is NULL");
  if (k == 0) return fail(EHX_EINVAL, "k is 0");
  if (k > EHX_MAX_K_GROUPED) return fail(EHX_EUNSUPPORTED, "k=%u exceeds %u", k, EHX_MAX_K_GROUPED);
  if (!ptrs_ok) return fail(EHX_EINVAL, "NULL argument");
  return check_batch_size(nq);
}

int except_check_ld(const ehx_space* s) {
  if (int rc = check_rows_fit_lds(s, "search with exclusion lists")) return rc;
  if (s->ld > except_rerank_max_ld())
    return fail(EHX_EUNSUPPORTED, "search with exclusion lists keeps a pool, a list and a prepared query in LDS: rows of %u floats exceed %u",
                s->ld, except_rerank_max_ld());
  return EHX_OK;
}

// the offsets of a call, host memory: non-decreasing, ending at n_excl, no list longer than the kernel's (instead: the entry
// point the message names for longer lists)
int except_check_off(const uint64_t* off, size_t nq, size_t n_excl, const char* name, const char* n_name, const char* instead) {
  for (size_t i = 0; i < nq; ++i) {
    if (off[i] > off[i + 1]) return fail(EHX_EINVAL, "%s is not non-decreasing at query %zu", name, i);
    if (off[i + 1] - off[i] > EHX_EXCEPT_MAX_LIST)
      return fail(EHX_EINVAL, "query %zu excludes %llu entries, more than EHX_EXCEPT_MAX_LIST = %u: use %s with a bitmap per query",
                  i, (unsigned long long)(off[i + 1] - off[i]), EHX_EXCEPT_MAX_LIST, instead);
  }
  if (off[nq] != n_excl)
    return fail(EHX_EINVAL, "%s ends at %llu, not at %s = %zu", name, (unsigned long long)off[nq], n_name, n_excl);
  return EHX_OK;
}

// The exact route for nq queries, enqueued on `st`.  Their lists: d_excl_ids / d_excl_off (the entry of query 0 first),
// sorted here per device batch; or, with d_excl_off == nullptr, the lists the scan route's device batch left sorted in the
// scratch, query j's being list d_list_of[j] (nq <= kSideChunk then).
int except_exact(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const float* d_queries, uint32_t k,
                 const uint64_t* d_excl_ids, const uint64_t* d_excl_off, const uint32_t* d_list_of, uint64_t* d_ids, float* d_dist,
                 uint32_t* d_count, bool count_queries) {
  ehx_space::Except& w = s->except;
  const size_t cap = std::min(kSideChunk, nq);
  int rc;
  if ((rc = s->scr.dQ.ensure(cap * s->ld)) || (rc = w.dPool.ensure(cap * kPoolCap)) || (rc = w.dCtl.ensure(2 * cap)) ||
      (rc = w.exact.dTop.ensure(cap * kLargeKMax)) || (rc = w.exact.dTopCnt.ensure(cap)) || (rc = w.exact.dRadius.ensure(cap)) ||
      (rc = w.exact.dWork.ensure(cap)) || (rc = w.dRange.ensure(2 * cap)))
    return rc;
  if (d_excl_off && ((rc = w.dSorted.ensure(cap * kExceptMaxList)) || (rc = w.dSortedCnt.ensure(cap)))) return rc;
  std::vector<uint64_t> up(2 * cap, 0);   // a device batch's [m] starts | [m] ends: every query walks the whole prefix
  const uint64_t n_slabs = std::max<uint64_t>(1, (n_pub + kPoolCap - 1) / kPoolCap);   // (no row: one empty slab writes the page)
  for (size_t q0 = 0; q0 < nq; q0 += kSideChunk) {
    const size_t m = std::min(kSideChunk, nq - q0);
    std::fill(up.begin() + m, up.begin() + 2 * m, n_pub);
    // (searches on other streams have read and written this scratch; this batch's fence makes a Set that rewrites rows in
    // place wait for it in turn)
    if ((rc = wait_searches_in_flight(s, st))) return rc;
    if ((rc = s->clock.begin(st, BatchClock::kOutOfRing))) return rc;
    HIP_TRY(hipMemsetAsync(w.dCtl.p, 0, 2 * m * sizeof(uint32_t), st));
    // (pageable host memory: the runtime stages it before the call returns)
    HIP_TRY(hipMemcpyAsync(w.dRange.p, up.data(), 2 * m * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(launch_prep_queries(d_queries + q0 * s->dims, (uint32_t)m, s->dims, s->ld, (uint32_t)m, s->metric, s->scr.dQ.p, st));
    if (d_excl_off)
      HIP_TRY(launch_except_lists(d_excl_ids, d_excl_off + q0, (uint32_t)m, n_pub, w.dSorted.p, w.dSortedCnt.p, st));
    ExceptRerankArgs e = {};
    e.sorted = w.dSorted.p;
    e.sorted_cnt = w.dSortedCnt.p;
    e.list_of = d_excl_off ? nullptr : d_list_of;
    RadiusRerankArgs& r = e.r;
    r.Q = s->scr.dQ.p;
    r.rows = rows_view(s, n_pub);
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
      HIP_TRY(launch_grouped_range_slab(nullptr, w.dRange.p, w.dRange.p + m, b, b == 0, w.dPool.p, w.dCtl.p, r.radius, r.top_cnt,
                                        r.work, (uint32_t)m, st));
      r.mode = b + 1 == n_slabs ? kRadiusLast : kRadiusPass;
      HIP_TRY(launch_except_rerank(e, st));
    }
    if ((rc = s->clock.scan_end(st)) || (rc = s->clock.finish(st))) return rc;
  }
  if (count_queries) s->n_queries += nq;
  s->n_dist += (uint64_t)nq * n_pub;
  return EHX_OK;
}

// the row ids of a call's stored keys (space locked shared; takes kmu shared).  A key that is not stored names no row: an id
// no prefix holds, which the list preparation drops
int except_key_ids(ehx_space* s, const char* const* keys, const size_t* klens, size_t n_keys, std::vector<uint64_t>* ids) {
  ids->assign(n_keys, ~0ull);
  std::shared_lock<std::shared_mutex> kl(s->kmu);
  for (size_t i = 0; i < n_keys; ++i) {
    if (!keys[i]) return fail(EHX_EINVAL, "NULL argument");
    if (implicit_id(s, keys[i], klens[i], &(*ids)[i])) continue;
    auto it = s->key_to_id.find(std::string(keys[i], klens[i]));
    if (it != s->key_to_id.end()) (*ids)[i] = it->second;
  }
  return EHX_OK;
}

}  // namespace ehx_impl

// an unsharded space, locked shared, scratch_mu held, its device current, not poisoned, its rows within except_check_ld;
// everything is enqueued on `st`.  The lists are on the device and their offsets checked (except_check_off).  n_pub: the
// call's ONE read of the row count — except_locked's own, or the profile search's, whose targets were summed under it.
int ehx_impl::except_locked_at(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const float* d_queries, uint32_t k,
                               const uint64_t* d_excl_ids, const uint64_t* d_excl_off, const ResultBlock& out) {
  int rc;
  ehx_space::Except& w = s->except;
  s->except_ctr[4] += 1;
  const bool scans = s->params.mode != EHX_MODE_GRAPH && !s->x_perm && n_pub > 0 && i8_serves_radius(s, n_pub);
  // (a last device batch below the gate goes with the exact route's queries)
  const size_t tail = nq % kSideChunk;
  const size_t n_scan = !scans ? 0 : (tail && tail < kLargeKMinQueries ? nq - tail : nq);
  if (n_scan) {
    const size_t cap = std::min(kSideChunk, n_scan);
    if ((rc = w.dSorted.ensure(cap * kExceptMaxList)) || (rc = w.dSortedCnt.ensure(cap))) return rc;
    RadiusKnn c;
    c.passes = largek_passes(n_pub, env().largek_growth);
    const uint64_t stride = (n_pub + kLargeKSample - 1) / kLargeKSample;
    const uint32_t n_sample = (uint32_t)((n_pub + stride - 1) / stride);
    c.out = ResultBlock{out.ids, out.dist, out.cnt, nullptr, n_scan, k};
    // stage 0 of a device batch [q0, q0 + m): its lists sorted into the scratch, then the large-k route's strided sample
    c.fill_pool = [&](size_t q0, size_t m, uint64_t* pool, uint32_t* pool_cnt) -> int {
      HIP_TRY(launch_except_lists(d_excl_ids, d_excl_off + q0, (uint32_t)m, n_pub, w.dSorted.p, w.dSortedCnt.p, st));
      HIP_TRY(launch_radius_seed(pool, pool_cnt, (uint32_t)m, n_pub, stride, n_sample, st));
      return EHX_OK;
    };
    c.rerank = [&](const RadiusRerankArgs& r, hipStream_t on) {
      return launch_except_rerank(ExceptRerankArgs{r, w.dSorted.p, w.dSortedCnt.p, nullptr}, on);
    };
    // the flagged queries of a device batch, each with its own list: ONE sub-batch on the exact route (the gather's index
    // array, still on the device when the answer runs, names their lists)
    c.handed = [&](size_t, const std::vector<uint32_t>& todo, const float* q, const ResultBlock& o) -> int {
      return w.scan.sub.rerun(
          s, st, q, todo, k,
          [&](size_t n, const float* sq, uint64_t* i2, float* d2, uint32_t* c2) {
            return except_exact(s, st, n_pub, n, sq, k, nullptr, nullptr, w.scan.sub.dFbIdx.p, i2, d2, c2, false);
          },
          o.ids, o.dist, o.cnt);
    };
    test_pause();
    RadiusKnnTally t;
    const int r = radius_knn(s, st, w.scan, n_pub, d_queries, c, &t);
    for (uint64_t b = 0; b < t.batches; ++b)   // (the int8 scan copy: every query of a batch against every row once)
      count_scan_batch(s, (size_t)std::min<uint64_t>(kSideChunk, t.queries - b * kSideChunk), n_pub, k, 1);
    s->n_i8_queries += t.queries;
    s->n_i8_fallback += t.handed;
    s->n_exhaustive += t.handed;
    s->except_ctr[0] += t.queries - t.handed;
    s->except_ctr[1] += t.handed;
    s->except_ctr[2] += t.overflowed;
    s->except_ctr[3] += t.batches * c.passes.size();
    if (r) return r;
  }
  if (n_scan == nq) return EHX_OK;
  s->except_ctr[1] += nq - n_scan;
  return except_exact(s, st, n_pub, nq - n_scan, d_queries + n_scan * s->dims, k, d_excl_ids, d_excl_off + n_scan, nullptr,
                      out.ids + n_scan * k, out.dist + n_scan * k, out.cnt + n_scan, true);
}

namespace {

int except_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, const uint64_t* d_excl_ids,
                  const uint64_t* d_excl_off, const ResultBlock& out) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  if ((rc = except_check_ld(s))) return rc;   // (before anything is enqueued)
  const uint64_t n_pub = s->n.load(std::memory_order_acquire);   // the ONE read of the row count
  return except_locked_at(s, st, n_pub, nq, d_queries, k, d_excl_ids, d_excl_off, out);
}

// host pointers in, host pointers out, on the space's stream (on_device): ids | offsets staged in except.dLists
int except_host_locked(ehx_space* s, size_t nq, const float* queries, uint32_t k, const uint64_t* excl_ids,
                       const uint64_t* excl_off, size_t n_excl, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  ehx_space::Except& w = s->except;
  int rc;
  if ((rc = w.dLists.ensure(n_excl + nq + 1)) || (rc = w.host.up(s->stream, queries, nq, s->dims, k, false))) return rc;
  // (earlier calls' launches on other streams may still read the lists)
  if ((rc = wait_searches_in_flight(s, s->stream))) return rc;
  uint64_t* d_ids = w.dLists.p;
  uint64_t* d_off = d_ids + n_excl;
  // (pageable host memory: the runtime stages it before the call returns)
  if (n_excl) HIP_TRY(hipMemcpyAsync(d_ids, excl_ids, n_excl * sizeof(uint64_t), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(d_off, excl_off, (nq + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s->stream));
  if ((rc = except_locked(s, s->stream, nq, w.host.q, k, d_ids, d_off, w.host.out))) return rc;
  return w.host.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
}

}  // namespace

extern "C" {

int ehx_knn_except_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                          const uint64_t* d_excl_ids, const uint64_t* d_excl_off, size_t n_excl, uint64_t* d_out_ids,
                          float* d_out_dist, uint32_t* d_out_count) {
  if (int rc = except_check(s, n_queries, k,
                            d_out_ids && d_out_dist && d_out_count && (!n_queries || (d_queries && d_excl_off)) &&
                                (!n_excl || d_excl_ids)))
    return rc;
  if (int rc = ehx_init(nullptr, 0)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_knn_except_device", kExceptWhy, n_queries, &st, [&]() -> int {
    // the kernels trust the offsets: they are read back and checked before anything reads a list
    std::vector<uint64_t> off(n_queries + 1);
    HIP_TRY(hipMemcpyAsync(off.data(), d_excl_off, off.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (int rc = except_check_off(off.data(), n_queries, n_excl, "d_excl_off", "n_excl")) return rc;
    return except_locked(s, st, n_queries, d_queries, k, d_excl_ids, d_excl_off,
                         ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_knn_except(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const uint64_t* excl_ids,
                   const uint64_t* excl_off, size_t n_excl, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (int rc = except_check(s, n_queries, k,
                            out_ids && out_dist && out_count && (!n_queries || (queries && excl_off)) && (!n_excl || excl_ids)))
    return rc;
  if (n_queries)
    if (int rc = except_check_off(excl_off, n_queries, n_excl, "excl_off", "n_excl")) return rc;
  if (int rc = ehx_init(nullptr, 0)) return rc;
  return search_on_device(s, "ehx_knn_except", kExceptWhy, n_queries, nullptr, [&] {
    return except_host_locked(s, n_queries, queries, k, excl_ids, excl_off, n_excl, out_ids, out_dist, out_count);
  });
}

int ehx_knn_except_keys(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const char* const* keys,
                        const size_t* klens, const uint64_t* key_off, size_t n_keys, uint64_t* out_ids, float* out_dist,
                        uint32_t* out_count) {
  if (int rc = except_check(s, n_queries, k,
                            out_ids && out_dist && out_count && (!n_queries || (queries && key_off)) && (!n_keys || (keys && klens))))
    return rc;
  if (n_queries)
    if (int rc = except_check_off(key_off, n_queries, n_keys, "key_off", "n_keys")) return rc;
  if (int rc = ehx_init(nullptr, 0)) return rc;
  // ONE shared hold for key lookup and search: the answer describes one state of the space
  return search_shared(s, "ehx_knn_except_keys", kExceptWhy, [&]() -> int {
    std::vector<uint64_t> ids;
    if (int rc = except_key_ids(s, keys, klens, n_keys, &ids)) return rc;
    return on_device(s, n_queries, s->stream, [&] {
      return except_host_locked(s, n_queries, queries, k, ids.data(), key_off, n_keys, out_ids, out_dist, out_count);
    });
  });
}

}  // extern "C"
