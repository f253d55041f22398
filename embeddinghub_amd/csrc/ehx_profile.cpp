// Profile search: the query is a weighted sum of rows the space already holds, and the same list is the query's exclusion
// list — "items near what this user liked, weighted by recency, minus what they disliked, and none of the items already in
// their history".  ehx_combine_rows_device sums the targets alone (combine_rows_kernel, k_profile.hip: include/ehx.h has the
// byte-exact definition); ehx_knn_profile_device sums them into the space's scratch and hands them, with the same lists, to
// the except route (except_locked_at, ehx_except.cpp) under ONE read of the row count, then blanks the queries whose list
// names no row; ehx_knn_profile takes host pointers, ehx_knn_profile_keys the lists as stored keys.  Nothing here scores a
// row: every distance, route and counter is the except search's.
#include "ehx_internal.h"

namespace {

constexpr const char* kProfileWhy = "profile search over shards is not built yet";

static_assert(EHX_PROFILE_MAX_LIST == kProfileMaxList, "the header's limit is the kernel's LDS list");
static_assert(EHX_PROFILE_MAX_LIST == EHX_EXCEPT_MAX_LIST, "a profile's list is its exclusion list");

// the offsets of a call, host memory: non-decreasing, ending at n_entries, no list longer than the kernel's
int profile_check_off(const uint64_t* off, size_t nq, size_t n_entries, const char* name, const char* n_name) {
  for (size_t i = 0; i < nq; ++i) {
    if (off[i] > off[i + 1]) return fail(EHX_EINVAL, "%s is not non-decreasing at query %zu", name, i);
    if (off[i + 1] - off[i] > EHX_PROFILE_MAX_LIST)
      return fail(EHX_EINVAL, "query %zu combines %llu entries, more than EHX_PROFILE_MAX_LIST = %u", i,
                  (unsigned long long)(off[i + 1] - off[i]), EHX_PROFILE_MAX_LIST);
  }
  if (off[nq] != n_entries)
    return fail(EHX_EINVAL, "%s ends at %llu, not at %s = %zu", name, (unsigned long long)off[nq], n_name, n_entries);
  return EHX_OK;
}

// a device form's offsets: read back and checked before any kernel trusts them
int profile_read_off(hipStream_t st, const uint64_t* d_off, size_t nq, size_t n_entries) {
  std::vector<uint64_t> off(nq + 1);
  HIP_TRY(hipMemcpyAsync(off.data(), d_off, off.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return profile_check_off(off.data(), nq, n_entries, "d_off", "n_entries");
}

// Both bodies below: an unsharded space, locked shared, scratch_mu held, its device current, the lists on the device and
// their offsets checked; everything is enqueued on `st`.  A call's launches sit between a wait for and a record of by.by_ev.
template <class Body>
int between_by_events(ehx_space* s, hipStream_t st, Body&& body) {
  if (int rc = s->by.by_ev.ensure(hipEventDisableTiming)) return rc;
  HIP_TRY(hipStreamWaitEvent(st, s->by.by_ev, 0));
  const int rc = body();
  (void)hipEventRecord(s->by.by_ev, st);
  return rc;
}

int combine_enqueue(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const uint64_t* d_ids, const uint64_t* d_off,
                    const float* d_weights, float* d_out, uint32_t* d_valid) {
  CombineRowsArgs a = {};
  a.ids = d_ids;
  a.off = d_off;
  a.weights = d_weights;
  a.rows = rows_view(s, n_pub);
  a.out = d_out;
  a.valid = d_valid;
  a.nq = (uint32_t)nq;
  HIP_TRY(launch_combine_rows(a, engine().n_cus, st));
  return EHX_OK;
}

int combine_locked(ehx_space* s, hipStream_t st, size_t nq, const uint64_t* d_ids, const uint64_t* d_off, const float* d_weights,
                   float* d_out, uint32_t* d_valid) {
  if (int rc = check_not_poisoned(s)) return rc;
  return between_by_events(s, st, [&] {
    const uint64_t n_pub = s->n.load(std::memory_order_acquire);   // the ONE read of the row count
    return combine_enqueue(s, st, n_pub, nq, d_ids, d_off, d_weights, d_out, d_valid);
  });
}

int profile_locked(ehx_space* s, hipStream_t st, size_t nq, const uint64_t* d_ids, const uint64_t* d_off, const float* d_weights,
                   uint32_t k, const ResultBlock& out) {
  int rc;
  if ((rc = check_not_poisoned(s)) || (rc = except_check_ld(s))) return rc;   // (before anything is enqueued)
  ehx_space::Profile& w = s->profile;
  if ((rc = w.dTarget.ensure(nq * s->dims)) || (rc = w.dValid.ensure(nq))) return rc;
  return between_by_events(s, st, [&]() -> int {
    // the ONE read of the row count: the targets are summed over, and the search answers for, the same prefix
    const uint64_t n_pub = s->n.load(std::memory_order_acquire);
    if (int r = combine_enqueue(s, st, n_pub, nq, d_ids, d_off, d_weights, w.dTarget.p, w.dValid.p)) return r;
    if (int r = except_locked_at(s, st, n_pub, nq, w.dTarget.p, k, d_ids, d_off, out)) return r;
    HIP_TRY(launch_blank_invalid(w.dValid.p, (uint32_t)nq, k, out.ids, out.dist, out.cnt, st));
    return EHX_OK;
  });
}

// host pointers in, host pointers out, on the space's stream (on_device): ids | offsets, weights and results staged in
// ehx_space::Profile, as except_host_locked stages its lists
int profile_host_locked(ehx_space* s, size_t nq, const uint64_t* ids, const uint64_t* off, const float* weights, size_t n_entries,
                        uint32_t k, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  ehx_space::Profile& w = s->profile;
  int rc;
  if ((rc = w.dLists.ensure(n_entries + nq + 1)) || (rc = w.dWeights.ensure(weights ? n_entries : 0)) ||
      (rc = w.dOut.ensure(ResultBlock::bytes(nq, k, false))) || (rc = s->by.by_ev.ensure(hipEventDisableTiming)))
    return rc;
  // (an earlier call's launches, on whatever stream it was given, may still read the staged lists)
  HIP_TRY(hipStreamWaitEvent(s->stream, s->by.by_ev, 0));
  uint64_t* d_ids = w.dLists.p;
  uint64_t* d_off = d_ids + n_entries;
  const bool has_w = weights && n_entries;
  // (pageable host memory: the runtime stages it before the call returns)
  if (n_entries) HIP_TRY(hipMemcpyAsync(d_ids, ids, n_entries * sizeof(uint64_t), hipMemcpyHostToDevice, s->stream));
  if (has_w) HIP_TRY(hipMemcpyAsync(w.dWeights.p, weights, n_entries * sizeof(float), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(d_off, off, (nq + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s->stream));
  const ResultBlock o = ResultBlock::at(w.dOut.p, nq, k, false);
  if ((rc = profile_locked(s, s->stream, nq, d_ids, d_off, has_w ? w.dWeights.p : nullptr, k, o))) return rc;
  return o.copy_out(s->stream, out_ids, out_dist, out_count, nullptr);
}

}  // namespace

extern "C" {

int ehx_combine_rows_device(ehx_space* s, void* stream, size_t n_queries, const uint64_t* d_ids, const uint64_t* d_off,
                            const float* d_weights, size_t n_entries, float* d_out, uint32_t* d_valid) {
  if (!s) return fail(EHX_EINVAL, "space is NULL");
  if (!(d_out && d_valid && (!n_queries || d_off) && (!n_entries || d_ids))) return fail(EHX_EINVAL, "NULL argument");
  if (int rc = check_batch_size(n_queries)) return rc;
  if (int rc = ehx_init(nullptr, 0)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_combine_rows_device", kProfileWhy, n_queries, &st, [&]() -> int {
    if (int rc = profile_read_off(st, d_off, n_queries, n_entries)) return rc;
    return combine_locked(s, st, n_queries, d_ids, d_off, d_weights, d_out, d_valid);
  });
}

int ehx_knn_profile_device(ehx_space* s, void* stream, size_t n_queries, const uint64_t* d_ids, const uint64_t* d_off,
                           const float* d_weights, size_t n_entries, uint32_t k, uint64_t* d_out_ids, float* d_out_dist,
                           uint32_t* d_out_count) {
  if (int rc = except_check(s, n_queries, k, d_out_ids && d_out_dist && d_out_count && (!n_queries || d_off) && (!n_entries || d_ids)))
    return rc;
  if (int rc = ehx_init(nullptr, 0)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_knn_profile_device", kProfileWhy, n_queries, &st, [&]() -> int {
    if (int rc = profile_read_off(st, d_off, n_queries, n_entries)) return rc;
    return profile_locked(s, st, n_queries, d_ids, d_off, d_weights, k,
                          ResultBlock{d_out_ids, d_out_dist, d_out_count, nullptr, n_queries, k});
  });
}

int ehx_knn_profile(ehx_space* s, size_t n_queries, const uint64_t* ids, const uint64_t* off, const float* weights,
                    size_t n_entries, uint32_t k, uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (int rc = except_check(s, n_queries, k, out_ids && out_dist && out_count && (!n_queries || off) && (!n_entries || ids))) return rc;
  if (n_queries)
    if (int rc = profile_check_off(off, n_queries, n_entries, "off", "n_entries")) return rc;
  if (int rc = ehx_init(nullptr, 0)) return rc;
  return search_on_device(s, "ehx_knn_profile", kProfileWhy, n_queries, nullptr, [&] {
    return profile_host_locked(s, n_queries, ids, off, weights, n_entries, k, out_ids, out_dist, out_count);
  });
}

int ehx_knn_profile_keys(ehx_space* s, size_t n_queries, const char* const* keys, const size_t* klens, const uint64_t* key_off,
                         const float* weights, size_t n_keys, uint32_t k, uint64_t* out_ids, float* out_dist,
                         uint32_t* out_count) {
  if (int rc = except_check(s, n_queries, k,
                            out_ids && out_dist && out_count && (!n_queries || key_off) && (!n_keys || (keys && klens))))
    return rc;
  if (n_queries)
    if (int rc = profile_check_off(key_off, n_queries, n_keys, "key_off", "n_keys")) return rc;
  if (int rc = ehx_init(nullptr, 0)) return rc;
  // ONE shared hold for key lookup and search: the answer describes one state of the space
  return search_shared(s, "ehx_knn_profile_keys", kProfileWhy, [&]() -> int {
    // (a key that is not stored names no row: an id no prefix holds — it keeps its place in the list, so the strands of the
    // entries behind it do not move, and contributes and excludes nothing)
    std::vector<uint64_t> ids(n_keys, ~0ull);
    {
      std::shared_lock<std::shared_mutex> kl(s->kmu);
      for (size_t i = 0; i < n_keys; ++i) {
        if (!keys[i]) return fail(EHX_EINVAL, "NULL argument");
        if (implicit_id(s, keys[i], klens[i], &ids[i])) continue;
        auto it = s->key_to_id.find(std::string(keys[i], klens[i]));
        if (it != s->key_to_id.end()) ids[i] = it->second;
      }
    }
    return on_device(s, n_queries, s->stream, [&] {
      return profile_host_locked(s, n_queries, ids.data(), key_off, weights, n_keys, k, out_ids, out_dist, out_count);
    });
  });
}

}  // extern "C"
