// Nearest-centroid assignment, centroid sums and k-means over the rows a space holds: ehx_assign_device,
// ehx_centroid_sums_device, ehx_kmeans_device.  include/ehx.h has the contract, k_assign.hip the assignment's kernels,
// k_profile.hip the sums' (combine_rows_kernel's sorted form), DESIGN.md §e.33 the certificate.
//   assign   the centroids prepared like queries, padded to whole tiles of the filter; their |c|^2 and the finiteness flag; the
//            matrix-core filter over the range (plain rows whose stride fits its LDS), which writes the rows it certifies and
//            lists the rest; the call's ONE wait, for the list's length; the exact kernel over the list — or over every row
//            where the filter may not run.
//   sums     the range's positions ordered by label with two of the column index's stable 8-bit passes (labels that name no
//            centroid share the key n_centroids <= 4096), then one workgroup per (centroid, slab of components) sums its run
//            in the profile search's strands.  Unbalanced on skewed clusterings: a known cost.
//   kmeans   iters x (assign, sums, divide) and a last assignment, all under ONE snapshot of the row count; the rows the last
//            assignment moved are counted against a copy of the labels from before it.
// Everything is enqueued on the caller's stream under one shared hold of the space's lock (search_on_device).
#include "ehx_internal.h"

namespace {

constexpr const char* kAssignWhy = "assignment over shards is not built yet";

static_assert(EHX_ASSIGN_MAX_CENTROIDS == kAssignMaxCentroids, "the header's limit is the kernels'");
static_assert(EHX_ASSIGN_MAX_CENTROIDS <= 0xFFFFu, "the sums' sort orders by two 8-bit digits");

// what is decided before the device is looked for (s is not read)
int assign_check(const ehx_space* s, uint32_t n_centroids, bool ptrs_ok) {
  if (!s) return fail(EHX_EINVAL, "space is NULL");
  if (n_centroids == 0 || n_centroids > EHX_ASSIGN_MAX_CENTROIDS)
    return fail(EHX_EINVAL, "n_centroids=%u is not in [1, %u]", n_centroids, EHX_ASSIGN_MAX_CENTROIDS);
  if (!ptrs_ok) return fail(EHX_EINVAL, "NULL argument");
  return ehx_init(nullptr, 0);
}

// ... and with the space locked: the call's ONE read of the row count, and the range against it
int assign_open(ehx_space* s, uint64_t row0, uint64_t n_rows, uint64_t* n_pub) {
  if (int rc = check_not_poisoned(s)) return rc;
  *n_pub = s->n.load(std::memory_order_acquire);
  if (row0 > *n_pub || n_rows > *n_pub - row0)
    return fail(EHX_EINVAL, "rows [%llu, %llu + %llu) do not lie inside the %llu rows of the space", (unsigned long long)row0,
                (unsigned long long)row0, (unsigned long long)n_rows, (unsigned long long)*n_pub);
  if (n_rows > 0xFFFFFFFFull) return fail(EHX_EUNSUPPORTED, "n_rows=%llu exceeds 2^32 - 1", (unsigned long long)n_rows);
  if (s->ld > assign_exact_max_ld())
    return fail(EHX_EUNSUPPORTED, "assignment keeps a block of prepared centroids in LDS: rows of %u floats exceed %u", s->ld,
                assign_exact_max_ld());
  return EHX_OK;
}

// a call's launches sit between a wait for and a record of by.by_ev, as the profile search's
template <class Body>
int between_by_events(ehx_space* s, hipStream_t st, Body&& body) {
  if (int rc = s->by.by_ev.ensure(hipEventDisableTiming)) return rc;
  HIP_TRY(hipStreamWaitEvent(st, s->by.by_ev, 0));
  const int rc = body();
  (void)hipEventRecord(s->by.by_ev, st);
  return rc;
}

// All three below: an unsharded space, locked shared, scratch_mu held, its device current, the range inside n_pub, n > 0.
int assign_enqueue(ehx_space* s, hipStream_t st, uint64_t n_pub, uint64_t row0, uint32_t n, const float* d_centroids, uint32_t C,
                   uint32_t* d_label, float* d_dist) {
  ehx_space::Assign& w = s->assign;
  const uint32_t c_rows = (C + kAssignTileC - 1) / kAssignTileC * kAssignTileC;
  int rc;
  if ((rc = w.dQ.ensure((size_t)c_rows * s->ld)) || (rc = w.dCn2.ensure(c_rows)) || (rc = w.dList.ensure(n)) ||
      (rc = w.dCtl.ensure_zeroed_once(4)) || (rc = w.hCtl.ensure(4)))
    return rc;
  HIP_TRY(hipMemsetAsync(w.dCtl.p, 0, 3 * sizeof(uint32_t), st));
  HIP_TRY(launch_prep_queries(d_centroids, C, s->dims, s->ld, c_rows, s->metric, w.dQ.p, st));
  HIP_TRY(launch_centroid_stats(w.dQ.p, c_rows, C, s->ld, w.dCn2.p, w.dCtl.p + 2, st));
  AssignArgs a = {};
  a.rows = rows_view(s, n_pub);
  a.cent = w.dQ.p;
  a.cn2 = w.dCn2.p;
  a.bad = w.dCtl.p + 2;
  a.row0 = row0;
  a.n_rows = n;
  a.n_cent = C;
  a.label = d_label;
  a.dist = d_dist;
  a.list = w.dList.p;
  a.ctl = w.dCtl.p;
  const int n_cus = engine().n_cus;
  if (s->x_perm || s->ld > assign_max_ld()) {   // the filter may not run: every row is the exact kernel's
    HIP_TRY(launch_assign_exact(a, n, false, n_cus, st));
    s->assign_ctr[1].fetch_add(n, std::memory_order_relaxed);
    return EHX_OK;
  }
  HIP_TRY(launch_assign_filter(a, st));
  HIP_TRY(hipMemcpyAsync(w.hCtl.p, w.dCtl.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));   // the call's one wait: how many rows the filter handed on
  const uint32_t handed = w.hCtl.p[0], certified = w.hCtl.p[1];
  if (handed > n || certified != n - handed)
    return fail(EHX_EINTERNAL, "assignment: %u rows certified and %u handed on of %u", certified, handed, n);
  HIP_TRY(launch_assign_exact(a, handed, true, n_cus, st));
  s->assign_ctr[0].fetch_add(certified, std::memory_order_relaxed);
  s->assign_ctr[1].fetch_add(handed, std::memory_order_relaxed);
  return EHX_OK;
}

int sums_enqueue(ehx_space* s, hipStream_t st, uint64_t n_pub, uint64_t row0, uint32_t n, const uint32_t* d_label, uint32_t C,
                 float* d_sums, uint32_t* d_count) {
  ehx_space::Assign& w = s->assign;
  const uint32_t blocks = colindex_blocks(n);
  int rc;
  if ((rc = w.dKey[0].ensure(n)) || (rc = w.dKey[1].ensure(n)) || (rc = w.dVal[0].ensure(n)) || (rc = w.dVal[1].ensure(n)) ||
      (rc = w.dHist.ensure(256 * (size_t)blocks + 1024)))
    return rc;
  uint32_t* d_ghist = w.dHist.p + 256 * (size_t)blocks;
  HIP_TRY(launch_label_keys(d_label, n, C, w.dKey[0].p, st));
  HIP_TRY(launch_colindex_digits(w.dKey[0].p, n, d_ghist, st));
  HIP_TRY(launch_colindex_pass(w.dKey[0].p, nullptr, w.dKey[1].p, w.dVal[1].p, n, 0, d_ghist, w.dHist.p, st));
  HIP_TRY(launch_colindex_pass(w.dKey[1].p, w.dVal[1].p, w.dKey[0].p, w.dVal[0].p, n, 1, d_ghist, w.dHist.p, st));
  CombineRowsArgs c = {};
  c.rows = rows_view(s, n_pub);
  c.out = d_sums;
  c.nq = C;
  c.sorted_key = w.dKey[0].p;
  c.sorted_pos = w.dVal[0].p;
  c.row0 = row0;
  c.n_sorted = n;
  c.count = d_count;
  HIP_TRY(launch_combine_rows(c, engine().n_cus, st));
  return EHX_OK;
}

int kmeans_enqueue(ehx_space* s, hipStream_t st, uint64_t n_pub, uint64_t row0, uint32_t n, uint32_t C, uint32_t iters,
                   float* d_centroids, uint32_t* d_label, float* d_dist, uint32_t* out_moved) {
  ehx_space::Assign& w = s->assign;
  int rc;
  if ((rc = w.dSums.ensure((size_t)C * s->dims)) || (rc = w.dCount.ensure(C)) || (rc = w.dPrev.ensure(n))) return rc;
  for (uint32_t it = 0; it < iters; ++it) {
    if ((rc = assign_enqueue(s, st, n_pub, row0, n, d_centroids, C, d_label, nullptr))) return rc;
    if ((rc = sums_enqueue(s, st, n_pub, row0, n, d_label, C, w.dSums.p, w.dCount.p))) return rc;
    HIP_TRY(launch_lloyd_divide(w.dSums.p, w.dCount.p, C, s->dims, d_centroids, st));
  }
  if (out_moved) HIP_TRY(hipMemcpyAsync(w.dPrev.p, d_label, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  if ((rc = assign_enqueue(s, st, n_pub, row0, n, d_centroids, C, d_label, d_dist))) return rc;
  if (out_moved) {
    HIP_TRY(hipMemsetAsync(w.dCtl.p + 3, 0, sizeof(uint32_t), st));
    HIP_TRY(launch_count_moved(w.dPrev.p, d_label, n, w.dCtl.p + 3, st));
    HIP_TRY(hipMemcpyAsync(w.hCtl.p + 3, w.dCtl.p + 3, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *out_moved = w.hCtl.p[3];
  }
  return EHX_OK;
}

}  // namespace

extern "C" {

int ehx_assign_device(ehx_space* s, void* stream, uint64_t row0, uint64_t n_rows, const float* d_centroids, uint32_t n_centroids,
                      uint32_t* d_out_label, float* d_out_dist) {
  if (int rc = assign_check(s, n_centroids, d_centroids && (!n_rows || d_out_label))) return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_assign_device", kAssignWhy, 1, &st, [&]() -> int {
    uint64_t n_pub;
    if (int rc = assign_open(s, row0, n_rows, &n_pub)) return rc;
    if (n_rows == 0) return EHX_OK;
    return between_by_events(s, st, [&] {
      return assign_enqueue(s, st, n_pub, row0, (uint32_t)n_rows, d_centroids, n_centroids, d_out_label, d_out_dist);
    });
  });
}

int ehx_centroid_sums_device(ehx_space* s, void* stream, uint64_t row0, uint64_t n_rows, const uint32_t* d_label,
                             uint32_t n_centroids, float* d_out_sums, uint32_t* d_out_count) {
  if (int rc = assign_check(s, n_centroids, d_out_sums && d_out_count && (!n_rows || d_label))) return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_centroid_sums_device", kAssignWhy, 1, &st, [&]() -> int {
    uint64_t n_pub;
    if (int rc = assign_open(s, row0, n_rows, &n_pub)) return rc;
    if (n_rows == 0) return EHX_OK;
    return between_by_events(s, st, [&] {
      return sums_enqueue(s, st, n_pub, row0, (uint32_t)n_rows, d_label, n_centroids, d_out_sums, d_out_count);
    });
  });
}

int ehx_kmeans_device(ehx_space* s, void* stream, uint64_t row0, uint64_t n_rows, uint32_t n_centroids, uint32_t iters,
                      float* d_centroids, uint32_t* d_out_label, float* d_out_dist, uint32_t* out_moved) {
  if (int rc = assign_check(s, n_centroids, d_centroids && (!n_rows || d_out_label))) return rc;
  const hipStream_t st = (hipStream_t)stream;
  return search_on_device(s, "ehx_kmeans_device", kAssignWhy, 1, &st, [&]() -> int {
    uint64_t n_pub;
    if (int rc = assign_open(s, row0, n_rows, &n_pub)) return rc;
    if (n_rows == 0) return EHX_OK;
    return between_by_events(s, st, [&] {
      return kmeans_enqueue(s, st, n_pub, row0, (uint32_t)n_rows, n_centroids, iters, d_centroids, d_out_label, d_out_dist,
                            out_moved);
    });
  });
}

}  // extern "C"
