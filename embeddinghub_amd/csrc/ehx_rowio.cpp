// Rows in and out without staging: ehx_set_batch_device (the rows of a Set read from device memory by scatter_rows_kernel,
// k_rowio.hip — the front only: the body is ehx_set_batch's, ehx_write.cpp), ehx_get_batch (MultiGet / Download: n keys, one
// gather, one copy) and ehx_get_by_ids_device (the gather alone, on the caller's stream).  The gather is the one that feeds
// ehx_knn_by_keys (gather_rows_kernel, k_bykey.hip): "the bytes ehx_get_by_id returns".
#include "ehx_internal.h"

namespace {

// rows d_row_ids[0, n) of the space (locked shared, scratch_mu held, the gathering device current) -> d_out [n][dims],
// d_valid [n], enqueued on `st`; wait: the stream is waited for before the shards' locks are released.  The ONE read of the
// row count is taken here.  by_ev orders the call behind the last one that used the by-key scratch (d_out may be it) and is
// what a writer that rewrites rows in place waits for (write_rows).
int gather_locked(ehx_space* s, hipStream_t st, size_t n, const uint64_t* d_row_ids, float* d_out, uint32_t* d_valid, bool wait) {
  int rc;
  if ((rc = s->by.by_ev.ensure(hipEventDisableTiming))) return rc;
  HIP_TRY(hipStreamWaitEvent(st, s->by.by_ev, 0));
  const uint64_t n_pub = s->n.load(std::memory_order_acquire);
  std::vector<std::shared_lock<std::shared_mutex>> held;   // a parent's shards, until the gather has read the rows
  GatherRowsArgs g = {};
  if (is_parent(s)) {
    if ((rc = parent_gather_view(s, n_pub, &held, &g))) return rc;
    wait = true;   // (a shard grows behind its own lock and drains its own device: the rows are read before the locks go)
  } else {
    if ((rc = check_not_poisoned(s))) return rc;
    g.rows = rows_view(s, n_pub);
    g.bases.p[0] = g.rows.X;
    g.G = 1;
  }
  g.row_ids = d_row_ids;
  g.out = d_out;
  g.valid = d_valid;
  g.n = (uint32_t)n;
  HIP_TRY(launch_gather_rows(g, st));
  HIP_TRY(hipEventRecord(s->by.by_ev, st));
  if (wait) HIP_TRY(hipStreamSynchronize(st));
  return EHX_OK;
}

}  // namespace

extern "C" {

int ehx_set_batch_device(ehx_space* s, void* stream, size_t n, const char* const* keys, const size_t* klens,
                         const void* d_vecs, int src_dtype) {
  int rc = ehx_init(nullptr, 0);   // (no device: EHX_ENODEVICE, whatever else is wrong with the call)
  if (rc) return rc;
  if (!valid_space(s)) return fail(EHX_EINVAL, "space is NULL");
  if (n == 0) return EHX_OK;
  if (!keys || !klens || !d_vecs) return fail(EHX_EINVAL, "NULL argument");
  if (src_dtype != EHX_DTYPE_F32 && src_dtype != EHX_DTYPE_F16)
    return fail(EHX_EINVAL, "src_dtype %d is neither EHX_DTYPE_F32 nor EHX_DTYPE_F16", src_dtype);
  // where the rows are, before anything is enqueued
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, d_vecs) != hipSuccess || at.type != hipMemoryTypeDevice) {
    (void)hipGetLastError();
    return fail(EHX_EINVAL, "d_vecs is not device memory");
  }
  if (is_parent(s)) {
    const std::vector<int>& devs = engine().devices;
    if (std::find(devs.begin(), devs.end(), at.device) == devs.end())
      return fail(EHX_EINVAL, "d_vecs is on device %d, which is not one of ehx_init's", at.device);
  } else if (!s->keyless && at.device != s->device) {   // (a shard's handle is refused below, whatever it was given)
    return fail(EHX_EINVAL, "d_vecs is on device %d, space '%s' on device %d", at.device, s->name.c_str(), s->device);
  }
  RowSource src;
  src.dev = d_vecs;
  src.dtype = src_dtype;
  src.device = at.device;
  // "the rows are complete": recorded on the producer's stream, waited for by the writers' — the producer's is never drained
  Event ready;
  HIP_TRY(hipSetDevice(at.device));
  if ((rc = ready.ensure(hipEventDisableTiming))) return rc;
  HIP_TRY(hipEventRecord(ready, (hipStream_t)stream));
  src.ready = ready;
  return set_batch_from(s, n, keys, klens, src);   // (returns after the rows are published: nothing waits for `ready` any more)
}

int ehx_get_batch(ehx_space* s, size_t n, const char* const* keys, const size_t* klens, float* out_vecs, size_t* bad_index) {
  int rc = ehx_init(nullptr, 0);
  if (rc) return rc;
  if (!valid_space(s)) return fail(EHX_EINVAL, "space is NULL");
  if (n == 0) return EHX_OK;
  if (!keys || !klens || !out_vecs) return fail(EHX_EINVAL, "NULL argument");
  if ((rc = check_batch_size(n))) return rc;
  yield_to_writer(s);
  // ONE shared hold for key lookup and gather: the rows describe one state of the space
  std::shared_lock<std::shared_mutex> rl(s->mu);
  if (s->dropped) return fail(EHX_ENOTFOUND, "Not found");
  std::vector<uint64_t> ids;
  if ((rc = lookup_keys(s, n, keys, klens, &ids, bad_index))) return rc;
  ehx_space* home = is_parent(s) ? s->shards[0] : s;
  std::lock_guard<std::mutex> sl(s->scratch_mu);
  HIP_TRY(hipSetDevice(home->device));
  const size_t row_elems = (size_t)n * s->dims;
  if ((rc = s->by.dByQ.ensure(row_elems)) || (rc = s->by.dByIds.ensure(n)) || (rc = s->by.dByOut.ensure(n * sizeof(uint32_t))))
    return rc;
  DrainUnlessOk drain{s->stream};
  // (pageable host memory: the runtime stages it before the call returns)
  HIP_TRY(hipMemcpyAsync(s->by.dByIds.p, ids.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, s->stream));
  if ((rc = gather_locked(s, s->stream, n, s->by.dByIds.p, s->by.dByQ.p, (uint32_t*)s->by.dByOut.p, false))) return rc;
  HIP_TRY(hipMemcpyAsync(out_vecs, s->by.dByQ.p, row_elems * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return drain.done(EHX_OK);
}

int ehx_get_by_ids_device(ehx_space* s, void* stream, size_t n, const uint64_t* d_row_ids, float* d_out, uint32_t* d_valid) {
  int rc = ehx_init(nullptr, 0);
  if (rc) return rc;
  if (!valid_space(s)) return fail(EHX_EINVAL, "space is NULL");
  if (n == 0) return EHX_OK;
  if (!d_row_ids || !d_out || !d_valid) return fail(EHX_EINVAL, "NULL device pointer");
  if ((rc = check_batch_size(n))) return rc;
  yield_to_writer(s);
  std::shared_lock<std::shared_mutex> rl(s->mu);
  if (s->dropped) return fail(EHX_ENOTFOUND, "Not found");
  ehx_space* home = is_parent(s) ? s->shards[0] : s;
  std::lock_guard<std::mutex> sl(s->scratch_mu);   // (by_ev)
  HIP_TRY(hipSetDevice(home->device));
  DrainUnlessOk drain{(hipStream_t)stream};
  return drain.done(gather_locked(s, (hipStream_t)stream, n, d_row_ids, d_out, d_valid, false));
}

}  // extern "C"
