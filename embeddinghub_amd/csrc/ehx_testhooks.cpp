// Test hooks of the int8 filter scan (not in include/ehx.h, like ehx_test_range_counters and ehx_test_live_resources):
//   ehx_test_i8_array   a slice of one array of the int8 scan copy, raw, as the writers left it
//   ehx_test_i8_pass    ONE launch of flat_scan_i8_kernel over a window of tiles with the arguments a search would give
//                       it: the sample form (every lower bound of the window) or a collect pass under the caller's
//                       thresholds (the pools as the pass left them, before select256 and the re-rank reduce them)
// tests/test_i8_device_bound.py checks the scan copy, the bound and the hit path on them.
//   ehx_test_i8_balance_force / ehx_test_i8_balance_read   the share planner of the flat chain's long passes: forced factors,
//                       and the bounds, stamps and factors of the last batch (tests/test_i8_balance.py)
// ... and of the fp16 filter scan and the fp32 scan, which share the candidate-list path (k_scan_common.h):
//   ehx_test_f16_array  a slice of one array of the fp16 scan copy, raw
//   ehx_test_f16_pass   ONE launch of flat_scan16_kernel: the sample form (the dump, and what sample_select makes of it) or a
//                       collect pass under the caller's 64-bit threshold keys (the lists as the pass published them, then
//                       flat_merge_kernel's view of them)
//   ehx_test_f32_pass   the collect form for flat_scan8_kernel
// tests/test_f16_device_bound.py checks them.
// ... and of the large-k scan route (ehx_largek.cpp):
//   ehx_test_largek_counters   what the route did so far on a space
//   ehx_test_largek_plan       the route's pass planner, host arithmetic only (no device, no space)
// ... and of the Set from device memory (ehx_rowio.cpp, ehx_write.cpp):
//   ehx_test_last_writers      the duplicate rule of its scatter, host arithmetic only (no device, no space)
//   ehx_test_write_batch       what a batch of row ids touches (WriteBatch), host arithmetic only (no device, no space)
//   ehx_test_write_times       device time of the last write's upload (or scatter) and of its derived copies (scripts/bench_rowio.py)
//   ehx_test_shard             the handle of one shard of a row-sharded space (what a caller that kept one would hold)
// ... and of the filtered searches (ehx_masked.cpp, k_masked.hip):
//   ehx_test_filter_routes     the routing rule (filter_routes_cut, then _gate), host arithmetic only (no device, no space)
//   ehx_test_rows_prefix       launch_rows_prefix on host arrays (a device, no space)
// No production path calls in here.
#include "ehx_internal.h"

namespace {

enum { kArrX8, kArrRowp8, kArrTilep8, kArrTileg8, kArrPerm8, kArrUnsafe8, kArrLd8, kArrCap };
constexpr uint32_t kSampleTiles = 8;   // the sample pass's window (flat_pass8)

int hook_space(ehx_space* s, const char* what, int need = 8) {
  int rc = ehx_init(nullptr, 0);
  if (rc) return rc;
  if (!valid_space(s)) return fail(EHX_EINVAL, "space is NULL");
  if (s->dropped) return fail(EHX_ENOTFOUND, "Not found");
  if (is_parent(s)) return fail(EHX_EUNSUPPORTED, "%s: space '%s' is row-sharded", what, s->name.c_str());
  if (need == 8 && !s->has8) return fail(EHX_EUNSUPPORTED, "%s: space '%s' keeps no int8 scan copy", what, s->name.c_str());
  if (need == 16 && !s->has16) return fail(EHX_EUNSUPPORTED, "%s: space '%s' keeps no fp16 scan copy", what, s->name.c_str());
  return EHX_OK;
}

template <class T>
int copy_slice(ehx_space* s, const ehx_impl::DevBuf<T>& b, uint64_t off, uint64_t n, void* out, hipStream_t st) {
  if (off > b.n || n > b.n - off) return fail(EHX_EINVAL, "slice [%llu, +%llu) of an array of %llu elements",
                                              (unsigned long long)off, (unsigned long long)n, (unsigned long long)b.n);
  if (n == 0) return EHX_OK;
  HIP_TRY(hipMemcpyAsync(out, b.p + off, n * sizeof(T), hipMemcpyDeviceToHost, st));
  return sync_stream(s, st);
}

enum { kArrX16, kArrRowp16, kArrUnsafe16, kArrLd16, kArrCap16 };

// ONE launch of flat_scan16_kernel (F16) or flat_scan8_kernel over tiles [tile0, +n_tiles), arguments as flat_pass fills them,
// on scratch of this call alone.  keys == NULL (F16 only): the sample form.
template <bool F16>
int list_pass(ehx_space* s, const char* what, uint32_t nq, const float* queries, uint32_t kprime, const uint64_t* keys,
              uint32_t tile0, uint32_t n_tiles, float* out_dump, uint64_t* out_gthr, uint64_t* out_part, uint32_t* out_err,
              uint64_t* out_merged, uint16_t* out_q16, float* out_qgamma, float* out_quv, uint32_t* out_info) {
  int rc = hook_space(s, what, F16 ? 16 : 0);
  if (rc) return rc;
  if (s->params.mode != EHX_MODE_FLAT) return fail(EHX_EUNSUPPORTED, "%s: space '%s' is not a flat space", what, s->name.c_str());
  if (!queries || !out_gthr || !out_info) return fail(EHX_EINVAL, "NULL argument");
  if (F16 && (!out_q16 || !out_qgamma || !out_quv)) return fail(EHX_EINVAL, "NULL argument");
  if (keys ? (!out_part || !out_err || !out_merged) : !out_dump) return fail(EHX_EINVAL, "NULL argument");
  if (nq == 0 || nq > 4 * kTileQ) return fail(EHX_EINVAL, "nq=%u outside [1, %u]", nq, 4 * kTileQ);
  if (kprime == 0 || kprime > 56) return fail(EHX_EINVAL, "k'=%u outside [1, 56]", kprime);
  if (!keys && n_tiles != kSampleTiles) return fail(EHX_EINVAL, "the sample form scans %u tiles", kSampleTiles);
  constexpr uint32_t tile_rows = F16 ? kTileRows16 : kTileRows;
  yield_to_writer(s);
  std::shared_lock<std::shared_mutex> rl(s->mu);
  if (s->dropped) return fail(EHX_ENOTFOUND, "Not found");
  // (the window may reach beyond the published rows, never beyond the arrays: the scan reads whole tiles)
  if (n_tiles == 0 || (uint64_t)tile0 + n_tiles > s->cap / tile_rows)
    return fail(EHX_EINVAL, "tiles [%u, +%u) of a space of %llu", tile0, n_tiles, (unsigned long long)(s->cap / tile_rows));
  std::lock_guard<std::mutex> sl(s->scratch_mu);
  HIP_TRY(hipSetDevice(s->device));
  Engine& E = engine();
  const hipStream_t st = s->stream;
  const uint64_t n_pub = s->n.load(std::memory_order_acquire);
  ScanPlan p = plan_scan(nq, n_tiles, 1, E.n_cus);
  p.kprime = kprime;
  constexpr uint32_t lpc = kScanListsPerChunk;
  const uint32_t lists_total = p.n_chunks * lpc;
  // scratch of this call alone (owners: freed on every return)
  DevBuf<float> dQraw, dQ, dQgamma, dDump;
  DevBuf<__half> dQ16;
  DevBuf<float2> dQuv;
  DevBuf<uint64_t> dCand, dPart, dMerged, dGthr;
  DevBuf<uint32_t> dErr;
  const size_t q16_halves = F16 ? scanq16_halves(p.q_rows, s->ld16) : 0;
  const size_t dump_elems = (size_t)kSampleTiles * kTileRows16 * p.q_rows;
  const size_t part_elems = (size_t)p.q_rows * lists_total * kprime;
  if ((rc = dQraw.ensure((size_t)nq * s->dims)) || (rc = dCand.ensure((size_t)p.grid * 512 * kCandSlots)) ||
      (rc = dPart.ensure(part_elems)) || (rc = dMerged.ensure((size_t)p.q_rows * 64)) ||
      (rc = dGthr.ensure((size_t)p.q_rows + 8)) || (rc = dErr.ensure(1)))
    return rc;
  if (F16 ? ((rc = dQ16.ensure(q16_halves)) || (rc = dQgamma.ensure(p.q_rows)) || (rc = dQuv.ensure(p.q_rows)))
          : (rc = dQ.ensure((size_t)p.q_rows * s->ld)))
    return rc;
  if (!keys && (rc = dDump.ensure(dump_elems))) return rc;
  const float eps = scan16_eps(s->dims);
  auto run = [&]() -> int {
    int r;
    HIP_TRY(hipMemcpyAsync(dQraw.p, queries, (size_t)nq * s->dims * sizeof(float), hipMemcpyHostToDevice, st));
    if ((r = wait_searches_in_flight(s, st))) return r;
    if ((r = s->clock.begin(st, BatchClock::kOutOfRing))) return r;
    HIP_TRY(hipMemsetAsync(dErr.p, 0, sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(dPart.p, 0xFF, part_elems * sizeof(uint64_t), st));   // (chunks with no tiles publish empty lists)
    HIP_TRY(hipMemsetAsync(dGthr.p, 0xFF, ((size_t)p.q_rows + 8) * sizeof(uint64_t), st));
    if (keys) HIP_TRY(hipMemcpyAsync(dGthr.p, keys, (size_t)nq * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if ((r = s->clock.scan_begin(st))) return r;
    if constexpr (F16) {
      HIP_TRY(launch_prep_queries16(dQraw.p, nq, s->dims, s->ld16, p.q_rows, s->metric, dQ16.p, dQgamma.p, dQuv.p, st));
      ScanArgs16 h;
      scan_args_shared(h, dCand.p, dPart.p, dErr.p, dGthr.p, p, lists_total, n_pub);
      h.Q = dQ16.p;
      h.X = s->f16.dX16.p;
      h.rowp = s->f16.dRowp16.p;
      h.qgamma = dQgamma.p;
      h.eps = eps;
      h.cos = s->metric == EHX_METRIC_COSINE;
      h.ld = s->ld16;
      set_scan_pass(h, p, tile0);
      h.dump = keys ? nullptr : dDump.p;
      HIP_TRY(launch_flat_scan16(h, st));
      if (!keys)
        HIP_TRY(launch_sample_select(dDump.p, kSampleTiles * kTileRows16, p.q_rows, nq, kprime, (unsigned long long*)dGthr.p, st));
    } else {
      HIP_TRY(launch_prep_queries(dQraw.p, nq, s->dims, s->ld, p.q_rows, s->metric, dQ.p, st));
      ScanArgs a;
      scan_args_shared(a, dCand.p, dPart.p, dErr.p, dGthr.p, p, lists_total, n_pub);
      a.Q = dQ.p;
      a.X = s->rows.dX.p;
      a.x_half = (uint32_t)s->x_half;
      a.rowp = s->rows.dRowp.p;
      a.ld = s->ld;
      set_scan_pass(a, p, tile0);
      HIP_TRY(launch_flat_scan8(a, st));
    }
    if ((r = s->clock.scan_end(st))) return r;
    if (keys) {
      HIP_TRY(hipMemcpyAsync(out_err, dErr.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(out_part, dPart.p, (size_t)nq * lists_total * kprime * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
      HIP_TRY(launch_flat_merge(dPart.p, nq, lists_total, kprime, dMerged.p, st, lists_total, false, (unsigned long long*)dGthr.p));
      HIP_TRY(hipMemcpyAsync(out_merged, dMerged.p, (size_t)nq * 64 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    } else {
      HIP_TRY(hipMemcpyAsync(out_dump, dDump.p, dump_elems * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    if ((r = s->clock.finish(st))) return r;
    HIP_TRY(hipMemcpyAsync(out_gthr, dGthr.p, (size_t)nq * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (F16) {
      HIP_TRY(hipMemcpyAsync(out_q16, dQ16.p, q16_halves * sizeof(__half), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(out_qgamma, dQgamma.p, (size_t)p.q_rows * sizeof(float), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(out_quv, dQuv.p, (size_t)p.q_rows * sizeof(float2), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return EHX_OK;
  };
  rc = run();
  if (rc) {  // launches of this call may still be in flight: drain them before the scratch is freed
    (void)hipStreamSynchronize(st);
    (void)hipGetLastError();
    return rc;
  }
  out_info[0] = p.q_rows;
  out_info[1] = F16 ? s->ld16 : s->ld;
  out_info[2] = p.n_chunks;
  out_info[3] = p.tiles_per_chunk;
  out_info[4] = p.xcd_map;
  out_info[5] = (uint32_t)n_pub;
  memcpy(&out_info[6], &eps, sizeof(float));
  out_info[7] = lists_total;
  return EHX_OK;
}

}  // namespace

extern "C" {

// which: 0 X8 (int8) | 1 rowp8 (float, four per row) | 2 tilep8 (float, four per tile) | 3 tileg8 (float, sixteen per tile)
// | 4 perm8 (u8) | 5 the two counters of dUnsafe8 (u64) | 6 ld8 | 7 cap (one u64 each); offset and length in those elements
int ehx_test_i8_array(ehx_space* s, int which, uint64_t elem_offset, uint64_t n_elems, void* out) {
  int rc = hook_space(s, "ehx_test_i8_array");
  if (rc) return rc;
  if (!out && n_elems) return fail(EHX_EINVAL, "NULL argument");
  // writers are serialised by wmu and enqueue on the writers' stream (grow: on the space's): with wmu held and both
  // streams drained the arrays are what the last write left
  std::lock_guard<std::mutex> wl(s->wmu);
  std::shared_lock<std::shared_mutex> rl(s->mu);
  if (s->dropped) return fail(EHX_ENOTFOUND, "Not found");
  HIP_TRY(hipSetDevice(s->device));
  const hipStream_t ws = s->wr.wstream ? (hipStream_t)s->wr.wstream : (hipStream_t)s->stream;
  if ((rc = sync_stream(s, ws)) || (rc = sync_stream(s, s->stream))) return rc;
  switch (which) {
    case kArrX8: return copy_slice(s, s->i8.dX8, elem_offset, n_elems, out, ws);
    case kArrPerm8: return copy_slice(s, s->i8.dPerm8, elem_offset, n_elems, out, ws);
    case kArrTileg8: return copy_slice(s, s->i8.dTileg8, elem_offset, n_elems, out, ws);
    case kArrUnsafe8: return copy_slice(s, s->i8.dUnsafe8, elem_offset, n_elems, out, ws);
    case kArrRowp8:
    case kArrTilep8: {
      const DevBuf<float4>& b = which == kArrRowp8 ? s->i8.dRowp8 : s->i8.dTilep8;
      if (elem_offset > b.n * 4 || n_elems > b.n * 4 - elem_offset) return fail(EHX_EINVAL, "slice beyond the array");
      if (n_elems == 0) return EHX_OK;
      HIP_TRY(hipMemcpyAsync(out, (const float*)b.p + elem_offset, n_elems * sizeof(float), hipMemcpyDeviceToHost, ws));
      return sync_stream(s, ws);
    }
    case kArrLd8:
    case kArrCap:
      if (elem_offset != 0 || n_elems != 1) return fail(EHX_EINVAL, "a scalar: offset 0, one element");
      *(uint64_t*)out = which == kArrLd8 ? (uint64_t)s->ld8 : s->cap;
      return EHX_OK;
  }
  return fail(EHX_EINVAL, "unknown array %d", which);
}

// queries [nq][dims] and thr [nq] (or NULL) are host pointers, as are the outputs:
//   thr == NULL (n_tiles must be 8): out_dump[q_rows * n_tiles * 256], scan8_dump_index layout, raw
//   thr != NULL: out_cnt[nq] (the pool counter: it counts past the pool's end), out_ovf[nq], out_ids / out_scores
//                [nq][kPoolCap], the first min(count, kPoolCap) of a query valid, in the pool's order
//   both: out_qparams[nq][4], out_quv[nq][2], out_q8[scanq8_bytes(q_rows, ld8)] raw,
//         out_info[8] = q_rows, ld8, group_b, n_chunks, tiles_per_chunk, xcd_map, published rows, lock-step on
// (outputs of the other form may be NULL)
int ehx_test_i8_pass(ehx_space* s, uint32_t nq, const float* queries, const float* thr, uint32_t tile0, uint32_t n_tiles,
                     float* out_dump, uint32_t* out_cnt, uint32_t* out_ovf, uint32_t* out_ids, float* out_scores,
                     float* out_qparams, float* out_quv, int8_t* out_q8, uint32_t* out_info) {
  int rc = hook_space(s, "ehx_test_i8_pass");
  if (rc) return rc;
  if (!queries || !out_qparams || !out_quv || !out_q8 || !out_info) return fail(EHX_EINVAL, "NULL argument");
  if (thr ? (!out_cnt || !out_ovf || !out_ids || !out_scores) : !out_dump) return fail(EHX_EINVAL, "NULL argument");
  if (nq == 0 || nq > 4 * kTileQ) return fail(EHX_EINVAL, "nq=%u outside [1, %u]", nq, 4 * kTileQ);
  if (!thr && n_tiles != kSampleTiles) return fail(EHX_EINVAL, "the sample form scans %u tiles", kSampleTiles);
  yield_to_writer(s);
  std::shared_lock<std::shared_mutex> rl(s->mu);
  if (s->dropped) return fail(EHX_ENOTFOUND, "Not found");
  // (the window may reach beyond the published rows, never beyond the arrays: the scan reads whole tiles)
  if (n_tiles == 0 || (uint64_t)tile0 + n_tiles > s->cap / kTileRows16)
    return fail(EHX_EINVAL, "tiles [%u, +%u) of a space of %llu", tile0, n_tiles, (unsigned long long)(s->cap / kTileRows16));
  std::lock_guard<std::mutex> sl(s->scratch_mu);
  HIP_TRY(hipSetDevice(s->device));
  Engine& E = engine();
  const hipStream_t st = s->stream;
  const uint64_t n_pub = s->n.load(std::memory_order_acquire);
  const ScanPlan p = plan_scan(nq, n_tiles, 1, E.n_cus);
  if (p.n_chunks > 256) return fail(EHX_EINTERNAL, "scan plan with %u chunks", p.n_chunks);
  // scratch of this call alone (owners: freed on every return)
  ehx_space::I8Set::Buffers b;
  DevBuf<float> dQraw, dDump;
  const size_t q8_bytes = scanq8_bytes(p.q_rows, s->ld8);
  const size_t dump_elems = (size_t)p.q_rows * n_tiles * kTileRows16;
  ScanArgsI8 a;   // filled as flat_pass8 fills it
  if ((rc = dQraw.ensure((size_t)nq * s->dims)) || (rc = i8_scan_args(s, b, p, n_pub, &a))) return rc;
  if (!thr && (rc = dDump.ensure(dump_elems))) return rc;
  DevBuf<float>&dQ = b.dQ, &dThr = b.dThr8;
  DevBuf<int8_t>& dQ8 = b.dQ8;
  DevBuf<float4>& dQp = b.dQp8;
  DevBuf<float2>& dQuv = b.dQuv;
  DevBuf<uint64_t>& dPool = b.dPool;
  DevBuf<uint32_t>& dCtl = b.dI8Ctl;
  std::vector<uint64_t> pool(thr ? (size_t)nq * kPoolCap : 0);
  uint32_t lockstep = 0;
  auto run = [&]() -> int {
    int r;
    HIP_TRY(hipMemcpyAsync(dQraw.p, queries, (size_t)nq * s->dims * sizeof(float), hipMemcpyHostToDevice, st));
    if ((r = wait_searches_in_flight(s, st))) return r;
    if ((r = s->clock.begin(st, BatchClock::kOutOfRing))) return r;
    // thr[q] = +inf (-inf for the padding queries), control words zero ...
    HIP_TRY(launch_prep_queries_i8(dQraw.p, nq, s->dims, s->ld, s->ld8, p.q_rows, s->metric, dQ.p, dQ8.p, dQp.p, dQuv.p, dThr.p,
                                   dCtl.p, st));
    // ... then the caller's thresholds
    if (thr) HIP_TRY(hipMemcpyAsync(dThr.p, thr, (size_t)nq * sizeof(float), hipMemcpyHostToDevice, st));
    set_scan_pass(a, p, tile0);
    a.dump = thr ? nullptr : dDump.p;
    a.sync = nullptr;
    if (thr && env().i8_sync > 0 && p.xcd_map && p.q_tiles > 1 && p.tiles_per_chunk >= 4 && p.n_chunks * 4u <= kSyncWordsI8) {
      a.sync = dCtl.p + 2 * (size_t)p.q_rows;   // (zeroed by the query preparation)
      a.sync_tol = (uint32_t)env().i8_sync;
      lockstep = 1;
    }
    out_info[2] = a.group_b;
    if ((r = s->clock.scan_begin(st))) return r;
    HIP_TRY(launch_flat_scan_i8(a, st));
    if ((r = s->clock.scan_end(st)) || (r = s->clock.finish(st))) return r;
    if (thr) {
      HIP_TRY(hipMemcpyAsync(out_cnt, dCtl.p, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(out_ovf, dCtl.p + p.q_rows, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(pool.data(), dPool.p, pool.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    } else {
      HIP_TRY(hipMemcpyAsync(out_dump, dDump.p, dump_elems * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(out_qparams, dQp.p, (size_t)nq * sizeof(float4), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_quv, dQuv.p, (size_t)nq * sizeof(float2), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_q8, dQ8.p, q8_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return EHX_OK;
  };
  rc = run();
  if (rc) {  // launches of this call may still be in flight: drain them before the scratch is freed
    (void)hipStreamSynchronize(st);
    (void)hipGetLastError();
    return rc;
  }
  out_info[0] = p.q_rows;
  out_info[1] = s->ld8;
  out_info[3] = p.n_chunks;
  out_info[4] = p.tiles_per_chunk;
  out_info[5] = p.xcd_map;
  out_info[6] = (uint32_t)n_pub;
  out_info[7] = lockstep;
  if (thr) {
    for (size_t q = 0; q < nq; ++q) {
      const size_t m = std::min<size_t>(out_cnt[q], kPoolCap);
      for (size_t i = 0; i < kPoolCap; ++i) {
        const uint64_t key = i < m ? pool[q * kPoolCap + i] : kKeyInf;
        out_ids[q * kPoolCap + i] = (uint32_t)key;
        out_scores[q * kPoolCap + i] = i < m ? ordered_to_f32((uint32_t)(key >> 32)) : __builtin_inff();
      }
    }
  }
  return EHX_OK;
}

// The share planner of the flat int8 chain's long passes (ehx_balance.h, flat_pass8).
// f8 != NULL: eight factors of any non-negative size, used as they are (no clamp, no averaging) for every stamped pass of
// the space until released; f8 == NULL: released, and the learnt factors forgotten.  min_tiles_per_chunk: from how many
// tiles per chunk a pass is stamped and balanced (0: the default, 64) — the tests' spaces have chunks of a few tiles.
int ehx_test_i8_balance_force(ehx_space* s, const double* f8, uint32_t min_tiles_per_chunk) {
  int rc = hook_space(s, "ehx_test_i8_balance_force");
  if (rc) return rc;
  if (f8) {
    double sum = 0.0;
    for (uint32_t x = 0; x < kXcds; ++x) {
      if (!(f8[x] >= 0.0) || !std::isfinite(f8[x])) return fail(EHX_EINVAL, "factor %u is not a non-negative number", x);
      sum += f8[x];
    }
    if (!(sum > 0.0)) return fail(EHX_EINVAL, "all factors are zero");
    s->i8_balance.force(f8);
  } else {
    s->i8_balance.reset();
  }
  s->i8_balance_min_tpc.store(min_tiles_per_chunk ? min_tiles_per_chunk : 64u, std::memory_order_relaxed);
  return EHX_OK;
}

// The final pass of the last int8 batch that had a stamped pass (EHX_ENOTFOUND: none yet):
//   out_info[8] = measured batches so far, grid, q_tiles, n_tiles, n_chunks, tile0, 1 if the kernel read the table (0: it
//                 computed the uniform split, which out_bounds then restates), wall_clock64 ticks per millisecond
//   out_bounds[n_chunks + 1 <= 257] tile range of every chunk, relative to tile0
//   out_stamps[2 * grid <= 1024]    start | finish of every workgroup (workgroup b ran on XCD b & 7)
//   out_factors[8], out_rates[8]    the shape's factors after that batch; the batch's own relative XCD rates (0: no tiles)
int ehx_test_i8_balance_read(ehx_space* s, uint64_t* out_info, uint32_t* out_bounds, uint64_t* out_stamps, double* out_factors,
                             double* out_rates) {
  int rc = hook_space(s, "ehx_test_i8_balance_read");
  if (rc) return rc;
  if (!out_info || !out_bounds || !out_stamps || !out_factors || !out_rates) return fail(EHX_EINVAL, "NULL argument");
  int khz = 0;
  HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, s->device));
  ehx_space::I8BalanceLast& l = s->i8_balance_last;
  std::lock_guard<std::mutex> g(l.mu);
  if (l.batches == 0) return fail(EHX_ENOTFOUND, "no stamped pass yet");
  const uint64_t info[8] = {l.batches, l.grid, l.q_tiles, l.n_tiles, l.n_chunks, l.tile0, l.table, (uint64_t)khz};
  std::copy(info, info + 8, out_info);
  std::copy(l.bounds, l.bounds + l.n_chunks + 1, out_bounds);
  std::copy(l.stamps.begin(), l.stamps.end(), out_stamps);
  std::copy(l.factors, l.factors + kXcds, out_factors);
  std::copy(l.rate, l.rate + kXcds, out_rates);
  return EHX_OK;
}

// which: 0 X16 (binary16 as u16, the three blocks of tail padding included) | 1 rowp16 (float, two per row, cap + 512 rows)
// | 2 the unsafe-row counter (u64) | 3 ld16 | 4 cap (one u64 each); offset and length in those elements
int ehx_test_f16_array(ehx_space* s, int which, uint64_t elem_offset, uint64_t n_elems, void* out) {
  int rc = hook_space(s, "ehx_test_f16_array", 16);
  if (rc) return rc;
  if (!out && n_elems) return fail(EHX_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> wl(s->wmu);   // (as ehx_test_i8_array)
  std::shared_lock<std::shared_mutex> rl(s->mu);
  if (s->dropped) return fail(EHX_ENOTFOUND, "Not found");
  HIP_TRY(hipSetDevice(s->device));
  const hipStream_t ws = s->wr.wstream ? (hipStream_t)s->wr.wstream : (hipStream_t)s->stream;
  if ((rc = sync_stream(s, ws)) || (rc = sync_stream(s, s->stream))) return rc;
  switch (which) {
    case kArrX16: return copy_slice(s, s->f16.dX16, elem_offset, n_elems, out, ws);
    case kArrUnsafe16: return copy_slice(s, s->f16.dUnsafe, elem_offset, n_elems, out, ws);
    case kArrRowp16: {
      const DevBuf<float2>& b = s->f16.dRowp16;
      if (elem_offset > b.n * 2 || n_elems > b.n * 2 - elem_offset) return fail(EHX_EINVAL, "slice beyond the array");
      if (n_elems == 0) return EHX_OK;
      HIP_TRY(hipMemcpyAsync(out, (const float*)b.p + elem_offset, n_elems * sizeof(float), hipMemcpyDeviceToHost, ws));
      return sync_stream(s, ws);
    }
    case kArrLd16:
    case kArrCap16:
      if (elem_offset != 0 || n_elems != 1) return fail(EHX_EINVAL, "a scalar: offset 0, one element");
      *(uint64_t*)out = which == kArrLd16 ? (uint64_t)s->ld16 : s->cap;
      return EHX_OK;
  }
  return fail(EHX_EINVAL, "unknown array %d", which);
}

// queries [nq][dims] and gthr_keys [nq] (or NULL) are host pointers, as are the outputs (those of the other form may be NULL):
//   gthr_keys == NULL (n_tiles must be 8): out_dump[8 * 256][q_rows], out_gthr[nq] = what sample_select makes of it for k'
//   gthr_keys != NULL: out_part[nq][lists][k'] as the pass published them (lists = 2 n_chunks = info[7], list = 2 chunk + wr;
//                      lists <= 2 n_tiles), out_err[1]; then, after flat_merge_kernel on the same stream: out_merged[nq][64]
//                      and out_gthr[nq], the threshold the merge hands to the next pass
//   both: out_q16[scanq16_halves(q_rows, ld16)] raw, out_qgamma[q_rows], out_quv[q_rows][2] (the padding queries included),
//         out_info[8] = q_rows, ld16, n_chunks, tiles_per_chunk, xcd_map, published rows, eps (float bits), lists
int ehx_test_f16_pass(ehx_space* s, uint32_t nq, const float* queries, uint32_t kprime, const uint64_t* gthr_keys,
                      uint32_t tile0, uint32_t n_tiles, float* out_dump, uint64_t* out_gthr, uint64_t* out_part,
                      uint32_t* out_err, uint64_t* out_merged, uint16_t* out_q16, float* out_qgamma, float* out_quv,
                      uint32_t* out_info) {
  return list_pass<true>(s, "ehx_test_f16_pass", nq, queries, kprime, gthr_keys, tile0, n_tiles, out_dump, out_gthr, out_part,
                         out_err, out_merged, out_q16, out_qgamma, out_quv, out_info);
}

// the collect form for flat_scan8_kernel, arguments as flat_pass sets them for the fp32 scan; tiles of kTileRows = 128 rows,
// list = 2 chunk + wr covers rows wr * 64 .. wr * 64 + 63 of each of the chunk's tiles; info[1] = ld, info[6] unused
int ehx_test_f32_pass(ehx_space* s, uint32_t nq, const float* queries, uint32_t kprime, const uint64_t* gthr_keys,
                      uint32_t tile0, uint32_t n_tiles, uint64_t* out_gthr, uint64_t* out_part, uint32_t* out_err,
                      uint64_t* out_merged, uint32_t* out_info) {
  if (!gthr_keys) return fail(EHX_EINVAL, "NULL argument");
  return list_pass<false>(s, "ehx_test_f32_pass", nq, queries, kprime, gthr_keys, tile0, n_tiles, nullptr, out_gthr, out_part,
                          out_err, out_merged, nullptr, nullptr, nullptr, out_info);
}

// queries answered on the large-k scan route, queries it handed to the exhaustive pass, of those the overflowed ones, scan
// passes launched, calls
void ehx_test_largek_counters(ehx_space* s, uint64_t out[5]) {
  for (int i = 0; i < 5; ++i) out[i] = s ? s->largek_ctr[i].load(std::memory_order_relaxed) : 0;
}

// largek_passes(n_rows, growth) as (tile0, n_tiles) pairs into out_pairs[2 * cap]; returns the number of passes (the first
// `cap` of them are written); out_consts[4] (optional) = sample rows, smallest k above the certified engines', largest k, fewest queries
uint32_t ehx_test_largek_plan(uint64_t n_rows, uint32_t growth, uint32_t* out_pairs, uint32_t cap, uint32_t* out_consts) {
  const std::vector<TileRange> p = largek_passes(n_rows, growth);
  for (size_t i = 0; i < p.size() && i < cap; ++i) {
    out_pairs[2 * i] = p[i].first;
    out_pairs[2 * i + 1] = p[i].second;
  }
  if (out_consts) {
    out_consts[0] = kLargeKSample;
    out_consts[1] = EHX_MAX_K + 1;
    out_consts[2] = kLargeKScanMax;
    out_consts[3] = (uint32_t)kLargeKMinQueries;
  }
  return (uint32_t)p.size();
}

// last_writers(ids[0, n)) into out[0, n): every id's last occurrence keeps it, the ones before it become 2^64 - 1
void ehx_test_last_writers(const uint64_t* ids, size_t n, uint64_t* out) { last_writers(ids, n, out); }

// write_batch(ids[0, n), old_n): out = {lo, hi, dense_run, touches_committed, all_appended}
void ehx_test_write_batch(const uint64_t* ids, size_t n, uint64_t old_n, uint64_t out[5]) {
  const WriteBatch b = write_batch(ids, n, old_n);
  const uint64_t v[5] = {b.lo, b.hi, b.dense_run, b.touches_committed, b.all_appended};
  std::copy(v, v + 5, out);
}

// The writers' stream's time of the last ehx_set_batch / ehx_set_batch_device on an unsharded space, in ms: out[0] the rows
// (staging copies and uploads, or the wait for the producer and the scatter), out[1] what follows up to the publish (block
// permutation, row statistics, scan copies).  The first call arms the events and answers EHX_ENOTFOUND: time the writes after it.
int ehx_test_write_times(ehx_space* s, float out[2]) {
  int rc = hook_space(s, "ehx_test_write_times", 0);
  if (rc) return rc;
  if (!out) return fail(EHX_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> wl(s->wmu);
  HIP_TRY(hipSetDevice(s->device));
  if (!s->wr.timed) {
    for (Event& e : s->wr.tev)
      if ((rc = e.ensure())) return rc;
    s->wr.timed = true;
    return fail(EHX_ENOTFOUND, "no write timed yet");
  }
  if (hipEventElapsedTime(&out[0], s->wr.tev[0], s->wr.tev[1]) != hipSuccess ||
      hipEventElapsedTime(&out[1], s->wr.tev[1], s->wr.tev[2]) != hipSuccess) {
    (void)hipGetLastError();
    return fail(EHX_ENOTFOUND, "no write timed yet");
  }
  return EHX_OK;
}

// filter_routes_cut, then filter_routes_gate: scans[0, n_filters) as every filtered search decides them (host arithmetic)
void ehx_test_filter_routes(int scan_serves, uint64_t cut, const uint64_t* n_allowed, uint32_t n_filters, const uint32_t* filter_of,
                            size_t nq, size_t min_scan_queries, char* scans) {
  filter_routes_cut(scan_serves != 0, cut, n_allowed, n_filters, scans);
  filter_routes_gate(filter_of, nq, min_scan_queries, n_filters, scans);
}

// launch_rows_prefix on host arrays, no space: out[rows][n + 1] and ONE word behind go up as they are, counts[rows][n] into
// the first n words of every row; all rows * (n + 1) + 1 words come back
int ehx_test_rows_prefix(const uint32_t* counts, uint32_t rows, uint32_t n, uint32_t* out) {
  int rc = ehx_init(nullptr, 0);
  if (rc) return rc;
  if (!out || (!counts && rows && n)) return fail(EHX_EINVAL, "NULL argument");
  const size_t words = (size_t)rows * ((size_t)n + 1) + 1;
  DevBuf<uint32_t> d;
  if ((rc = d.ensure(words))) return rc;
  HIP_TRY(hipMemcpy(d.p, out, words * sizeof(uint32_t), hipMemcpyHostToDevice));
  for (uint32_t r = 0; n && r < rows; ++r)
    HIP_TRY(hipMemcpy(d.p + (size_t)r * (n + 1), counts + (size_t)r * n, n * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_TRY(launch_rows_prefix(d.p, rows, n, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, d.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return EHX_OK;
}

// shard i of a row-sharded space, NULL for any other space or index
ehx_space* ehx_test_shard(ehx_space* s, uint32_t i) { return s && i < s->shards.size() ? s->shards[i] : nullptr; }

// how many ehx_knn calls the one-launch kernels answered (single_query_kernel, the graph search's one-launch form)
uint64_t ehx_test_one_launch_count(ehx_space* s) { return s ? s->n_one_launch.load(std::memory_order_relaxed) : 0; }

}  // extern "C"
