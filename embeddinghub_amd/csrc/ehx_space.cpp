// Engine state, error text, HBM residency of a space (capacity doubling, index.cc:29-32), key <-> dense id maps
// (ANNIndex's key_to_label_ / label_to_key_, embeddinghub/embeddingstore/index.h:30-32).
#include "ehx_internal.h"

namespace ehx_impl {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

Engine& engine() {
  static Engine e;
  return e;
}


int ensure_stage(ehx_space* s, size_t bytes) {
  return s->wr.hStage.ensure((bytes + sizeof(float) - 1) / sizeof(float));
}

// pieces of grow(): the first `count` elements of the old array, and zeroes from element `from` to the new array's end
template <class T>
static int keep_prefix(DevBuf<T>& to, const DevBuf<T>& old, size_t count, hipStream_t st) {
  if (count) HIP_TRY(hipMemcpyAsync(to.p, old.p, count * sizeof(T), hipMemcpyDeviceToDevice, st));
  return EHX_OK;
}
template <class T>
static int zero_tail(DevBuf<T>& b, size_t from, hipStream_t st) {
  HIP_TRY(hipMemsetAsync(b.p + from, 0, (b.n - from) * sizeof(T), st));
  return EHX_OK;
}

// the groups of grow(), each: new arrays in local owners, filled on `st`, swapped in behind the synchronisation
static int grow_scan16(ehx_space* s, uint64_t want, uint64_t keep, hipStream_t st) {
  int rc;
  const char* nm = s->name.c_str();
  const unsigned long long wantl = want;
  const uint64_t keep_t = round_up(keep, kTileRows16);   // the copy is stored in whole 256-row tiles: those that hold rows
  DevBuf<__half> nx16;
  DevBuf<float2> nr16;
  // (+ tail padding: the scan's DMA reads three stage blocks / two tiles of row parameters ahead)
  if (nx16.fresh(want * s->ld16 + kScan16TailPadHalves) || nr16.fresh(want + 2 * kTileRows16))
    return fail(EHX_ENOMEM, "hipMalloc failed growing the scan copy of space '%s' to %llu rows", nm, wantl);
  if ((rc = keep_prefix(nx16, s->f16.dX16, keep_t * s->ld16, st)) ||
      (rc = keep_prefix(nr16, s->f16.dRowp16, keep, st)) || (rc = zero_tail(nx16, keep_t * s->ld16, st)))
    return rc;
  HIP_TRY(launch_rowp_pad(nr16.p, keep, nr16.n - keep, st));
  HIP_TRY(hipStreamSynchronize(st));
  s->f16.dX16.swap(nx16);
  s->f16.dRowp16.swap(nr16);
  return EHX_OK;
}

static int grow_scan8(ehx_space* s, uint64_t want, uint64_t keep, hipStream_t st) {
  int rc;
  const char* nm = s->name.c_str();
  const unsigned long long wantl = want;
  const uint64_t keep_t = round_up(keep, kTileRows16);   // the copy is stored in whole 256-row tiles: those that hold rows
  DevBuf<int8_t> nx8;
  DevBuf<float4> nr8, nt8;
  DevBuf<float> ng8;
  DevBuf<uint8_t> np8;
  const uint64_t tiles = want / kTileRows16, keep_tiles = keep_t / kTileRows16;
  if (nx8.fresh(want * s->ld8 + kScan8TailPadBytes) || nr8.fresh(want + 2 * kTileRows16) || nt8.fresh(tiles + 2) ||
      ng8.fresh((tiles + 2) * 16) || np8.fresh(want))
    return fail(EHX_ENOMEM, "hipMalloc failed growing the int8 scan copy of space '%s' to %llu rows", nm, wantl);
  if ((rc = keep_prefix(nx8, s->i8.dX8, keep_t * s->ld8, st)) || (rc = keep_prefix(nr8, s->i8.dRowp8, keep_t, st)) ||
      (rc = keep_prefix(nt8, s->i8.dTilep8, keep_tiles, st)) ||
      (rc = keep_prefix(ng8, s->i8.dTileg8, keep_tiles * 16, st)) || (rc = keep_prefix(np8, s->i8.dPerm8, keep_t, st)) ||
      (rc = zero_tail(ng8, keep_tiles * 16, st)))
    return rc;
  HIP_TRY(launch_perm8_pad(np8.p, keep_t, want - keep_t, st));
  if ((rc = zero_tail(nx8, keep_t * s->ld8, st))) return rc;
  HIP_TRY(launch_rowp8_pad(nr8.p, keep_t, nr8.n - keep_t, st));
  HIP_TRY(launch_tilep8_pad(nt8.p, keep_tiles, nt8.n - keep_tiles, st));
  HIP_TRY(hipStreamSynchronize(st));
  s->i8.dX8.swap(nx8);
  s->i8.dRowp8.swap(nr8);
  s->i8.dTilep8.swap(nt8);
  s->i8.dTileg8.swap(ng8);
  s->i8.dPerm8.swap(np8);
  return EHX_OK;
}

static int grow_search_copy(ehx_space* s, uint64_t want, uint64_t keep, hipStream_t st) {
  int rc;
  const char* nm = s->name.c_str();
  const unsigned long long wantl = want;
  DevBuf<float> nxs;
  if (nxs.fresh(want * s->ld))
    return fail(EHX_ENOMEM, "hipMalloc failed growing the search copy of space '%s' to %llu rows", nm, wantl);
  if ((rc = keep_prefix(nxs, s->rows.dXs, keep * s->ld, st)) || (rc = zero_tail(nxs, keep * s->ld, st))) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  s->rows.dXs.swap(nxs);
  return EHX_OK;
}

// grow HBM arrays to hold `rows` rows (multiple of 256, zero-initialised, rowp = pad).  Each group of arrays is built in
// local owners, filled on the space's stream and swapped in behind the synchronisation that follows its copies: the old
// arrays die with the locals, and an error return frees what it had allocated.  (Group by group, not all at the end: old
// and new scan copies of every group at once would raise the peak; a group that has moved is larger than `cap` needs.)
int grow(ehx_space* s, uint64_t rows) {
  const uint64_t want = round_up(rows < 256 ? 256 : rows, 256);
  if (want <= s->cap) return EHX_OK;
  HIP_TRY(hipDeviceSynchronize());  // no search may still read the old arrays
  const hipStream_t st = s->stream;
  const char* nm = s->name.c_str();
  const unsigned long long wantl = want;
  const uint64_t keep = s->n, row_bytes = s->ld * s->esz;
  DevBuf<char> nx;
  DevBuf<float2> nr;
  DevBuf<float> ni;
  int rc;
  if ((rc = nx.fresh(want * row_bytes))) return rc;
  if (nr.fresh(want) || ni.fresh(want)) return fail(EHX_ENOMEM, "hipMalloc failed growing space '%s' to %llu rows", nm, wantl);
  if ((rc = keep_prefix(nx, s->rows.dX, keep * row_bytes, st)) || (rc = keep_prefix(nr, s->rows.dRowp, keep, st)) ||
      (rc = keep_prefix(ni, s->rows.dInv, keep, st)) || (rc = zero_tail(nx, keep * row_bytes, st)) || (rc = zero_tail(ni, keep, st)))
    return rc;
  HIP_TRY(launch_rowp_pad(nr.p, keep, want - keep, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (s->has16 && (rc = grow_scan16(s, want, keep, st))) return rc;
  if (s->has8 && (rc = grow_scan8(s, want, keep, st))) return rc;
  if (s->params.mode == EHX_MODE_GRAPH && !s->x_perm && (rc = grow_search_copy(s, want, keep, st))) return rc;
  if ((rc = grow_columns(s, want, keep, st))) return rc;
  s->rows.dX.swap(nx);  // (single-copy graph spaces: the rows ARE the search copy, ehx_space::xs)
  s->rows.dRowp.swap(nr);
  s->rows.dInv.swap(ni);
  s->cap = want;
  return EHX_OK;
}

// capacity policy of ANNIndex::set (index.cc:29-32): double when the next label hits capacity
int ensure_rows(ehx_space* s, uint64_t rows) {
  if (rows < s->cap) return EHX_OK;
  uint64_t want = s->cap ? s->cap : 256;
  while (want <= rows) want *= 2;
  return grow(s, want);
}


int BatchClock::begin(hipStream_t st, uint32_t every) {
  if (!ev.start) {  // (created on first use, on the space's device; `start` last: it marks the set complete)
    int rc;
    for (Event* e : {&ev.end, &ev.fence_ev, &ev.spare[0], &ev.spare[1]})
      if ((rc = e->ensure())) return rc;
    for (auto& pr : ev.ring)
      for (auto& e : pr)
        if ((rc = e.ensure())) return rc;
    if ((rc = ev.start.ensure())) return rc;
  }
  const uint64_t b = every == kOutOfRing ? 0 : batches++;
  in_ring = every != kOutOfRing && b % every == every - 1;
  timed = in_ring || b == 0;
  pair = in_ring ? ev.ring[ring_count % kRing] : ev.spare;
  if (timed) {
    timed_valid = false;   // (a pass that fails half way leaves no half-recorded batch for ehx_stats)
    last = nullptr;
    HIP_TRY(hipEventRecord(ev.start, st));
  }
  return EHX_OK;
}

int BatchClock::scan_begin(hipStream_t st) {
  if (timed) HIP_TRY(hipEventRecord(pair[0], st));
  return EHX_OK;
}

int BatchClock::scan_end(hipStream_t st) {
  if (!timed) return EHX_OK;
  HIP_TRY(hipEventRecord(pair[1], st));
  last = pair;
  if (in_ring) ring_count++;
  return EHX_OK;
}

int BatchClock::finish(hipStream_t st) {
  {
    std::lock_guard<std::mutex> l(fence_mu);
    Event& closing = timed ? ev.end : ev.fence_ev;
    HIP_TRY(hipEventRecord(closing, st));
    fence = closing;
    fence_own = st == own;
  }
  if (timed) {
    timed_valid = last != nullptr;
    seq = ++*counter;
  }
  return EHX_OK;
}

int BatchClock::extend(hipStream_t st) {
  std::lock_guard<std::mutex> l(fence_mu);
  if (!fence) return EHX_OK;
  HIP_TRY(hipEventRecord(fence, st));
  fence_own = st == own;
  return EHX_OK;
}

int BatchClock::order(hipStream_t st) {
  // Only the space's own stream skips the wait for a fence recorded on it — the host pipeline's case: the stream's order
  // already holds it, and the wait packets (three per batch) were ~10 us of queue time (round 6).  A caller's stream always
  // waits: a stream destroyed and created again may come back with the handle of the one the fence was recorded on.
  std::lock_guard<std::mutex> l(fence_mu);
  if (fence && !(fence_own && st == own)) HIP_TRY(hipStreamWaitEvent(st, fence, 0));
  return EHX_OK;
}

int BatchClock::read(uint64_t* newest, double* last_scan_ms, double* last_total_ms, double* sum, uint64_t* got) {
  hipEvent_t f;   // (the caller holds the owner's lock: only the wait for it happens outside fence_mu)
  {
    std::lock_guard<std::mutex> l(fence_mu);
    f = fence;
  }
  if (!f) return EHX_OK;
  HIP_TRY(hipEventSynchronize(f));
  float ms = 0;
  if (timed_valid && seq > *newest) {
    HIP_TRY(hipEventSynchronize(ev.end));
    *newest = seq;
    if (hipEventElapsedTime(&ms, last[0], last[1]) == hipSuccess) *last_scan_ms = ms;
    if (hipEventElapsedTime(&ms, ev.start, ev.end) == hipSuccess) *last_total_ms = ms;
  }
  for (uint64_t i = 0; i < std::min<uint64_t>(ring_count, kRing); ++i)
    if (hipEventElapsedTime(&ms, ev.ring[i][0], ev.ring[i][1]) == hipSuccess) {
      *sum += ms;
      ++*got;
    }
  return EHX_OK;
}

void BatchClock::release() {
  std::lock_guard<std::mutex> l(fence_mu);
  ev = {};
  fence = nullptr;
  last = pair = nullptr;
  timed_valid = false;
  batches = ring_count = 0;
}

int wait_searches_in_flight(ehx_space* s, hipStream_t st) {
  int rc;
  if ((rc = s->clock.order(st))) return rc;
  for (auto& o : s->i8set)
    if ((rc = o.clock.order(st))) return rc;
  return EHX_OK;
}

int key_for_id(ehx_space* s, uint64_t id, std::string* out) {
  std::shared_lock<std::shared_mutex> kl(s->kmu);
  if (id < s->implicit_n) {
    *out = std::to_string(id);
    return EHX_OK;
  }
  if (id - s->implicit_n < s->id_to_key.size()) {
    *out = s->id_to_key[id - s->implicit_n];
    return EHX_OK;
  }
  return EHX_ENOTFOUND;
}

// the row a decimal key names among the implicitly keyed rows [0, implicit_n) (canonical decimals only: "007" is a key
// of its own)
bool implicit_id(const ehx_space* s, const char* key, size_t klen, uint64_t* id) {
  if (s->implicit_n == 0 || klen == 0 || klen > 20 || (klen > 1 && key[0] == '0')) return false;
  uint64_t v = 0;
  for (size_t i = 0; i < klen; ++i) {
    if (key[i] < '0' || key[i] > '9') return false;
    v = v * 10 + (uint64_t)(key[i] - '0');
  }
  if (v >= s->implicit_n) return false;
  *id = v;
  return true;
}

int lookup_key(ehx_space* s, const char* key, size_t klen, uint64_t* id) {
  std::shared_lock<std::shared_mutex> kl(s->kmu);
  if (implicit_id(s, key, klen, id)) return EHX_OK;
  auto it = s->key_to_id.find(std::string(key, klen));
  if (it == s->key_to_id.end()) return EHX_ENOTFOUND;
  *id = it->second;
  return EHX_OK;
}


// resolve the keys of a batch to row ids (upsert: an existing key keeps its label, index.cc:21-35); a key repeated
// inside the batch resolves to one row and the LAST vector wins, as sequential Sets would leave it.  Fresh keys are
// resolved against a batch-local map and committed to key_to_id / id_to_key only after their rows are in HBM with
// statistics: a failing upload leaves the key maps and the row count untouched.
void resolve_keys(ehx_space* s, size_t n, const char* const* keys, const size_t* klens, std::vector<uint64_t>* ids,
                         uint64_t* next_out, std::vector<std::string>* new_keys) {
  ids->resize(n);
  uint64_t next = s->n;
  std::shared_lock<std::shared_mutex> kl(s->kmu);
  std::unordered_map<std::string, uint64_t> fresh;
  fresh.reserve(n);
  new_keys->reserve(n);
  for (size_t i = 0; i < n; ++i) {
    std::string k(keys[i], klens[i]);
    if (implicit_id(s, keys[i], klens[i], &(*ids)[i])) continue;
    auto it = s->key_to_id.find(k);
    if (it != s->key_to_id.end()) {
      (*ids)[i] = it->second;
      continue;
    }
    auto f = fresh.try_emplace(k, next);  // (one hash for "seen in this batch?" and the insert)
    if (!f.second) {
      (*ids)[i] = f.first->second;
      continue;
    }
    (*ids)[i] = next;
    new_keys->push_back(std::move(k));
    ++next;
  }
  *next_out = next;
}

}  // namespace ehx_impl

// Test hook (not in include/ehx.h, in the spirit of EHX_TEST_PAUSE_US): how many device allocations, pinned allocations,
// events and streams the owners of ehx_own.h hold in this process right now.
extern "C" void ehx_test_live_resources(uint64_t out[4]) {
  for (int i = 0; i < 4; ++i) out[i] = g_live[i].load(std::memory_order_relaxed);
}
