// Move-only owners of what a space holds on the device: HBM arrays, pinned host blocks, events, streams.  Every raw
// hipMalloc / hipFree / hipHostMalloc / hipEventCreate / hipStreamCreate of the host sources lives here; a member of
// ehx_space that is one of these is freed by its destructor (ehx_space::release_device resets groups of them).  They are
// created on whatever device is current: callers hipSetDevice first, as before.  Included by ehx_internal.h (HIP_TRY).
#pragma once

namespace ehx_impl {

// what is alive in this process, by kind (relaxed; read by the test hook ehx_test_live_resources, ehx_space.cpp)
enum { kLiveDevice, kLivePinned, kLiveEvents, kLiveStreams };
inline std::atomic<uint64_t> g_live[4];

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept { swap(o); }
  DevBuf& operator=(DevBuf&& o) noexcept {   // (what this held dies with `o`)
    swap(o);
    return *this;
  }
  ~DevBuf() { release(); }
  void swap(DevBuf& o) noexcept {
    std::swap(p, o.p);
    std::swap(n, o.n);
  }
  // a new allocation of exactly `want` elements, contents undefined (what it held before is freed first)
  int fresh(size_t want) {
    release();
    HIP_TRY(hipMalloc((void**)&p, want * sizeof(T)));
    g_live[kLiveDevice].fetch_add(1, std::memory_order_relaxed);
    n = want;
    return EHX_OK;
  }
  int ensure(size_t want, bool zero = false) {
    if (want <= n) return EHX_OK;
    int rc = fresh(want);
    if (rc) return rc;
    if (zero) {
      n = 0;   // (not `want` elements until they are zero)
      // (the fill runs on the NULL stream; the spaces' streams are non-blocking, i.e. not ordered with it: wait)
      HIP_TRY(hipMemset(p, 0, want * sizeof(T)));
      HIP_TRY(hipStreamSynchronize(nullptr));
      n = want;
    }
    return EHX_OK;
  }
  // a few zeroed words created once and kept (verdict words, counters, the one-launch ticket): the kernels count into
  // them, the host zeroes them again after it has read them
  int ensure_zeroed_once(size_t want) {
    if (p) return EHX_OK;
    int rc = fresh(want);
    if (rc) return rc;
    HIP_TRY(hipMemset(p, 0, want * sizeof(T)));
    return EHX_OK;
  }
  void release() {
    if (p) {
      (void)hipFree(p);
      g_live[kLiveDevice].fetch_sub(1, std::memory_order_relaxed);
    }
    p = nullptr;
    n = 0;
  }
};

// pinned host memory; `flags`: hipHostMallocDefault, or Coherent | Mapped for a block kernels read and write directly
template <class T>
struct PinBuf {
  T* p = nullptr;
  size_t n = 0;
  PinBuf() = default;
  PinBuf(PinBuf&& o) noexcept { swap(o); }
  PinBuf& operator=(PinBuf&& o) noexcept {
    swap(o);
    return *this;
  }
  ~PinBuf() { release(); }
  void swap(PinBuf& o) noexcept {
    std::swap(p, o.p);
    std::swap(n, o.n);
  }
  int ensure(size_t want, unsigned flags = hipHostMallocDefault, bool zero = false) {
    if (want <= n) return EHX_OK;
    release();
    HIP_TRY(hipHostMalloc((void**)&p, want * sizeof(T), flags));
    g_live[kLivePinned].fetch_add(1, std::memory_order_relaxed);
    if (zero) memset(p, 0, want * sizeof(T));
    n = want;
    return EHX_OK;
  }
  void release() {
    if (p) {
      (void)hipHostFree(p);
      g_live[kLivePinned].fetch_sub(1, std::memory_order_relaxed);
    }
    p = nullptr;
    n = 0;
  }
};

struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(Event&& o) noexcept { std::swap(e, o.e); }
  Event& operator=(Event&& o) noexcept {
    std::swap(e, o.e);
    return *this;
  }
  ~Event() { release(); }
  operator hipEvent_t() const { return e; }
  int ensure(unsigned flags = hipEventDefault) {   // created on first use
    if (e) return EHX_OK;
    HIP_TRY(hipEventCreateWithFlags(&e, flags));
    g_live[kLiveEvents].fetch_add(1, std::memory_order_relaxed);
    return EHX_OK;
  }
  void release() {
    if (e) {
      (void)hipEventDestroy(e);
      g_live[kLiveEvents].fetch_sub(1, std::memory_order_relaxed);
    }
    e = nullptr;
  }
};

struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(Stream&& o) noexcept { std::swap(s, o.s); }
  Stream& operator=(Stream&& o) noexcept {
    std::swap(s, o.s);
    return *this;
  }
  ~Stream() { release(); }
  operator hipStream_t() const { return s; }
  int ensure(unsigned flags) {
    if (s) return EHX_OK;
    HIP_TRY(hipStreamCreateWithFlags(&s, flags));
    g_live[kLiveStreams].fetch_add(1, std::memory_order_relaxed);
    return EHX_OK;
  }
  void release() {
    if (s) {
      (void)hipStreamDestroy(s);
      g_live[kLiveStreams].fetch_sub(1, std::memory_order_relaxed);
    }
    s = nullptr;
  }
};

// The verdict of one stage of the exact flat chain: how many of its queries the re-rank could not certify, and which.
// The re-rank kernels count into `count` and flag the queries in `flags` (1: uncertified; 2: because the candidate LIST was
// too short).  The stage's caller posts the copy of the count behind its launches, waits in its own way — the device path
// on the stream, the pipelined host path on `ev` (blocking-sync: the thread sleeps) — reads it, and only when it is not
// zero collects the flags: 8 bytes and one wait per stage of a clean batch.
// `extra` words may ride behind the count (the int8 sets' start / finish stamps, ehx_flat.cpp): the stage's kernels write
// them, and the first `riding` of them land with the count in the ONE copy the host waits for anyway.
struct Verdict {
  DevBuf<unsigned long long> count;    // [1 + extra] zeroed once; collect() clears the count again
  DevBuf<uint32_t> flags;              // [q_rows]
  PinBuf<unsigned long long> landed;   // (PINNED: a copy to pageable memory goes through a staging buffer and a copy kernel)
  Event ev;                            // post_and_record: the count has landed
  size_t riding = 0;                   // words behind the count the next post() takes along (<= extra; the stage's caller sets it)

  // (a verdict is always ensured with the same `extra`: the words are created once and kept)
  int ensure(size_t q_rows, size_t extra = 0) {
    int rc;
    if ((rc = count.ensure_zeroed_once(1 + extra)) || (rc = flags.ensure(q_rows))) return rc;
    return landed.ensure(1 + extra);
  }
  unsigned long long* extra_dev() const { return count.p + 1; }
  const unsigned long long* extra_landed() const { return landed.p + 1; }
  int post(hipStream_t st) {
    const size_t words = 1 + std::min(riding, count.n ? count.n - 1 : 0);
    HIP_TRY(hipMemcpyAsync(landed.p, count.p, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    return EHX_OK;
  }
  // (the one event of a pipelined batch: a marker of its own costs the queue another ~6 us per batch)
  int post_and_record(hipStream_t st) {
    int rc;
    if ((rc = ev.ensure(hipEventBlockingSync | hipEventDisableTiming)) || (rc = post(st))) return rc;
    HIP_TRY(hipEventRecord(ev, st));
    return EHX_OK;
  }
  // after the caller's wait: queries of the stage left uncertified
  unsigned long long read() const {
#if defined(EHX_ABL) && EHX_ABL
    return 0;  // profiling builds with ablated (wrong-by-construction) kernels: time the first stage only
#endif
    return *landed.p;
  }
  // the uncertified queries of a stage of m (subset: their indices in the whole batch) -> *out, those flagged 2 counted in
  // *n_short; clears the count for the next stage.  Waits for the stream.
  int collect(hipStream_t st, size_t m, const std::vector<uint32_t>* subset, std::vector<uint32_t>* out, size_t* n_short) {
    std::vector<uint32_t> f(m);
    HIP_TRY(hipMemsetAsync(count.p, 0, sizeof(unsigned long long), st));
    HIP_TRY(hipMemcpyAsync(f.data(), flags.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    out->clear();
    *n_short = 0;
    for (size_t j = 0; j < m; ++j)
      if (f[j]) {
        out->push_back(subset ? (*subset)[j] : (uint32_t)j);
        *n_short += f[j] == 2u;
      }
    return EHX_OK;
  }
};

}  // namespace ehx_impl
