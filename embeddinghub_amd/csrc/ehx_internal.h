// Internal declarations shared by the translation units of the C-ABI library (not installed, not part of the ABI):
//   ehx_space.cpp   engine state, error text, HBM residency and capacity doubling, key <-> id maps
//   ehx_flat.cpp    the exact flat chain: scan plans, fp32 / fp16 / int8 pipelines, exhaustive pass, engine fall-through
//   ehx_graph.cpp   graph mode: GPU-side insertion, update-in-place repair, the graph search pipeline
//   ehx_shards.cpp  row-sharded spaces inside one process (ehx_params.shards)
//   ehx_write.cpp   the write path (Set / BatchSet, the generator): landers, row statistics, derived copies, publish, write combiner
//   ehx_rowio.cpp   rows in and out without staging: Set from device memory, batched Get, Get by row ids on the device
//   ehx_search.cpp  ehx_knn_device / ehx_knn (host pointers: four routes behind the request combiner, ehx_combine.h) / keys / merge
//   ehx_call.cpp    what the batched entry points share: argument checks, the entry scaffold, key lookup, result blocks, host
//                   staging, sub-batches, the int8 radius scan
//   ehx_api.cpp     init, registry, Get, synthetic fill, graph import / export, statistics
#pragma once
// (was the head of ehx_api.cpp) C-ABI of the engine (include/ehx.h): process-global space registry, key <-> dense id map
// (ANNIndex's key_to_label_/label_to_key_, embeddinghub/embeddingstore/index.h:30-32), HBM
// residency and capacity doubling (index.cc:29-32), and the kNN pipelines that chain the gfx950
// kernels.  No vector arithmetic happens on the host: if the device is unavailable every compute
// entry point fails with EHX_ENODEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <map>
#include <random>
#include <set>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <system_error>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/ehx.h"
#include "ehx_balance.h"
#include "ehx_combine.h"
#include "ehx_env.h"
#include "ehx_kernels.h"

using namespace ehx;


struct ehx_space;

namespace ehx_impl {

extern thread_local char g_err[512];   // text of the calling thread's last error

int fail(int code, const char* fmt, ...);   // sets the thread's error text (ehx_last_error), returns `code`

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess) {                                                                   \
      (void)hipGetLastError();                                                                \
      return fail(_e == hipErrorOutOfMemory ? EHX_ENOMEM : EHX_ENODEVICE, "%s failed: %s (%s:%d)", \
                  #expr, hipGetErrorString(_e), __FILE__, __LINE__);                          \
    }                                                                                         \
  } while (0)

struct Engine {
  std::mutex mu;
  bool inited = false;
  int device = 0;            // devices[0]: where unsharded spaces live
  std::vector<int> devices;  // ehx_init's device list: shard i of a sharded space lives on devices[i % size]
  bool peer_all = true;      // every ordered pair of them has peer access open (false only under EHX_ALLOW_NO_PEER=1)
  int n_cus = 256;
  std::unordered_map<std::string, std::unique_ptr<ehx_space>> spaces;
  std::vector<std::unique_ptr<ehx_space>> graveyard;  // dropped spaces (tombstones), freed by ehx_shutdown
};
Engine& engine();   // the process-global engine state (ehx_space.cpp)

inline uint64_t round_up(uint64_t v, uint64_t m) { return (v + m - 1) / m * m; }

}  // namespace ehx_impl
#include "ehx_own.h"
namespace ehx_impl {

// The per-batch events of one search pipeline: the timing events behind ehx_stats (last_scan_ms / last_total_ms of the
// last timed batch, the ring of scan windows behind scan_ms_mean) and the fence — "every launch of the last batch has run"
// — that writers and searches on other streams wait for (wait_searches_in_flight).  A space has three: ehx_space::clock
// (fp32 / fp16 scans, exhaustive pass, graph search — a space is flat or graph, never both) and one per int8 scratch set.
// Sampling, begin(st, every): batch b since the last reset is timed when b == 0 or b % every == every - 1, and only the
// latter go into the ring (every = 1: every batch, batch 0 included; with every > 1 the first batch behind a reset, which
// starts on an idle queue and ran 5-10 % long in the bench's 10-step runs, stays out of the mean); every = kOutOfRing:
// timed, never in the ring, not counted.  An event record between two kernels idles the queue ~6 us (round 6), so a timed
// batch records four events — start, scan begin, scan end, end (which is also its fence) — and an untimed one its fence.
// The owner's lock (scratch_mu / the set's mu) serialises a clock's batches and ehx_stats; fence_mu guards the fence, which
// every other thread reads.
struct BatchClock {
  static constexpr int kRing = 64;
  static constexpr uint32_t kOutOfRing = 0;
  hipStream_t own = nullptr;                 // the space's search stream (create_one; not owned)
  std::atomic<uint64_t>* counter = nullptr;  // ehx_space::ev_counter: which of a space's clocks timed a batch last

  int begin(hipStream_t st, uint32_t every);
  int scan_begin(hipStream_t st);  // the timed scan window of the batch
  int scan_end(hipStream_t st);
  int finish(hipStream_t st);      // every launch of the batch is enqueued: its fence (and end)
  int extend(hipStream_t st);      // work enqueued behind the last batch belongs to it: re-records the event that closed it
  int order(hipStream_t st);       // work enqueued on `st` from here on starts after the last batch
  void reset() { batches = ring_count = 0; }   // (the next batch is a timed one)
  // ehx_stats: waits for the last batch; the last timed batch's times if it is newer than *newest; the ring's windows
  int read(uint64_t* newest, double* last_scan_ms, double* last_total_ms, double* sum, uint64_t* got);
  void release();

 private:
  struct Events {
    Event start, end, fence_ev;
    Event ring[kRing][2];
    Event spare[2];              // scan window of a timed batch outside the ring
  } ev;
  Event* last = nullptr;         // scan window of the last timed batch: a ring pair or the spare
  Event* pair = nullptr;         // ... of this batch
  uint64_t batches = 0, ring_count = 0;
  uint64_t seq = 0;              // *counter when the last timed batch finished
  bool timed = false, in_ring = false;  // this batch
  bool timed_valid = false;      // start / last / end hold the last timed batch, complete
  std::mutex fence_mu;
  hipEvent_t fence = nullptr;    // the event that closed the last batch (end or fence_ev); null before the first
  bool fence_own = false;        // ... recorded on `own`
};

}  // namespace ehx_impl
using namespace ehx_impl;

// A sub-batch of a call's queries: rows idx[0, m) of the batch gathered into a dense matrix, answered on their own into
// [m][k] lists, and those written back to the rows they belong to (ehx_call.cpp).  An instance per nesting level — the
// engine chain's (ehx_space::Scratch), the range and bitmap searches', whose re-runs may go through the engine chain
// themselves, and the graph walk's under a table of bitmaps, whose exact part goes through the bitmap search's.
struct SubsetBufs {
  DevBuf<float> dFbQ, dFbDist;
  DevBuf<uint64_t> dFbIds;
  DevBuf<uint32_t> dFbCnt, dFbIdx;
  typedef std::function<int(size_t, const float*, uint64_t*, float*, uint32_t*)> Answer;   // (m, d_q, d_ids, d_dist, d_cnt)
  // queries idx of the batch d_queries: gathered, answered by another path (on `st`), scattered into the batch's arrays;
  // the scatter belongs to the last batch of the space's clock (BatchClock::extend: writers wait for it too)
  int rerun(ehx_space* s, hipStream_t st, const float* d_queries, const std::vector<uint32_t>& idx, uint32_t k,
            const Answer& answer, uint64_t* d_ids, float* d_dist, uint32_t* d_count);
};

// What a falling-radius kNN (radius_knn, ehx_call.cpp) keeps per query of a device batch besides its int8 scratch set, and the
// sub-batch of the queries it hands on.
struct RadiusKnnBufs {
  DevBuf<uint64_t> dTop;       // [queries][kLargeKMax] carried exact keys
  DevBuf<uint32_t> dTopCnt;    // [queries] their number
  DevBuf<float> dRadius;       // [queries]
  DevBuf<uint32_t> dWork;      // [queries] rows re-ranked
  SubsetBufs sub;
};

// The result arrays of one batched call, [nq][k] ids | [nq] totals (range search; may be absent) | [nq][k] distances |
// [nq] counts: the caller's device arrays, or carved from one staging buffer of a host call (ehx_call.cpp).
struct ResultBlock {
  uint64_t* ids;
  float* dist;
  uint32_t* cnt;
  uint64_t* total;   // may be nullptr
  size_t nq;
  uint32_t k;
  static size_t bytes(size_t nq, uint32_t k, bool with_total);
  static ResultBlock at(unsigned char* p, size_t nq, uint32_t k, bool with_total);   // p: 8-byte aligned
  ResultBlock from(size_t q0, size_t m) const {   // queries [q0, q0 + m)
    return {ids + q0 * k, dist + q0 * k, cnt + q0, total ? total + q0 : nullptr, m, k};
  }
  int copy_out(hipStream_t st, uint64_t* h_ids, float* h_dist, uint32_t* h_cnt, uint64_t* h_total) const;  // ... and waits
  // A block `at` carved from one buffer, without totals: ONE copy of all of it into pinned memory, enqueued on `st` and not
  // waited for; and, once the caller has waited, the host block unpacked into the caller's arrays.
  int copy_block_out(hipStream_t st, void* h_pin) const;
  void unpack(const void* h_pin, uint64_t* h_ids, float* h_dist, uint32_t* h_cnt) const;
};

// Launches of a call that failed may still be in flight: unless the call succeeded they are drained — and the runtime's
// error cleared — before the call's scratch goes to the next caller.  `return drain.done(rc);` ends the guarded scope.
struct DrainUnlessOk {
  hipStream_t st;
  bool ok = false;
  int done(int rc) {
    ok = rc == EHX_OK;
    return rc;
  }
  ~DrainUnlessOk() {
    if (ok) return;
    (void)hipStreamSynchronize(st);
    (void)hipGetLastError();
  }
};

// What a host form of a side search stages on the device, one per path (scratch_mu): the queries, n_tail more floats behind
// them (the range search's radii) and the results.  up: both sized, the queries copied up on `st`; then q and out are set.
struct HostStage {
  DevBuf<float> dQraw;
  DevBuf<unsigned char> dOut;
  float* q = nullptr;   // the device queries [nq][dims] | the caller's tail
  ResultBlock out{};
  int up(hipStream_t st, const float* queries, size_t nq, uint32_t dims, uint32_t k, bool with_total, size_t n_tail = 0);
};

// Persistent host threads of a sharded space: worker i drives shard i + 1 (the caller's thread drives shard 0).  Round 2
// started G - 1 std::threads per CALL; these live as long as the space and sleep on a condition variable between jobs.
struct ShardWorkers {
  std::mutex run_mu;  // one job at a time
  std::mutex mu;
  std::condition_variable cv_go, cv_done;
  std::vector<std::thread> th;
  const std::function<int(size_t)>* job = nullptr;
  uint64_t gen = 0;
  size_t pending = 0;
  bool stop = false;
  std::vector<int> rcs;
  std::vector<std::string> errs;

  explicit ShardWorkers(size_t G) : rcs(G, 0), errs(G) {
    for (size_t i = 1; i < G; ++i) th.emplace_back([this, i] { loop(i); });
  }
  ~ShardWorkers() {
    {
      std::lock_guard<std::mutex> lk(mu);
      stop = true;
    }
    cv_go.notify_all();
    for (auto& t : th) t.join();
  }
  void loop(size_t i) {
    uint64_t seen = 0;
    for (;;) {
      const std::function<int(size_t)>* f;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv_go.wait(lk, [&] { return stop || gen != seen; });
        if (stop) return;
        seen = gen;
        f = job;
      }
      const int rc = (*f)(i);
      std::string err = rc ? g_err : "";
      {
        std::lock_guard<std::mutex> lk(mu);
        rcs[i] = rc;
        errs[i] = std::move(err);
        if (--pending == 0) cv_done.notify_all();
      }
    }
  }

  int run(const std::function<int(size_t)>& f) {
    std::lock_guard<std::mutex> one(run_mu);
    {
      std::lock_guard<std::mutex> lk(mu);
      job = &f;
      pending = th.size();
      ++gen;
    }
    cv_go.notify_all();
    rcs[0] = f(0);
    errs[0] = rcs[0] ? g_err : "";
    {
      std::unique_lock<std::mutex> lk(mu);
      cv_done.wait(lk, [&] { return pending == 0; });
      job = nullptr;
    }
    for (size_t i = 0; i < rcs.size(); ++i)
      if (rcs[i]) {
        snprintf(g_err, sizeof(g_err), "shard %zu: %s", i, errs[i].c_str());
        return rcs[i];
      }
    return EHX_OK;
  }
};

struct ehx_space {
  std::string name;
  uint32_t dims = 0, ld = 0;
  int metric = EHX_METRIC_L2SQ;
  ehx_params params{};
  bool frozen = false;
  bool dropped = false;        // ehx_space_drop ran: HBM released, the host object stays (tombstone) so that a
                               // thread still holding the handle fails with EHX_ENOTFOUND instead of touching
                               // freed memory; reclaimed by ehx_shutdown
  bool implicit_keys = false;  // rows appended by ehx_fill_synthetic / ehx_fill_manifold: key == decimal row id ...
  uint64_t implicit_n = 0;     // ... for rows [0, implicit_n); rows Set afterwards (unsharded spaces) carry their own keys:
                               // id_to_key[id - implicit_n].  A Set of the key "123" on such a space rewrites row 123.
  std::atomic<bool> poisoned{false};  // single-copy graph space (x_perm): an in-place overwrite of committed rows failed
                               // between the raw upload and the permutation — those rows sit in raw order inside a
                               // permuted store; searches and Gets refuse (EHX_EINTERNAL) instead of answering wrongly
  std::shared_mutex mu;        // writers: set/drop/reserve ; readers: knn/get
  // Exclusive writers of ehx_set_batch — ONLY those: growth of an appending Set, drop, reserve, freeze and graph import take
  // `mu` exclusively without it — waiting for `mu`.  The lock prefers readers: two callers searching back to back never
  // leave it free, and a batch that rewrites rows (or any graph write) waited tens of seconds for its turn
  // (tests/test_rewrite_under_search.py: 3 of 12 batches in 60 s beside one knn and one knn_device caller on 8 000 rows).
  // ehx_knn and ehx_knn_device let a waiting writer in first (yield_to_writer, ehx_search.cpp).
  std::atomic<uint32_t> excl_waiting{0};
  std::mutex wmu;              // every mutator takes wmu first, then mu: writers are serialised among themselves, and
                               // a batch of fresh keys does its upload / statistics / scan copies holding wmu only —
                               // the rows land beyond the published row count — and takes mu just to publish
  struct Writer {              // what writers use (wmu), created by create_one
    Stream wstream;            // the writers' stream (uploads, row statistics, derived copies)
    Event wev;                 // blocking-sync event: a writer waiting for its stream sleeps instead of spinning
    Event sev[2];              // "upload out of staging half i has finished" (ping-pong staging)
    PinBuf<float> hStage;      // pinned staging (Set / Get / query upload), ensure_stage
    DevBuf<uint64_t> dDstRows; // a Set from device memory: the stored row of every source row (~0: not written)
    DevBuf<uint32_t> dSrcIdx;  // ... a shard's: the batch positions of its rows
    Event tev[3];              // test hook ehx_test_write_times: rows in flight | rows landed | derived copies made, of the
    bool timed = false;        // last write (recorded only once the hook has asked for them)
  } wr;
  int device = 0;              // HIP device of this space's HBM state
  // Row sharding behind the C ABI (ehx_params.shards > 1): the PARENT keeps the key maps and no rows; global row g
  // lives in shard g % G at local row g / G (streamed Sets stay balanced); the shards are ordinary
  // keyless spaces, one per device of ehx_init's list, searched concurrently and merged on shard 0's device.
  bool keyless = false;            // a shard: rows are addressed by local id only, hidden from ehx_space_open
  std::vector<ehx_space*> shards;  // parent only (the shards are owned by the registry under hidden names)
  std::unique_ptr<ShardWorkers> workers;  // parent only: one persistent host thread per shard beyond the first
  struct ShardExchange {
    Event xev;                       // shard only: "my local top-k has reached the gather buffer" (the parent's stream waits)
    DevBuf<unsigned char> dOutPack;  // shard only: ids | distances | counts of one batch, contiguous: ONE peer copy
    DevBuf<unsigned char> dGPack;    // parent scratch on shards[0]'s device: the G packed results, one slot per shard
    DevBuf<unsigned char> dMergedOut;  // ... and the merged result, one block
  } xch;

  // HBM-resident state.  Every device / pinned resource below is an owner (ehx_own.h) inside a group named after what
  // guards and uses it; release_device resets the groups, so a buffer added to a group is freed with no further edit.
  struct Rows {                // the stored rows (moved by grow under mu held exclusively)
    DevBuf<char> dX;           // [cap][ld] rows, fp32 or fp16 (x_half)
    DevBuf<float2> dRowp;      // [cap]
    DevBuf<float> dInv;        // [cap] (cosine)
    DevBuf<float> dMaxSumsq;   // device scalar: largest |x|^2 ever written (certification margin, cert_margin)
    DevBuf<float> dXs;         // [cap][ld] two-copy graph spaces: the search copy (permuted blocks, cosine rows normalised)
    DevBuf<uint64_t> dPermIds; // rows of a batch written in place (non-contiguous ids), for launch_permute_blocks
  } rows;
  int x_half = 0;            // EHX_DTYPE_F16: rows stored as IEEE binary16 (flat mode only)
  size_t esz = sizeof(float);  // bytes per stored element
  char* xrow(uint64_t id) const { return rows.dX.p + id * ld * esz; }
  const float* xf32() const { return (const float*)rows.dX.p; }
  bool x_perm = false;       // graph mode, fp32 rows (round 4): the rows are stored ONCE — dX holds them in the search
                             // copy's block order, RAW, and rows.dXs stays empty; cosine rows are scaled by inv_norm on
                             // the fly in the kernels (GraphArgs / InsertArgs .xscale); Get undoes the permutation
  float* xs() const { return x_perm ? (float*)rows.dX.p : rows.dXs.p; }  // graph mode: the search copy
  uint64_t cap = 0;
  // published row count.  Atomic (round 6): an appending Set publishes its rows with ONE release store under the space's lock
  // held SHARED — rows below the new count are resident and described before the store, the arrays do not move while any search
  // holds the lock shared — where it used to take the lock exclusively "for the length of one store": glibc's rwlock prefers
  // readers, two pipelined search callers overlap without a gap, and the writer waited ~4 batches per chunk (12.5 M x 1536
  // under search: 63 ms per 8192-row chunk against 3 un-contended).
  // A search loads it ONCE (acquire) and passes that snapshot down to every pass, page, launch and statistic of the call: two
  // reads of it may differ, and a pass planned on one prefix and masked by another answers for no prefix at all.
  std::atomic<uint64_t> n{0};
  // fp16-MFMA filter scan (k_flat16.hip): unit-normalised binary16 scan copy of the rows
  bool has16 = false;          // the space keeps the fp16 scan copy (maintained on every write, whatever engine scans)
  struct Scan16 {
    DevBuf<__half> dX16;       // [cap][ld16] in the stage-blocked scan16_index layout
    DevBuf<float2> dRowp16;    // [cap + 512] (two tiles of tail padding: the scan's row parameters are fetched two tiles ahead)
    DevBuf<unsigned long long> dUnsafe;  // rows the filter cannot bound (then every scan is the fp32 scan)
  } f16;
  uint32_t ld16 = 0;
  // (the three counters below are written by an appending Set while searches run: atomic, stored BEFORE the release store of n —
  // a search reads them after its snapshot of n, so a prefix it scans never holds a row they do not count)
  std::atomic<uint64_t> h_unsafe{0};
  // int8-MFMA filter scan (k_flati8.hip): per-row-scaled int8 scan copy of the unit-normalised rows
  bool has8 = false;           // the space keeps the int8 scan copy (flat spaces whose row length makes it pay)
  struct Scan8 {
    DevBuf<int8_t> dX8;        // [cap][ld8] in the stage-blocked scan8_index layout
    DevBuf<float4> dRowp8;     // [cap + 512] (A, B, C, D)
    DevBuf<float4> dTilep8;    // [cap/256 + 2]
    DevBuf<float> dTileg8;     // [cap/256 + 2][16] per-lane-group max |A| (k_misc.hip: rows of a tile ordered by step)
    DevBuf<uint8_t> dPerm8;    // [cap] position -> row index inside the tile
    DevBuf<uint64_t> dTileList;  // scratch of launch_make_scan8
    DevBuf<unsigned long long> dUnsafe8;
  } i8;
  uint32_t ld8 = 0;
  std::atomic<uint64_t> h_unsafe8{0};
  std::atomic<uint64_t> h_margin8{0};     // tiles written so far with a lane group whose min B lies > 0.1 % above the tile's (dUnsafe8[1])
  uint64_t i8_min_rows = 16384;  // below this the fp16 filter serves (sample pass + cascade need a few thousand rows)
  uint32_t scan_sel = EHX_SCAN_AUTO;  // EHX_SCAN_*: what ehx_space_set_scan selected

  // graph (graph mode): adjacency, re-laid-out for the GPU (k_graph.hip), and the GPU-side insertion's scratch
  struct Graph {
    DevBuf<uint32_t> dAdj0;      // [g_n][2M]
    DevBuf<uint32_t> dUpStart;   // [g_n]
    DevBuf<uint32_t> dUpLists;   // [*][M]
    DevBuf<uint32_t> dVisited;
    DevBuf<uint32_t> dInsIds, dInsSel, dInsVislog, dItemTgt, dItemKind, dItemOff, dItemIds;
    DevBuf<uint32_t> dLinkHead, dLinkNext, dLinkCount;  // bulk build: device-side link work items (k_insert.hip)
    DevBuf<uint64_t> dLinkTouched;
    DevBuf<int32_t> dInsLevels, dItemLevel;
    DevBuf<unsigned long long> dGraphCounters;  // n_dist, n_hops0, n_hops_up, n_prefetch_hit, [4..11] profile builds
  } graph;
  uint64_t g_n = 0;              // rows covered by the graph (0 = no graph)
  uint32_t g_entry = 0;
  int g_maxlevel = -1;
  // one query per call in one launch, host-visible in / out (knn_host_direct; scratch_mu)
  struct OneLaunch {
    PinBuf<char> hOnePin;        // host-coherent pinned: query | ids[64] | dist[64] | count | flag
    DevBuf<uint64_t> dOnePart;   // [n_blocks][64] workgroup lists
    DevBuf<uint32_t> dOneTicket;
  } one;
  uint32_t one_seq = 0;
  std::atomic<uint64_t> n_one_launch{0};
  // Host-pointer batches (ehx_knn with more than a handful of queries): every call in flight owns a SLOT — pinned
  // staging for its queries and results, device buffers for both, a copy stream — so that the upload of call i + 1
  // and the download of call i - 1 run beside the scan of call i (which alone needs scratch_mu).  One caller sees its
  // own copies in series as before; two or more callers keep the scan kernels back to back.
  struct HostSlot {
    Stream st;
    Event in_ev, done_ev;
    PinBuf<char> pin;
    DevBuf<float> dq;
    DevBuf<unsigned char> dout;
    bool busy = false;   // (hs_mu; a call holds the space's lock shared for as long as it holds a slot)
  };
  static constexpr int kHostSlots = 3;
  HostSlot hslot[kHostSlots];
  std::mutex hs_mu;
  std::condition_variable hs_cv;
  // Adaptation of the int8 pipeline's candidate list (i8_adapt): batches run in either scratch set, under the pipeline
  // lock or not (knn_host_direct), so the score lives under its own small mutex and the lengths are atomics — a batch
  // reads them ONCE, at its start.
  std::mutex i8_adapt_mu;
  uint32_t i8_fb_score = 0;      // recent batches that lost queries to the next engine (i8_adapt_mu)
  std::atomic<uint32_t> i8_width{kMerged8};  // width of the int8 pipeline's candidate list (doubles when batches lose
                                 // queries; create_one seeds it from the row length)
  std::atomic<uint32_t> i8_kprime_min{0};    // floor of the list's logical length k' (raised when queries lose their
                                 // certificate to a short list; flat_pass8 picks k' from the row count above it)
  std::atomic<uint32_t> i8_kprime_last{0};   // the k' the last batch ran with (statistics only)
  bool vis_dirty = false;    // a search that clears its bitmaps with a memset BEFORE the kernel leaves them marked; the
                             // visit-log mode needs them all-zero at launch
  // GPU-side insertion state
  uint64_t g_cap_rows = 0;       // rows the adjacency arrays are sized for
  uint64_t g_lists_cap = 0, g_lists_used = 0;  // upper-level lists (M ids each)
  std::vector<int32_t> h_levels;  // level of every node in the graph
  std::default_random_engine level_rng;  // hnswlib: level_generator_ (libstdc++ minstd_rand0)
  bool level_rng_seeded = false;
  uint64_t g_stale_updates = 0;  // rows overwritten in place after their insertion (no graph repair)

  // key map (explicit keys only)
  // key <-> row id.  Their own lock (taken INSIDE mu when both are held, or alone): a streamed batch inserts its
  // 8192 keys — milliseconds of hashing and allocation — without stopping the searches, which only need mu for the
  // device arrays and the row count; the row count is published after the keys, so every id a search can return
  // already has its key.
  std::shared_mutex kmu;
  std::unordered_map<std::string, uint64_t> key_to_id;
  std::vector<std::string> id_to_key;

  // scratch for the kNN pipeline (serialised by scratch_mu)
  std::mutex scratch_mu;
  Stream stream;               // the space's search stream (create_one)
  struct Scratch {
    DevBuf<float> dQraw, dQ;
    DevBuf<uint64_t> dCand, dPart, dMerged, dGthr;
    DevBuf<uint32_t> dScanErr;                 // one word: times a scan kernel tripped its bounded-retry guard (ehx_stats)
    // filter scratch: fp16 queries, per-query (gamma, u, v), re-run buffers
    DevBuf<__half> dQ16;
    DevBuf<float> dQgamma, dSample;
    DevBuf<float2> dQuv;
    SubsetBufs sub;                            // the queries a stage of the engine chain re-runs
    Verdict verdict;                           // of the fp16 / fp32 / exhaustive stage that ran last
    PinBuf<char> hSmallPin;                    // pinned staging of small host calls: [queries | ids, distances, counts]
    DevBuf<uint64_t> dSmallOut;                // their results, one block (one device-to-host copy)
  } scr;
  // neighbours of stored rows (ehx_knn_by_keys / ehx_knn_by_ids_device): the gathered query batch, the row ids of a host
  // call, the (k + 1)-long lists | validity flags | a host call's k-long results; by_ev: the last call's launches have run
  // (the next call's stream waits for it before it writes them again)
  struct ByKey {
    DevBuf<float> dByQ;
    DevBuf<uint64_t> dByIds;
    DevBuf<unsigned char> dByOut;
    Event by_ev;
  } by;
  // exact kNN among a caller's id lists (ehx_among.cpp; scratch_mu): a host call's staged ids | offsets, queries and
  // results.  The prepared queries, the workgroups' key lists, the merged keys and the page floor are the exhaustive pass's
  // (scr.dQ / dPart / dMerged / dGthr); the space's batch clock fences all of them across streams.
  struct Among {
    DevBuf<uint64_t> dLists;
    HostStage host;
  } among;
  // exact range search (ehx_range.cpp; scratch_mu): the queries' pools and control words of the exact kernel, the list of
  // queries a stage answers, the sub-batch an overflow sends through the exact kNN pipeline, and a host call's staged
  // queries | radii and results.  The prepared queries are the exhaustive pass's (scr.dQ), fenced by the space's clock.
  struct Range {
    DevBuf<uint64_t> dPool;      // [slots][kPoolCap]
    DevBuf<uint32_t> dCtl;       // [slots] pool counts (= totals) | [queries] members kept by the int8 path's re-rank
    DevBuf<uint32_t> dSel;       // [slots] query of every slot
    SubsetBufs sub;              // the overflowed queries, answered by the exact kNN pipeline
    DevBuf<uint64_t> dIota;
    HostStage host;              // host form: queries | radii, and ids | totals | distances | counts
  } range;
  std::atomic<uint64_t> range_ctr[4] = {};   // test hook: queries answered by the int8 path, by the exact path, pool overflows, truncated
  // exact kNN under row bitmaps, one for the call or a table with one per query (ehx_masked.cpp; scratch_mu): the bitmaps'
  // compaction — allowed rows before every 256-row tile, the ascending lists of allowed ids, a sample of each — the scan
  // route's buffers (RadiusKnnBufs; flagged queries are answered by the exact kNN among their mask's whole list), and a
  // host call's staged queries and results.
  struct Masked {
    DevBuf<uint32_t> dBlock;     // [kSideChunk] word offset of the bitmap of every query of a device batch | the bitmaps,
                                 // [n_masks][words below the row count]: ONE block, the int8 scan's flush reads both.
                                 // Host bitmaps and tables are staged here; ONE device bitmap is used where it lies
    DevBuf<uint32_t> dCum;       // [n_masks][n_tiles + 1]
    DevBuf<uint64_t> dList;      // the masks' ascending lists of allowed ids, back to back
    DevBuf<uint64_t> dSample;    // [n_masks][256]
    RadiusKnnBufs scan;          // (its sub-batch: the flagged queries of one mask)
    SubsetBufs group;            // the call's queries ordered by route and mask
    HostStage host;              // host form: queries, and ids | distances | counts
    DevBuf<unsigned long long> dCapHits;   // [1] the graph walk under a bitmap: queries whose list reached its cap
    // the graph walk under a TABLE of bitmaps (ehx_graph_knn_masked_multi*): per walked query the word offset of its bitmap
    // from the first (GraphArgs::allow_of; its own buffer: the head of dBlock is the scan route's, rewritten per device
    // batch), and the walked / exact parts of a batch that EHX_WALK_AUTO splits (their own: masked_answer re-runs through
    // `group` and scan.sub)
    DevBuf<uint32_t> dWalkOf;
    SubsetBufs split;
    // the predicate searches (ehx_where.cpp): [kMaskedMaxMasks] the call's predicates, where the kernel that builds the
    // bitmaps into dBlock reads them; sized once
    DevBuf<WherePred> dPreds;
    // the Boolean filter searches (ehx_filter.cpp): [kFilterExprWords] the call's packed expression — clauses | values |
    // filter runs — where k_filter.hip's kernel reads it; sized once
    DevBuf<uint32_t> dFilter;
  } masked;
  // test hook: queries answered on the scan route, on the exact route, queries that overflowed, scan passes launched, calls
  // (ehx_knn_masked* and ehx_knn_masked_multi* both count here)
  std::atomic<uint64_t> masked_ctr[5] = {};
  // exact kNN under a label column (ehx_labeled.cpp; scratch_mu): per device batch the compaction of the column for the
  // batch's distinct wanted labels ("slots").  The lists, the scanning slots' tile prefixes and samples, the scan route's
  // buffers and the grouping are the bitmap search's (masked.dList / dCum / dSample / scan / group: one answer serves both).
  struct Labeled {
    DevBuf<uint32_t> dBlock;     // [kLabelHead] wanted label of every query of a device batch | a copy of label_of[0, n_eff):
                                 // ONE block, the int8 scan's flush reads both
    DevBuf<uint32_t> dSlots;     // [slots] the ascending table | [slots] row counts | [slots] scanning index | [slots] cursors
    DevBuf<uint16_t> dSlotOf;    // [n_eff] the slot of every row's label
    DevBuf<uint64_t> dOff;       // [slots] where every slot's list starts in masked.dList | [scanning slots] the same by index
    DevBuf<uint64_t> dRange;     // [queries] start | [queries] end of every query's list in the ONE per-query launch
    DevBuf<uint32_t> dCol;       // a host call's staged label column, the rows below the row count
    HostStage host;              // host form: queries, and ids | distances | counts
  } labeled;
  // test hook: queries answered on the scan route, on the list route, queries that overflowed, scan passes launched, calls
  std::atomic<uint64_t> labeled_ctr[5] = {};
  // test hook (scripts/bench_labeled.py's crossover sweep): 0 the cut decides; 1 every non-empty label takes the scan route
  // where the int8 scan serves (a batch may then name at most 127 of them); 2 every label takes the list route
  std::atomic<uint32_t> labeled_route{0};
  // exact range search under row bitmaps (ehx_rangem.cpp; scratch_mu): the compaction is the bitmap search's (masked), the
  // pools, control words and slot queries the range search's (range.dPool / dCtl / dSel); its own are the scan route's radii
  // (NaN for the queries of a device batch the scan does not answer), every list-route slot's list, the sub-batch of the
  // queries whose pool overflowed, and a host call's staged queries | radii and results
  struct RangeMasked {
    DevBuf<float> dRadius;       // [queries of a device batch]
    DevBuf<uint32_t> dScans;     // [queries of a device batch] non-zero: the scan answers the query
    DevBuf<uint64_t> dListOff;   // [slots] where the slot's list starts in masked.dList
    DevBuf<uint32_t> dListLen;   // [slots] its length
    SubsetBufs sub;
    HostStage host;
  } rangem;
  // test hook: queries answered on the scan route, on the list route, queries whose pool overflowed, truncated answers, calls
  std::atomic<uint64_t> rangem_ctr[5] = {};
  // test hook (scripts/bench_range_masked.py's crossover sweep): 0 the cut decides; 1 every non-empty mask takes the scan
  // route where the int8 scan serves a radius; 2 every mask takes the list route
  std::atomic<uint32_t> rangem_route{0};
  // test hook of the graph walk under a bitmap (ehx_graph_knn_masked*, ehx_graph_knn_masked_multi*): queries walked, queries
  // answered exactly, calls
  std::atomic<uint64_t> graphm_ctr[3] = {};
  // exact kNN for EHX_MAX_K < k <= kLargeKScanMax on the int8 radius scan (ehx_largek.cpp; scratch_mu): flagged queries are
  // answered by the exhaustive pass
  RadiusKnnBufs largek;
  // test hook: queries answered on the route, handed to the exhaustive pass, of those the overflowed, scan passes launched, calls
  std::atomic<uint64_t> largek_ctr[5] = {};
  // grouped kNN in its three forms — unfiltered, under row bitmaps, under a label column (ehx_grouped.cpp's grouped_answer;
  // scratch_mu): the scan route's buffers (RadiusKnnBufs; its sub-batch: the queries the scan hands on), the list route's own
  // — carried keys, radii, every query's slab of row ids and its control words — the queries ordered by route and filter,
  // every query's [start | end) of a device batch, and a host call's staged labels, queries and results.  The compactions
  // are the bitmap search's and the label search's (masked, labeled).
  struct Grouped {
    RadiusKnnBufs scan;
    RadiusKnnBufs exact;         // (its sub-batch is not used: the list route hands nothing on)
    SubsetBufs group;
    DevBuf<uint64_t> dPool;      // [queries of a device batch][kPoolCap]
    DevBuf<uint32_t> dCtl;       // [queries] pool counts | [queries] flags, all zero
    DevBuf<uint64_t> dRange;     // [queries of a device batch] start | [queries] end of every query's list
    DevBuf<uint32_t> dLabels;    // host form: the labels of the prefix searched
    HostStage host;
  } grouped;
  // test hooks, one per form: queries answered on the scan route, on the list route (by the gate or handed on by the scan),
  // of those the overflowed, scan passes launched, calls
  std::atomic<uint64_t> grouped_ctr[5] = {};
  std::atomic<uint64_t> groupedm_ctr[5] = {};
  std::atomic<uint64_t> groupedl_ctr[5] = {};
  // Stored label columns (ehx_columns.cpp): column c is one uint32_t per row, written through the write path by key.
  // dCol[c] is sized to `cap` and moved by grow with the rows; col_live[c] turns true under mu held exclusively, at the
  // column's first write (readers hold mu at least shared; the writers, serialised by wmu, may read it under wmu alone).  A
  // column that is not live reads as EHX_GROUP_NONE everywhere.  col_gen[c] counts the writes to entries below the published
  // row count (mu exclusive) — with the row count it tells a search whether the column's index still describes it.
  struct Columns {
    DevBuf<uint32_t> dCol[EHX_MAX_COLUMNS];
    DevBuf<uint64_t> dDst;       // a write by key (wmu): the row of every entry of the batch (~0: a later entry writes it)
    DevBuf<uint32_t> dVals;      // ... and its values, a column after the other
    DevBuf<uint64_t> dGetIds;    // ehx_column_get (scratch_mu): the rows asked for | their values
    DevBuf<uint32_t> dGetVals;
    DevBuf<uint32_t> dNone;      // EHX_GROUP_NONE for every row of a prefix: a group column never written (scratch_mu)
  } cols;
  bool col_live[EHX_MAX_COLUMNS] = {};
  std::atomic<uint64_t> col_gen[EHX_MAX_COLUMNS] = {};
  // The index of a stored column over a prefix of n rows (k_colindex.hip; scratch_mu): valid for a search's snapshot n_pub iff
  // gen == col_gen[c] and n == n_pub, else rebuilt on the search's stream by the search that finds it stale.
  struct ColIndex {
    bool valid = false;
    uint64_t gen = 0, n = 0;
    uint32_t n_tiles = 0;
    DevBuf<uint32_t> dBlock;     // [kLabelHead] the head filtered_answer rewrites per device batch | the column's prefix as
                                 // the index was built from it: the block of the int8 scan's flush (allow_label)
    DevBuf<uint32_t> dKey[2], dVal[2];   // the sort's ping-pong arrays
    DevBuf<uint32_t> dHist;      // [256][tiles of 4096] | [4][256] the column's digit histograms
    DevBuf<uint32_t> dBounds;    // [n / 256 + 2] labels that begin in every 256-key tile, prefixed
    DevBuf<uint32_t> dLabels, dStart;    // [L] | [L + 1]
    DevBuf<uint64_t> dPerm;      // [n] row ids by (label, row id): the lists of every label, back to back
    DevBuf<uint64_t> dRun;       // [heavy] start | [heavy] end in dPerm of the labels that may scan
    DevBuf<uint32_t> dCum;       // [heavy][n_tiles + 1]
    DevBuf<uint64_t> dSample;    // [heavy][256]
    // the host mirror: planning a search touches the device for nothing that grows with the row count
    std::vector<uint32_t> labels, start;     // [L] ascending | [L + 1]
    std::vector<uint32_t> heavy;             // positions in `labels` of the labels with more than masked_exact_cut(n) rows
    std::vector<uint32_t> cum;               // [heavy][n_tiles + 1]
    uint64_t builds = 0, served_fresh = 0, last_passes = 0;   // test hook ehx_test_column_counters
  } colidx[EHX_MAX_COLUMNS];
  // int8 filter scratch: everything ONE in-flight batch of the int8 pipeline owns — prepared queries, query tiles +
  // parameters, per-pass thresholds, sample scores, pools, running best list, verdict, batch clock.  TWO sets: a host
  // caller's batch can be enqueued behind another caller's on the space's stream while that one still waits for its
  // verdict (knn_host_direct), so the scan kernels of consecutive batches run back to back with no host in between.
  struct I8Set {
    struct Buffers {
      DevBuf<float> dQ;
      DevBuf<int8_t> dQ8;
      DevBuf<float4> dQp8;
      DevBuf<float2> dQuv;
      DevBuf<float> dThr8, dSample8;
      DevBuf<uint64_t> dPool, dMerged8;
      DevBuf<uint32_t> dI8Ctl;  // [q_rows] pool counts | [q_rows] overflow flags | [kSyncWordsI8] lock-step progress words
      DevBuf<uint64_t> dCnt;    // [8] epilogue counters of diagnosis builds (EHX_I8_COUNT); the set's own: nothing shared
      Verdict verdict;          // of the set's int8 stage, on the device path and the pipelined one; the stamps of the
                                // batch's long passes ride behind its count (kStampWords)
      PinBuf<uint32_t> hBounds; // host-mapped: [kStampedPasses][kBalanceMaxChunks + 1] the share planner's tables the
                                // batch's long passes read (ScanArgsI8::bounds); written at the enqueue, under the set's mutex
    } buf;
    BatchClock clock;              // timed: batch 0 and every EHX_STATS_EVERY-th batch of the set
    std::mutex mu;
    // The long passes of the batch in flight (flat_pass8 -> i8_stage_outcome; the set's mutex): what each was planned with
    // and where its stamps ride.  At most the last kStampedPasses of a cascade, each of at most kStampGrid workgroups.
    static constexpr uint32_t kStampedPasses = 2, kStampGrid = 512;
    static constexpr size_t kStampWords = (size_t)kStampedPasses * 2 * kStampGrid;
    struct StampedPass {
      uint64_t key;                // BalanceState::key_of
      uint32_t grid, q_tiles, n_tiles, n_chunks, tile0;
      uint32_t stamp_off;          // words into the verdict's extra block
      bool table;                  // the kernel read `bounds` (else it computed the uniform split itself)
      uint32_t bounds[kBalanceMaxChunks + 1];
    } stamped[kStampedPasses];
    uint32_t n_stamped = 0;
  };
  I8Set i8set[2];
  // The share of every XCD in the int8 scan's long passes (ehx_balance.h): the factors per pass shape, and what the last
  // measured batch's final pass looked like (test hooks, scripts/i8_xcd_skew.py).
  BalanceState i8_balance;
  std::atomic<uint32_t> i8_balance_min_tpc{64};   // a pass is stamped (and balanced) from this many tiles per chunk
  struct I8BalanceLast {
    std::mutex mu;
    uint64_t batches = 0;          // measured batches so far
    uint32_t grid = 0, q_tiles = 0, n_tiles = 0, n_chunks = 0, tile0 = 0, table = 0;
    uint32_t bounds[kBalanceMaxChunks + 1] = {};
    std::vector<uint64_t> stamps;  // [2 * grid]
    double factors[kXcds] = {}, rate[kXcds] = {};   // the factors after the update; the batch's own relative rates
  } i8_balance_last;
  std::atomic<uint64_t> ev_counter{0};   // orders the timed batches of the space's three clocks (BatchClock::counter)
  std::atomic<uint32_t> i8_next_set{0};
  std::mutex i8_enqueue_mu;  // held while ONE host batch's int8 stage is enqueued on the space's stream (not while its
                             // verdict is awaited): two callers in different scratch sets must not interleave their
                             // launches — the batches' kernels would alternate on the stream and every per-batch scan
                             // time (the timing ring, ehx_stats) would span both
  std::atomic<uint64_t> n_filter_queries{0}, n_filter_fallback{0}, n_exhaustive{0}, n_uncertified_final{0};
  std::atomic<uint64_t> n_i8_queries{0}, n_i8_fallback{0};
  // the batch clock of the passes under scratch_mu: fp32 / fp16 scans time every batch, the exhaustive pass every batch
  // outside the ring, the graph search batch 0 and every EHX_STATS_EVERY-th batch (round 6: six event records per batch
  // idled the queue ~36 us of a 0.35-ms batch)
  BatchClock clock;

  // micro-batcher: concurrent small ehx_knn calls are coalesced into one device batch (ehx_search.cpp)
  struct KnnReq : CombineReq {
    const float* q;
    size_t nq;
    uint32_t k;
    uint64_t* ids;   // the caller's [nq][k] ids, [nq][k] distances, [nq] counts
    float* dist;
    uint32_t* cnt;
  };
  Combiner<KnnReq> knn_combiner;
  std::atomic<uint64_t> n_coalesced_batches{0}, n_coalesced_queries{0};
  // write-combiner: concurrent single-row ehx_set calls (runner/copy.go: 500 goroutines per chunk) become one batch
  struct SetReq : CombineReq {
    const char* key;
    size_t klen;
    const float* vec;
  };
  Combiner<SetReq> set_combiner;
  std::atomic<uint64_t> n_combined_sets{0}, n_combined_batches{0};

  // stats
  std::atomic<uint64_t> n_queries{0}, n_dist{0}, n_rerank{0}, bytes_algo{0};

  // frees every device / pinned resource (idempotent); the host-side object stays usable as a tombstone
  void release_device() {
    rows = {};
    f16 = {};
    i8 = {};
    graph = {};
    scr = {};
    by = {};
    among = {};
    range = {};
    masked = {};
    largek = {};
    grouped = {};
    cols = {};
    for (auto& x : colidx) x = ColIndex{};
    one = {};
    xch = {};
    wr = {};
    for (auto& c : i8set) {
      c.buf = {};
      c.clock.release();
    }
    for (auto& h : hslot) h = {};
    clock.release();
    stream = {};
    cap = 0;
    n = 0;
    g_n = 0;
  }
  ~ehx_space() { release_device(); }
};


namespace ehx_impl {
// ---- ehx_space.cpp ----
int ensure_stage(ehx_space* s, size_t bytes);
int grow(ehx_space* s, uint64_t rows);
int ensure_rows(ehx_space* s, uint64_t rows);
inline bool valid_space(ehx_space* s) { return s != nullptr; }
inline bool is_parent(const ehx_space* s) { return !s->shards.empty(); }

// work enqueued on stream `st` from here on starts after every search of this space that is already in flight (whatever
// stream it was given, whichever scratch set it runs in): BatchClock::order of the space's three clocks
int wait_searches_in_flight(ehx_space* s, hipStream_t st);
int key_for_id(ehx_space* s, uint64_t id, std::string* out);
int lookup_key(ehx_space* s, const char* key, size_t klen, uint64_t* id);
bool implicit_id(const ehx_space* s, const char* key, size_t klen, uint64_t* id);  // (caller holds kmu or mu)
void resolve_keys(ehx_space* s, size_t n, const char* const* keys, const size_t* klens, std::vector<uint64_t>* ids,
                         uint64_t* next_out, std::vector<std::string>* new_keys);

// ---- ehx_graph.cpp ----
int graph_ensure_arrays(ehx_space* s);
int graph_ensure_lists(ehx_space* s, uint64_t lists);
int graph_insert(ehx_space* s, uint64_t id0, uint64_t count, uint32_t batch);
int graph_update(ehx_space* s, uint32_t id);
struct GraphOneLaunch {   // one query per call in one launch (knn_graph_locked)
  const float* q_host;     // the raw query, host-visible
  uint32_t* done_flag;     // host-visible; the kernel stores `seq` there when the results are written
  uint32_t seq;
};
struct GraphMask {        // the walk under a row bitmap (k_graphm.hip): always the batch form, always the strict order
  const uint32_t* allow;   // device words; row r is allowed iff r < n_bits and bit r & 31 of word r >> 5 is set
  uint64_t n_bits;         // already cut at the call's snapshot of the row count
  unsigned long long* cap_hits;   // device counter: queries whose list reached its cap
  const uint32_t* allow_of;       // nullptr: ONE bitmap; else device [nq]: query i's bitmap begins allow_of[i] words into allow
};
// the walk list's length under a bitmap, a function of ef alone: max(ef, min(EHX_WALK_LIST_FACTOR * ef, EHX_WALK_LIST_MAX))
inline uint32_t graph_walk_cap(uint32_t ef) {
  return std::max<uint32_t>(ef, std::min<uint32_t>(EHX_WALK_LIST_FACTOR * ef, EHX_WALK_LIST_MAX));
}
int knn_graph_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, uint64_t* d_ids,
                     float* d_dist, uint32_t* d_count, const GraphOneLaunch* one = nullptr, const GraphMask* mask = nullptr);

// ---- ehx_flat.cpp ----
struct ScanPlan {
  uint32_t q_tiles, q_rows, n_tiles, n_chunks, tiles_per_chunk, kprime, xcd_map, grid;
};
ScanPlan plan_scan(uint32_t nq, uint32_t n_tiles, uint32_t k, int n_cus);   // one scan pass over `n_tiles` row tiles
struct ScanPass {
  uint32_t tile0;
  ScanPlan plan;
};
// the passes of a scan cascade over n_tiles row tiles: the first `first_tiles`, then x `growth` in tiles seen per pass while
// less than half of them are, then the rest (first_tiles >= n_tiles / 2: one pass)
std::vector<ScanPass> plan_cascade(uint32_t nq, uint32_t n_tiles, uint32_t k, int n_cus, uint64_t first_tiles, uint64_t growth);
// the fields of one pass in the arguments of any of the three scans (ScanArgs, ScanArgs16, ScanArgsI8)
template <class Args>
inline void set_scan_pass(Args& a, const ScanPlan& pl, uint32_t tile0) {
  a.tile0 = tile0;
  a.n_tiles = pl.n_tiles;
  a.n_chunks = pl.n_chunks;
  a.tiles_per_chunk = pl.tiles_per_chunk;
  a.xcd_map = pl.xcd_map;
}
// what the fp32 and the fp16 scan's arguments share: the candidate slots and list slots of the batch, its error word and
// thresholds (every pass writes its lists from slot 0)
template <class Args>
inline void scan_args_shared(Args& a, uint64_t* cand, uint64_t* part, uint32_t* err, uint64_t* gthr, const ScanPlan& p,
                             uint32_t lists_total, uint64_t n_pub) {
  a.cand = cand;
  a.part = part;
  a.n = (uint32_t)n_pub;
  a.q_tiles = p.q_tiles;
  a.kprime = p.kprime;
  a.list0 = 0;
  a.lists_total = lists_total;
  a.err = err;
  a.gthr = (unsigned long long*)gthr;
}
constexpr uint64_t kNoSnapshot = ~0ull;   // knn_device_locked: no snapshot of the row count yet, take one
int resolve_engine(const ehx_space* s, uint64_t n_pub);
// n_pub: the search's one snapshot of the published row count (s->n.load(std::memory_order_acquire))
int exhaustive_pass(ehx_space* s, uint64_t n_pub, hipStream_t st, size_t nq, const float* d_queries, uint32_t k,
                    uint64_t* d_ids, float* d_dist, uint32_t* d_count);
// The int8 stage of a batch, for both of its callers (knn_device_locked; knn_host_direct's pipelined stage).  The caller
// holds the scratch set's mutex from the enqueue to the outcome and waits in between in its own way.
struct I8Outcome {
  std::vector<uint32_t> failed;   // queries the stage could not certify: the next engine's
  size_t n_short = 0;             // ... of them because their candidate LIST was too short
  uint32_t kprime = 0;            // the list's logical length the stage ran with
};
// enqueues the stage on `st` as one block (i8_enqueue_mu), behind `after` if given, and posts its verdict: with the verdict's
// event recorded (pipelined: Verdict::post_and_record) or without
int i8_stage_enqueue(ehx_space* s, uint64_t n_pub, int set, hipStream_t st, hipEvent_t after, bool pipelined, size_t nq,
                     const float* d_queries, uint32_t k, uint64_t* d_ids, float* d_dist, uint32_t* d_count, I8Outcome* o);
// after the caller's wait: the landed verdict -> *o, and ALL of the stage's accounting (work counters, n_i8_queries,
// n_i8_fallback, the list's adaptation)
int i8_stage_outcome(ehx_space* s, uint64_t n_pub, int set, hipStream_t st, size_t nq, uint32_t k, I8Outcome* o);
int knn_device_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k,
                      uint64_t* d_ids, float* d_dist, uint32_t* d_count, uint64_t n_pub = kNoSnapshot);
// the work counters of a batch of nq queries whose first engine scanned n_pub rows of elem_bytes-wide elements
void count_scan_batch(ehx_space* s, size_t nq, uint64_t n_pub, uint32_t k, uint64_t elem_bytes);
// the rest of the chain after the int8 stage: fp16 filter, fp32 scan, exhaustive pass, each for what the one before left.
// eng: what resolve_engine gave for the batch; i8: the outcome of its int8 stage when that is EHX_ENGINE_I8 (the failed
// queries continue), else nullptr
int flat_chain_rest(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const float* d_queries, uint32_t k,
                    uint64_t* d_ids, float* d_dist, uint32_t* d_count, int eng, const I8Outcome* i8);

// ---- ehx_search.cpp ----
// The gather's view of a row-sharded parent (locked shared) on the prefix of n_pub rows: every shard locked shared into
// *held (parent, then shards, as ehx_get_by_id takes them; hold them until the gather has read the rows), its rows' base in
// g->bases, shape and layout in g->rows, g->G.  A dropped or poisoned shard, more than kMaxShardBases shards, or a shard
// without peer access to shard 0's device (EHX_ALLOW_NO_PEER) is refused.
int parent_gather_view(ehx_space* p, uint64_t n_pub, std::vector<std::shared_lock<std::shared_mutex>>* held, GatherRowsArgs* g);
void yield_to_writer(const ehx_space* s);   // a search lets an exclusive writer that waits for the space's lock in first
// the keys of result lists [n][k] (counts out_count) packed into key_arena, key_off[n * k + 1]: ehx_knn_keys' layout
int fill_key_arena(ehx_space* s, size_t n, uint32_t k, const uint64_t* out_ids, const uint32_t* out_count, char* key_arena,
                   size_t arena_cap, uint64_t* key_off);

// ---- ehx_call.cpp ----
int check_not_poisoned(const ehx_space* s);   // a single-copy graph space whose rows an aborted overwrite left in raw order
// a NULL space; k (or max_results: k_name) of 0 unless zero_k_ok, or above EHX_MAX_K_PAGED
int check_space_and_k(const ehx_space* s, uint32_t k, const char* k_name, bool zero_k_ok);
int check_batch_size(size_t nq);
// the two around "a pointer the call needs is NULL" (ptrs_ok false: EHX_EINVAL with null_text)
int check_batch_call(const ehx_space* s, size_t nq, uint32_t k, const char* k_name, bool zero_k_ok, bool ptrs_ok,
                     const char* null_text = "NULL argument");
// (space locked) dropped: EHX_ENOTFOUND; a row-sharded parent: EHX_EUNSUPPORTED "<what>: space '<name>' is row-sharded (<why>)"
int check_unsharded(const ehx_space* s, const char* what, const char* why);
// ids of n stored keys (space locked shared; takes kmu shared); an unknown key: EHX_ENOTFOUND, its index in *bad_index
int lookup_keys(ehx_space* s, size_t n, const char* const* keys, const size_t* klens, std::vector<uint64_t>* ids,
                size_t* bad_index);
RowsView rows_view(const ehx_space* s, uint64_t n_pub);   // where the rows are, for a search on the prefix of n_pub rows
// The int8 scan's arguments for a batch planned as `p` in the buffers `b` (grown as needed), all but the pass's own fields
// (set_scan_pass; dump, sync).  The control words are b.dI8Ctl: [q_rows] pool counts | [q_rows] overflow flags | lock-step.
int i8_scan_args(ehx_space* s, ehx_space::I8Set::Buffers& b, const ScanPlan& p, uint64_t n_pub, ScanArgsI8* a);
// The entry scaffold of the list, range and bitmap searches, behind a path's own argument checks.  search_shared: a waiting
// writer goes first, the space locked shared, a dropped or row-sharded one refused ("<what>: ... (<why>)"), body() under that
// ONE hold.  on_device, inside it, for nq > 0 queries: scratch_mu, the space's device current, body(); unless that gives
// EHX_OK, what it left on `st` (the caller's stream; the space's own for a host form) is drained.  search_on_device: both,
// for an entry point with nothing in between (caller: the caller's stream; nullptr: a host form, on the space's own).
template <class Body>
int search_shared(ehx_space* s, const char* what, const char* why, Body&& body) {
  yield_to_writer(s);
  std::shared_lock<std::shared_mutex> rl(s->mu);
  const int rc = check_unsharded(s, what, why);
  return rc ? rc : body();
}
template <class Body>
int on_device(ehx_space* s, size_t nq, hipStream_t st, Body&& body) {
  if (nq == 0) return EHX_OK;
  std::lock_guard<std::mutex> sl(s->scratch_mu);
  HIP_TRY(hipSetDevice(s->device));
  DrainUnlessOk drain{st};
  return drain.done(body());
}
template <class Body>
int search_on_device(ehx_space* s, const char* what, const char* why, size_t nq, const hipStream_t* caller, Body&& body) {
  return search_shared(s, what, why, [&] { return on_device(s, nq, caller ? *caller : (hipStream_t)s->stream, body); });
}
constexpr size_t kSideChunk = 2048;   // queries per device batch of the range and bitmap searches: their pools are 64 MiB
// "<subject> keeps a prepared query in LDS": rows longer than among_max_ld() are refused before anything is enqueued
int check_rows_fit_lds(const ehx_space* s, const char* subject);
// this space's int8 scan serves a radius (range search; the bitmap search's scan route) on the prefix of n_pub rows
inline bool i8_serves_radius(const ehx_space* s, uint64_t n_pub) {
  return resolve_engine(s, n_pub) == EHX_ENGINE_I8 && s->ld <= range_rerank_max_ld();
}
// Passes of the int8 scan over disjoint tile ranges in one int8 scratch set, nq <= kSideChunk queries: each under the
// threshold mapped from d_radius[q] as it stands then, each followed by its re-rank.  The set's mutex, then i8_enqueue_mu
// around the launches; ONE wait, then *out (word: d_word[0, nq)).
struct RadiusScanOut {
  std::vector<uint32_t> ctl, word;
  const uint32_t *pool_cnt, *flag;   // [nq] inside ctl; flag 1: the pool overflowed, else non-zero: the bound does not serve
};
typedef std::pair<uint32_t, uint32_t> TileRange;   // (tile0, n_tiles)
struct RadiusScan {
  const std::vector<TileRange>* passes = nullptr;
  const uint32_t* allow = nullptr;   // optional row bitmap allow[0, allow_bits) in the scan's flush
  uint32_t allow_bits = 0;
  bool allow_per_query = false;      // allow is the block of ScanArgsI8::allow_per_query: a bitmap per query
  bool allow_label = false;          // allow is the block of ScanArgsI8::allow_label: wanted labels | the label column
  bool time_thr = false;            // the timed scan phase opens in front of the first threshold kernel, not behind it
  // rerank(i, last, a, sc) enqueues pass i's re-rank and records sc.clock.scan_end where its path's timed scan phase ends
  std::function<int(size_t, bool, const ScanArgsI8&, ehx_space::I8Set&)> rerank;
  const uint32_t* d_word = nullptr;  // [nq] the caller's words of the verdict
  // optional: enqueued behind the query preparation and in front of the first pass, inside the timed scan phase (which then
  // opens here) — what writes the first radii from the set's prepared queries
  std::function<int(const ScanArgsI8&, ehx_space::I8Set&)> seed;
};
int i8_radius_scan(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const float* d_queries, const float* d_radius,
                   const RadiusScan& c, RadiusScanOut* out);

// Exact kNN by the radius scan under a radius that falls (k_radius.hip's header has the algorithm and why it is exact), for
// every query of c.out in device batches of kSideChunk: stage 0 gives the first radii, every pass's re-rank merges its hits
// into the carried keys and lowers the radius, ONE verdict is read behind the last pass, and the queries it flags (pool
// overflow, or the bound does not serve them) are gathered, answered by c.exact and scattered back.  Adds the rows
// re-ranked to n_dist; the caller's own counters take *t, which holds the batches whose verdict was read whatever is returned.
struct RadiusKnn {
  std::vector<TileRange> passes;
  const uint32_t* allow = nullptr;     // optional row bitmap, as RadiusScan's
  uint32_t allow_bits = 0;
  bool allow_per_query = false;        // ... or the block of a bitmap per query, as RadiusScan's
  bool allow_label = false;            // ... or the block of a label column, as RadiusScan's
  // stage 0, one of two.  first_radius(m, d_q, o, d_radius): enqueued in front of a batch's scan, writes the exact k-th
  // distance over ANY k rows the search may return (+Inf: none known) for its m queries; it may use o's rows, which are
  // written again behind it.  Or, without it, the seed inside the scan's timed phase: the strided sample of rows 0, stride,
  // 2 stride, ... (n_sample <= kLargeKSample of them) re-ranked in every query's pool
  std::function<int(size_t, const float*, const ResultBlock&, float*)> first_radius;
  uint64_t seed_stride = 0;
  uint32_t n_sample = 0;
  // optional, instead of that strided sample (seed_stride and n_sample are then unused): fill_pool(q0, m, pool, pool_cnt)
  // enqueues what writes the sample of every query of the device batch [q0, q0 + m) of the call — pool[j][0, pool_cnt[j]),
  // at most kLargeKSample row ids each, any rows the search may return — where launch_radius_seed would be
  std::function<int(size_t, size_t, uint64_t*, uint32_t*)> fill_pool;
  ResultBlock out;                     // out.k <= kLargeKMax
  SubsetBufs::Answer exact;
  // optional, instead of exact, where the exact answer depends on which query it is (a bitmap per query):
  // handed(q0, todo, d_q, o) answers the flagged queries todo (ascending, inside the device batch that starts at query q0
  // of the call, whose queries are d_q and whose rows of the output are o) and writes their rows of o
  std::function<int(size_t, const std::vector<uint32_t>&, const float*, const ResultBlock&)> handed;
  // optional, instead of launch_radius_rerank: the re-rank of the seed and of every pass (the grouped kNN's, which caps the
  // keys per label: k_grouped.hip)
  std::function<hipError_t(const RadiusRerankArgs&, hipStream_t)> rerank;
};
struct RadiusKnnTally {
  uint64_t batches = 0, queries = 0;     // device batches whose verdict was read, and their queries
  uint64_t handed = 0, overflowed = 0;   // of those: queries left to c.exact; of these, the ones whose pool overflowed
};
int radius_knn(ehx_space* s, hipStream_t st, RadiusKnnBufs& w, uint64_t n_pub, const float* d_queries, const RadiusKnn& c,
               RadiusKnnTally* t);

// ---- ehx_largek.cpp ----
constexpr uint32_t kLargeKScanMax = kLargeKMax;   // the large-k scan route serves EHX_MAX_K < k <= this
constexpr size_t kLargeKMinQueries = 64;          // ... for batches of at least one query tile of the int8 wave tile (128 x 64)
// tile ranges of the route's passes over n_rows rows: pass j (j = 1, 2, ...; the seed is stage 0) ends at the first tile
// boundary at or beyond kLargeKSample * growth^j rows, the last pass takes the rest (n_rows <= kLargeKSample * growth: one pass)
std::vector<TileRange> largek_passes(uint64_t n_rows, uint32_t growth);
// knn_device_locked's gate: this flat-space batch takes the route (i8_serves_radius is part of it)
bool largek_serves(const ehx_space* s, size_t nq, uint32_t k, uint64_t n_pub);
// the route, for a batch largek_serves accepts: scratch_mu held, NO int8 scratch set's mutex held (radius_knn takes one);
// returns with the stream drained
int largek_locked(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const float* d_queries, uint32_t k,
                  uint64_t* d_ids, float* d_dist, uint32_t* d_count);

// ---- ehx_range.cpp ----
constexpr uint32_t kRangeGridTarget = 4096;   // workgroups an exact range kernel's launch aims for (16 per CU): chosen, not measured
// The bitmaps of a filtered range search in the int8 scan's flush (RadiusScan's allow fields) and the tiles below their n_bits
struct RangeAllow {
  const uint32_t* allow;
  uint32_t allow_bits;
  bool per_query;
  uint32_t n_tiles;
};
// What the int8 range stage found for a device batch: the queries it leaves to an exact path (counted[j] = 1: todo[j]'s pool
// overflowed; else the bound does not serve it), and of the queries it answered the rows re-ranked and the truncated answers
struct RangeI8Verdict {
  std::vector<uint32_t> todo;
  std::vector<uint8_t> counted;
  uint64_t n_pairs = 0, n_trunc = 0, n_over = 0;
};
// ONE pass of the int8 radius scan over all tiles (allow: over the tiles its bitmaps cover, the bitmaps tested in the flush)
// under the threshold mapped from d_radius, the survivors re-ranked, cut at the radius and emitted into o; nq <= kSideChunk
int range_i8_stage(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const float* d_queries, const float* d_radius,
                   uint32_t max_results, const ResultBlock& o, const RangeAllow* allow, RangeI8Verdict* out);

// ---- ehx_masked.cpp ----
constexpr size_t kTabWords = kSideChunk;    // word offsets in front of the bitmaps of ehx_space::Masked::dBlock
// At most this many allowed rows: the exact route of the bitmap searches
uint64_t masked_exact_cut(uint64_t n_pub);
int check_mask_of(const uint32_t* mask_of, size_t nq, uint32_t n_masks);   // an entry at or above n_masks: EHX_EINVAL
// Where a call's bitmaps come from: n_masks >= 1 bitmaps of `stride` words each, in host or device memory — or, with `build`
// set (p and stride unused), made on the device by build(n_eff, words, dst, st): it enqueues on `st` what writes bitmap m's
// words of the plan's n_eff rows at dst + m * words, dense.  masked_maps calls it where it would copy the table — after
// masked.dBlock is ensured and `st` is ordered behind the searches in flight — so a builder sees exactly the plan's snapshot
// (the predicate searches: ehx_where.cpp).
struct MaskTable {
  const uint32_t* p;
  uint64_t stride;
  uint32_t n_masks;
  bool host;
  // (last, with a default: MaskTable stays an aggregate under C++14's rules, so the brace-inits {p, stride, n_masks, host} of
  // the bitmap forms leave it empty)
  std::function<int(uint64_t, uint64_t, uint32_t*, hipStream_t)> build = nullptr;
};
// The bitmaps of one call, compacted: the call's ONE read of the row count, the rows the bitmaps cover below it, per mask the
// allowed rows before every tile (read back), their number and where its ascending list of allowed ids starts in
// masked.dList, and which mask every query is searched under.
struct MaskedPlan {
  uint64_t n_pub = 0, n_eff = 0, words = 0;   // words: of one bitmap below the row count, and the stride between two
  uint32_t n_tiles = 0, n_masks = 0;
  const uint32_t* d_maps = nullptr;           // where the bitmaps live on the device (masked_maps)
  std::vector<uint32_t> cum;                  // [n_masks][n_tiles + 1]
  std::vector<uint64_t> n_allowed;            // [n_masks]
  MaskedOffsets off = {};                     // list of mask m: masked.dList.p + off.off[m]
  const uint32_t* mask_of = nullptr;          // [queries], host memory, checked; nullptr: every query is mask 0
  std::vector<uint32_t> mask_of_read;         // ... of a table's device form
  const uint32_t* cum_of(uint32_t m) const { return cum.data() + (size_t)m * (n_tiles + 1); }
};
// an unsharded space, locked shared, scratch_mu held, its device current; everything is enqueued on `st`.  mask_of: in host
// memory and checked; or d_mask_of (a table's device form): read back with the allowed counts — the ONE wait of the
// compaction — and checked then, the outputs unwritten; or neither: every query is mask 0 and nothing is read back for it.
int masked_plan(ehx_space* s, hipStream_t st, const MaskTable& tab, uint64_t n_bits, size_t nq, const uint32_t* mask_of,
                const uint32_t* d_mask_of, MaskedPlan* p);
// The argument checks and the locked bodies of the three exact searches that take a table of bitmaps, as their entry points
// run them (an unsharded space, locked shared, scratch_mu held, its device current; everything is enqueued on `st`; mask_of /
// d_mask_of: masked_plan's) — the predicate searches (ehx_where.cpp) enter them with a table that is built, not copied.
// ehx_knn_masked_multi* (ehx_masked.cpp):
int masked_table_check(const ehx_space* s, size_t nq, uint32_t k, const void* q, const void* masks, uint32_t n_masks,
                       uint64_t n_bits, const void* mask_of, const void* o_ids, const void* o_dist, const void* o_cnt);
int masked_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, const MaskTable& tab,
                  uint64_t n_bits, const uint32_t* mask_of, const uint32_t* d_mask_of, const ResultBlock& out);
// ehx_knn_grouped_masked* (ehx_groupedm.cpp):
int groupedm_check(const ehx_space* s, size_t nq, uint32_t k, uint32_t per_group, const void* q, const void* group_of,
                   uint64_t n_labels, const void* masks, uint32_t n_masks, uint64_t n_bits, const void* mask_of,
                   const void* o_ids, const void* o_dist, const void* o_cnt);
int groupedm_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, uint32_t per_group,
                    const uint32_t* group_of, bool labels_on_host, uint64_t n_labels, const MaskTable& tab, uint64_t n_bits,
                    const uint32_t* mask_of, const uint32_t* d_mask_of, const ResultBlock& out);
// ehx_range_masked* (ehx_rangem.cpp):
int rangem_check(const ehx_space* s, size_t nq, uint32_t max_results, const void* q, const void* radius, const void* masks,
                 uint32_t n_masks, uint64_t n_bits, const void* mask_of, const void* o_ids, const void* o_dist,
                 const void* o_cnt);
int rangem_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, const float* d_radius, uint32_t max_results,
                  const MaskTable& tab, uint64_t n_bits, const uint32_t* mask_of, const uint32_t* d_mask_of,
                  const ResultBlock& out);
// ehx_graph_knn_masked_multi* (ehx_masked.cpp): the walk, the exact answer or both, by `route` and per mask
int graphm_table_check(const ehx_space* s, size_t nq, uint32_t k, const void* q, const void* masks, uint32_t n_masks,
                       uint64_t n_bits, const void* mask_of, uint32_t route, const void* o_ids, const void* o_dist,
                       const void* o_cnt);
int graphm_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, const MaskTable& tab,
                  uint64_t n_bits, const uint32_t* mask_of, const uint32_t* d_mask_of, uint32_t route, const ResultBlock& out);
// ---- ehx_where.cpp: what the searches under BUILT tables share (predicates; Boolean filters, ehx_filter.cpp) ----
constexpr uint64_t kAllRows = ~0ull;   // n_bits (and n_labels) of a built table: the call's snapshot alone bounds the rows
constexpr const char* kWhereWhy = "stored columns over shards are not built yet";
// the columns a build kernel reads: those SOME of the n_preds conjunctions names and that are live (the space locked at least
// shared)
WhereCols where_cols(const ehx_space* s, const ehx_pred* preds, uint32_t n_preds);
int check_group_col(uint32_t col);   // at or above EHX_MAX_COLUMNS: EHX_EINVAL
// groupedm_locked under a built table, the stored column group_col of the whole prefix as its labels, read where it lies
int grouped_built_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, uint32_t per_group,
                         uint32_t group_col, const MaskTable& tab, const uint32_t* mask_of, const uint32_t* d_mask_of,
                         const ResultBlock& out);
// what the builders' test hooks share: the builder alone under the search's locks, as masked_maps runs it — the snapshot
// into *out_n, the table built behind masked.dBlock's head — then then(n_pub, words, table, stream), unless the space is empty
int built_table_hook(ehx_space* s, const char* what, const MaskTable& tab, uint64_t* out_n,
                     const std::function<int(uint64_t, uint64_t, uint32_t*, hipStream_t)>& then);
// What the exact answer needs of compacted per-query row filters, whatever they were compacted from: a table of bitmaps
// (masked_answer, ehx_masked.cpp) or the wanted labels of a label column (ehx_labeled.cpp).  Host arrays unless named d_.
struct FilterView {
  uint64_t n_pub = 0, n_eff = 0, list_rows = 0;   // list_rows: entries of d_list the filters' lists hold together
  uint32_t n_tiles = 0, n_filters = 0;
  const uint64_t* n_allowed = nullptr;   // [n_filters] rows the filter allows
  const uint64_t* off = nullptr;         // [n_filters] its list: d_list + off[f] (ascending where the filter scans)
  const uint32_t* filter_of = nullptr;   // [queries] checked; nullptr: every query is filter 0
  const char* scans = nullptr;           // [n_filters] the filter takes the scan route (filter_scan_serves and the cut)
  const uint32_t* cum = nullptr;         // [rows][n_tiles + 1] allowed rows before every tile, of the filters that scan
  const uint32_t* scan_of = nullptr;     // [n_filters] the filter's row of cum and of the samples; nullptr: f itself
  const uint64_t* d_list = nullptr;
  const DevBuf<uint64_t>* sample = nullptr;   // [rows][256], filled by samples()
  std::function<int()> samples;          // enqueues the scanning filters' samples (the scan route's stage 0 alone pays)
  // the row test in the int8 scan's flush (RadiusKnn's allow fields); where it is per query, d_head is the head of the
  // block — kTabWords words, rewritten for every device batch — and head_of[f] the word of a query under filter f
  const uint32_t* allow = nullptr;
  bool allow_per_query = false, allow_label = false;
  uint32_t* d_head = nullptr;
  const uint32_t* head_of = nullptr;
  // the list route: a filter that at least shared_min queries of the batch name takes the shared-list kernel over their
  // range; the others go through ONE per-query launch together, their [start | end) in d_range.  1: every filter shares.
  uint32_t shared_min = 1;
  DevBuf<uint64_t>* d_range = nullptr;
  std::atomic<uint64_t>* ctr = nullptr;  // [5] scan route, list route, overflowed, scan passes, calls (the caller counts calls)
};
bool filter_scan_serves(const ehx_space* s, uint32_t k, uint64_t n_pub);   // the scan route serves this k on this prefix
// THE route of a filter in every filtered search, in two steps (colindex_plan restricts the scanning filters between them);
// the caller says which scan_serves, which cut (masked_exact_cut, or a forced 0 / ~0) and which gate (0, kLargeKMinQueries).
//   cut    scans[f] = scan_serves && n_allowed[f] > cut
//   gate   min_scan_queries > 0 and fewer queries name scanning filters (all of them together): none scans; filter_of ==
//          nullptr: every query is filter 0
void filter_routes_cut(bool scan_serves, uint64_t cut, const uint64_t* n_allowed, uint32_t n_filters, char* scans);
void filter_routes_gate(const uint32_t* filter_of, size_t nq, size_t min_scan_queries, uint32_t n_filters, char* scans);
// The view over a plan of bitmaps, every field but ctr.  It BORROWS p, scans[p.n_masks] (the caller's routes) and
// head_of[p.n_masks] (the caller's storage, filled here): all three outlive it.  st: where v.samples() enqueues.
FilterView masked_view(ehx_space* s, hipStream_t st, const MaskedPlan& p, const char* scans, uint32_t* head_of);
int filtered_answer(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, const FilterView& v,
                    const ResultBlock& out);

// ---- ehx_grouped.cpp ----
// the checks every grouped entry point starts with, with their codes and in their order; the caller appends its own
int grouped_check_head(const ehx_space* s, size_t nq, uint32_t k, uint32_t per_group, const void* q, const void* group_of,
                       uint64_t n_labels, const void* o_ids, const void* o_dist, const void* o_cnt);
int grouped_check_ld(const ehx_space* s);   // rows wider than grouped_rerank_max_ld() floats: EHX_EUNSUPPORTED
// the grouped scan route serves a prefix of n_eff rows: a flat space with plain rows whose int8 scan serves a radius on it
bool grouped_scan_serves(const ehx_space* s, uint64_t n_eff);
// The grouped list route, any space kind: query j over d_list[range[j], range[nq + j]) (range: host memory; d_list ==
// nullptr: the identity list, the range is of row ids), in slabs of kPoolCap.  count_queries: its queries are not in
// n_queries yet.
int grouped_list(ehx_space* s, hipStream_t st, uint64_t n_eff, const uint64_t* d_list, const uint64_t* range, size_t nq,
                 const float* d_queries, uint32_t k, uint32_t per_group, const uint32_t* d_group_of, uint64_t* d_ids,
                 float* d_dist, uint32_t* d_count, bool count_queries);
// The grouped answer over compacted per-query row filters, whatever they were compacted from — nothing (one filter that
// allows the prefix, a null d_list), a table of bitmaps, the wanted labels of a column.  Of v it reads n_pub, n_eff,
// n_filters, n_allowed, off, filter_of, scans, d_list, allow*, d_head, head_of and ctr.
int grouped_answer(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, uint32_t per_group,
                   const uint32_t* d_group_of, const FilterView& v, const ResultBlock& out);

// ---- ehx_labeled.cpp ----
// The label column of one device batch, compacted for the batch's distinct wanted labels ("slots"): the slot of every query,
// per slot its rows in the prefix and where its list starts in masked.dList, which slots scan, and the scanning slots' rows
// before every tile.  On the device behind it: the table and the lists (masked.dList: ascending where the slot scans), the
// scanning slots' prefixes (masked.dCum), their lists' starts by scanning index (labeled.dOff + kLabeledMaxSlots), and —
// where some slot scans — the column behind the head of labeled.dBlock.
struct LabeledPlan {
  uint32_t n_tiles = 0, n_slots = 0, n_scan = 0;
  uint64_t total = 0;                     // entries of masked.dList the lists hold together
  std::vector<uint32_t> table, slot_of;   // [n_slots] the wanted labels, ascending | [queries] the slot of every query
  std::vector<uint64_t> n_allowed, off;   // [n_slots]
  std::vector<char> scans;                // [n_slots]
  std::vector<uint32_t> scan_of;          // [n_slots] the slot's row of cum (kLabeledNoScan: it does not scan)
  std::vector<uint32_t> cum;              // [n_scan][n_tiles + 1]
};
// an unsharded space, locked shared, scratch_mu held, its device current, `st` ordered behind the searches in flight;
// everything is enqueued on `st`.  m <= kSideChunk queries under want[0, m) (host memory) over d_label_of[0, n_eff).  Waits
// once for the counts, and a second time — for the tile prefixes — only where some slot scans.  A slot scans iff scan_serves
// and it has more than `cut` rows — and, with min_scan_queries, only if at least that many queries of the batch name such
// slots (else none scans).  *col_copied: the column's copy is in place (made once per call, and only where some slot scans).
int labeled_plan(ehx_space* s, hipStream_t st, uint64_t n_eff, size_t m, const uint32_t* d_label_of, const uint32_t* want,
                 bool scan_serves, uint64_t cut, size_t min_scan_queries, bool* col_copied, LabeledPlan* p);

// the slots of a device batch: p->table (the distinct wanted labels, ascending), p->n_slots, p->slot_of
void labeled_slots(const uint32_t* want, size_t m, LabeledPlan* p);
// The view over a device batch's plan, every field but ctr; ix: the plan was read from a stored column's index (lists, tile
// prefixes, samples and the flush's block are the index's).  It BORROWS p and *ix: both outlive it.  st: as masked_view's.
FilterView labeled_view(ehx_space* s, hipStream_t st, uint64_t n_pub, uint64_t n_eff, const LabeledPlan& p,
                        const ehx_space::ColIndex* ix);
// How a call under a label column names its column and its wanted labels, and what its search passes the plan.
struct LabelCall {
  const uint32_t* label_of;   // the column on the device, or with on_host in host memory (staged in labeled.dCol); unused
  bool on_host;               // with label_col >= 0: the space's stored column of that number
  int label_col;
  uint64_t n_labels;          // entries of the column (a stored one: the row count's snapshot)
  const uint32_t *want, *d_want;   // [queries] host memory; or device memory, read back once (the call's one wait for it)
  bool scan_serves = false;   // labeled_plan's routing inputs
  uint64_t cut = 0;
  size_t min_scan_queries = 0;
  int (*fits)(const ehx_space*) = nullptr;   // refuses rows the search cannot hold
  std::atomic<uint64_t>* ctr = nullptr;      // [5] FilterView's
};
// The body of every call under a label column (an unsharded space, locked shared, scratch_mu held, its device current;
// everything is enqueued on `st`; n_pub: the call's ONE read of the row count): poison check, c.fits, the calls counter, the
// plan's scratch, `st` ordered behind the searches in flight, a stored column's index, stage() (may be empty), a host column
// staged, d_want read back; then per device batch [q0, q0 + m) the plan, its view (ctr set) and batch(q0, m, view).
int labeled_call(ehx_space* s, hipStream_t st, uint64_t n_pub, size_t nq, const LabelCall& c, const std::function<int()>& stage,
                 const std::function<int(size_t, size_t, FilterView&)>& batch);

// ---- ehx_columns.cpp ----
struct WriteBatch;
// The values a Set carries for stored columns: vals[c][i] for column cols[c] of the batch's row i (host memory).
struct ColumnWrite {
  uint32_t n_cols = 0;
  uint32_t cols[EHX_MAX_COLUMNS] = {};
  const uint32_t* vals[EHX_MAX_COLUMNS] = {};
  ColumnWrite from(size_t i) const {   // the batch without its first i rows
    ColumnWrite r = *this;
    for (uint32_t c = 0; c < n_cols; ++c) r.vals[c] += i;
    return r;
  }
};
// (wmu held, mu not) the columns cw names exist from here on: the first write of a column takes mu exclusively once
int columns_create(ehx_space* s, const ColumnWrite& cw);
// grow()'s group: every live column moved to `want` rows, the first `keep` kept, EHX_GROUP_NONE behind them
int grow_columns(ehx_space* s, uint64_t want, uint64_t keep, hipStream_t st);
// write_rows' step, enqueued on the writers' stream in front of the rows: EHX_GROUP_NONE into [old_n, next) of every live
// column, then cw's values (may be nullptr) by the rows' duplicate rule; a batch that touches committed rows bumps the
// generation of the columns it writes
int columns_land(ehx_space* s, hipStream_t ws, const WriteBatch& b, uint64_t old_n, uint64_t next, const ColumnWrite* cw);
// (scratch_mu held, the space locked shared, `st` ordered behind the searches in flight) the index of column `col` for the
// prefix of n_pub rows, rebuilt on `st` if it is stale
int colindex_ensure(ehx_space* s, hipStream_t st, uint32_t col, uint64_t n_pub, const ehx_space::ColIndex** out);
// labeled_plan's result read from an index instead of compacted: no device work.  p->cum stays empty — the tile prefixes
// are ix.cum, p->scan_of[f] their row (and the samples') for the slots that scan
void colindex_plan(const ehx_space::ColIndex& ix, size_t m, const uint32_t* want, bool scan_serves, uint64_t cut,
                   size_t min_scan_queries, LabeledPlan* p);
// device pointer to the prefix [0, n_pub) of a stored column as a group column (never written: EHX_GROUP_NONE for every
// row, made on `st`); scratch_mu held
int column_as_groups(ehx_space* s, hipStream_t st, uint32_t col, uint64_t n_pub, const uint32_t** out);

// ---- ehx_among.cpp ----
// exact kNN among row ids on an unsharded space, locked shared, scratch_mu held, its device current (d_off == nullptr: one
// list shared by every query; max_list: an upper bound of one list's length, 0 = n_cand)
// count_queries = false: a stage of a larger search (the masked kNN's sample) — its pairs are counted, its queries are not
// d_end (with d_off): query q's list is d_ids[d_off[q], d_end[q]) — queries may share a list — and end_pairs those lists'
// lengths together; the public among entry points never pass it
int among_locked(ehx_space* s, hipStream_t st, size_t nq, const float* d_queries, uint32_t k, const uint64_t* d_ids,
                 const uint64_t* d_off, size_t n_cand, size_t max_list, uint64_t* d_out_ids, float* d_out_dist,
                 uint32_t* d_out_count, bool count_queries = true, const uint64_t* d_end = nullptr, uint64_t end_pairs = 0);

// ---- ehx_write.cpp ----
int sync_stream(ehx_space* s, hipStream_t st);
int refresh_derived_copies(ehx_space* s, uint64_t row0, uint64_t n, hipStream_t st, bool exclusive, uint64_t n_after);
// Where the rows of a Set come from: host floats [n][dims], staged and uploaded (ehx_set_batch), or a dense [*][dims] matrix
// in device memory, scattered by scatter_rows_kernel (ehx_set_batch_device).
struct RowSource {
  const float* host = nullptr;
  const void* dev = nullptr;       // device rows, EHX_DTYPE_F32 or EHX_DTYPE_F16 (dtype), on `device`
  int dtype = EHX_DTYPE_F32;
  int device = 0;
  hipEvent_t ready = nullptr;      // recorded behind the work that produced them: the writers' stream waits for it
  const uint32_t* idx = nullptr;   // device rows of a shard: the positions of its rows in the batch (nullptr: 0, 1, ...)
  size_t elem_bytes() const { return dtype == EHX_DTYPE_F16 ? sizeof(_Float16) : sizeof(float); }
  RowSource from(size_t i, uint32_t dims) const {   // the batch without its first i rows
    RowSource r = *this;
    if (host) r.host = host + i * dims;
    else r.dev = (const char*)dev + i * dims * elem_bytes();
    return r;
  }
};
// the body of ehx_set_batch and ehx_set_batch_device: locking, the append-only fast path, graph batches that rewrite keys
// (cw: the values of stored columns the rows carry, ehx_set_batch_cols; nullptr: none)
int set_batch_from(ehx_space* s, size_t n, const char* const* keys, const size_t* klens, const RowSource& src,
                   const ColumnWrite* cw = nullptr);
bool is_dense_run(const uint64_t* ids, size_t n);   // ids[i] == ids[0] + i for every i
// What a batch of row ids touches, host arithmetic only, computed once per batch by write_batch from the ids and the published
// row count `old_n` (ids == nullptr: the generator's rows old_n, old_n + 1, ...).
struct WriteBatch {
  const uint64_t* ids = nullptr;
  size_t n = 0;
  uint64_t lo = ~0ull, hi = 0;      // the touched id range (an empty batch: the identities of min and max)
  bool dense_run = true;            // one run of ids
  bool touches_committed = false;   // some id < old_n: a published row is rewritten in place
  bool all_appended = false;        // the run old_n, old_n + 1, ...: a pure append of fresh, distinct keys
};
WriteBatch write_batch(const uint64_t* ids, size_t n, uint64_t old_n);
// the write path behind every Set (new_keys == nullptr: a shard's rows, whose parent publishes the keys); invariants at its head
int write_rows(ehx_space* s, const WriteBatch& b, uint64_t next, const RowSource& src, std::vector<std::string>* new_keys,
               bool append_only, const ColumnWrite* cw = nullptr);
// new_keys (moved from) become the keys of rows old_n, old_n + 1, ...; under kmu
void publish_keys(ehx_space* s, uint64_t old_n, std::vector<std::string>& new_keys);
// The duplicate rule of a parallel scatter: out[i] = ids[i] for the LAST occurrence of every id, ~0 for the ones before it —
// a key given twice in one batch keeps its last row, as the host path's in-order copies leave it.
void last_writers(const uint64_t* ids, size_t n, uint64_t* out);
// the generator's rows through the same tail (the space locked exclusively by the caller)
int fill_synthetic_locked(ehx_space* s, uint64_t seed, uint64_t row0, uint64_t n_rows, int normalize, uint64_t stride,
                          uint32_t latent = 0);

// ---- ehx_shards.cpp ----
int sharded_set_batch(ehx_space* p, size_t n, const char* const* keys, const size_t* klens, const RowSource& src);
int sharded_fill_synthetic(ehx_space* p, uint64_t seed, uint64_t row0, uint64_t n_rows, int normalize, uint32_t latent = 0);
int sharded_knn(ehx_space* p, size_t nq, const float* h_queries, const float* d_queries, int qdev, uint32_t k,
                uint64_t* out_ids, float* out_dist, uint32_t* out_count, bool out_on_device, hipStream_t caller_stream);
// the same with the parent's scratch_mu already held by the caller
int sharded_knn_locked(ehx_space* p, size_t nq, const float* h_queries, const float* d_queries, int qdev, uint32_t k,
                       uint64_t* out_ids, float* out_dist, uint32_t* out_count, bool out_on_device,
                       hipStream_t caller_stream);

}  // namespace ehx_impl
