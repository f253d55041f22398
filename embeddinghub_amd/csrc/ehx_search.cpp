// Search entry points: ehx_knn_device, ehx_knn from host pointers (four routes behind the request combiner), key lookups,
// top-k merge of shard lists.
#include "ehx_internal.h"

// A search that finds an exclusive writer waiting for the space's lock lets it in first: the caller holds no lock here, and
// the wait is bounded (50 ms), so it can delay a search and never block one.  Once the writer has the lock the search
// queues behind it on the lock itself.  (50 us per step, 50 ms in all: chosen, not measured.  With no writer waiting the
// cost is one atomic load per call.)
void ehx_impl::yield_to_writer(const ehx_space* s) {
  for (int i = 0; i < 1000 && s->excl_waiting.load(std::memory_order_acquire) != 0; ++i)
    std::this_thread::sleep_for(std::chrono::microseconds(50));
}

// ---- neighbours of rows the space holds (ehx_knn_by_keys, ehx_knn_by_ids_device) ----
// The query batch never leaves the device: gather_rows_kernel reads it from the stored rows (the bytes Get returns), the
// space's own pipeline searches it with k + 1, drop_self_kernel removes every row from its own list (k_bykey.hip).
struct ByKeyScratch {   // carved from ehx_space::dByOut (scratch_mu)
  ResultBlock l;        // [n][k + 1] lists of the k + 1 search
  uint32_t* valid;      // [n]
  ResultBlock out;      // [n][k] a host call's results (host_out)
};

static int by_scratch(ehx_space* s, size_t n, uint32_t k, bool host_out, ByKeyScratch* b) {
  const size_t o_valid = ResultBlock::bytes(n, k + 1, false);
  const size_t o_out = round_up(o_valid + n * sizeof(uint32_t), 8);
  int rc;
  if ((rc = s->by.dByQ.ensure(n * s->dims)) || (rc = s->by.by_ev.ensure(hipEventDisableTiming)) ||
      (rc = s->by.dByOut.ensure(o_out + (host_out ? ResultBlock::bytes(n, k, false) : 0))))
    return rc;
  unsigned char* p = s->by.dByOut.p;
  b->l = ResultBlock::at(p, n, k + 1, false);
  b->valid = (uint32_t*)(p + o_valid);
  b->out = host_out ? ResultBlock::at(p + o_out, n, k, false) : ResultBlock{};
  return EHX_OK;
}

static int by_drop_self(const ByKeyScratch& b, hipStream_t st, size_t n, const uint64_t* d_row_ids, uint32_t k,
                        uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count) {
  DropSelfArgs d;
  d.ids = b.l.ids;
  d.dist = b.l.dist;
  d.count = b.l.cnt;
  d.row_ids = d_row_ids;
  d.valid = b.valid;
  d.out_ids = d_out_ids;
  d.out_dist = d_out_dist;
  d.out_count = d_out_count;
  d.n = (uint32_t)n;
  d.k = k;
  HIP_TRY(launch_drop_self(d, st));
  return EHX_OK;
}

// an unsharded space, locked shared, scratch_mu held, its device current; everything is enqueued on `st`
static int by_ids_locked(ehx_space* s, hipStream_t st, size_t n, const uint64_t* d_row_ids, uint32_t k,
                         const ByKeyScratch& b, uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count) {
  int rc;
  if ((rc = check_not_poisoned(s))) return rc;
  // (the last call's launches — on whatever stream it was given — have read and written this scratch)
  HIP_TRY(hipStreamWaitEvent(st, s->by.by_ev, 0));
  // the ONE read of the row count: the gather's range check and the flat chain's passes answer for the same prefix
  const uint64_t n_pub = s->n.load(std::memory_order_acquire);
  GatherRowsArgs g = {};
  g.row_ids = d_row_ids;
  g.rows = rows_view(s, n_pub);
  g.bases.p[0] = g.rows.X;
  g.out = s->by.dByQ.p;
  g.valid = b.valid;
  g.n = (uint32_t)n;
  g.G = 1;
  HIP_TRY(launch_gather_rows(g, st));
  if (n_pub > 0)   // (an empty space: every query is invalid, the lists are never read)
    rc = knn_device_locked(s, st, n, s->by.dByQ.p, k + 1, b.l.ids, b.l.dist, b.l.cnt, n_pub);
  if (!rc) rc = by_drop_self(b, st, n, d_row_ids, k, d_out_ids, d_out_dist, d_out_count);
  (void)hipEventRecord(s->by.by_ev, st);
  return rc;
}

int ehx_impl::parent_gather_view(ehx_space* p, uint64_t n_pub, std::vector<std::shared_lock<std::shared_mutex>>* held,
                                 GatherRowsArgs* g) {
  const size_t G = p->shards.size();
  const int home = p->shards[0]->device;
  if (G > kMaxShardBases) return fail(EHX_EUNSUPPORTED, "%zu shards exceed %u", G, kMaxShardBases);
  if (!engine().peer_all)
    for (ehx_space* c : p->shards)
      if (c->device != home)
        return fail(EHX_EUNSUPPORTED, "space '%s': device %d has no peer access to device %d (EHX_ALLOW_NO_PEER): the rows "
                                      "of a key batch are gathered over it", p->name.c_str(), home, c->device);
  held->reserve(G);
  for (size_t i = 0; i < G; ++i) {
    ehx_space* c = p->shards[i];
    held->emplace_back(c->mu);
    if (c->dropped) return fail(EHX_ENOTFOUND, "Not found");
    if (int rcp = check_not_poisoned(c)) return rcp;
    g->bases.p[i] = c->rows.dX.p;
  }
  g->rows = rows_view(p->shards[0], n_pub);   // (shape and layout are the shards'; the rows: bases)
  g->G = (uint32_t)G;
  return EHX_OK;
}

// a row-sharded parent, locked shared, its scratch_mu held, shard 0's device current: gathered over peer access into the
// parent's scratch, searched by every shard, merged and trimmed on shard 0's device (on the parent's stream)
static int sharded_by_ids_locked(ehx_space* p, size_t n, const uint64_t* d_row_ids, uint32_t k, const ByKeyScratch& b) {
  const int home = p->shards[0]->device;
  const uint64_t n_pub = p->n.load(std::memory_order_acquire);
  {
    // held until the gather has read the rows
    std::vector<std::shared_lock<std::shared_mutex>> held;
    GatherRowsArgs g = {};
    if (int rcv = parent_gather_view(p, n_pub, &held, &g)) return rcv;
    g.row_ids = d_row_ids;
    g.out = p->by.dByQ.p;
    g.valid = b.valid;
    g.n = (uint32_t)n;
    HIP_TRY(launch_gather_rows(g, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
  }
  int rc = sharded_knn_locked(p, n, nullptr, p->by.dByQ.p, home, k + 1, b.l.ids, b.l.dist, b.l.cnt, true, p->stream);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(home));
  return by_drop_self(b, p->stream, n, d_row_ids, k, b.out.ids, b.out.dist, b.out.cnt);
}

// ---- ehx_knn from host pointers: knn_host_direct and its four routes ----
// The host-coherent pinned block of the one-launch routes: the kernel reads the raw query from it, writes the answer into
// it and raises the flag (zeroed at creation: no sequence number is ever 0); created on the space's device on first use.
constexpr size_t kOneQ = 16384;   // query slot (ld <= 4096 floats)
struct OneLaunchBlock {
  char query[kOneQ];
  uint64_t ids[64];
  float dist[64];
  uint32_t count;
  char pad0[252];
  uint32_t done_flag;
  char pad1[1020];
};
static_assert(offsetof(OneLaunchBlock, ids) == kOneQ && offsetof(OneLaunchBlock, dist) == kOneQ + 512 &&
                  offsetof(OneLaunchBlock, count) == kOneQ + 768 && offsetof(OneLaunchBlock, done_flag) == kOneQ + 1024 &&
                  sizeof(OneLaunchBlock) == kOneQ + 2048,
              "the one-launch kernels are handed these addresses");

static int one_launch_block(ehx_space* s, OneLaunchBlock** h) {
  int rc = s->one.hOnePin.ensure(sizeof(OneLaunchBlock), hipHostMallocCoherent | hipHostMallocMapped, true);
  *h = (OneLaunchBlock*)s->one.hOnePin.p;
  return rc;
}

static uint32_t one_launch_next_seq(ehx_space* s) {   // never 0: the block starts zeroed
  if (++s->one_seq == 0) ++s->one_seq;
  return s->one_seq;
}

// spins on the flag the kernel's last wave raises (~ tens of milliseconds at most), then asks the runtime
static int one_launch_wait(ehx_space* s, const uint32_t* done_flag, uint32_t seq, const char* what) {
  volatile const uint32_t* flag = done_flag;
  for (uint32_t spin = 0; *flag != seq && spin < 4000000u; ++spin) __builtin_ia32_pause();
  if (*flag != seq) {
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (*flag != seq) return fail(EHX_EINTERNAL, "%s finished without publishing its result", what);
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return EHX_OK;
}

// ... and the k results out of the block
static int one_launch_collect(ehx_space* s, const OneLaunchBlock* h, uint32_t seq, const char* what, uint32_t k,
                              uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (int rc = one_launch_wait(s, &h->done_flag, seq, what)) return rc;
  memcpy(out_ids, h->ids, k * sizeof(uint64_t));
  memcpy(out_dist, h->dist, k * sizeof(float));
  out_count[0] = h->count;
  s->n_one_launch += 1;
  return EHX_OK;
}

// ONE query against a small flat shard — the reference's request (server.cc:172-210; BASELINE configs[0]): a single
// launch reads the query from host-visible memory, scans every row in the oracle's arithmetic, and the last workgroup
// writes the answer into host-visible memory and raises a flag this thread spins on (k_flat.hip: single_query_kernel).
// 10 k x 128: ~130 us through the three-launch path -> see DESIGN §e.
// Locks: the space shared and scratch_mu on entry; takes none.  n_pub: the call's one read of the row count.
static int host_one_launch_flat(ehx_space* s, uint64_t n_pub, const float* query, uint32_t k, uint64_t* out_ids,
                                float* out_dist, uint32_t* out_count) {
  int rc;
  OneLaunchBlock* h;
  if ((rc = one_launch_block(s, &h))) return rc;
  if ((rc = s->one.dOneTicket.ensure_zeroed_once(1))) return rc;
  const uint32_t rpb = (uint32_t)std::max<uint64_t>(64, ((n_pub + 1023) / 1024 + 63) / 64 * 64);  // <= 1024 workgroups
  const uint32_t n_blocks = (uint32_t)((n_pub + rpb - 1) / rpb);
  if ((rc = s->one.dOnePart.ensure((size_t)n_blocks * 64))) return rc;
  test_pause();
  if ((rc = wait_searches_in_flight(s, s->stream))) return rc;  // (device searches queued on other streams)
  memcpy(h->query, query, s->dims * sizeof(float));
  SingleQueryArgs a;
  a.q_in = (const float*)h->query;
  a.rows = rows_view(s, n_pub);
  a.part = s->one.dOnePart.p;
  a.ticket = s->one.dOneTicket.p;
  a.out_ids = h->ids;
  a.out_dist = h->dist;
  a.out_count = &h->count;
  a.done_flag = &h->done_flag;
  a.seq = one_launch_next_seq(s);
  a.rows_per_block = rpb;
  a.k = k;
  HIP_TRY(launch_single_query(a, n_blocks, s->stream));
  if ((rc = one_launch_collect(s, h, a.seq, "single-query kernel", k, out_ids, out_dist, out_count))) return rc;
  s->n_queries += 1;
  s->n_exhaustive += 1;
  s->n_dist += n_pub;
  return EHX_OK;
}

// ... and in GRAPH mode (round 5; the reference's own index and request: HNSW, one query per NearestNeighbor RPC): the
// graph search kernel reads the raw query from host-visible memory, prepares it itself, walks the graph (one wave) and
// writes the answer into host-visible memory — one launch instead of prepare + search + two copies.
// Locks: the space shared and scratch_mu on entry; takes none.
static int host_one_launch_graph(ehx_space* s, const float* query, uint32_t k, uint64_t* out_ids, float* out_dist,
                                 uint32_t* out_count) {
  int rc;
  OneLaunchBlock* h;
  if ((rc = one_launch_block(s, &h))) return rc;
  memcpy(h->query, query, s->dims * sizeof(float));
  GraphOneLaunch one;
  one.q_host = (const float*)h->query;
  one.done_flag = &h->done_flag;
  one.seq = one_launch_next_seq(s);
  if ((rc = knn_graph_locked(s, s->stream, 1, nullptr, k, h->ids, h->dist, &h->count, &one))) return rc;
  return one_launch_collect(s, h, one.seq, "graph search kernel", k, out_ids, out_dist, out_count);
}

// A small call (the reference's request shape: one query, ten keys) is all fixed cost: its queries go through a pinned
// staging buffer (an asynchronous copy instead of the runtime's pageable-memory path) and its three result arrays come
// back as ONE block into pinned memory instead of three blocking copies.
// Locks: the space shared and scratch_mu on entry; takes none.
constexpr size_t kSmallCall = 32u << 10;   // queries and results of at most this many bytes each
static int host_small_call(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint64_t* out_ids,
                           float* out_dist, uint32_t* out_count) {
  int rc;
  const size_t qbytes = n_queries * s->dims * sizeof(float);
  if ((rc = s->scr.dQraw.ensure(n_queries * s->dims)) || (rc = s->scr.hSmallPin.ensure(2 * kSmallCall)) ||
      (rc = s->scr.dSmallOut.ensure(kSmallCall / sizeof(uint64_t))))
    return rc;
  const ResultBlock out = ResultBlock::at((unsigned char*)s->scr.dSmallOut.p, n_queries, k, false);
  memcpy(s->scr.hSmallPin.p, queries, qbytes);
  HIP_TRY(hipMemcpyAsync(s->scr.dQraw.p, s->scr.hSmallPin.p, qbytes, hipMemcpyHostToDevice, s->stream));
  if ((rc = knn_device_locked(s, s->stream, n_queries, s->scr.dQraw.p, k, out.ids, out.dist, out.cnt))) return rc;
  char* h = s->scr.hSmallPin.p + kSmallCall;
  if ((rc = out.copy_block_out(s->stream, h))) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  out.unpack(h, out_ids, out_dist, out_count);
  return EHX_OK;
}

// A call's hold of one of the space's host slots (ehx_space::HostSlot): waits for a free one; gives it back when the call
// ends, and unless the call succeeded drains what it may have left in flight before the slot's pinned and device buffers go
// to the next caller.  Takes hs_mu for the hand-over only.
struct HostSlotHold {
  ehx_space* s;
  ehx_space::HostSlot* h = nullptr;
  bool ok = false;   // set on the success path; an early error return may leave copies / kernels of this call in flight
  explicit HostSlotHold(ehx_space* sp) : s(sp) {
    std::unique_lock<std::mutex> hl(s->hs_mu);
    s->hs_cv.wait(hl, [&] {
      for (auto& c : s->hslot)
        if (!c.busy) {
          h = &c;
          return true;
        }
      return false;
    });
    h->busy = true;
  }
  HostSlotHold(const HostSlotHold&) = delete;
  ~HostSlotHold() {
    if (!ok) {
      if (h->st) (void)hipStreamSynchronize(h->st);
      if (s->stream) (void)hipStreamSynchronize(s->stream);
    }
    {
      std::lock_guard<std::mutex> hl(s->hs_mu);
      h->busy = false;
    }
    s->hs_cv.notify_one();
  }
};

// A batch: through a slot of its own — only the device pipeline itself is serialised (the pipeline's lock is NOT held while
// the queries are staged: the first version took it on entry and two callers ran strictly one after the other).
// Locks: the space shared on entry.  Takes, in this order and never two at once: a host slot (hs_mu for the hand-over); for
// the pipelined int8 stage one int8 scratch set's mutex, from the enqueue to the outcome (i8_enqueue_mu inside the enqueue);
// then scratch_mu around what is left of the chain.
static int host_slot_batch(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint64_t* out_ids,
                           float* out_dist, uint32_t* out_count) {
  int rc;
  HostSlotHold hold(s);
  ehx_space::HostSlot* hs = hold.h;
  const size_t qbytes = n_queries * s->dims * sizeof(float), out_bytes = ResultBlock::bytes(n_queries, k, false);
  if ((rc = hs->st.ensure(hipStreamNonBlocking)) || (rc = hs->in_ev.ensure(hipEventDisableTiming)) ||
      (rc = hs->done_ev.ensure(hipEventDisableTiming)))
    return rc;
  if (hs->pin.n < qbytes + out_bytes) {
    HIP_TRY(hipStreamSynchronize(hs->st));
    if ((rc = hs->pin.ensure(qbytes + out_bytes))) return rc;
  }
  if ((rc = hs->dq.ensure(n_queries * s->dims)) || (rc = hs->dout.ensure(out_bytes))) return rc;
  const ResultBlock out = ResultBlock::at(hs->dout.p, n_queries, k, false);
  char* const ho = hs->pin.p + qbytes;   // the results' pinned block, behind the queries
  memcpy(hs->pin.p, queries, qbytes);
  HIP_TRY(hipMemcpyAsync(hs->dq.p, hs->pin.p, qbytes, hipMemcpyHostToDevice, hs->st));
  HIP_TRY(hipEventRecord(hs->in_ev, hs->st));
  // The int8 engine's first stage — all of a batch unless queries lose their certificate — runs in one of the space's two
  // scratch sets WITHOUT the pipeline-wide lock: this call's launches queue up on the space's stream behind the other
  // caller's while that one still waits for its verdict, so the scan kernels of consecutive batches run back to back with
  // no host round trip (launches, verdict copy, thread wake-up: ~0.1 ms per batch) between them.  The queries a batch does
  // lose continue through the rest of the chain under the lock (rare).
  const bool pipe_on = env().host_pipeline;
  bool done = false;   // answered by the pipelined stage alone, the results on their way back
  I8Outcome o;
  // the ONE read of the row count in this call: the pipelined int8 stage and the rest of the chain answer for the same prefix
  const uint64_t n_pub = s->n.load(std::memory_order_acquire);
  const bool pipelined =
      pipe_on && s->params.mode == EHX_MODE_FLAT && k <= EHX_MAX_K && n_pub > 0 && resolve_engine(s, n_pub) == EHX_ENGINE_I8;
  if (pipelined) {
    const int set = (int)(s->i8_next_set.fetch_add(1, std::memory_order_relaxed) & 1u);   // consecutive batches alternate
    ehx_space::I8Set& sc = s->i8set[set];
    test_pause();
    std::lock_guard<std::mutex> l(sc.mu);
    if ((rc = i8_stage_enqueue(s, n_pub, set, s->stream, hs->in_ev, true, n_queries, hs->dq.p, k, out.ids, out.dist, out.cnt, &o))) return rc;
    // the results start their way back NOW, before the verdict is known (it is clean for all but a few batches in a
    // thousand): one host wait per batch instead of two in a row — verdict, then copy.  A batch that did lose queries runs
    // the rest of the chain below and copies again (same slot stream: in order, the later copy wins).
    // (it waits for the verdict's event — recorded right behind the re-rank and the 8-byte verdict copy; a marker of its own
    // cost the queue another ~6 us per batch)
    HIP_TRY(hipStreamWaitEvent(hs->st, sc.buf.verdict.ev, 0));
    if ((rc = out.copy_block_out(hs->st, ho))) return rc;
    HIP_TRY(hipEventSynchronize(sc.buf.verdict.ev));
    if ((rc = i8_stage_outcome(s, n_pub, set, s->stream, n_queries, k, &o))) return rc;
    done = o.failed.empty();
  }
  if (!done) {  // the whole chain, or what is left of it for the queries the stage above lost: under the pipeline lock
    {
      std::lock_guard<std::mutex> sl2(s->scratch_mu);
      HIP_TRY(hipStreamWaitEvent(s->stream, hs->in_ev, 0));
      if (pipelined) rc = flat_chain_rest(s, s->stream, n_pub, n_queries, hs->dq.p, k, out.ids, out.dist, out.cnt, EHX_ENGINE_I8, &o);
      else rc = knn_device_locked(s, s->stream, n_queries, hs->dq.p, k, out.ids, out.dist, out.cnt, n_pub);
      if (rc) return rc;
      HIP_TRY(hipEventRecord(hs->done_ev, s->stream));
    }
    HIP_TRY(hipStreamWaitEvent(hs->st, hs->done_ev, 0));
    if ((rc = out.copy_block_out(hs->st, ho))) return rc;
  }
  HIP_TRY(hipStreamSynchronize(hs->st));
  out.unpack(ho, out_ids, out_dist, out_count);
  hold.ok = true;
  return EHX_OK;
}

// ehx_knn behind its request combiner, and every call too large for it
static int knn_host_direct(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint64_t* out_ids,
                           float* out_dist, uint32_t* out_count) {
  if (!valid_space(s)) return fail(EHX_EINVAL, "space is NULL");
  if (n_queries == 0) return EHX_OK;
  if (!out_count) return fail(EHX_EINVAL, "out_count is NULL");
  if (k == 0) {
    for (size_t i = 0; i < n_queries; ++i) out_count[i] = 0;
    return EHX_OK;
  }
  if (!queries || !out_ids || !out_dist) return fail(EHX_EINVAL, "NULL argument");
  yield_to_writer(s);
  std::shared_lock<std::shared_mutex> rl(s->mu);
  if (s->dropped) return fail(EHX_ENOTFOUND, "Not found");
  if (is_parent(s)) return sharded_knn(s, n_queries, queries, nullptr, 0, k, out_ids, out_dist, out_count, false, nullptr);
  HIP_TRY(hipSetDevice(s->device));
  const size_t qbytes = n_queries * s->dims * sizeof(float), out_bytes = ResultBlock::bytes(n_queries, k, false);
  if (qbytes <= kSmallCall && out_bytes <= kSmallCall) {
    std::lock_guard<std::mutex> sl(s->scratch_mu);
    const uint64_t one_bytes = env().small_exact_bytes;
    const bool one_on = env().one_launch;
    const uint64_t n_pub = s->n.load(std::memory_order_acquire);   // (the one-launch routes' one read of the row count)
    if (one_on && n_queries == 1 && k <= 64 && s->params.mode == EHX_MODE_FLAT && s->scan_sel == EHX_SCAN_AUTO && n_pub > 0 &&
        s->ld <= 4096 && n_pub * s->ld * s->esz <= one_bytes)
      return host_one_launch_flat(s, n_pub, queries, k, out_ids, out_dist, out_count);
    if (one_on && n_queries == 1 && k <= 64 && s->params.mode == EHX_MODE_GRAPH && s->n > 0 && s->ld <= 4096)
      return host_one_launch_graph(s, queries, k, out_ids, out_dist, out_count);
    return host_small_call(s, n_queries, queries, k, out_ids, out_dist, out_count);
  }
  return host_slot_batch(s, n_queries, queries, k, out_ids, out_dist, out_count);
}

// Small calls (the reference's usage: one query per RPC, server.cc:172-210; Go Nearest, online.go:63) are coalesced by the
// space's request combiner (ehx_combine.h): one group = the oldest request's k, in arrival order, up to kCoalesceMaxBatch
// queries; requests with another k stay queued.  An uncontended call runs immediately; under load the batch size grows by
// itself with the scan time.
constexpr size_t kCoalesceMaxCall = 64;     // calls above this size already are batches
constexpr size_t kCoalesceMaxBatch = 1024;
typedef Combiner<ehx_space::KnnReq>::Group KnnGroup;

static KnnGroup knn_take(KnnGroup& queue) {
  KnnGroup group;
  const uint32_t gk = queue.front()->k;
  size_t total = 0;
  for (auto it = queue.begin(); it != queue.end();) {
    if ((*it)->k == gk && total + (*it)->nq <= kCoalesceMaxBatch) {
      total += (*it)->nq;
      group.push_back(*it);
      it = queue.erase(it);
    } else {
      ++it;
    }
  }
  return group;
}

// ONE device batch for the group (a group of one: straight through, no copy), the results handed back
static int knn_serve(ehx_space* s, const KnnGroup& group) {
  const uint32_t gk = group[0]->k;
  if (group.size() == 1) return knn_host_direct(s, group[0]->nq, group[0]->q, gk, group[0]->ids, group[0]->dist, group[0]->cnt);
  size_t total = 0;
  for (auto* r : group) total += r->nq;
  std::vector<float> q(total * s->dims), dist(total * gk);
  std::vector<uint64_t> ids(total * gk);
  std::vector<uint32_t> cnt(total);
  size_t off = 0;
  for (auto* r : group) {
    memcpy(q.data() + off * s->dims, r->q, r->nq * s->dims * sizeof(float));
    off += r->nq;
  }
  const int rc = knn_host_direct(s, total, q.data(), gk, ids.data(), dist.data(), cnt.data());
  off = 0;
  for (auto* r : group) {
    if (rc == EHX_OK) {
      memcpy(r->ids, ids.data() + off * gk, r->nq * gk * sizeof(uint64_t));
      memcpy(r->dist, dist.data() + off * gk, r->nq * gk * sizeof(float));
      memcpy(r->cnt, cnt.data() + off, r->nq * sizeof(uint32_t));
    }
    off += r->nq;
  }
  s->n_coalesced_batches += 1;
  s->n_coalesced_queries += total;
  return rc;
}

// keys of the rows a batch returned, packed into the caller's arena: key_off[i * k + j] .. key_off[i * k + j + 1] is the
// key of result j of query i (empty beyond out_count[i], or for a row without a key)
int ehx_impl::fill_key_arena(ehx_space* s, size_t n, uint32_t k, const uint64_t* out_ids, const uint32_t* out_count,
                          char* key_arena, size_t arena_cap, uint64_t* key_off) {
  uint64_t off = 0;
  std::string key;
  for (size_t i = 0; i < n; ++i) {
    for (uint32_t j = 0; j < k; ++j) {
      key_off[i * k + j] = off;
      if (j < out_count[i] && key_for_id(s, out_ids[i * k + j], &key) == EHX_OK) {
        if (off + key.size() > arena_cap) return fail(EHX_ERANGE, "key arena too small");
        memcpy(key_arena + off, key.data(), key.size());
        off += key.size();
      }
    }
  }
  key_off[n * k] = off;
  return EHX_OK;
}

extern "C" {

int ehx_knn_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                   uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count) {
  if (!valid_space(s)) return fail(EHX_EINVAL, "space is NULL");
  if (n_queries && k && (!d_queries || !d_out_ids || !d_out_dist || !d_out_count))
    return fail(EHX_EINVAL, "NULL device pointer");
  yield_to_writer(s);
  std::shared_lock<std::shared_mutex> rl(s->mu);
  if (s->dropped) return fail(EHX_ENOTFOUND, "Not found");
  if (is_parent(s)) {
    if (n_queries == 0 || k == 0) return EHX_OK;
    hipPointerAttribute_t at;
    HIP_TRY(hipPointerGetAttributes(&at, d_queries));
    return sharded_knn(s, n_queries, nullptr, d_queries, at.device, k, d_out_ids, d_out_dist, d_out_count, true,
                       (hipStream_t)stream);
  }
  std::lock_guard<std::mutex> sl(s->scratch_mu);
  HIP_TRY(hipSetDevice(s->device));
  return knn_device_locked(s, (hipStream_t)stream, n_queries, d_queries, k, d_out_ids, d_out_dist, d_out_count);
}

int ehx_knn(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint64_t* out_ids,
            float* out_dist, uint32_t* out_count) {
  if (!valid_space(s)) return fail(EHX_EINVAL, "space is NULL");
  if (n_queries == 0) return EHX_OK;
  if (n_queries > kCoalesceMaxCall || k == 0 || !queries || !out_ids || !out_dist || !out_count)
    return knn_host_direct(s, n_queries, queries, k, out_ids, out_dist, out_count);
  ehx_space::KnnReq me{{}, queries, n_queries, k, out_ids, out_dist, out_count};
  return s->knn_combiner.submit(me, knn_take, [s](const KnnGroup& g) { return knn_serve(s, g); }, g_err, sizeof(g_err));
}

int ehx_knn_keys(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint64_t* out_ids,
                 float* out_dist, uint32_t* out_count, char* key_arena, size_t arena_cap, uint64_t* key_off) {
  if (!key_off || (!key_arena && arena_cap)) return fail(EHX_EINVAL, "NULL argument");
  int rc = ehx_knn(s, n_queries, queries, k, out_ids, out_dist, out_count);
  if (rc) return rc;
  std::shared_lock<std::shared_mutex> rl(s->mu);
  if (s->dropped) return fail(EHX_ENOTFOUND, "Not found");
  return fill_key_arena(s, n_queries, k, out_ids, out_count, key_arena, arena_cap, key_off);
}

int ehx_knn_by_key(ehx_space* s, const char* key, size_t klen, uint32_t k, uint64_t* out_ids, float* out_dist,
                   uint32_t* out_count) {
  if (!valid_space(s) || !key || !out_count) return fail(EHX_EINVAL, "NULL argument");
  if (k > EHX_MAX_K_PAGED) return fail(EHX_EUNSUPPORTED, "k=%u exceeds %u", k, EHX_MAX_K_PAGED);  // (before k + 1, before any allocation)
  uint64_t id;
  std::vector<float> v(s->dims);
  {
    std::shared_lock<std::shared_mutex> rl(s->mu);
    if (s->dropped || lookup_key(s, key, klen, &id)) return fail(EHX_ENOTFOUND, "Not found");
  }
  int rc = ehx_get_by_id(s, id, v.data());  // Version::get(key), server.cc:195
  if (rc) return rc;
  const uint32_t kk = k + 1;               // server.cc:198
  std::vector<uint64_t> ids(kk);
  std::vector<float> dist(kk);
  uint32_t cnt = 0;
  if ((rc = ehx_knn(s, 1, v.data(), kk, ids.data(), dist.data(), &cnt))) return rc;
  // server.cc:205-207: erase own key if present, else drop the last
  uint32_t o = 0;
  bool removed = false;
  for (uint32_t j = 0; j < cnt; ++j) {
    if (!removed && ids[j] == id) {
      removed = true;
      continue;
    }
    if (o < k) {
      if (out_ids) out_ids[o] = ids[j];
      if (out_dist) out_dist[o] = dist[j];
      ++o;
    }
  }
  if (!removed && cnt == kk && o == k) { /* last one already dropped by the o<k bound */ }
  *out_count = o;
  return EHX_OK;
}

int ehx_knn_by_key_keys(ehx_space* s, const char* key, size_t klen, uint32_t k, uint64_t* out_ids, float* out_dist,
                        uint32_t* out_count, char* key_arena, size_t arena_cap, uint64_t* key_off) {
  if (!key_off || !out_count || (!key_arena && arena_cap)) return fail(EHX_EINVAL, "NULL argument");
  if (k > EHX_MAX_K_PAGED) return fail(EHX_EUNSUPPORTED, "k=%u exceeds %u", k, EHX_MAX_K_PAGED);
  std::vector<uint64_t> ids(k ? k : 1);
  int rc = ehx_knn_by_key(s, key, klen, k, ids.data(), out_dist, out_count);
  if (rc) return rc;
  std::shared_lock<std::shared_mutex> rl(s->mu);
  if (s->dropped) return fail(EHX_ENOTFOUND, "Not found");
  uint64_t off = 0;
  std::string nk;
  for (uint32_t j = 0; j < k; ++j) {
    key_off[j] = off;
    if (j < *out_count) {
      // (a returned row without a key cannot be answered as "": the RPC would hand back an empty neighbour key)
      if (key_for_id(s, ids[j], &nk) != EHX_OK)
        return fail(EHX_EINTERNAL, "row %llu was returned by the search but has no key", (unsigned long long)ids[j]);
      if (off + nk.size() > arena_cap) return fail(EHX_ERANGE, "key arena too small");
      memcpy(key_arena + off, nk.data(), nk.size());
      off += nk.size();
    }
    if (out_ids) out_ids[j] = j < *out_count ? ids[j] : ~0ull;
  }
  key_off[k] = off;
  return EHX_OK;
}

int ehx_knn_by_keys(ehx_space* s, size_t n, const char* const* keys, const size_t* klens, uint32_t k, uint64_t* out_ids,
                    float* out_dist, uint32_t* out_count, size_t* bad_index) {
  int rc = check_space_and_k(s, k, "k", true);   // (before k + 1, before any allocation)
  if (rc) return rc;
  if (n == 0) return EHX_OK;
  if (!out_count) return fail(EHX_EINVAL, "out_count is NULL");
  if (k == 0) {
    for (size_t i = 0; i < n; ++i) out_count[i] = 0;
    return EHX_OK;
  }
  if (!keys || !klens || !out_ids || !out_dist) return fail(EHX_EINVAL, "NULL argument");
  if ((rc = check_batch_size(n))) return rc;
  yield_to_writer(s);
  // ONE shared hold for key lookup, gather and search: the answer describes one state of the space
  std::shared_lock<std::shared_mutex> rl(s->mu);
  if (s->dropped) return fail(EHX_ENOTFOUND, "Not found");
  std::vector<uint64_t> ids;
  if ((rc = lookup_keys(s, n, keys, klens, &ids, bad_index))) return rc;
  ehx_space* home = is_parent(s) ? s->shards[0] : s;   // the device the batch is gathered, merged and trimmed on
  std::lock_guard<std::mutex> sl(s->scratch_mu);
  HIP_TRY(hipSetDevice(home->device));
  ByKeyScratch b;
  if ((rc = by_scratch(s, n, k, true, &b))) return rc;
  if ((rc = s->by.dByIds.ensure(n))) return rc;
  DrainUnlessOk drain{s->stream};
  // (pageable host memory: the runtime stages it before the call returns)
  HIP_TRY(hipMemcpyAsync(s->by.dByIds.p, ids.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, s->stream));
  if (is_parent(s)) rc = sharded_by_ids_locked(s, n, s->by.dByIds.p, k, b);
  else rc = by_ids_locked(s, s->stream, n, s->by.dByIds.p, k, b, b.out.ids, b.out.dist, b.out.cnt);
  if (rc) return rc;
  return drain.done(b.out.copy_out(s->stream, out_ids, out_dist, out_count, nullptr));
}

int ehx_knn_by_keys_keys(ehx_space* s, size_t n, const char* const* keys, const size_t* klens, uint32_t k,
                         uint64_t* out_ids, float* out_dist, uint32_t* out_count, size_t* bad_index, char* key_arena,
                         size_t arena_cap, uint64_t* key_off) {
  if (!key_off || (!key_arena && arena_cap)) return fail(EHX_EINVAL, "NULL argument");
  int rc = ehx_knn_by_keys(s, n, keys, klens, k, out_ids, out_dist, out_count, bad_index);
  if (rc) return rc;
  std::shared_lock<std::shared_mutex> rl(s->mu);
  if (s->dropped) return fail(EHX_ENOTFOUND, "Not found");
  return fill_key_arena(s, n, k, out_ids, out_count, key_arena, arena_cap, key_off);
}

int ehx_knn_by_ids_device(ehx_space* s, void* stream, size_t n, const uint64_t* d_row_ids, uint32_t k,
                          uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count) {
  int rc = check_batch_call(s, n, k, "k", true, !(n && k) || (d_row_ids && d_out_ids && d_out_dist && d_out_count),
                            "NULL device pointer");
  if (rc) return rc;
  yield_to_writer(s);
  std::shared_lock<std::shared_mutex> rl(s->mu);
  if ((rc = check_unsharded(s, "ehx_knn_by_ids_device", "use ehx_knn_by_keys"))) return rc;
  if (n == 0 || k == 0) return EHX_OK;
  std::lock_guard<std::mutex> sl(s->scratch_mu);
  HIP_TRY(hipSetDevice(s->device));
  ByKeyScratch b;
  if ((rc = by_scratch(s, n, k, false, &b))) return rc;
  return by_ids_locked(s, (hipStream_t)stream, n, d_row_ids, k, b, d_out_ids, d_out_dist, d_out_count);
}

int ehx_merge_topk_strided_device(void* stream, size_t n_queries, uint32_t k, uint32_t n_lists, const uint64_t* d_ids,
                                  size_t ids_stride, const float* d_dist, size_t dist_stride, const uint32_t* d_count,
                                  size_t count_stride, uint64_t* d_out_ids, float* d_out_dist,
                                  uint32_t* d_out_count) {
  if (n_queries == 0 || k == 0) return EHX_OK;
  if (k > 64 && n_lists > 64) return fail(EHX_EUNSUPPORTED, "merging k > 64 takes at most 64 lists (%u)", n_lists);
  if (!d_ids || !d_dist || !d_out_ids || !d_out_dist) return fail(EHX_EINVAL, "NULL device pointer");
  if (ids_stride % 8 || dist_stride % 4 || count_stride % 4) return fail(EHX_EINVAL, "misaligned list stride");
  int rc = ehx_init(nullptr, 0);
  if (rc) return rc;
  HIP_TRY(launch_merge_lists(d_ids, d_dist, d_count, (uint32_t)n_queries, k, n_lists, d_out_ids, d_out_dist,
                             d_out_count, (hipStream_t)stream, ids_stride, dist_stride, count_stride));
  return EHX_OK;
}

int ehx_merge_topk_device(void* stream, size_t n_queries, uint32_t k, uint32_t n_lists, const uint64_t* d_ids,
                          const float* d_dist, const uint32_t* d_count, uint64_t* d_out_ids, float* d_out_dist,
                          uint32_t* d_out_count) {
  return ehx_merge_topk_strided_device(stream, n_queries, k, n_lists, d_ids, n_queries * k * sizeof(uint64_t), d_dist,
                                       n_queries * k * sizeof(float), d_count, n_queries * sizeof(uint32_t),
                                       d_out_ids, d_out_dist, d_out_count);
}

}  // extern "C"
