/*
 * ehx.h — C ABI of the MI355X-native nearest-neighbour engine ("ehx") that drops in behind
 * featureform/embeddinghub's two vector-store boundaries.
 *
 * This header is the drop-in boundary: plain pointers and sizes, C linkage, no C++/torch
 * types, no callbacks, and the engine never retains a caller pointer after a call returns
 * (cgo rule).  Each entry point cites the reference interface it replaces
 * (paths relative to the reference checkout):
 *
 *   embeddingstore (C++):  embeddinghub/embeddingstore/index.h:19-33, index.cc:10-52 (ANNIndex)
 *                          embeddinghub/embeddingstore/server.cc:172-210 (NearestNeighbor RPC)
 *                          embeddinghub/embeddingstore/embedding_store.proto:9-19 (service)
 *   Go provider:           provider/online.go:42-70 (OnlineStore / VectorStore / VectorStoreTable /
 *                          BatchOnlineTable), provider/redis.go:245-262,454-493
 *   Python offline index:  embeddinghub/sdk/python/offlinehub.py:27-141
 *
 * INTEGRATION.md shows the cgo / C++ / ctypes stubs a maintainer adds on the reference side.
 *
 * Conventions
 *   - every function returns EHX_OK (0) or a negative EHX_E* code; ehx_last_error() returns a
 *     thread-local message for the last failing call on the calling thread;
 *   - all entry points are re-entrant; ehx_set* is linearizable with respect to a following
 *     ehx_knn* from the same thread (index_test.cc:39-49 relies on it);
 *   - caller allocates every output buffer; inputs are copied before the call returns;
 *   - ids are dense row ids in first-Set order (index.cc:24-28 labels), keys are arbitrary bytes;
 *   - results are nearest first (index.cc:43-50 reverses hnswlib's heap for the same reason);
 *   - all vector arithmetic runs in hand-written HIP kernels on gfx950; there is no CPU
 *     fallback: without a usable device every compute entry point fails with EHX_ENODEVICE.
 */
#ifndef EHX_H_
#define EHX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EHX_ABI_VERSION 5

/* ---- error codes (shim mapping: gRPC status for contract 1, fferr type for contract 2) ---- */
enum {
  EHX_OK = 0,
  EHX_EINVAL = -1,        /* INVALID_ARGUMENT (server.cc:184-188) / fferr.NewInvalidArgumentError   */
  EHX_ENOTFOUND = -2,     /* NOT_FOUND "Not found" (server.cc:178) / DatasetNotFound, EntityNotFound */
  EHX_EEXISTS = -3,       /* ALREADY_EXISTS / fferr.NewDatasetAlreadyExistsError (redis.go:161)       */
  EHX_EIMMUTABLE = -4,    /* FAILED_PRECONDITION "Cannot write to immutable space" (server.cc:125-127) */
  EHX_ENODEVICE = -5,     /* no usable gfx950 device / HIP runtime error: INTERNAL                      */
  EHX_ENOMEM = -6,        /* RESOURCE_EXHAUSTED                                                          */
  EHX_ERANGE = -7,        /* caller buffer too small (key arena)                                         */
  EHX_EUNSUPPORTED = -8,  /* UNIMPLEMENTED (e.g. k above EHX_MAX_K)                                      */
  EHX_EINTERNAL = -9
};

/* ---- metric / dtype / mode ---- */
enum {
  EHX_METRIC_L2SQ = 0,   /* sum (a-b)^2, no sqrt — hnswlib::L2Space, index.cc:13 (embeddingstore default) */
  EHX_METRIC_IP = 1,     /* 1 - sum a*b   — hnswlib::InnerProductSpace                                     */
  EHX_METRIC_COSINE = 2  /* normalise on Set and on query, then IP — Go providers (redis.go:253)           */
};
enum {
  EHX_DTYPE_F32 = 0, /* rows stored as given (the reference's std::vector<float>, index.h:14)                     */
  EHX_DTYPE_F16 = 1  /* rows rounded to IEEE binary16 (nearest-even) when written and widened exactly to fp32
                        wherever they are read — results are those of an F32 space fed the rounded rows; halves
                        the footprint of the stored rows (BASELINE.json configs[5]); the API still speaks fp32
                        (Get returns the widened stored values).  Graph mode: the fp32 search copy is made from
                        the rounded rows (6 instead of 8 bytes per stored dimension)                              */
};
enum {
  EHX_MODE_FLAT = 0,  /* exhaustive scan on the matrix cores + canonical re-rank: exact kNN */
  EHX_MODE_GRAPH = 1  /* HNSW-style level-0 best-first search over an HBM-resident graph      */
};

/* scan engine selection of a flat space (ehx_params.scan, ehx_space_set_scan); results are identical for all */
enum {
  EHX_SCAN_AUTO = 0, /* the fastest certified filter the space supports: int8 where it pays, else fp16 */
  EHX_SCAN_F32 = 1,  /* fp32 matrix-core scan only */
  EHX_SCAN_F16 = 2   /* fp16 matrix-core filter (never the int8 one) */
};
/* what ehx_space_scan_engine reports: the engine that answers first right now */
enum { EHX_ENGINE_F32 = 0, EHX_ENGINE_F16 = 1, EHX_ENGINE_I8 = 2 };

#define EHX_MAX_K 48u /* largest k served by the certified engine chain: one scan pass holds k + 8 slack < 64 candidate
                         slots per query */
#define EHX_MAX_K_PAGED 1024u /* flat mode serves EHX_MAX_K < k <= this exactly too.  Which k is served how:
                                  48 < k <= 256, at least 64 queries in the device batch, a space whose first engine is
                                  the int8 filter: the large-k scan route — passes of that filter's scan under a radius
                                  that falls, an exact re-rank behind every pass; a batch path, the
                                  exhaustive pass's answer byte for byte.
                                  Everything else (k > 256, fewer than 64 queries, spaces below the int8 engine's row
                                  count, EHX_SCAN_F32 / EHX_SCAN_F16): the exhaustive canonical pass in pages of 64
                                  results — the whole shard is read once per page and query; fine for the occasional
                                  large request, not a batch path.
                                  Graph mode serves any k <= this from its result list of max(ef, k) entries, as
                                  hnswlib's searchKnn does */

/* The graph walk under a row bitmap (ehx_graph_knn_masked*) keeps ONE list of walked nodes, allowed or not, of at most
 * cap = max(ef, min(EHX_WALK_LIST_FACTOR * ef, EHX_WALK_LIST_MAX)) entries.  The factor is the reciprocal of the smallest
 * allowed share at which the list can still hold ef allowed entries — below it a walk stops paying, which is where
 * EHX_WALK_AUTO hands the request to the exact route — and the maximum is the list the kernel keeps in LDS.
 * The factor was 16 as a choice and is 12 as MEASURED (scripts/bench_graph_masked.py, profiles/graph_masked_bench.jsonl,
 * batch 1024, k 10, ef 60, one MI355X): with a list of 16 ef the exact route costs what the walk costs at an allowed share
 * of 1 / 14 on 1 M x 128 L2 rows and of 1 / 11 on 200 k x 768 cosine rows, and at 1 / 16 the walk was 1.14 and 1.66 times
 * slower than the exact route.  DESIGN.md §e.15 has the table. */
#define EHX_WALK_LIST_FACTOR 12u
#define EHX_WALK_LIST_MAX 4096u
/* route of ehx_graph_knn_masked* (A/B and diagnosis, as ehx_space_set_scan) */
enum {
  EHX_WALK_AUTO = 0,  /* walk iff allowed rows * EHX_WALK_LIST_FACTOR >= rows the bitmap covers, else the exact route */
  EHX_WALK_GRAPH = 1, /* always walk the graph */
  EHX_WALK_EXACT = 2  /* always the exact route: ehx_knn_masked_device's answer */
};

typedef struct ehx_space ehx_space; /* opaque; owned by the process-global registry */

/* Index parameters.  Zero-initialise and set what you need; 0 means "reference default"
 * (hnswlib defaults as used by index.cc:14-15: M=16, ef_construction=200, seed=100, ef=10). */
typedef struct ehx_params {
  uint32_t mode;            /* EHX_MODE_*                                   */
  uint32_t M;               /* graph degree (level 0 holds 2*M); 2..32, GPU-side insertion needs M <= 31 */
  uint32_t ef_construction; /*                                              */
  uint32_t ef;              /* search ef; effective ef = max(ef, k)         */
  uint64_t seed;            /* level generator seed                         */
  uint64_t initial_capacity;/* rows; 0 -> 128 (index.h:21), doubles on fill */
  uint32_t build_batch;     /* graph mode: rows inserted concurrently per round by bulk loads; 0 = auto
                               (ehx_fill_synthetic: up to 4096 per round; ehx_set / ehx_set_batch: strictly
                               sequential = hnswlib's single-threaded addPoint order, graph bit-identical to
                               the oracle's), 1 = strictly sequential everywhere, N > 1 = rounds of up to N
                               rows, ALSO for an ehx_set_batch made only of fresh keys (hnswlib-python's
                               multi-threaded add_items), 0xFFFFFFFF = no graph building (import one).    */
  uint32_t scan;            /* flat mode: EHX_SCAN_AUTO (0) = a matrix-core FILTER scan (int8 on rows of up to 2048 dims and
                               >= 16 Ki rows, else fp16) in front of the canonical fp32 re-rank; every query a
                               filter cannot certify is re-run by the next engine (int8 -> fp16 -> fp32 scan ->
                               exhaustive canonical pass) — results identical to EHX_SCAN_F32 (1) = fp32
                               matrix-core scan only; EHX_SCAN_F16 (2) = start from the fp16 filter.          */
  uint32_t shards;          /* 0 / 1: one shard on ehx_init's first device.  G > 1: the space is ROW-SHARDED inside this
                               process — row g lives in shard g % G on device_ids[(g % G) % n_devices] of ehx_init;
                               ehx_set* route by row id, ehx_knn* search every shard concurrently, copy each local
                               top-k peer-to-peer (xGMI) to shard 0's device and merge there; ids stay the dense
                               global row ids; k as for an unsharded space.  Graph import / export are per-shard operations.   */
  uint32_t search_width;    /* graph mode: level-0 expansions per search step.  0 / 1: the strict walk — one node at a time
                               in hnswlib's order (searchBaseLayerST): ids, distances and work counters identical to the
                               reference algorithm's on the same graph.  2 / 4: the WIDE walk, a throughput mode — a step
                               expands the 2 / 4 closest unexpanded candidates together (same ef bound, same termination
                               rule, same canonical distances): fewer dependent memory round trips per query, a few per
                               cent more rows fetched, recall@k within 0.005 of the strict walk at equal ef (the gate of
                               tests/test_graph_wide.py); the result's tail may differ from hnswlib's.  Short lists are
                               walked more narrowly whatever is set here: ef < 16 (the reference's default 10 included) is
                               always the strict walk, ef < 64 expands at most 2 per step; graphs of M > 16 are always
                               searched strictly. */
  uint32_t reserved[4];
} ehx_params;

/* Work and time counters, same definitions as the oracle. */
typedef struct ehx_stats_t {
  uint64_t n_rows;           /* rows currently stored                                                */
  uint64_t capacity;         /* rows allocated in HBM                                                */
  uint64_t n_queries;        /* queries served since creation / last reset                           */
  uint64_t n_dist;           /* distances actually evaluated (one per vector row fetched)            */
  uint64_t n_hops;           /* graph nodes expanded (graph mode)                                    */
  uint64_t n_rerank;         /* candidates re-ranked in canonical order                              */
  uint64_t n_uncertified;    /* always 0: a call never returns EHX_OK with an uncertified result (what the matrix-
                                core scans cannot certify is answered by the exhaustive canonical pass; kept in
                                the struct as the audit counter of that invariant)                  */
  uint64_t bytes_algorithmic;/* SURVEY §8d algorithmic bytes of the scans/searches served            */
  double   last_scan_ms;     /* device time of the last scan/search kernel (HIP events)              */
  double   last_total_ms;    /* device time of the last full ehx_knn* pipeline                       */
  double   scan_ms_mean;     /* mean device time of the last <=64 scan/search kernel launches        */
  uint64_t scan_launches;    /* number of launches averaged in scan_ms_mean                          */
  uint64_t n_filter_queries; /* queries answered through the fp16 filter scan                        */
  uint64_t n_filter_fallback;/* ... of which the filter could not certify and the fp32 scan re-ran   */
  uint64_t n_exhaustive;     /* queries answered by the exhaustive canonical pass (fp32 scan uncertified) */
  uint64_t n_i8_queries;     /* queries answered through the int8 filter scan                         */
  uint64_t n_i8_fallback;    /* ... of which it could not certify (pool overflow / margin): next engine */
} ehx_stats_t;

/* ---- process / device ---- */

/* Once per process (idempotent).  device_ids==NULL or n_devices==0 -> device 0.  Unsharded spaces live on the first
 * listed device; the shards of a space created with ehx_params.shards = G are spread over the whole list (one
 * process drives all of them: what a Go / C++ caller of this ABI uses on an 8-GPU node).  The one-process-per-GPU
 * form (torch.distributed + RCCL all-gather, embeddinghub_amd/sharded.py) lists one device per process.
 * With more than one device listed, peer access is opened explicitly between every ordered pair (the shards' exchange
 * step is a peer copy over xGMI); a pair that cannot be opened fails the call with EHX_ENODEVICE naming the two devices
 * (environment EHX_ALLOW_NO_PEER=1: accept it, the copies then stage through host memory). */
int ehx_init(const int* device_ids, int n_devices);
int ehx_shutdown(void);
int ehx_abi_version(void);
const char* ehx_last_error(void);

/* ---- spaces: CreateSpace/DeleteSpace/FreezeSpace (embedding_store.proto:10-12),
 *      VectorStore.CreateIndex/DeleteIndex + OnlineStore.CreateTable/GetTable (online.go:42-59) ---- */
int ehx_space_create(const char* name, size_t name_len, uint32_t dims, int metric, int dtype,
                     const ehx_params* params /* may be NULL */, ehx_space** out);
int ehx_space_open(const char* name, size_t name_len, ehx_space** out); /* EHX_ENOTFOUND if absent */
int ehx_space_drop(ehx_space* s);
int ehx_space_freeze(ehx_space* s);            /* later ehx_set* -> EHX_EIMMUTABLE (version.cc:47-50) */
int ehx_space_size(ehx_space* s, uint64_t* n); /* number of distinct keys                              */
int ehx_space_dims(ehx_space* s, uint32_t* dims);
int ehx_space_reserve(ehx_space* s, uint64_t rows);
int ehx_space_set_ef(ehx_space* s, uint32_t ef);
/* graph spaces: expansions per search step from now on (ehx_params.search_width: 0 / 1 strict, 2 / 4 wide); EHX_EINVAL
 * for any other value.  The graph is the same for every width: only the order it is walked in changes. */
int ehx_space_set_search_width(ehx_space* s, uint32_t width);
/* flat spaces: switch between EHX_SCAN_AUTO (certified filter scan, the default), EHX_SCAN_F16 and EHX_SCAN_F32.
 * Results are identical; A/B measurement and diagnosis.  The scan copies stay current whatever is selected. */
int ehx_space_set_scan(ehx_space* s, uint32_t scan);
/* the engine that answers first on this space right now: EHX_ENGINE_* */
int ehx_space_scan_engine(ehx_space* s, uint32_t* engine);

/* ---- writes: Set/MultiSet (server.cc:113-149 -> Version::set -> ANNIndex::set, index.cc:20-37),
 *      OnlineStoreTable.Set / BatchOnlineTable.BatchSet (online.go:50-53,66-70) ---- */
int ehx_set(ehx_space* s, const char* key, size_t klen, const float* vec /* dims floats */);
int ehx_set_batch(ehx_space* s, size_t n, const char* const* keys, const size_t* klens,
                  const float* vecs /* n x dims, row-major */);
/* ehx_set_batch with the rows read from device memory (embeddings that a model on the same GPU just produced): d_vecs is
 * n x dims, dense and row-major, of float (src_dtype EHX_DTYPE_F32) or IEEE binary16 (EHX_DTYPE_F16) — any other src_dtype:
 * EHX_EINVAL; element-aligned is enough (a tensor view).  The keys stay on the host.  For the same values the call does what
 * ehx_set_batch does — row ids, stored bytes, statistics, scan copies, graph insertion and update in call order, the
 * append-only path that leaves searches running, every error code — except that no row passes through host memory: one
 * kernel scatters them into the stored rows.  fp32 into an F16 space: rounded to nearest-even binary16
 * on the device, overflow to +-Inf; binary16 into an F16 space: bit for bit; binary16 into an F32 space: widened exactly.
 * A key given twice in one batch keeps the row of its last occurrence.  `stream` (a hipStream_t as void*, NULL = default
 * stream) is the stream whose work produced d_vecs: the writers' stream waits for it through an event, it is not drained.
 * The call returns after the rows are published, as ehx_set_batch does: d_vecs may be reused at once.  d_vecs must be device
 * memory (a host pointer: EHX_EINVAL) on the space's device; for a row-sharded space on any device of ehx_init's list — the
 * shards read it over peer access (EHX_EUNSUPPORTED under EHX_ALLOW_NO_PEER when they have none).  n == 0: EHX_OK. */
int ehx_set_batch_device(ehx_space* s, void* stream, size_t n, const char* const* keys, const size_t* klens,
                         const void* d_vecs /* n x dims, row-major, in HBM */, int src_dtype);

/* ---- stored label columns: labels written with the rows, indexed once ----
 * A space owns up to EHX_MAX_COLUMNS columns of one uint32_t per row, in device memory, sized and moved with the rows.  A
 * column exists from its first write (which takes the space's exclusive lock once); a column that was never written reads as
 * EHX_GROUP_NONE (0xFFFFFFFF) for every row, and searches on it work.  A row whose value was never given holds the default
 * EHX_GROUP_NONE: rows appended by ehx_set, ehx_set_batch, ehx_set_batch_device and ehx_fill_* after the column exists.
 * Rewriting a row's vector in place (a Set on a known key) keeps its column values.  Errors common to all of the entry points
 * below: a NULL space: EHX_EINVAL, before the device is looked for; a column number at or above EHX_MAX_COLUMNS: EHX_EINVAL;
 * a dropped space: EHX_ENOTFOUND; a row-sharded space: EHX_EUNSUPPORTED; for the writes, a frozen space: EHX_EIMMUTABLE.
 * n == 0: EHX_OK. */
#define EHX_MAX_COLUMNS 4
/* ehx_set_batch plus values[c][i] for column cols[c] of keys[i] (values: n_cols host arrays of n entries).  The labels land
 * before the row count is published — on the writers' stream, in front of the rows, on the append-only path; inside the same
 * exclusive section for a batch that touches committed rows — so no search ever sees a new row with a stale or default
 * label.  A key given twice in one batch keeps its last value, as it keeps its last row.  n_cols == 0 is ehx_set_batch.  A
 * column named twice, NULL cols / values with n_cols > 0: EHX_EINVAL. */
int ehx_set_batch_cols(ehx_space* s, size_t n, const char* const* keys, const size_t* klens, const float* vecs, uint32_t n_cols,
                       const uint32_t* cols, const uint32_t* const* values);
/* Relabels existing rows by key: column col of keys[i] becomes values[i] (a key given twice keeps its last value).  An unknown
 * key fails the whole call with EHX_ENOTFOUND, stores its index in *bad_index (may be NULL) as ehx_get_batch does, and
 * nothing is written.  A rewrite in place: it takes the exclusive lock and waits for the searches in flight, as a Set on
 * known keys does. */
int ehx_column_set(ehx_space* s, uint32_t col, size_t n, const char* const* keys, const size_t* klens, const uint32_t* values,
                   size_t* bad_index /* may be NULL */);
/* column col of keys[i] -> out_values[i]; an unknown key: EHX_ENOTFOUND, its index in *bad_index, out_values unwritten. */
int ehx_column_get(ehx_space* s, uint32_t col, size_t n, const char* const* keys, const size_t* klens, uint32_t* out_values,
                   size_t* bad_index /* may be NULL */);
/* Bulk load of the contiguous row ids [row0, row0 + n) of a column from device memory (for example after
 * ehx_fill_synthetic), copied on `stream` (a hipStream_t as void*); the call returns with the values in place.  The range
 * must lie below the row count: otherwise EHX_EINVAL.  A rewrite in place, as ehx_column_set. */
int ehx_column_load_device(ehx_space* s, void* stream, uint32_t col, uint64_t row0, uint64_t n, const uint32_t* d_values);
/* ... and the same range read back into device memory; the call returns with d_out written. */
int ehx_column_read_device(ehx_space* s, void* stream, uint32_t col, uint64_t row0, uint64_t n, uint32_t* d_out);

/* ---- reads: Get (server.cc:95-111), OnlineStoreTable.Get (online.go:52) ---- */
int ehx_get(ehx_space* s, const char* key, size_t klen, float* out_vec /* dims floats */);
int ehx_get_by_id(ehx_space* s, uint64_t id, float* out_vec);
/* ehx_get for n keys in ONE call (MultiGet / Download, embedding_store.proto:15-18; the same key may appear several times):
 * all keys are looked up under one hold of the space's lock, the rows gathered on the device and copied back once; row i
 * equals what ehx_get(keys[i]) returns.  An unknown key fails the whole call with EHX_ENOTFOUND, stores its index in
 * *bad_index (may be NULL) and leaves out_vecs unwritten (ehx_knn_by_keys' rule).  Flat and graph spaces, F32 and F16,
 * row-sharded spaces (peer access as for ehx_knn_by_keys).  n == 0: EHX_OK. */
int ehx_get_batch(ehx_space* s, size_t n, const char* const* keys, const size_t* klens,
                  float* out_vecs /* n x dims */, size_t* bad_index /* may be NULL */);
/* key of a row id: copies up to cap bytes, stores the full length in *klen */
int ehx_key_of(ehx_space* s, uint64_t id, char* out_key, size_t cap, size_t* klen);

/* ---- kNN: ANNIndex::approx_nearest (index.cc:39-52), NearestNeighbor RPC (server.cc:172-210),
 *      VectorStoreTable.Nearest (online.go:63), offlinehub.Index.nearest_neighbor (offlinehub.py:102-131).
 *      Batched: n_queries x dims row-major in, n_queries x k out, nearest first.
 *      out_count[i] <= k is the number of valid results of query i (fewer than k when the space holds
 *      fewer than k rows — the reference has UB there, index.cc:46-50 — or pairs are left out by the NaN rule).
 *      Contract: the first k (query, row) pairs in (canonical distance, id) order; a pair whose distance is NaN
 *      is no neighbour; +-Inf distances are.  The filter scans bound rows and queries with |x|^2 == 0 or in
 *      (1e-24, 1e30); outside that band the fp32 scan / exhaustive pass answers.  DTYPE_F16 rows are stored
 *      rounded to nearest-even binary16 (overflow to +-Inf), and searched as stored. ---- */
int ehx_knn(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint64_t* out_ids,
            float* out_dist, uint32_t* out_count);
/* as ehx_knn, plus keys: key j of query i is key_arena[key_off[i*k+j] .. key_off[i*k+j+1]) ;
 * key_off has n_queries*k+1 entries; missing results have empty keys. */
int ehx_knn_keys(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint64_t* out_ids,
                 float* out_dist, uint32_t* out_count, char* key_arena, size_t arena_cap,
                 uint64_t* key_off);
/* server.cc:193-207 / offlinehub.py:113-130: query by stored key, ask for k+1, drop the key
 * itself if present else drop the last.  EHX_ENOTFOUND for an unknown key (the reference has UB). */
int ehx_knn_by_key(ehx_space* s, const char* key, size_t klen, uint32_t k, uint64_t* out_ids,
                   float* out_dist, uint32_t* out_count);
/* as ehx_knn_by_key, plus the neighbours' KEYS in one call — the whole NearestNeighbor RPC by key (server.cc:172-210:
 * look the key up, search k+1, drop the key itself, answer with keys) without k calls of ehx_key_of: key j is
 * key_arena[key_off[j] .. key_off[j+1]), key_off has k+1 entries; EHX_ERANGE if the arena is too small.
 * out_ids / out_dist may be NULL. */
int ehx_knn_by_key_keys(ehx_space* s, const char* key, size_t klen, uint32_t k, uint64_t* out_ids, float* out_dist,
                        uint32_t* out_count, char* key_arena, size_t arena_cap, uint64_t* key_off);
/* ehx_knn_by_key for n stored keys in ONE call (the same key may appear several times): the rows are gathered into a query
 * batch on the device (the bytes ehx_get returns), searched with k + 1 by the space's own pipeline, and every key is
 * dropped from its own list on the device — the rule above, so row i equals ehx_knn_by_key(keys[i]).  Outputs laid out
 * [n][k] as in ehx_knn.  Key lookup, gather and search see ONE state of the space.  An unknown key fails the whole call
 * with EHX_ENOTFOUND, stores its index in *bad_index (may be NULL) and leaves the outputs unwritten; k > EHX_MAX_K_PAGED:
 * EHX_EUNSUPPORTED.  Flat and graph spaces, F32 and F16, row-sharded spaces (whose shards must have peer access to shard
 * 0's device: EHX_EUNSUPPORTED under EHX_ALLOW_NO_PEER when they do not). */
int ehx_knn_by_keys(ehx_space* s, size_t n, const char* const* keys, const size_t* klens, uint32_t k,
                    uint64_t* out_ids, float* out_dist, uint32_t* out_count, size_t* bad_index);
/* as ehx_knn_by_keys, plus the neighbours' keys, laid out as ehx_knn_keys lays them out (key_off has n*k+1 entries);
 * EHX_ERANGE if the arena is too small. */
int ehx_knn_by_keys_keys(ehx_space* s, size_t n, const char* const* keys, const size_t* klens, uint32_t k,
                         uint64_t* out_ids, float* out_dist, uint32_t* out_count, size_t* bad_index, char* key_arena,
                         size_t arena_cap, uint64_t* key_off);
/* ehx_knn among lists of row ids, from host pointers: ehx_knn_among_device (below: contract, duplicate rule, intended
 * regime) plus the H2D / D2H copies.  cand_off == NULL: ONE list cand_ids[0, n_cand) shared by every query; else query i
 * owns cand_ids[cand_off[i], cand_off[i+1]) and cand_off has n_queries + 1 entries — checked here: not non-decreasing, or
 * not ending at n_cand: EHX_EINVAL.  Outputs laid out [n_queries][k] as in ehx_knn. */
int ehx_knn_among(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const uint64_t* cand_ids,
                  const uint64_t* cand_off, size_t n_cand, uint64_t* out_ids, float* out_dist, uint32_t* out_count);
/* ehx_knn_among with the shared list given as n_allowed stored keys, resolved under the same hold of the space's lock as
 * the search: key lookup and search see ONE state of the space.  An unknown key fails the whole call with EHX_ENOTFOUND,
 * stores its index in *bad_index (may be NULL) and leaves the outputs unwritten (ehx_knn_by_keys' rule).  A key given twice
 * is a repeated id (the duplicate rule of ehx_knn_among_device). */
int ehx_knn_among_keys(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, size_t n_allowed,
                       const char* const* keys, const size_t* klens, uint64_t* out_ids, float* out_dist,
                       uint32_t* out_count, size_t* bad_index);
/* Exact kNN under a row bitmap from host pointers: ehx_knn_masked_device (below: the contract) plus the H2D / D2H copies.
 * mask has ceil(n_bits / 32) words. */
int ehx_knn_masked(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const uint32_t* mask, uint64_t n_bits,
                   uint64_t* out_ids, float* out_dist, uint32_t* out_count);
/* Exact kNN under a table of row bitmaps, one per query, from host pointers: ehx_knn_masked_multi_device (below: the
 * contract) plus the H2D / D2H copies.  masks has n_masks * ceil(n_bits / 32) words, mask_of n_queries entries; mask_of is
 * checked here, before anything is enqueued. */
int ehx_knn_masked_multi(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const uint32_t* masks,
                         uint32_t n_masks, uint64_t n_bits, const uint32_t* mask_of, uint64_t* out_ids, float* out_dist,
                         uint32_t* out_count);
/* Graph search under a row bitmap from host pointers: ehx_graph_knn_masked_device (below: the contract) plus the H2D / D2H
 * copies.  mask has ceil(n_bits / 32) words. */
int ehx_graph_knn_masked(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const uint32_t* mask,
                         uint64_t n_bits, uint32_t route, uint64_t* out_ids, float* out_dist, uint32_t* out_count);
/* Graph search under a table of row bitmaps, one per query, from host pointers: ehx_graph_knn_masked_multi_device (below:
 * the contract) plus the H2D / D2H copies.  masks has n_masks * ceil(n_bits / 32) words, mask_of n_queries entries; mask_of
 * is checked here, before anything is enqueued. */
int ehx_graph_knn_masked_multi(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const uint32_t* masks,
                               uint32_t n_masks, uint64_t n_bits, const uint32_t* mask_of, uint32_t route, uint64_t* out_ids,
                               float* out_dist, uint32_t* out_count);
/* Grouped kNN from host pointers: ehx_knn_grouped_device (below: the contract) plus the H2D / D2H copies.  group_of has
 * n_labels entries; the labels of the prefix searched are staged on EVERY call — 4 bytes per row, 4 MB at 1 M rows: the
 * device form, with the labels resident, is the serving path. */
int ehx_knn_grouped(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint32_t per_group,
                    const uint32_t* group_of, uint64_t n_labels, uint64_t* out_ids, float* out_dist, uint32_t* out_count);
/* Grouped kNN under a table of row bitmaps from host pointers: ehx_knn_grouped_masked_device (below: the contract) plus the
 * H2D / D2H copies.  group_of has n_labels entries, masks n_masks * ceil(n_bits / 32) words, mask_of n_queries entries (it may
 * be NULL with n_masks == 1); mask_of is checked here, before anything is enqueued.  The labels and the bitmaps' words of the
 * prefix searched are staged on EVERY call: the device form, with both resident, is the serving path. */
int ehx_knn_grouped_masked(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint32_t per_group,
                           const uint32_t* group_of, uint64_t n_labels, const uint32_t* masks, uint32_t n_masks,
                           uint64_t n_bits, const uint32_t* mask_of, uint64_t* out_ids, float* out_dist, uint32_t* out_count);
/* Exact kNN under a label column from host pointers: ehx_knn_labeled_device (below: the contract) plus the H2D / D2H copies.
 * label_of has n_labels entries, want n_queries.  The labels of the prefix searched are staged on EVERY call — 4 bytes per
 * row: the device form, with the column resident, is the serving path. */
int ehx_knn_labeled(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const uint32_t* label_of,
                    uint64_t n_labels, const uint32_t* want, uint64_t* out_ids, float* out_dist, uint32_t* out_count);
/* Grouped kNN under a label column from host pointers: ehx_knn_grouped_labeled_device (below: the contract) plus the H2D /
 * D2H copies.  group_of and label_of have n_labels entries each, want n_queries.  BOTH columns' prefixes searched are staged
 * on EVERY call — 8 bytes per row, 8 MB at 1 M rows: the device form, with both columns resident, is the serving path. */
int ehx_knn_grouped_labeled(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint32_t per_group,
                            const uint32_t* group_of, const uint32_t* label_of, uint64_t n_labels, const uint32_t* want,
                            uint64_t* out_ids, float* out_dist, uint32_t* out_count);
/* Exact range search from host pointers: ehx_range_device (below: the contract) plus the H2D / D2H copies.  radius has
 * n_queries entries; out_total may be NULL. */
int ehx_range(ehx_space* s, size_t n_queries, const float* queries, const float* radius, uint32_t max_results,
              uint64_t* out_ids, float* out_dist, uint32_t* out_count, uint64_t* out_total);
/* ehx_range plus the members' keys, laid out as ehx_knn_keys lays them out (key_off has n_queries * max_results + 1
 * entries), looked up under the same hold of the space's lock as the search. */
int ehx_range_keys(ehx_space* s, size_t n_queries, const float* queries, const float* radius, uint32_t max_results,
                   uint64_t* out_ids, float* out_dist, uint32_t* out_count, uint64_t* out_total, char* key_arena,
                   size_t arena_cap, uint64_t* key_off);
/* Exact range search under a table of row bitmaps, one per query, from host pointers: ehx_range_masked_device (below: the
 * contract) plus the H2D / D2H copies.  masks has n_masks * ceil(n_bits / 32) words, radius n_queries entries, mask_of
 * n_queries entries (may be NULL with n_masks == 1: every query is under bitmap 0); mask_of is checked here, before anything
 * is enqueued.  out_total may be NULL. */
int ehx_range_masked(ehx_space* s, size_t n_queries, const float* queries, const float* radius, uint32_t max_results,
                     const uint32_t* masks, uint32_t n_masks, uint64_t n_bits, const uint32_t* mask_of, uint64_t* out_ids,
                     float* out_dist, uint32_t* out_count, uint64_t* out_total);

/* ---- device-resident entry points (inputs/outputs already in HBM; `stream` is a hipStream_t
 *      passed as void*, NULL = default stream).  These are what a batching shim and bench.py
 *      call; ehx_knn above is ehx_knn_device plus the H2D/D2H copies.
 *      Completion: the results are in place when `stream` reaches the point the call returned at — wait for the stream
 *      (or an event recorded on it) before reading them.  Most paths have waited for the device themselves by the time
 *      they return (every flat stage reads its verdict back); ONE query against a small flat shard (the exhaustive
 *      canonical pass, EHX_SMALL_EXACT_BYTES) and graph searches return with work still queued on `stream`.  A writer
 *      that rewrites rows in place waits for searches in flight on whatever stream they were given; a writer that only
 *      appends does not need to (it touches rows beyond the row count the search was launched with, and growing the
 *      arrays takes the space exclusively and drains the device first). ---- */
int ehx_knn_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                   uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count);
/* The neighbours of rows the space holds, by row id, without the rows leaving HBM: query i is row d_row_ids[i] as stored
 * (what ehx_get_by_id returns), searched with k + 1, the row itself dropped from its list (ehx_knn_by_key's rule).
 * Completion as for ehx_knn_device.  An id at or above the row count gives d_out_count[i] = 0, not an error.
 * k > EHX_MAX_K_PAGED and row-sharded spaces: EHX_EUNSUPPORTED. */
int ehx_knn_by_ids_device(ehx_space* s, void* stream, size_t n, const uint64_t* d_row_ids, uint32_t k,
                          uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count);
/* The stored rows themselves, by row id, without leaving HBM: d_out[i] = what ehx_get_by_id(d_row_ids[i]) returns (F16 rows
 * widened, a single-copy graph space's block order undone), d_valid[i] = 1.  An id at or above the row count — ONE acquire
 * load of it per call — gives a zero row and d_valid[i] = 0, not an error.  Completion as for ehx_knn_device; on a
 * row-sharded space (served too: the buffers on shard 0's device, or one with peer access to it) the call waits for the
 * gather itself.  A Set that rewrites rows in place waits for the call like for any search.  n == 0: EHX_OK. */
int ehx_get_by_ids_device(ehx_space* s, void* stream, size_t n, const uint64_t* d_row_ids,
                          float* d_out /* n x dims */, uint32_t* d_valid /* n */);
/* Exact kNN restricted to lists of row ids (filtered search, re-ranking of candidates found elsewhere): query i has a
 * candidate list L_i of global row ids and the answer is the first k (query, row) pairs over the rows of L_i in (canonical
 * distance, id) order — ehx_knn's contract (NaN rule, +-Inf, cosine normalisation, F16 rows as stored, out_count[i] <= k,
 * entries beyond the count id ~0 / +Inf) with "every row" replaced by "the rows of L_i".  The listed rows are scanned
 * exhaustively in the oracle's arithmetic, in flat AND graph spaces (a graph space's graph is not walked).
 * d_cand_off == NULL: ONE list d_cand_ids[0, n_cand) shared by every query; else query i owns
 * d_cand_ids[d_cand_off[i], d_cand_off[i+1]), n_queries + 1 offsets, the last equal to n_cand.  The order of ids in a list
 * does not matter; an id at or above the row count the call took its ONE snapshot of is ignored, not an error; an empty
 * list gives count 0.  An id should appear at most once per list: a list that repeats one may get that row back more than
 * once — nothing else (no id outside the list, distances canonical and non-decreasing).  k <= EHX_MAX_K_PAGED, served in
 * pages of 64 as the exhaustive pass serves them; above: EHX_EUNSUPPORTED; k == 0 or NULL outputs: EHX_EINVAL; row-sharded
 * spaces, and rows longer than 40 960 floats (a prepared query must fit in a CU's LDS): EHX_EUNSUPPORTED.  The offsets cannot be checked here: max_list_hint is an upper bound of any one list's length
 * (0 = unknown: n_cand) and sizes the launch ONLY — a workgroup walks its list to the end whatever the hint, so a hint that
 * is too small costs time and never rows.  Completion as for ehx_knn_device; a Set that rewrites rows in place waits for
 * the call like for any search.
 * Intended regime: selective filters and re-ranking — this is an exact scan in fp32 vector arithmetic, not a faster scan.
 * A shared list is cheaper than ehx_knn_device on the whole space only while it names a small share of the rows (estimated,
 * NOT measured: 1-2 % of the rows at batch 1024 on 1 M x 768), and per-query lists are a gather bound by the memory
 * system: DESIGN.md §e.10 has the rooflines and says what scripts/bench_among.py will record. */
int ehx_knn_among_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                         const uint64_t* d_cand_ids, const uint64_t* d_cand_off, size_t n_cand, size_t max_list_hint,
                         uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count);
/* Exact kNN under a row bitmap (filters of ordinary selectivity: a predicate resolved to one bit per row).  Row r is allowed
 * iff r < n_bits, r is below the call's ONE acquire-load snapshot of the row count, and bit r & 31 of word r >> 5 of d_mask
 * is set; d_mask has ceil(n_bits / 32) words, bits of the last word beyond n_bits are ignored.  The answer is, byte for
 * byte, that of ehx_knn_among_device with the one shared list of allowed rows: the first k (query, row) pairs over the
 * allowed rows in (canonical distance, id) order, with ehx_knn's NaN rule, +-Inf, cosine normalisation, F16 rows as stored
 * and sentinels (id 2^64 - 1, +Inf) beyond d_out_count[i].  Every space kind ehx_knn_among serves is served; a graph space
 * answers from its stored rows, its graph is not walked.  n_bits == 0 or a bitmap with no bit set: count 0 for every query.
 * Errors as ehx_knn_among_device (k == 0 or NULL outputs: EHX_EINVAL; k > EHX_MAX_K_PAGED, row-sharded spaces, rows longer
 * than 40 960 floats: EHX_EUNSUPPORTED; a dropped space: EHX_ENOTFOUND; no device: EHX_ENODEVICE), and a NULL mask with
 * n_bits > 0: EHX_EINVAL.  The bitmap is compacted on the device to the ascending list of allowed ids; flat spaces whose
 * first engine is the int8 filter, at k <= 48 and more than max(1024, rows / 128) allowed rows, are then answered by passes
 * of that filter's scan under a threshold mapped from a radius — the exact k-th distance among the allowed rows seen so
 * far, first of a sample of 256 of them — with the bitmap applied where the scan collects its hits and an exact re-rank of
 * the survivors behind every pass; everything else, and the queries that scan cannot bound or whose pool overflowed, by
 * the exact scan of the listed rows (ehx_knn_among_device).  The call waits for the device before it returns (it reads the
 * tiles' allowed counts back); a Set that rewrites rows in place waits for it like for any search.  DESIGN.md §e.12. */
int ehx_knn_masked_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                          const uint32_t* d_mask, uint64_t n_bits, uint64_t* d_out_ids, float* d_out_dist,
                          uint32_t* d_out_count);
/* Exact kNN under a TABLE of row bitmaps, one per query: what a serving process needs when one micro-batch carries requests
 * of several tenants, ACL groups or categories — one call and one set of scan passes instead of one ehx_knn_masked_device
 * call per filter.  d_masks holds n_masks bitmaps, dense, [n_masks][ceil(n_bits / 32)] words, each laid out as
 * ehx_knn_masked_device's; query i is searched under bitmap d_mask_of[i].  Row i of the answer is, byte for byte, what
 * ehx_knn_masked_device returns for query i alone under that bitmap: the same definition of an allowed row with ONE
 * acquire-load snapshot of the row count for the whole call, (canonical distance, id) order, the NaN rule, +-Inf, cosine
 * normalisation, F16 rows as stored, the sentinels beyond d_out_count[i]; a bitmap with no bit set gives count 0 for ITS
 * queries only.  With n_masks == 1 (d_mask_of all zero) the call equals ehx_knn_masked_device byte for byte.  Every space
 * kind ehx_knn_masked serves is served; a graph space answers from its stored rows.
 * Errors as ehx_knn_masked_device, and: n_masks == 0 with n_queries > 0, a NULL d_mask_of, an entry of d_mask_of at or above
 * n_masks: EHX_EINVAL, the outputs unwritten (the device form reads d_mask_of back together with the tiles' allowed counts:
 * the one wait ehx_knn_masked_device has too); n_masks > 64: EHX_EUNSUPPORTED; n_queries == 0: EHX_OK.  A NULL space is
 * refused (EHX_EINVAL) before the device is looked for.
 * The limit of 64 bitmaps is a CHOICE, not a measured bound and not a knob: the offsets of the masks' lists travel as one
 * kernel argument (512 bytes), a call stages n_masks * rows / 8 bytes of bitmaps (8 MB at 64 x 1 M rows), and 64 covers a
 * micro-batch of 1024 requests at 16 per filter, below which the scan's query tiles stop being shared.
 * Served as ehx_knn_masked_device serves it, query by query through its own bitmap (exact route: k > 48, spaces the int8
 * filter does not serve first, bitmaps of at most max(1024, rows / 128) allowed rows; else the scan route), with every
 * bitmap compacted in one set of launches, ONE plan of scan passes for the batch and the bit of the hit's own query's
 * bitmap tested where the scan collects its hits.  The plan is the batch's: a pass ends where the bitmap that has shown most
 * allowed rows reaches its quota (4096, 65 536, ...).  A bitmap whose rows CLUSTER late in the id space, behind rows the
 * other bitmaps of the batch allow, therefore meets its rows in one late pass under its sample's radius; when more than
 * about 4096 * 256 / k of them lie there (105 000 rows at k = 10, 22 000 at k = 48) its queries' pools overflow and they
 * are answered by the exact scan of the bitmap's list — the same answer, at that scan's cost (ehx_knn_among_device's
 * regime).  Bitmaps spread over the ids do not meet this.  DESIGN.md §e.16. */
int ehx_knn_masked_multi_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                const uint32_t* d_masks, uint32_t n_masks, uint64_t n_bits, const uint32_t* d_mask_of,
                                uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count);
/* Filtered search on the graph path: the k nearest ALLOWED rows found by walking a graph space's HNSW graph under a row
 * bitmap (allowed as ehx_knn_masked_device defines it: r < n_bits, r below the call's ONE snapshot of the row count, bit
 * r & 31 of word r >> 5 of d_mask set).  The walk, in words (tests/filtered_walk_model.py states it as code, DESIGN.md
 * §e.15 has the argument): the upper levels are descended greedily as in ehx_knn_device, the bitmap ignored; at level 0
 * there is one list of (distance, id) entries sorted by (distance, id), each expanded or not, starting with the descent's
 * end node whether or not it is allowed.  A step expands the closest unexpanded entry — rows that are not allowed are walked
 * through, never returned — and merges its unvisited level-0 neighbours into the list (NaN distances dropped); then, if the
 * list holds at least ef allowed entries, everything behind the ef-th allowed one is deleted, and everything behind position
 * cap (above, at EHX_WALK_LIST_FACTOR).  The walk ends when no entry is unexpanded; the answer is the first k allowed
 * entries.  ef = max(the space's ef, k).  This is the rule hnswlib >= 0.7 applies to a filter (isIdAllowed) plus the cap;
 * with every row allowed it is ehx_knn_device's strict walk, bit for bit.  ehx_params.search_width is ignored: this walk
 * always expands one node per step.  One query per call takes this batch form too.
 * route: EHX_WALK_GRAPH walks; EHX_WALK_EXACT gives ehx_knn_masked_device's answer, byte for byte; EHX_WALK_AUTO walks iff
 * allowed rows * EHX_WALK_LIST_FACTOR >= the rows the bitmap covers (min(n_bits, row count)) and is exact below; any other
 * value: EHX_EINVAL.  A flat space takes the exact route whatever a valid route says.
 * A walked answer is APPROXIMATE (recall as a graph search's, falling with the allowed share); the exact route has recall 1.
 * A walked answer may hold FEWER than k entries although k rows are allowed (the walk ended, or its list was cut at cap,
 * before it met k of them); n_bits == 0 or no bit set: count 0 on every route.  Sentinels (id 2^64 - 1, +Inf) beyond
 * d_out_count[i].  Errors as ehx_knn_masked_device: k == 0, NULL outputs, a NULL mask with n_bits > 0: EHX_EINVAL;
 * k > EHX_MAX_K_PAGED, row-sharded spaces, an effective ef above 4096, a walk over more than 2^30 rows, and on the exact
 * route rows longer than 40 960 floats: EHX_EUNSUPPORTED; a dropped space: EHX_ENOTFOUND; no device: EHX_ENODEVICE.
 * Completion as for ehx_knn_device (a walk returns with the kernel queued on `stream`; AUTO and EXACT have waited for the
 * device to read the allowed count back); a Set that rewrites rows in place waits for the call like for any search.
 * ehx_graph_counters accumulates the walk's rows fetched and expansions, ehx_stats its queries. */
int ehx_graph_knn_masked_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                const uint32_t* d_mask, uint64_t n_bits, uint32_t route, uint64_t* d_out_ids,
                                float* d_out_dist, uint32_t* d_out_count);
/* ehx_graph_knn_masked_device under a TABLE of row bitmaps, one per query: a micro-batch whose requests carry different
 * tenant, ACL or category filters, walked in ONE launch — one wavefront per query, each under its own bitmap — instead of
 * one ehx_graph_knn_masked_device call per distinct filter.  The table is ehx_knn_masked_multi_device's: d_masks holds
 * n_masks <= 64 bitmaps, dense, [n_masks][ceil(n_bits / 32)] words; query i is searched under bitmap d_mask_of[i].
 * Row i of the answer is, byte for byte (ids, distance bytes, count, the sentinels beyond it), what
 * ehx_graph_knn_masked_device returns for query i alone under bitmap d_mask_of[i] with the same route; the call takes ONE
 * snapshot of the row count, and bits at or above it are never looked at.  With n_masks == 1 the call equals
 * ehx_graph_knn_masked_device.
 * route: EHX_WALK_GRAPH walks every query; EHX_WALK_EXACT, and any valid route on a flat space, gives
 * ehx_knn_masked_multi_device's answer; EHX_WALK_AUTO decides PER BITMAP by ehx_graph_knn_masked_device's rule (allowed
 * rows of that bitmap * EHX_WALK_LIST_FACTOR >= the rows the bitmaps cover), so a batch may be MIXED: the queries of the
 * walked bitmaps go through one walk launch, the queries of the others through one exact answer
 * (ehx_knn_masked_multi_device's, over the same compaction), and every answer lands in its own row — approximate where
 * walked, exact elsewhere, as the one-bitmap call states.
 * Errors as ehx_graph_knn_masked_device and ehx_knn_masked_multi_device, with their codes: n_masks == 0 with
 * n_queries > 0, a NULL d_mask_of, an invalid route: EHX_EINVAL; n_masks > 64: EHX_EUNSUPPORTED; an entry of d_mask_of at
 * or above n_masks: EHX_EINVAL with the outputs unwritten, on every route (d_mask_of is read back — the call's one wait,
 * shared with the allowed counts where a route needs them — and checked before anything writes the outputs);
 * n_queries == 0: EHX_OK.  A NULL space is refused (EHX_EINVAL) before the device is looked for.
 * Completion as for ehx_graph_knn_masked_device, except that every route has waited once (for d_mask_of).
 * ehx_stats counts every query once; ehx_graph_counters the walked queries' work only.  DESIGN.md §e.17. */
int ehx_graph_knn_masked_multi_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                      const uint32_t* d_masks, uint32_t n_masks, uint64_t n_bits,
                                      const uint32_t* d_mask_of, uint32_t route, uint64_t* d_out_ids, float* d_out_dist,
                                      uint32_t* d_out_count);
/* Grouped kNN: exact top-k with at most per_group rows per group label — the k nearest ENTITIES of a caller who stores
 * several rows per entity (chunks of a document, frames of a video, variants of a product), without over-fetching.
 * d_group_of holds one label per row, d_group_of[0, n_labels); EHX_GROUP_NONE marks a row that is a group of its own.  The
 * call takes ONE acquire-load snapshot of the row count and searches the prefix n_eff = min(snapshot, n_labels); rows at or
 * above it are not searched, as with n_bits of a bitmap (n_labels above the row count is fine; rows appended after the
 * labels were built are not returned).  For query i, order the prefix rows by (canonical distance, id) under ehx_knn's
 * rules: NaN is never a neighbour, +-Inf are ordered, cosine is normalised, F16 rows are read as stored.  A row is
 * ELIGIBLE iff its label is EHX_GROUP_NONE, or fewer than per_group rows of the same label precede it in that order.  The
 * answer is the first k eligible rows in that order, with sentinels (id 2^64 - 1, +Inf) behind d_out_count[i].
 * Consequences: per_group >= k, or every label EHX_GROUP_NONE, gives ehx_knn's answer over the prefix, byte for byte;
 * per_group == 1 is "collapse": the best row of each of the k nearest groups.  (NOT served: the per_group nearest rows of
 * every winning group regardless of their distance — no radius bounds that.)
 * Errors: a NULL space: EHX_EINVAL, before the device is looked for; k == 0, per_group == 0, NULL outputs, a NULL d_group_of
 * with n_labels > 0: EHX_EINVAL; k > EHX_MAX_K_GROUPED, a row-sharded space, rows longer than 21 728 floats:
 * EHX_EUNSUPPORTED; a dropped space: EHX_ENOTFOUND.  n_labels == 0: count 0 for every query; n_queries == 0: EHX_OK.
 * Served by the falling-radius scan of the int8 filter where ehx_knn_device's large-k route would serve the prefix (flat
 * spaces whose first engine is the int8 filter, at least 64 queries; any k here) with a cap per label in its exact re-rank;
 * everything else — graph spaces (from their stored rows: the graph is not walked), small spaces, EHX_SCAN_F32 / _F16, small
 * batches, and the queries that scan hands on — by an exact pass over every prefix row in slabs of 4096, which costs what
 * the exhaustive pass costs plus a sort per slab.  A Set that rewrites rows in place waits for the call like for any
 * search.  Under row bitmaps: ehx_knn_grouped_masked_device; not on the graph walk.  DESIGN.md §e.19. */
#define EHX_GROUP_NONE 0xFFFFFFFFu
#define EHX_MAX_K_GROUPED 256u
int ehx_knn_grouped_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                           uint32_t per_group, const uint32_t* d_group_of, uint64_t n_labels, uint64_t* d_out_ids,
                           float* d_out_dist, uint32_t* d_out_count);
/* Grouped kNN under row bitmaps: "the k nearest documents this user may see, at most per_group chunks each" in one request —
 * ehx_knn_grouped_device's cap per label over the rows ehx_knn_masked_multi_device's filter allows.  Query i is answered
 * under bitmap d_mask_of[i] of a table laid out as ehx_knn_masked_multi_device's (n_masks <= 64 bitmaps of ceil(n_bits / 32)
 * words, back to back).  One bitmap is a table of one: with n_masks == 1, d_mask_of may be NULL and every query is under
 * bitmap 0.  d_group_of holds one label per row, as for ehx_knn_grouped_device.
 * The call takes ONE acquire-load snapshot of the row count and searches the prefix n_eff = min(snapshot, n_labels, n_bits).
 * Row r is ALLOWED for query i iff r < n_eff and bit r & 31 of word r >> 5 of its bitmap is set: a row at or above any of the
 * three limits is not allowed.
 * The rule is FILTER FIRST, THEN CAP.  Order the ALLOWED rows of query i by (canonical distance, id) under
 * ehx_knn_grouped_device's rules (NaN is never a neighbour, +-Inf are ordered, cosine is normalised, F16 rows are read as
 * stored).  An allowed row is ELIGIBLE iff its label is EHX_GROUP_NONE, or fewer than per_group ALLOWED rows of the same label
 * precede it in that order.  The answer is the first k eligible rows, with sentinels (id 2^64 - 1, +Inf) behind
 * d_out_count[i].  Rows that are not allowed neither appear nor count toward a cap: a group whose nearest row is forbidden is
 * represented by its nearest ALLOWED row — which ehx_knn_grouped_device followed by a filter on the host gets wrong.
 * Equivalences, byte for byte: with every bit set the call equals ehx_knn_grouped_device (at n_labels = min(n_labels,
 * n_bits)); with every label EHX_GROUP_NONE, or per_group at least the size of the largest group, it equals
 * ehx_knn_masked_multi_device (at n_bits = min(n_bits, n_labels)); a bitmap with no bit set gives count 0 for ITS queries
 * only.  n_bits == 0 (d_masks may then be NULL) or n_labels == 0: count 0 for every query.
 * Errors, the union of the two parents': a NULL space: EHX_EINVAL, before the device is looked for; k == 0, per_group == 0,
 * NULL outputs, a NULL d_group_of with n_labels > 0, a NULL d_masks with n_bits > 0, n_masks == 0 with n_queries > 0, a NULL
 * d_mask_of with n_masks > 1: EHX_EINVAL; d_mask_of[i] >= n_masks: EHX_EINVAL with the outputs unwritten (d_mask_of is read
 * back with the allowed counts and checked before anything writes the outputs); k > EHX_MAX_K_GROUPED, n_masks > 64, a
 * row-sharded space, rows longer than 21 728 floats: EHX_EUNSUPPORTED; a dropped space: EHX_ENOTFOUND; no device:
 * EHX_ENODEVICE.  n_queries == 0: EHX_OK.
 * Served per bitmap.  The falling-radius scan of the int8 filter, the bitmaps tested in its flush (one per query) and a cap
 * per label in its exact re-rank, where ehx_knn_grouped_device's scan would serve the prefix (flat spaces whose first engine
 * is the int8 filter), for bitmaps that allow more than max(1024, rows / 128) rows, given at least 64 such queries; its
 * first radius comes from a sample of at most 1024 allowed rows of the query's own bitmap.  Everything else — graph spaces
 * (from their stored rows: the graph is not walked), small spaces, EHX_SCAN_F32 / _F16, small batches, sparse bitmaps, and the
 * queries that scan hands on — by an exact pass over the bitmap's ALLOWED rows in slabs of 4096: the cost falls with the
 * allowed share.  The call waits for the device once (it reads the allowed counts back); a Set that rewrites rows in place
 * waits for the call like for any search.  Not on the graph walk.  DESIGN.md §e.20. */
int ehx_knn_grouped_masked_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                  uint32_t per_group, const uint32_t* d_group_of, uint64_t n_labels, const uint32_t* d_masks,
                                  uint32_t n_masks, uint64_t n_bits, const uint32_t* d_mask_of, uint64_t* d_out_ids,
                                  float* d_out_dist, uint32_t* d_out_count);
/* Partitioned kNN: exact kNN under a label column — the filter "this request may only see the rows of its own tenant /
 * namespace / collection", without a bitmap per tenant and without a limit on the tenants of one call.  d_label_of[0, n_labels)
 * holds one opaque 32-bit label per row, stored once (the column ehx_knn_grouped_device takes as d_group_of will do);
 * d_want[i] is the label query i is confined to.  NO value is special: 0xFFFFFFFF is an ordinary label here, although
 * EHX_GROUP_NONE uses that value in the grouped searches.  The call takes ONE acquire-load snapshot of the row count and
 * searches the prefix n_eff = min(snapshot, n_labels): row r is allowed for query i iff r < n_eff and d_label_of[r] ==
 * d_want[i].  Row i of the answer is, byte for byte, what ehx_knn_masked_device returns for query i alone under the bitmap
 * {r < n_eff : d_label_of[r] == d_want[i]}: (canonical distance, id) order, the NaN rule, +-Inf, cosine normalisation, F16
 * rows as stored, the sentinels beyond d_out_count[i].  A label no row carries gives count 0 for ITS queries only;
 * n_labels == 0 gives count 0 for every query; n_queries == 0: EHX_OK.  Every space kind ehx_knn_masked serves is served; a
 * graph space answers from its stored rows, its graph is not walked.
 * The number of distinct wanted labels is not limited: a call is served in device batches of 2048 queries, each compacting
 * the column for its own (at most 2048) labels.
 * Errors as ehx_knn_masked_multi_device: a NULL space: EHX_EINVAL, before the device is looked for; k == 0, NULL outputs or
 * queries, a NULL d_label_of with n_labels > 0, a NULL d_want: EHX_EINVAL; k > EHX_MAX_K_PAGED, a row-sharded space, rows
 * longer than the list scan's prepared query: EHX_EUNSUPPORTED; a dropped space: EHX_ENOTFOUND.
 * Served per wanted label by ehx_knn_masked_multi_device's rule — a label with more than max(1024, rows / 128) rows of the
 * prefix takes the int8 scan route when k <= 48 and the int8 filter serves the space (at most 127 labels can: they are
 * disjoint), with the test "the row's label is the query's" where the scan collects its hits; every other label is a short
 * list, scanned exactly, the labels few queries name all in ONE launch.  That cut was measured for the bitmap search and is
 * carried over, not measured for this call.  The pass plan is the batch's, as there: a label that clusters late in the id
 * space behind the others' rows may overflow its queries' pools, and they are then answered from its list — the same answer.
 * Waits: the device form reads d_want back (one wait for the whole call), then waits at most TWICE per device batch for the
 * compaction — the per-label row counts, and, only where a label scans, its rows before every tile — however many labels
 * the batch names; a batch on the scan route reads its verdict as ehx_knn_masked_multi_device does.  A Set that rewrites
 * rows in place waits for the call like for any search.  DESIGN.md §e.21. */
int ehx_knn_labeled_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                           const uint32_t* d_label_of, uint64_t n_labels, const uint32_t* d_want, uint64_t* d_out_ids,
                           float* d_out_dist, uint32_t* d_out_count);
/* Partitioned grouped kNN: "the k nearest documents OF THIS TENANT, at most per_group chunks each" in one request, for any
 * number of tenants per call — ehx_knn_grouped_device's cap per group label over the rows ehx_knn_labeled_device's filter
 * allows.  Two columns of n_labels entries each, under ONE length: d_group_of[r] is the entity row r belongs to
 * (EHX_GROUP_NONE: a group of its own, as in ehx_knn_grouped_device); d_label_of[r] is the partition — tenant, namespace,
 * collection — it lies in, where NO value is special (0xFFFFFFFF is an ordinary tenant here).  d_want[i] is the tenant query
 * i is confined to.
 * The call takes ONE acquire-load snapshot of the row count and searches the prefix n_eff = min(snapshot, n_labels).  Row r
 * is ALLOWED for query i iff r < n_eff and d_label_of[r] == d_want[i] (n_labels above the row count is fine; rows appended
 * after the columns were built are not returned).
 * The rule is FILTER FIRST, THEN CAP.  Row i of the answer is, byte for byte, what ehx_knn_grouped_masked_device returns for
 * query i alone under the bitmap {r < n_eff : d_label_of[r] == d_want[i]} with the same d_group_of, n_labels, k and
 * per_group: the ids, the distance bytes, the count, and the sentinels (id 2^64 - 1, +Inf) behind d_out_count[i].  What that
 * answer is, is defined there and in ehx_knn_grouped_device: (canonical distance, id) order; NaN is never a neighbour and
 * never counts toward a cap; +-Inf are ordered; cosine is normalised; F16 rows are read as stored.  Rows of other tenants
 * neither appear nor count toward a cap: a group whose nearest row belongs to another tenant is represented by its nearest
 * row OF THE QUERY'S TENANT — which ehx_knn_grouped_device followed by a filter on the host gets wrong.
 * Consequences, byte for byte: with every d_group_of entry EHX_GROUP_NONE, or per_group at least the size of the largest
 * group, the call equals ehx_knn_labeled_device; with every row carrying one label and every query wanting it, it equals
 * ehx_knn_grouped_device.  A label no row carries gives count 0 for ITS queries only; n_labels == 0 gives count 0 for every
 * query; n_queries == 0: EHX_OK.  The number of distinct wanted labels per call is not limited: a call is served in device
 * batches of 2048 queries, each compacting the label column for its own (at most 2048) labels.
 * Errors, the union of the two parents' with their codes and in their order: a NULL space: EHX_EINVAL, before the device is
 * looked for; k == 0, per_group == 0, NULL outputs, NULL queries with n_queries > 0, a NULL d_group_of or d_label_of with
 * n_labels > 0, a NULL d_want: EHX_EINVAL; k > EHX_MAX_K_GROUPED, a row-sharded space, rows longer than 21 728 floats:
 * EHX_EUNSUPPORTED; a dropped space: EHX_ENOTFOUND; no device: EHX_ENODEVICE.
 * Served per wanted label of a device batch, by ehx_knn_grouped_masked_device's rule: the falling-radius scan of the int8
 * filter, "the row's label is the query's" tested where the scan collects its hits and a cap per group in its exact re-rank,
 * on flat spaces whose first engine is the int8 filter, for labels with more than max(1024, rows / 128) rows of the prefix
 * (at most 127 can: they are disjoint), given at least 64 queries of the batch on such labels; any k here.  Its first radius
 * comes from a sample of at most 1024 rows of the query's own label.  Everything else — graph spaces (from their stored
 * rows: the graph is not walked), small spaces, EHX_SCAN_F32 / _F16, small batches, small tenants, and the queries that scan
 * hands on — by an exact pass over the label's rows in slabs of 4096, every query of the batch in ONE launch per slab
 * whatever number of labels they name: the cost falls with the tenant's share.  The cut was measured for the bitmap search
 * and is carried over, not measured for this call.
 * Waits: the device form reads d_want back (one wait for the whole call, the outputs unwritten until then), then waits at
 * most TWICE per device batch for the compaction — the per-label row counts, and, only where a label scans, its rows before
 * every tile; a batch on the scan route reads its verdict once.  A Set that rewrites rows in place waits for the call like
 * for any search.  Not on the graph walk.  DESIGN.md §e.22. */
int ehx_knn_grouped_labeled_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                   uint32_t per_group, const uint32_t* d_group_of, const uint32_t* d_label_of,
                                   uint64_t n_labels, const uint32_t* d_want, uint64_t* d_out_ids, float* d_out_dist,
                                   uint32_t* d_out_count);
/* Partitioned kNN on a STORED column: "the nearest rows of tenant T" with no side array.  label_col names a column of the
 * space (above); d_want[i] is the label query i is confined to.  Each call takes ONE acquire-load snapshot n_pub of the row
 * count and answers, byte for byte, what ehx_knn_labeled_device returns when given the stored column of that prefix with
 * n_labels = n_pub: ids, distance bytes, counts, sentinels, every error code of that call in its order, every space kind it
 * serves (a graph space answers from its stored rows).  0xFFFFFFFF is an ordinary label here — the rows never labelled.
 * label_col at or above EHX_MAX_COLUMNS: EHX_EINVAL.
 * The column's INDEX — row ids ordered by (label, row id), the table of distinct labels, where each begins, and for the
 * labels above the scan route's cut their rows before every 256-row tile and a by-rank sample — is built on the device once,
 * by a radix sort, and reused until the column or the row count changes: any write to an entry below the published row
 * count, and any append, leaves it stale.  With a fresh index a call makes no pass over the column, compacts nothing and takes
 * none of ehx_knn_labeled_device's two waits per device batch; the host form uploads queries and wanted labels only.  A stale
 * index costs one rebuild, on the call's stream, by the first search that finds it stale: one copy of the prefix, a histogram
 * pass, one sort pass per label byte that varies (one for fewer than 256 small tenant numbers), the boundary passes and four
 * short waits.  Measured once (scripts/bench_stored_labels.py): the rebuild takes 0.20 ms at 1 M rows and
 * 0.58 ms at 10 M rows for a column of 16 tenants, 0.79 and 6.8 ms for a column of random 32-bit labels.  A caller that appends
 * between every two searches pays the rebuild on every search.  Memory: an indexed column keeps 36 bytes per row of the
 * space's CAPACITY on the device beside the column's own 4 (the index's arrays are sized once, so a rebuild allocates
 * nothing), and 8 bytes per distinct label on the host. */
int ehx_knn_by_label_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k, uint32_t label_col,
                            const uint32_t* d_want, uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count);
/* ... from host pointers: the H2D / D2H copies of queries, wanted labels and results around it. */
int ehx_knn_by_label(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint32_t label_col, const uint32_t* want,
                     uint64_t* out_ids, float* out_dist, uint32_t* out_count);
/* Partitioned grouped kNN on STORED columns: group_col holds the entity of every row (EHX_GROUP_NONE: a group of its own —
 * also every row never given a value), label_col the tenant.  ONE snapshot n_pub of the row count; byte for byte what
 * ehx_knn_grouped_labeled_device returns when given the two stored columns of that prefix with n_labels = n_pub, with that
 * call's error codes in its order; a column number at or above EHX_MAX_COLUMNS: EHX_EINVAL.  group_col may equal label_col.
 * The index is label_col's, as above; group_col is read where it lies. */
int ehx_knn_grouped_by_label_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                    uint32_t per_group, uint32_t group_col, uint32_t label_col, const uint32_t* d_want,
                                    uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count);
int ehx_knn_grouped_by_label(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint32_t per_group,
                             uint32_t group_col, uint32_t label_col, const uint32_t* want, uint64_t* out_ids, float* out_dist,
                             uint32_t* out_count);
/* Exact range search: every row closer than a radius.  With D(q, x) the canonical distance ehx_knn reports (cosine, L2^2,
 * inner product as there), row x belongs to query i's answer iff D is not NaN and D <= d_radius[i] as a float comparison
 * (inclusive: a radius that equals a row's distance byte for byte includes that row; -Inf distances under inner product
 * are ordinary members).  The answer is ordered by (distance, id); its first min(total, max_results) pairs are written,
 * d_out_count[i] is that number, the rest of the row holds ehx_knn's sentinels (id 2^64 - 1, +Inf), and d_out_total[i]
 * (may be NULL) is the EXACT number of rows inside the radius even beyond max_results: total > count is how a caller sees
 * truncation.  Equivalently: ehx_knn(k = max_results) cut before the first distance above the radius, plus the count.
 * A NaN radius gives count 0 and total 0; +Inf every row with a non-NaN distance.  The answer describes the prefix of ONE
 * acquire load of the row count.  Outputs [n_queries][max_results].  1 <= max_results <= EHX_MAX_K_PAGED (0: EHX_EINVAL,
 * above: EHX_EUNSUPPORTED); NULL arguments, more than 2^24 queries: EHX_EINVAL; a row-sharded space, and rows longer than
 * 40 960 floats: EHX_EUNSUPPORTED; a dropped space: EHX_ENOTFOUND; no device: EHX_ENODEVICE.  Flat spaces whose first engine
 * is the int8 filter are answered by ONE pass of its scan under a threshold mapped from the radius and an exact re-rank of
 * the survivors; every other space, and the queries that scan cannot bound, by the canonical distance of every row — in
 * graph spaces too: the graph is not walked.  The call waits for the device before it returns (it reads a verdict back);
 * a Set that rewrites rows in place waits for it like for any search.  DESIGN.md §e.11. */
int ehx_range_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, const float* d_radius,
                     uint32_t max_results, uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count,
                     uint64_t* d_out_total);
/* Filtered range search: every ALLOWED row closer than a radius, query i under bitmap d_mask_of[i] of a table laid out as
 * ehx_knn_masked_multi_device's (n_masks <= 64 bitmaps of ceil(n_bits / 32) words, back to back).  One bitmap is a table of
 * one: with n_masks == 1, d_mask_of may be NULL and every query is under bitmap 0.  Row r is allowed for query i iff
 * r < n_bits, r is below the call's ONE acquire load of the row count and bit r & 31 of word r >> 5 of its bitmap is set.
 * The answer is ehx_range_device's over the allowed rows alone: ordered by (distance, id), the first min(total, max_results)
 * pairs written, d_out_count[i] that number, ehx_knn's sentinels behind them, and d_out_total[i] (may be NULL) the EXACT
 * number of allowed rows inside the radius, whatever was cut — rows the filter excludes are never counted.  Radii and
 * queries behave as in ehx_range_device (a NaN radius: count 0, total 0; +-Inf and non-finite queries are served).  An empty
 * bitmap, or n_bits == 0 (d_masks may then be NULL): count 0 and total 0.  Errors: max_results 0, n_masks 0 with queries,
 * NULL d_masks with n_bits > 0, NULL d_mask_of with n_masks > 1, other NULL arguments: EHX_EINVAL; d_mask_of[i] >= n_masks:
 * EHX_EINVAL with the outputs unwritten (d_mask_of is read back in the compaction's one wait); max_results >
 * EHX_MAX_K_PAGED, n_masks > 64, a row-sharded space, rows longer than 40 960 floats: EHX_EUNSUPPORTED; a dropped space:
 * EHX_ENOTFOUND; no device: EHX_ENODEVICE.  Routes, per query through its bitmap: a bitmap that allows more than
 * max(1024, rows / 128) rows of a flat space whose first engine is the int8 filter takes ONE pass of that scan with the
 * bitmap tested as candidates are collected, and an exact re-rank; every other query — sparse bitmaps, other engines, graph
 * spaces (the graph is not walked), radii the scan cannot bound — the canonical distance of every row of its bitmap's list.
 * The call waits for the device more than once (the compaction's counts, then a verdict per batch of 2048 queries).
 * DESIGN.md §e.18. */
int ehx_range_masked_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, const float* d_radius,
                            uint32_t max_results, const uint32_t* d_masks, uint32_t n_masks, uint64_t n_bits,
                            const uint32_t* d_mask_of, uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count,
                            uint64_t* d_out_total);
/* ---- predicate filters on stored columns: the bitmaps of the three exact searches above, built on the device ----
 * "tenant 7 AND timestamp >= T AND category != 3" without resolving it on the host and uploading n_masks * rows / 8 bytes per
 * call: a predicate is a CONJUNCTION of at most EHX_PRED_MAX_TERMS terms over the stored columns (above); a call carries up to
 * 64 predicates and searches query i under predicate pred_of[i].  A term holds for a row iff lo <= value <= hi, compared
 * UNSIGNED, where value is what column `col` stores for the row; EHX_TERM_NOT in flags inverts the term.
 * Row r is allowed by predicate P iff r is below the call's ONE acquire-load snapshot n_pub of the row count and every term of
 * P holds for the value stored in terms[t].col at row r.  A column never written reads as EHX_GROUP_NONE (0xFFFFFFFF) for
 * every row, a row never given a value reads as EHX_GROUP_NONE, as everywhere else.  lo == hi is equality; lo > hi is an
 * empty range: it never holds, and always holds under EHX_TERM_NOT; a column may be named by several terms; n_terms == 0
 * allows every row.  The comparison is unsigned: store signed or float attributes under an order-preserving map (a signed
 * integer with its sign bit flipped; a float's bits with the sign bit flipped when positive and all bits flipped when
 * negative).  Disjunctions and IN-lists are out of scope: split them into several predicates — several calls where one query
 * needs more than one — and merge the answers with ehx_merge_topk_device.
 * The answers are defined by the bitmap forms: byte for byte what ehx_knn_masked_multi_device, ehx_knn_grouped_masked_device
 * and ehx_range_masked_device return under the bitmaps the predicates describe with n_bits = n_pub — ids, distance bytes,
 * counts, totals, sentinels, routes, cuts and waits.  The bitmaps are evaluated by ONE kernel over the columns of the prefix
 * where they lie (no index, no copy: k_where.hip) into the table those searches compact; every column some
 * predicate names is read once, 4 bytes per row, and n_preds / 8 bytes per row are written.
 * preds is a HOST array of n_preds predicates in every form (at most 64 x 132 bytes), validated before anything is enqueued;
 * pred_of is a host array in the host forms and d_pred_of device memory in the _device forms, read back and checked in the
 * wait d_mask_of has.  Errors are those of the bitmap form, in its order, and: NULL preds or n_preds == 0 with
 * n_queries > 0, a term's column at or above EHX_MAX_COLUMNS, n_terms > EHX_PRED_MAX_TERMS, a flag bit other than
 * EHX_TERM_NOT, an entry of pred_of at or above n_preds: EHX_EINVAL, the outputs unwritten; n_preds > 64: EHX_EUNSUPPORTED,
 * the bitmap table's limit, for the reason given at ehx_knn_masked_multi_device; a NULL space: EHX_EINVAL before the device
 * is looked for; a row-sharded space: EHX_EUNSUPPORTED, as for every column call; n_queries == 0: EHX_OK.  A graph space
 * answers from its stored rows: the graph walk under predicates is NOT built.  (ORs of such predicates, IN-lists and the
 * graph walk under them are the Boolean filters' — ehx_knn_filter* and the block behind ehx_range_where.) */
#define EHX_PRED_MAX_TERMS 8
#define EHX_TERM_NOT 1u
typedef struct ehx_term {
  uint32_t col, lo, hi, flags; /* holds iff lo <= value <= hi, UNSIGNED; EHX_TERM_NOT inverts */
} ehx_term;
typedef struct ehx_pred {
  uint32_t n_terms;
  ehx_term terms[EHX_PRED_MAX_TERMS]; /* a conjunction */
} ehx_pred;
/* ehx_knn_masked_multi_device under the predicates' bitmaps. */
int ehx_knn_where_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k, const ehx_pred* preds,
                         uint32_t n_preds, const uint32_t* d_pred_of, uint64_t* d_out_ids, float* d_out_dist,
                         uint32_t* d_out_count);
int ehx_knn_where(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const ehx_pred* preds, uint32_t n_preds,
                  const uint32_t* pred_of, uint64_t* out_ids, float* out_dist, uint32_t* out_count);
/* ehx_knn_grouped_masked_device under the predicates' bitmaps, given the stored column group_col of the prefix as its labels
 * (read where it lies, as ehx_knn_grouped_by_label_device reads it; never written: every row a group of its own).  group_col
 * at or above EHX_MAX_COLUMNS: EHX_EINVAL.  With n_preds == 1, pred_of may be NULL: every query under predicate 0. */
int ehx_knn_grouped_where_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                 uint32_t per_group, uint32_t group_col, const ehx_pred* preds, uint32_t n_preds,
                                 const uint32_t* d_pred_of, uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count);
int ehx_knn_grouped_where(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint32_t per_group,
                          uint32_t group_col, const ehx_pred* preds, uint32_t n_preds, const uint32_t* pred_of,
                          uint64_t* out_ids, float* out_dist, uint32_t* out_count);
/* ehx_range_masked_device under the predicates' bitmaps.  With n_preds == 1, pred_of may be NULL. */
int ehx_range_where_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, const float* d_radius,
                           uint32_t max_results, const ehx_pred* preds, uint32_t n_preds, const uint32_t* d_pred_of,
                           uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count, uint64_t* d_out_total);
int ehx_range_where(ehx_space* s, size_t n_queries, const float* queries, const float* radius, uint32_t max_results,
                    const ehx_pred* preds, uint32_t n_preds, const uint32_t* pred_of, uint64_t* out_ids, float* out_dist,
                    uint32_t* out_count, uint64_t* out_total);
/* ---- Boolean filters on stored columns: OR of clauses, IN-lists, and the graph walk under them ----
 * "tenant = 3 OR timestamp >= T", "group IN (the 30 groups of this user)": a call carries a table of FILTERS and searches
 * query i under filter filter_of[i].  A filter is a DISJUNCTION of clauses: the run clauses[first_clause, first_clause +
 * n_clauses) of the call's clause array; runs of different filters may overlap, so clauses can be shared.  A clause is an
 * ehx_pred as above, unchanged: at most EHX_PRED_MAX_TERMS terms, ANDed.  In THIS form only, a term may carry EHX_TERM_IN:
 * then lo is the first index into values[] and hi the number of values, and the term holds iff the stored value equals one of
 * values[lo, lo + hi); EHX_TERM_NOT inverts it (NOT IN).  hi == 0 is the empty set: it never holds, and always holds under
 * EHX_TERM_NOT.  The values need not be sorted or distinct: the library packs a private, sorted, de-duplicated copy of every
 * term's set.  (ehx_knn_where* keep refusing every flag bit but EHX_TERM_NOT.)
 * Filter F allows row r iff r is below the call's ONE acquire-load snapshot n_pub of the row count and some clause of F's run
 * allows r; a clause allows r iff every one of its terms holds, range terms exactly as above (unsigned, a column never written
 * reading as EHX_GROUP_NONE, lo > hi the empty range).  A filter with n_clauses == 0 is the empty disjunction: it allows no
 * row and its queries get count 0.  A row that several clauses of a filter allow is ONE allowed row: it is returned once.
 * The answers are defined by the bitmap forms: byte for byte what ehx_knn_masked_multi_device, ehx_knn_grouped_masked_device,
 * ehx_range_masked_device and ehx_graph_knn_masked_multi_device return under the bitmaps the filters describe with n_bits =
 * n_pub — ids, distance bytes, counts, totals, sentinels, routes, cuts, counters and waits.  The bitmaps are evaluated by ONE
 * kernel over the columns of the prefix where they lie (k_filter.hip), every clause once however many filters
 * share it.  A graph space WALKS under the filters through ehx_graph_knn_filter* (ehx_knn_filter* answers from its stored
 * rows, like every exact search).
 * The table, its clauses, values and filters are HOST memory in every form, validated before anything is enqueued; filter_of
 * is a host array in the host forms and d_filter_of device memory in the _device forms, read back and checked in the wait
 * d_mask_of has.  Errors are those of the bitmap form, in its order (n_filters in the place of n_masks), and: a NULL table, NULL
 * clauses, filters or values where a count says there are some, n_filters == 0 with n_queries > 0, a filter's run past
 * n_clauses, an IN term with lo + hi > n_values, a term's column at or above EHX_MAX_COLUMNS, n_terms > EHX_PRED_MAX_TERMS,
 * a flag bit other than EHX_TERM_NOT | EHX_TERM_IN, an entry of filter_of at or above n_filters: EHX_EINVAL, the outputs
 * unwritten; n_filters > 64, n_clauses > EHX_FILTER_MAX_CLAUSES, more than EHX_FILTER_MAX_VALUES values summed over the IN
 * terms, a row-sharded space: EHX_EUNSUPPORTED; a NULL space: EHX_EINVAL before the device is looked for; n_queries == 0:
 * EHX_OK.  Not built: nesting beyond OR-of-AND, larger sets (a job for the column index), shards. */
#define EHX_TERM_IN 2u             /* lo = first index into values[], hi = number of values: holds iff the stored value equals one of them */
#define EHX_FILTER_MAX_CLAUSES 128 /* per call */
#define EHX_FILTER_MAX_VALUES 4096 /* per call: the sum of hi over the IN terms */
typedef struct ehx_filter {
  uint32_t first_clause, n_clauses; /* OR of clauses[first_clause .. first_clause + n_clauses) */
} ehx_filter;
typedef struct ehx_filters {
  const ehx_pred* clauses;
  uint32_t n_clauses;
  const uint32_t* values;
  uint32_t n_values;
  const ehx_filter* filters;
  uint32_t n_filters; /* <= 64, the bitmap table's limit */
} ehx_filters;        /* host memory in every form */
/* ehx_knn_masked_multi_device under the filters' bitmaps. */
int ehx_knn_filter_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                          const ehx_filters* filters, const uint32_t* d_filter_of, uint64_t* d_out_ids, float* d_out_dist,
                          uint32_t* d_out_count);
int ehx_knn_filter(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const ehx_filters* filters,
                   const uint32_t* filter_of, uint64_t* out_ids, float* out_dist, uint32_t* out_count);
/* ehx_knn_grouped_masked_device under the filters' bitmaps, the stored column group_col as its labels (as
 * ehx_knn_grouped_where*).  With n_filters == 1, filter_of may be NULL: every query under filter 0. */
int ehx_knn_grouped_filter_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                  uint32_t per_group, uint32_t group_col, const ehx_filters* filters,
                                  const uint32_t* d_filter_of, uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count);
int ehx_knn_grouped_filter(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, uint32_t per_group,
                           uint32_t group_col, const ehx_filters* filters, const uint32_t* filter_of, uint64_t* out_ids,
                           float* out_dist, uint32_t* out_count);
/* ehx_range_masked_device under the filters' bitmaps.  With n_filters == 1, filter_of may be NULL. */
int ehx_range_filter_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, const float* d_radius,
                            uint32_t max_results, const ehx_filters* filters, const uint32_t* d_filter_of, uint64_t* d_out_ids,
                            float* d_out_dist, uint32_t* d_out_count, uint64_t* d_out_total);
int ehx_range_filter(ehx_space* s, size_t n_queries, const float* queries, const float* radius, uint32_t max_results,
                     const ehx_filters* filters, const uint32_t* filter_of, uint64_t* out_ids, float* out_dist,
                     uint32_t* out_count, uint64_t* out_total);
/* ehx_graph_knn_masked_multi_device under the filters' bitmaps: route is EHX_WALK_AUTO, EHX_WALK_GRAPH or EHX_WALK_EXACT,
 * with that call's meaning (EHX_WALK_AUTO decides per filter from its allowed rows; a flat space takes the exact route). */
int ehx_graph_knn_filter_device(ehx_space* s, void* stream, size_t n_queries, const float* d_queries, uint32_t k,
                                const ehx_filters* filters, const uint32_t* d_filter_of, uint32_t route, uint64_t* d_out_ids,
                                float* d_out_dist, uint32_t* d_out_count);
int ehx_graph_knn_filter(ehx_space* s, size_t n_queries, const float* queries, uint32_t k, const ehx_filters* filters,
                         const uint32_t* filter_of, uint32_t route, uint64_t* out_ids, float* out_dist, uint32_t* out_count);
/* k-way merge of per-shard results (RCCL all-gather output): lists laid out
 * [n_lists][n_queries][k]; ids must already be global.  Ordered by (dist, id). */
int ehx_merge_topk_device(void* stream, size_t n_queries, uint32_t k, uint32_t n_lists,
                          const uint64_t* d_ids, const float* d_dist, const uint32_t* d_count,
                          uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count);
/* Same, with list l of each array starting l * stride BYTES after list 0 — e.g. the three arrays of every
 * shard packed into one buffer so that ONE all-gather moves them (embeddinghub_amd/sharded.py). */
int ehx_merge_topk_strided_device(void* stream, size_t n_queries, uint32_t k, uint32_t n_lists,
                                  const uint64_t* d_ids, size_t ids_stride, const float* d_dist, size_t dist_stride,
                                  const uint32_t* d_count, size_t count_stride, uint64_t* d_out_ids,
                                  float* d_out_dist, uint32_t* d_out_count);

/* ---- synthetic workload (EHX-GAUSS-1, include/ehx_datagen.h) ---- */
/* Appends rows [row0, row0+n_rows) of dataset `seed` to the space, generated on the device;
 * normalize!=0 L2-normalises each generated row first.  Rows get implicit decimal keys. */
int ehx_fill_synthetic(ehx_space* s, uint64_t seed, uint64_t row0, uint64_t n_rows, int normalize);
int ehx_gen_rows_device(void* stream, uint64_t seed, uint64_t row0, uint64_t n_rows, uint32_t dims,
                        int normalize, float* d_out /* n_rows x dims */);
/* EHX-MANIFOLD-1 (include/ehx_datagen.h): rows WITH STRUCTURE — points of a latent_dims-dimensional (1..64) linear
 * subspace of the dims-dimensional space plus 5 % isotropic noise — the workload on which a graph index meets a recall
 * target at a small ef (isotropic Gaussian rows at d = 768 defeat any graph: SURVEY.md §7).  Generated on
 * the device like ehx_fill_synthetic — a 10 M x 768 corpus never exists on the host; the host-side restatement
 * (oracle/datagen_oracle.hpp) produces the same bytes. */
int ehx_fill_manifold(ehx_space* s, uint64_t seed, uint64_t row0, uint64_t n_rows, uint32_t latent_dims, int normalize);
int ehx_gen_manifold_rows_device(void* stream, uint64_t seed, uint64_t row0, uint64_t n_rows, uint32_t dims,
                                 uint32_t latent_dims, int normalize, float* d_out /* n_rows x dims */);

/* ---- graph import (graph mode; persistence and strict-parity checks).  Graph spaces also build their
 * graph on the GPU as rows are Set (hnswlib addPoint semantics, k_insert.hip). ----
 * level0: n x (1 + 2M) u32 rows = [count, ids...]; levels: n ints; upper lists are passed as a CSR
 * over (node, level>=1): upper_off has n_upper+1 entries into upper_ids, upper_node/upper_level
 * name each list. */
int ehx_graph_import(ehx_space* s, uint64_t n, const uint32_t* level0, const int32_t* levels,
                     uint64_t n_upper, const uint32_t* upper_node, const int32_t* upper_level,
                     const uint64_t* upper_off, const uint32_t* upper_ids, uint32_t entry_point,
                     int32_t max_level);

/* Export of the graph built on the GPU (or imported): level0 [n][1+2M] u32 = (count, ids...), levels [n],
 * up_start [n] (index of a node's first upper list or 0xFFFFFFFF; lists of levels 1..L are consecutive),
 * up_lists [n_lists][M] padded with 0xFFFFFFFF.  Any output pointer may be NULL. */
int ehx_graph_export(ehx_space* s, uint32_t* level0, int32_t* levels, uint32_t* up_start, uint32_t* up_lists,
                     uint64_t up_lists_cap, uint64_t* n_lists, uint32_t* entry_point, int32_t* max_level);

/* ---- stats ---- */
int ehx_stats(ehx_space* s, ehx_stats_t* out);
int ehx_stats_reset(ehx_space* s);
/* Graph-search work counters since the last reset, the terms of SURVEY §8d's bytes-per-query formula plus a
 * kernel diagnostic: out[0] = rows fetched (n_dist), out[1] = level-0 expansions, out[2] = upper-level
 * expansions, out[3] = level-0 expansions whose adjacency row and visited words had been requested one
 * expansion ahead (k_graph.hip; wide walk: whose adjacency row the previous step had predicted and requested);
 * out[4] = steps of the wide walk (out[1] / out[4] = expansions per step); out[4..11] are phase timers in
 * -DEHX_GRAPH_PROFILE ablation builds (strict walk).  n_out <= 12.  Zeros for a space that never ran a graph search. */
int ehx_graph_counters(ehx_space* s, uint64_t* out, uint32_t n_out);

#ifdef __cplusplus
}
#endif
#endif /* EHX_H_ */
