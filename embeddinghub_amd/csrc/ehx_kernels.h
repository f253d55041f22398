// Internal launch interface between the C-ABI host code (ehx_*.cpp) and the gfx950 kernels.
// Not part of the public boundary (include/ehx.h is).
#pragma once

#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>

namespace ehx {

constexpr uint32_t kTileRows = 128;   // corpus rows per scan tile
constexpr uint32_t kTileQ = 256;      // queries per scan tile
constexpr uint32_t kTileRows16 = 256; // corpus rows per tile of the fp16 filter scan (k_flat16.hip)
constexpr uint32_t kBK = 32;          // k-depth of one LDS stage (floats)
constexpr uint32_t kCandSlots = 64;   // per-(query, block) candidate slots = one wave row
constexpr uint64_t kKeyInf = ~0ull;
constexpr uint32_t kNoNode = 0xFFFFFFFFu;  // graph kernels: no node / padding of an adjacency list

// (score, id) packed so that unsigned 64-bit order == (score asc, id asc).
__host__ __device__ inline uint32_t f32_to_ordered(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t u = __float_as_uint(f);
#else
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
#endif
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__host__ __device__ inline float ordered_to_f32(uint32_t o) {
  uint32_t u = o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu);
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(u);
#else
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
#endif
}

// LDS hand-over between the lanes of ONE wave (kernels launched with 64 threads per workgroup): the LDS accesses of
// a wave execute in program order, so a compiler-level fence is all a write -> read across lanes needs — no
// s_barrier and no drain of the LDS queue, which __syncthreads() would put on the dependent chain
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A value that is the same in every lane but reaches the wave through a shuffle or an LDS read is "divergent" to the
// compiler: everything derived from it sits in vector registers behind exec-mask branches.  readfirstlane moves it
// to a scalar register, and loop bookkeeping built on it runs on the scalar unit.
__device__ __forceinline__ uint32_t wave_uniform(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ float wave_uniform(float x) {
  return __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(x)));
}

// ascending bitonic sort of one u64 per lane across the 64-lane wave
__device__ __forceinline__ uint64_t wave_sort64(uint64_t key, int lane) {
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const uint64_t other = __shfl_xor(key, j, 64);
      const bool up = (lane & k) == 0;
      const bool lower = (lane & j) == 0;
      const uint64_t mn = key < other ? key : other;
      const uint64_t mx = key < other ? other : key;
      key = (lower == up) ? mn : mx;
    }
  }
  return key;
}

// input: bitonic sequence across lanes; output ascending
__device__ __forceinline__ uint64_t wave_bitonic_merge64(uint64_t key, int lane) {
#pragma unroll
  for (int j = 32; j > 0; j >>= 1) {
    const uint64_t other = __shfl_xor(key, j, 64);
    const uint64_t mn = key < other ? key : other;
    const uint64_t mx = key < other ? other : key;
    key = (lane & j) == 0 ? mn : mx;
  }
  return key;
}

// number of entries of the ascending array a[0..n) (any n) that are < key
__device__ __forceinline__ uint32_t lower_bound_lds(const uint64_t* a, uint32_t n, uint64_t key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Certification margin of the re-rank (rerank_kernel*): an upper bound of
//     | scan score of a row  -  that row's canonical (oracle-order) distance |
// for EVERY row of the space, so that  "worst kept score - margin > exact k-th distance"  proves that no
// row outside the candidate list can enter the top-k.  Both numbers are fp32 evaluations of the same real
// quantity T over the same fp32 inputs; with u = 2^-24 and Higham's gamma_n ~ n*u:
//   * matrix-core scan: one fma chain over d products                      -> |err| <= gamma_d     * W
//   * canonical order : products rounded, 4 chains of d/4 adds, 3 joining adds, cosine also rounds
//     x_i * inv_norm                                                        -> |err| <= gamma_(d/4+5) * W
//   with W = sum|q_i x_i| <= |q| |x| (Cauchy-Schwarz): cosine W <= 1.01 (both operands normalised by their
//   fp32 norms), inner product W <= |q| * max|x|, L2^2: every term is bounded by (|q| + max|x|)^2 (the row and
//   query norms enter the scan score through their own d-term sums).
//   eps_d = 1.3 * (d + 16) * u  >=  gamma_d + gamma_(d/4+5)  for every d <= 65536.
//   * the last affine operations (score = dot*a + b, D = u*S + v, 1 - sum) round relative to the result:
//     2e-6 * scale  (>= 32 u).
// Filter scans (fp16 / int8 lower bounds) need only the canonical-order term; the same formula covers them.
// max_sumsq = the largest |x|^2 ever written to the space (launch_row_stats); Inf or NaN there makes the
// margin infinite, i.e. nothing is certified and the exhaustive canonical pass answers.
__device__ __forceinline__ float cert_margin(int metric, uint32_t dims, float qn, float max_sumsq, float scale) {
  const float eps_d = 1.3f * ((float)dims + 16.0f) * 5.9604645e-8f;
  float base;
  if (metric == 2) {
    base = eps_d * 1.01f;
  } else {
    const float qb = __builtin_sqrtf(qn), mx = __builtin_sqrtf(max_sumsq);
    base = metric == 1 ? eps_d * 1.01f * qb * mx : eps_d * 1.01f * (qb + mx) * (qb + mx);
  }
  return base + 2e-6f * fmaxf(scale, fmaxf(qn, 1.0f));
}

// Int8 filter, L2^2: the B margin of a 32-row lane group over its tile — every row of the group has B_r >= bt + the
// margin, given bg <= min B of the group's rows and bt <= min B of the tile's (tileg8[tile][8 + g], tilep8[tile].w,
// k_misc.hip).  (bg - bt) rounded down, never negative: whichever writes of the two bounds a scan reads, bt + margin
// <= max(bg, bt) (erring low), which bounds the rows both describe.  bt = +inf (a tile of padding rows): 0.
__device__ __forceinline__ float i8_group_b_margin(float bg, float bt) {
  float m = 0.0f;
  if (bt < __builtin_inff()) m = bg < __builtin_inff() ? (bg - bt) * (1.0f - 1e-6f) : __builtin_inff();
  return m > 0.0f ? m : 0.0f;
}

}  // namespace ehx
#include "k_canon.h"          // the canonical distance arithmetic and every walker built on it: the ONE statement of the order
#include "k_exact_common.h"   // RowsView, the row layouts and the exact paths' walk, built on those walkers
namespace ehx {

struct ScanArgs {
  const float* Q;        // [q_tiles*256][ld] prepared queries (zero padded)
  const void* X;         // [cap][ld] stored rows (fp32, or fp16 when x_half), cap % 256 == 0, pad columns zero
  uint32_t x_half;       // 1: rows are IEEE fp16
  const float2* rowp;    // [cap] epilogue (a, b): approx distance = dot*a + b
  uint64_t* cand;        // [grid][256][64] per-block candidate slots (scratch)
  uint64_t* part;        // [q_tiles*256][n_chunks][lists_per_chunk][kprime] sorted partial top-k' keys
  uint32_t n;            // valid rows
  uint32_t ld;           // row stride in floats, % 32 == 0
  uint32_t tile0;        // first tile of this pass
  uint32_t n_tiles;      // tiles of this pass (tile = 128 rows)
  uint32_t list0;        // first sorted-list slot of this pass in `part`
  uint32_t lists_total;  // sorted lists per query in `part` (all passes)
  uint32_t q_tiles;
  uint32_t n_chunks;
  uint32_t tiles_per_chunk;
  uint32_t kprime;       // <= 64
  uint32_t* err;         // device error counter (bounded-retry guard tripped)
  unsigned long long* gthr;  // [q_tiles*256] global per-query threshold keys (init ~0 per launch; 8-wave kernel)
  uint32_t xcd_map;      // 1: blocks of one chunk share an XCD (grid % 8 == 0, n_chunks % 8 == 0)
};

constexpr uint32_t kScanListsPerChunk = 2;  // sorted key lists each (query, chunk) publishes: one per wave row of the 8-wave kernels
hipError_t launch_flat_scan8(const ScanArgs& a, hipStream_t st);  // the fp32 matrix-core scan (k_flat8.hip: 8 waves, two per SIMD)

// ---- fp16-MFMA filter scan (k_flat16.hip) ----
struct ScanArgs16 {
  const __half* Q;       // [q_tiles*256][ld] unit-normalised queries, binary16 (zero padded), scan16_index layout
  const __half* X;       // [cap][ld] scan copy: unit-normalised rows, binary16, scan16_index layout; cap % 256 == 0
  const float2* rowp;    // [cap] (a_r, b_r): S = b_r*gamma_q + a_r*dot;  padding rows (0, +inf)
  const float* qgamma;   // [q_tiles*256] gamma_q
  float eps;             // accumulator start value: bound of |dot16 - true dot|
  uint32_t cos;          // 1: every valid row has (a, b) = (-1, 1) and gamma = 1 (cosine): fast phase 1
  float* dump = nullptr; // sample pass: write every score to dump[row - tile0*256][q_tiles*256] instead of keeping lists
  uint64_t* cand;
  uint64_t* part;
  uint32_t n;
  uint32_t ld;           // row stride in halves, % 128 == 0 (a tile = a whole number of LDS ring revolutions)
  uint32_t tile0, n_tiles, list0, lists_total, q_tiles, n_chunks, tiles_per_chunk, kprime;
  uint32_t* err;
  unsigned long long* gthr;
  uint32_t xcd_map;
};
// Stage-blocked layout of the fp16 scan copy and of the fp16 query tiles: the matrix is cut into tiles of
// 256 rows and stages of 32 columns; one (tile, stage) block is 256 rows x 64 bytes = 16 KiB, stored
// contiguously in exactly the image the kernel wants in LDS (16-byte chunk c of row r at physical chunk
// c ^ ((r>>2)&3)), blocks ordered [tile][stage].  A stage's DMA is then a linear 16-KiB copy: every
// global->LDS instruction moves 1 KiB = 8 full cache lines.  Index (in halves) of element (row, col):
__host__ __device__ inline size_t scan16_index(uint64_t row, uint32_t col, uint32_t ld16) {
  const uint64_t tile = row >> 8;
  const uint32_t rr = (uint32_t)(row & 255u), kt = col >> 5, cc = col & 31u;
  const uint32_t chunk = (cc >> 3) ^ ((rr >> 2) & 3u);
  return ((size_t)(tile * (ld16 >> 5) + kt) * 256u + rr) * 32u + chunk * 8u + (cc & 7u);
}
// The fp16 query tiles use the same blocks, [q_tile][stage], with stages 0..2 of every tile stored once more
// after its last stage (the kernel's DMA runs three stages ahead and wraps into the next row tile without
// re-basing its query pointer mid-tile): (ld16/32 + 3) blocks per query tile.
__host__ __device__ inline size_t scanq16_index(uint64_t row, uint32_t stage, uint32_t cc, uint32_t ld16) {
  const uint64_t tile = row >> 8;
  const uint32_t rr = (uint32_t)(row & 255u);
  const uint32_t chunk = (cc >> 3) ^ ((rr >> 2) & 3u);
  return ((size_t)(tile * ((ld16 >> 5) + 3u) + stage) * 256u + rr) * 32u + chunk * 8u + (cc & 7u);
}
inline size_t scanq16_halves(uint32_t q_rows, uint32_t ld16) { return (size_t)(q_rows >> 8) * ((ld16 >> 5) + 3u) * 256u * 32u; }
constexpr size_t kScan16TailPadHalves = 3u * 256u * 32u;  // X16 tail padding: three stage blocks (DMA read-ahead)
size_t scan16_lds_bytes();
hipError_t launch_flat_scan16(const ScanArgs16& a, hipStream_t st);
// bound of |<fp16(q^), fp16(x^)> accumulated in fp32 - <q^, x^>| for unit vectors of `dims` elements
inline float scan16_eps(uint32_t dims) { return 1.0e-3f + 2.0e-7f * (float)dims; }

// ---- int8-MFMA filter scan (k_flati8.hip) ----
// (kPoolCap, the candidate keys one query can collect in one pass, is k_exact_common.h's: the pool re-rank carves LDS by it)
constexpr uint32_t kSyncWordsI8 = 1024; // lock-step progress words of the int8 scan: [n_chunks <= 256][4 query tiles]
constexpr uint32_t kMerged8 = 256;     // default width of the running best list of the int8 pipeline
constexpr uint32_t kMerged8Max = 1024; // widest list (a space widens its list when queries go uncertified: ehx_flat.cpp)
constexpr uint32_t kLabelHead = 2048;  // wanted labels in front of the label column of ScanArgsI8::allow_label's block
struct ScanArgsI8 {
  const int8_t* Q;        // [q_tiles][ld/64 + 3][256][64] int8 query tiles, scan8 stage-blocked layout
  const int8_t* X;        // scan copy, scan8_index layout; cap % 256 == 0
  const float4* rowp;     // [cap + 512] (A, B, C, D) per row; padding rows (0, +inf, 0, 0)
  const float4* tilep;    // [cap/256 + 2] (max|A|, max|C|, max|D|, min B) per 256-row tile
  const float* tileg;     // [cap/256 + 2][16]: [0..8) max |A| of each 32-row lane group of the tile (g = 4 wr + (l >> 4)),
                          // [8..16) min B of the group, ABSOLUTE (-inf: no margin); the scan derives the group's B margin over
                          // tilep[tile].w itself (i8_group_b_margin; round 6)
  const uint8_t* perm;    // [cap] row index inside its tile of the row stored at each position (identity: unsorted tile)
  const float4* qparams;  // [q_tiles*256] (s_q, e_q, gamma_q, smallest threshold the query was scanned with so far)
  const float* thr;       // [q_tiles*256] score threshold of this pass per query (-inf: padding query)
  float* dump = nullptr;  // sample pass: every lower bound -> dump[scan8_dump_index(q, row - tile0*256, rows of the sample)]
  uint64_t* cand;         // [grid][512][64] staging slots
  uint64_t* pool;         // [q_tiles*256][pool_cap] collected (score, id) keys of this pass, unsorted
  uint32_t* pool_cnt;     // [q_tiles*256]
  uint32_t* ovf;          // [q_tiles*256] 1 = the pool overflowed: the query must be answered by another engine
  uint32_t pool_cap;
  uint32_t n;
  uint32_t ld;            // bytes (= k-values) per row of the scan copy, % 64 == 0 (whole 64-byte stages)
  uint32_t tile0, n_tiles, q_tiles, n_chunks, tiles_per_chunk;
  uint32_t xcd_map;
  uint32_t* sync = nullptr;  // lock-step words, zero before the launch (nullptr: off): sync_tol == 0: [n_chunks] counters,
                             // one add per workgroup and ring revolution; sync_tol > 0: [n_chunks][4] progress words,
                             // tiles completed by each of the chunk's (<= 4) query-tile workgroups
  uint32_t sync_tol = 0;     // > 0: a workgroup does not run more than this many TILES ahead of its slowest sibling
  uint32_t skew = 0;         // half-tile workgroups: the second-resident wave of a SIMD starts skew x 64 cycles late
  uint32_t group_b = 0;      // 1: the alarm level of a lane group uses the group's B margin (L2^2: B_r = |x_r|^2 varies)
  const uint32_t* allow = nullptr;  // optional row bitmap (masked kNN, ehx_masked.cpp): bit id & 31 of word id >> 5; a hit whose
  uint32_t allow_bits = 0;          // row id is >= allow_bits or whose bit is clear is dropped before it takes a pool slot
  uint32_t allow_per_query = 0;     // 1: a bitmap per query (ehx_knn_masked_multi*, several masks) — allow is ONE block,
                                    // [q_tiles * 256] word offsets from its start (query q: allow[q]) | the bitmaps
  uint32_t allow_label = 0;         // 1: a label column instead of bitmaps (ehx_knn_labeled*) — allow is ONE block,
                                    // [kLabelHead >= q_tiles * 256] wanted labels (query q: allow[q]) | label_of[0,
                                    // allow_bits); a hit survives iff its row's label is its query's
  // The flat int8 chain's long passes only (ehx_flat.cpp; the compile-time-slot loop without a bitmap): every other caller
  // leaves both null and launches the kernels it always launched.
  const uint32_t* bounds = nullptr;  // [n_chunks + 1] tile range of every chunk, relative to tile0 (the share planner's table,
                                     // ehx_balance.h; host-mapped or device memory); nullptr: chunk * tiles_per_chunk
  uint64_t* stamps = nullptr;        // [2 * grid] wall_clock64() of every workgroup before its prologue | after its last flush
};
// Stage-blocked layout of the int8 scan copy / query tiles: tiles of 256 rows, stages of 64 columns (bytes); one
// (tile, stage) block is 256 rows x 64 B = 16 KiB in exactly the LDS image of the kernel (16-byte chunk c of row r
// at physical chunk c ^ ((r>>2)&3)); blocks ordered [tile][stage].  Byte index of element (row, col):
// Chunk swizzle of a row: the scan reads a block's fragment with ONE ds_read_b128 — lane l takes chunk l >> 4 of row
// l & 15 — and the LDS serves that instruction in four groups of 16 lanes ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and
// the same + 32: MI355X_MICROARCH.md, LDS).  With g = (0, 2, 3, 1)[(row >> 2) & 3] the 16 lanes of every group fall
// into 16 different 16-byte slots of the 256-byte LDS row (rows r, r+4, r+8, r+12 of a group carry chunks that differ
// after the XOR): conflict-free.  (Rounds 2-3 used (row >> 2) & 3, made for the 32x32x32 fragment's lane pattern.)
__host__ __device__ inline uint32_t scan8_swz(uint32_t rr) { return (0x78u >> (((rr >> 2) & 3u) * 2u)) & 3u; }
__host__ __device__ inline size_t scan8_index(uint64_t row, uint32_t col, uint32_t ld8) {
  const uint64_t tile = row >> 8;
  const uint32_t rr = (uint32_t)(row & 255u), kt = col >> 6, cc = col & 63u;
  const uint32_t chunk = (cc >> 4) ^ scan8_swz(rr);
  return ((size_t)(tile * (ld8 >> 6) + kt) * 256u + rr) * 64u + chunk * 16u + (cc & 15u);
}
// query tiles: the same blocks, [q_tile][stage], stages 0..2 stored once more after the last (DMA read-ahead)
__host__ __device__ inline size_t scanq8_index(uint64_t row, uint32_t stage, uint32_t cc, uint32_t ld8) {
  const uint64_t tile = row >> 8;
  const uint32_t rr = (uint32_t)(row & 255u);
  const uint32_t chunk = (cc >> 4) ^ scan8_swz(rr);
  return ((size_t)(tile * ((ld8 >> 6) + 3u) + stage) * 256u + rr) * 64u + chunk * 16u + (cc & 15u);
}
// the sample pass's dump of lower bounds (flat_scan_i8_kernel<DUMP> -> sample_select256_kernel): blocks of 16 queries x 16
// sample rows = 1 KiB, inside a block a query's 16 rows are contiguous; element index of (query q, sample row `row`) when
// the sample holds n_s rows (n_s % 16 == 0)
__host__ __device__ inline size_t scan8_dump_index(uint32_t q, uint32_t row, uint32_t n_s) {
  return ((((size_t)(q >> 4) * (n_s >> 4)) + (row >> 4)) << 8) + ((q & 15u) << 4) + (row & 15u);
}
inline size_t scanq8_bytes(uint32_t q_rows, uint32_t ld8) { return (size_t)(q_rows >> 8) * ((ld8 >> 6) + 3u) * 256u * 64u; }
constexpr size_t kScan8TailPadBytes = 3u * 256u * 64u;  // X8 tail padding: three stage blocks (DMA read-ahead)
size_t scan_i8_lds_bytes();
hipError_t launch_flat_scan_i8(const ScanArgsI8& a, hipStream_t st);
// scan copy of rows [row0, row0+n): X8 = int8(x/|x| / s_r), rowp8 = (A, B, C, D); then the tile parameters of
// every tile touching the range.  n_unsafe[2]: [0] += rows the filter cannot bound, [1] += lane groups whose min B lies more
// than 0.1 % above their tile's (the scan uses the groups' B margins only in spaces that have any).
// Full tiles inside [sort_lo, sort_hi) (and inside the rows written) are stored ordered by quantisation step, every row's
// step raised to its 32-row lane group's maximum (perm8[position] = row index inside the tile, tileg8[tile][8 of 16] =
// |A| of each group: k_misc.hip, "rows of a tile ordered by quantisation step"); every other touched tile keeps the
// row order and the rows' own steps.  The caller guarantees that no scan can read the tiles of [sort_lo, sort_hi)
// meanwhile.  scratch: device memory of make_scan8_scratch_bytes(...) bytes.
size_t make_scan8_scratch_bytes(uint64_t row0, uint64_t n, uint64_t sort_lo, uint64_t sort_hi);
hipError_t launch_make_scan8(const void* X, int x_half, uint64_t row0, uint64_t n, uint32_t dims, uint32_t ld,
                             uint32_t ld8, int metric, int8_t* X8, float4* rowp8, float4* tilep8, uint8_t* perm8,
                             float* tileg8, uint64_t sort_lo, uint64_t sort_hi, void* scratch,
                             unsigned long long* n_unsafe, hipStream_t st);
hipError_t launch_tile_ids(uint64_t* out, uint64_t t0, uint64_t t1, uint64_t a0, uint64_t a1, hipStream_t st);
// perm8 of rows [row0, row0+n): identity
hipError_t launch_perm8_pad(uint8_t* perm8, uint64_t row0, uint64_t n, hipStream_t st);
// rowp8 for padding rows [row0, row0+n): (0, +inf, 0, 0); tilep8 for padding tiles [t0, t0+n): never alarm
hipError_t launch_rowp8_pad(float4* rowp8, uint64_t row0, uint64_t n, hipStream_t st);
hipError_t launch_tilep8_pad(float4* tilep8, uint64_t t0, uint64_t n, hipStream_t st);
// int8 query tiles + (s_q, e_q, gamma_q) + (u, v) with D = u*S + v; thr[q] = +inf for q < nq, -inf for padding
// ... in ONE launch with the prepared fp32 rows of the re-rank (launch_prep_queries' q_out) and the zeroing of the scan's
// control words ctl = [q_rows] pool counts | [q_rows] overflow flags | [256] lock-step counters
hipError_t launch_prep_queries_i8(const float* q_in, uint32_t nq, uint32_t dims, uint32_t ld, uint32_t ld8,
                                  uint32_t q_rows, int metric, float* q_out, int8_t* Q8, float4* qparams, float2* quv,
                                  float* thr, uint32_t* ctl, hipStream_t st);
// sample pass -> first thresholds: thr[q] = the rank-th (<= 64) smallest of scores[0..n_rows)[q] (+inf if fewer)
hipError_t launch_sample_select256(const float* scores, uint32_t n_rows, uint32_t q_rows, uint32_t nq,
                                   uint32_t rank, float* thr, hipStream_t st);
// merge one pass's pool into the query's running best kMerged8 keys (seed: keep what `merged` holds); publishes
// thr[q] = score of the kprime-th best (+inf while fewer are known), lowers qparams[q].w to the threshold the merged
// pass was scanned with, and empties the pool (pool_cnt = 0)
// (width: the list's length, a power of two in [256, kMerged8Max], kprime <= width)
hipError_t launch_select256(const uint64_t* pool, uint32_t* pool_cnt, uint32_t pool_cap, uint32_t nq, uint32_t kprime,
                            uint64_t* merged, uint32_t width, bool seed, float* thr, float4* qparams, hipStream_t st);
struct Rerank256Args {
  const float* Q;          // prepared (canonical) queries [*][ld]
  const void* X;
  uint32_t x_half;
  const float* inv_norm;
  const uint64_t* merged;  // [nq][width] keys (S_lower, id), ascending
  uint32_t width;          // list stride
  const uint32_t* ovf;     // [nq] pool overflow flags
  const float2* quv;       // [nq] D = u*S + v
  const float4* qparams;   // [nq] .w = the smallest threshold the query was scanned with (select256_kernel)
  const float* max_sumsq;
  uint64_t* out_ids;
  float* out_dist;
  uint32_t* out_count;
  unsigned long long* n_uncertified;
  uint32_t* uncert_flags;
  uint32_t nq, k, kprime, n, dims, ld;
  int metric;
};
hipError_t launch_rerank256(const Rerank256Args& a, hipStream_t st);

// sample pass -> starting thresholds: gthr[q] = key of the kprime-th smallest of scores[0..n_rows)[q] (id part
// 0xFFFFFFFF, so a row that ties the threshold still passes); one wave per query
hipError_t launch_sample_select(const float* scores, uint32_t n_rows, uint32_t q_rows, uint32_t nq, uint32_t kprime,
                                unsigned long long* gthr, hipStream_t st);

// scan copy of rows [row0, row0+n): X16 = fp16(x/|x|), rowp16 = (a_r, b_r) per metric.  Rows the filter
// cannot bound (non-finite or denormal-range norms) are counted in *n_unsafe (the space then stays on
// the fp32 scan).
hipError_t launch_make_scan16(const void* X, int x_half, uint64_t row0, uint64_t n, uint32_t dims, uint32_t ld,
                              uint32_t ld16, int metric, __half* X16, float2* rowp16, unsigned long long* n_unsafe,
                              hipStream_t st);
// filter-side query preparation: Q16 = fp16(q/|q|) padded to [q_rows][ld16]; qgamma[q]; quv[q] = (u, v) with
// D = u*S + v.  Queries the filter cannot bound get u = NaN (never certified -> fp32 re-run).
hipError_t launch_prep_queries16(const float* q_in, uint32_t nq, uint32_t dims, uint32_t ld16, uint32_t q_rows,
                                 int metric, __half* Q16, float* qgamma, float2* quv, hipStream_t st);

// one wave per query: k-way merge of the per-chunk sorted key lists -> top-kprime keys
// (merges `n_chunks` consecutive lists of each query; a query's lists are `lists_stride` apart)
// seed: start from the keys already in `merged` (earlier passes); gthr (optional): publish the k'-th best
hipError_t launch_flat_merge(const uint64_t* part, uint32_t nq, uint32_t n_chunks, uint32_t kprime,
                             uint64_t* merged /*[nq][64]*/, hipStream_t st, uint32_t lists_stride, bool seed = false,
                             unsigned long long* gthr = nullptr);

// canonical (oracle-order) distances of the merged candidates, sort by (dist, id), emit top-k.
struct RerankArgs {
  const float* Q;          // prepared queries [*][ld]
  RowsView rows;           // fp32 or fp16 rows, plain layout
  const uint64_t* merged;  // [nq][64] keys (approx score, id)
  uint64_t* out_ids;       // [nq][k]
  float* out_dist;         // [nq][k]
  uint32_t* out_count;     // [nq]
  unsigned long long* n_uncertified;  // device counter
  uint32_t nq, k, kprime;
  // fp16-filter scans: the keys hold S_lower; D = u*S + v maps the worst candidate back to a distance.
  // nullptr for the fp32 scan.
  const float2* quv = nullptr;
  uint32_t* uncert_flags = nullptr;  // [nq] 1 = not certified (optional)
  uint32_t exact_keys = 0;           // keys come from launch_exhaustive (exact distances): skip the certification
  const float* max_sumsq = nullptr;  // largest |x|^2 in the space (device scalar, launch_row_stats): margin of the certificate
  uint32_t out_stride = 0, out_offset = 0;  // paged output: row stride (0 = k) and first column of this page
};
hipError_t launch_rerank(const RerankArgs& a, hipStream_t st);
// canonical distance of every row for each of nq prepared queries: out[q][block][64] best (distance, id) keys
// (floor, optional: per query, only keys strictly above floor[q] are kept — paging for k > 64)
hipError_t launch_exhaustive(const float* Q, const RowsView& rows, uint32_t rows_per_block, uint32_t n_blocks, uint32_t nq,
                             const uint64_t* floor, uint64_t* out, hipStream_t st);
hipError_t launch_set_floor(const uint64_t* merged, uint32_t nq, uint64_t* floor, hipStream_t st);
// one query from host-visible memory against a small shard in one launch (k_flat.hip: single_query_kernel)
struct SingleQueryArgs {
  const float* q_in;        // [dims] raw query (host-visible pinned memory, or device memory)
  RowsView rows;            // fp32 or fp16 rows, plain layout
  uint64_t* part;           // [n_blocks][64] scratch: every workgroup's best keys
  uint32_t* ticket;         // device counter, 0 between calls
  uint64_t* out_ids;        // [k]  host-visible
  float* out_dist;          // [k]  host-visible
  uint32_t* out_count;      // [1]  host-visible
  uint32_t* done_flag;      // host-visible: set to `seq` when the results are in place
  uint32_t seq, rows_per_block, k;
};
hipError_t launch_single_query(const SingleQueryArgs& a, uint32_t n_blocks, hipStream_t st);

// prepared queries: copy into the padded [q_rows][ld] buffer, L2-normalise for cosine
hipError_t launch_prep_queries(const float* q_in, uint32_t nq, uint32_t dims, uint32_t ld,
                               uint32_t q_rows, int metric, float* q_out, hipStream_t st);

// sub-batches of the engine chain: rows idx[0..m) of the caller's query batch gathered into a dense [m][dims] matrix,
// and a sub-batch's results written back to the rows they belong to
hipError_t launch_gather_queries(const float* src, const uint32_t* idx, uint32_t m, uint32_t dims, float* dst,
                                 hipStream_t st);
hipError_t launch_scatter_results(const uint64_t* ids, const float* dist, const uint32_t* cnt, const uint32_t* idx,
                                  uint32_t m, uint32_t k, uint64_t* out_ids, float* out_dist, uint32_t* out_cnt,
                                  hipStream_t st);

// neighbours of stored rows (k_bykey.hip): the query batch gathered from the rows themselves, and the row's own id
// removed from its (k + 1)-long list
constexpr uint32_t kMaxShardBases = 64;   // (ehx_space_create accepts up to 64 shards)
struct ShardBases {
  const void* p[kMaxShardBases];   // dX of shard i (an unsharded space: p[0])
};
struct GatherRowsArgs {
  const uint64_t* row_ids;  // [n] global row ids
  RowsView rows;            // shape, layout and row count (an id at or above it gives a zero row, valid = 0); X: see bases
  ShardBases bases;         // rows of shard g % G, local row g / G; peers are read over the access ehx_init opened
  float* out;               // [n][dims] what ehx_get_by_id returns for every row
  uint32_t* valid;          // [n]
  uint32_t n, G;
};
hipError_t launch_gather_rows(const GatherRowsArgs& a, hipStream_t st);
struct DropSelfArgs {
  const uint64_t* ids;      // [n][k + 1] result lists of the k + 1 search
  const float* dist;        // [n][k + 1]
  const uint32_t* count;    // [n]
  const uint64_t* row_ids;  // [n] every query's own row id
  const uint32_t* valid;    // [n] launch_gather_rows: 0 = the query's row id was out of range (count 0)
  uint64_t* out_ids;        // [n][k]
  float* out_dist;          // [n][k]
  uint32_t* out_count;      // [n]
  uint32_t n, k;
};
hipError_t launch_drop_self(const DropSelfArgs& a, hipStream_t st);

// rows written from device memory (k_rowio.hip): the gather's mirror, one wave per source row
struct ScatterRowsArgs {
  const void* src;          // dense [*][dims] source rows, fp32 or binary16 (src_half); element-aligned
  const uint32_t* src_idx;  // [n] source row of work item i, or nullptr: i (a shard passes the batch positions of its rows)
  const uint64_t* dst_row;  // [n] stored row of work item i, ~0 = not written; or nullptr: row0 + i (a contiguous append)
  uint64_t row0;
  void* X;                  // the stored rows [*][ld], fp32 or binary16 (x_half); columns [dims, ld) are not touched
  uint32_t ld, dims, x_half, src_half;
  uint32_t n;
};
hipError_t launch_scatter_rows(const ScatterRowsArgs& a, hipStream_t st);

// exact kNN among a caller's list of row ids (k_among.hip): the canonical distance of every listed row, best 64
// (distance, id) keys per workgroup -> out[q][n_blocks][64] (launch_flat_merge's input)
constexpr uint32_t kAmongTileQ = 8;     // shared list: queries a workgroup applies a staged tile of rows to
constexpr uint32_t kAmongTileRows = 8;  // ... rows per staged tile
struct AmongArgs {
  const float* Q;            // prepared queries [nq][ld] (launch_prep_queries)
  RowsView rows;             // stored rows, any layout
  const uint64_t* cand_ids;  // [n_cand] global row ids; an id at or above rows.n_rows is ignored
  const uint64_t* cand_off;  // nullptr: every query shares cand_ids[0, n_cand); else [nq + 1], query q owns [off[q], off[q + 1])
  const uint64_t* floor;     // optional, per query: only keys strictly above floor[q] are kept (paging for k > 64)
  uint64_t* out;             // [nq][n_blocks][64]
  uint64_t n_cand;
  uint32_t nq;
  uint32_t n_blocks;         // workgroups per query (or query tile): each walks its steps of the list in a grid-stride loop
  const uint64_t* cand_end;  // optional, with cand_off: [nq], query q owns [off[q], end[q]) — queries may then share a list;
                             // nullptr: off + 1
};
bool among_tiled(const AmongArgs& a);          // the shared-list kernel serves (cand_off == nullptr and the tiles fit in LDS)
uint32_t among_max_ld();                       // longest row stride (floats) the kernels take: a prepared query must fit in LDS
uint32_t among_step_rows(const AmongArgs& a);  // list entries one workgroup takes per step of its loop
hipError_t launch_among(const AmongArgs& a, hipStream_t st);
// a page of results from merged keys that hold exact canonical distances ([nq][64] ascending, launch_flat_merge): columns
// [out_offset, out_offset + k) of rows of out_stride entries, k <= 64; the counts of pages after the first add up
hipError_t launch_among_emit(const uint64_t* merged, uint32_t nq, uint32_t k, uint32_t out_stride, uint32_t out_offset,
                             uint64_t* out_ids, float* out_dist, uint32_t* out_count, hipStream_t st);

// exact range search (k_range.hip): every row with canonical distance <= radius[q].  The control words are per query
// SLOT j (slot j answers query sel[j], or j when sel == nullptr): pool_cnt[j] counts every member — stored in
// pool[j][kPoolCap] only while a slot is free — so it is the exact total, and pool_cnt[j] > kPoolCap is the overflow verdict.
struct RangeArgs {
  const float* Q;            // prepared queries [*][ld] (launch_prep_queries), indexed by QUERY
  RowsView rows;             // stored rows, any layout
  const float* radius;       // [*] indexed by query
  const uint32_t* sel;       // optional [n_slots]: the queries this launch answers
  uint64_t* pool;            // [n_slots][kPoolCap] (canonical distance, id) keys, unsorted
  uint32_t* pool_cnt;        // [n_slots], zero before the launch
  uint32_t n_blocks;         // workgroups per query: each walks its steps of the rows in a grid-stride loop
};
uint32_t range_step_rows(const RangeArgs& a);   // rows one workgroup takes per step of its loop
hipError_t launch_range_exact(const RangeArgs& a, uint32_t n_slots, hipStream_t st);
// the pools sorted by (distance, id): the first min(total, max_results) pairs of every slot's query, sentinels behind
// them, the count, and out_total (optional) = the counter; an overflowed slot gets its total only
hipError_t launch_range_emit(const uint64_t* pool, const uint32_t* pool_cnt, const uint32_t* sel, uint32_t n_slots,
                             uint32_t max_results, uint64_t* out_ids, float* out_dist, uint32_t* out_count,
                             uint64_t* out_total, hipStream_t st);
// int8 path: thr[q] = the score below which every row with D <= radius[q] must lie (k_range.hip's header); ovf[q] = 2
// marks a query the bound does not serve (thr -inf)
hipError_t launch_range_thr(const float* radius, const float2* quv, const float* max_sumsq, uint32_t nq, uint32_t dims,
                            int metric, float* thr, uint32_t* ovf, hipStream_t st);
struct RangeRerankArgs {
  const float* Q;            // prepared queries [*][ld]
  RowsView rows;             // stored rows, fp32 or binary16, plain layout
  const float* radius;       // [nq]
  const uint64_t* pool;      // [*][kPoolCap] the scan's (S_lower, id) keys
  const uint32_t* pool_cnt;  // [*]
  const uint32_t* ovf;       // [*] non-zero: the query is answered elsewhere, nothing is written for it
  uint32_t* kept;            // [nq] members found = the exact total
  uint64_t* out_ids;         // [nq][max_results]
  float* out_dist;
  uint32_t* out_count;       // [nq]
  uint64_t* out_total;       // [nq] or nullptr
  uint32_t nq, max_results;
};
uint32_t range_rerank_max_ld();   // longest row stride (floats): the pool and the prepared query share the LDS
hipError_t launch_range_rerank(const RangeRerankArgs& a, hipStream_t st);
hipError_t launch_range_iota(uint64_t* out, uint64_t n, hipStream_t st);   // out[i] = i

// exact range search under row bitmaps, the list route (k_rangem.hip): RangeArgs' slots, pools and counters, but slot j walks
// its OWN list of row ids, ids[list_off[j] .. list_off[j] + list_len[j]) (a mask's ascending list of allowed rows), not
// every row.  launch_range_emit then sorts and writes as it does for the unfiltered search.
struct RangeListArgs {
  const float* Q;            // prepared queries [*][ld] (launch_prep_queries), indexed by QUERY
  RowsView rows;             // stored rows, any layout
  const float* radius;       // [*] indexed by query
  const uint32_t* sel;       // optional [n_slots]: the queries this launch answers
  const uint64_t* ids;       // the lists' row ids; an id at or above rows.n_rows is no row and is not read
  const uint64_t* list_off;  // [n_slots]
  const uint32_t* list_len;  // [n_slots]
  uint64_t* pool;            // [n_slots][kPoolCap] (canonical distance, id) keys, unsorted
  uint32_t* pool_cnt;        // [n_slots], zero before the launch
  uint32_t n_blocks;         // workgroups per slot, sized from the longest list: each walks its steps of the slot's list
};
uint32_t range_list_step_rows(const RangeListArgs& a);   // list entries one workgroup takes per step of its loop
hipError_t launch_range_list(const RangeListArgs& a, uint32_t n_slots, hipStream_t st);
// out[q] = scans[q] ? radius[q] : NaN — the radii the int8 scan of a device batch runs under: a NaN radius collects nothing
hipError_t launch_range_scan_radii(const float* radius, const uint32_t* scans, uint32_t nq, float* out, hipStream_t st);

// exact kNN under row bitmaps (k_masked.hip): one bitmap (ehx_knn_masked*, the graph walk's exact route) or a table, one per
// query (ehx_knn_masked_multi*).  Compaction of the first n_bits bits of n_masks <= kMaskedMaxMasks bitmaps at once, the
// mask a grid dimension (n_tiles = ceil(n_bits / 256) tiles of 8 words; words and bits beyond n_bits are not read).  maps:
// bitmap m starts at maps + m * stride words, stride >= ceil(n_bits / 32); ONE bitmap is used where it lies, the stride
// never applied.  cum: [n_masks][n_tiles + 1], allowed rows before every tile, the last entry their number.  Counts and
// prefixes first (the host reads them back and places the lists), then the ascending lists of allowed row ids — mask m's at
// list + off[m].  launch_masked_samples, for the scan route: every mask's sample of at most 256 ids by rank (write_sample,
// below), at sample + 256 m.  launch_rows_prefix: `rows` rows of n + 1 words, cum[row][0 .. n) counts -> their exclusive prefix
// in place, cum[row][n] the total (rows or n zero: nothing is launched); launch_labeled_tiles and launch_colindex_bounds use it.
constexpr uint32_t kMaskedMaxMasks = 64;
struct MaskedOffsets {
  uint64_t off[kMaskedMaxMasks];
};
hipError_t launch_masked_count(const uint32_t* maps, uint64_t stride, uint32_t n_masks, uint64_t n_bits, uint32_t n_tiles,
                               uint32_t* cum, hipStream_t st);
hipError_t launch_masked_fill(const uint32_t* maps, uint64_t stride, uint32_t n_masks, uint64_t n_bits, uint32_t n_tiles,
                              const uint32_t* cum, const MaskedOffsets& off, uint64_t* list, hipStream_t st);
hipError_t launch_masked_samples(const uint64_t* list, const MaskedOffsets& off, const uint32_t* cum, uint32_t n_masks,
                                 uint32_t n_tiles, uint64_t* sample, hipStream_t st);
hipError_t launch_rows_prefix(uint32_t* cum, uint32_t rows, uint32_t n, hipStream_t st);
// exact kNN under a label column (k_labeled.hip; ehx_knn_labeled*): compaction of the rows [0, n_rows) by label, for the
// n_slots <= kLabeledMaxSlots distinct wanted labels of one device batch (table: ascending, in device memory).
//   launch_labeled_count   slot_of[r] = the slot of row r's label (kLabeledNoSlot: nobody wants it), count[slot] += 1
//                          (count: zero before the launch is enqueued — the launch clears it itself)
//   launch_labeled_tiles   for the slots that scan (scan_of[slot] < n_scan <= kLabeledMaxScan, else kLabeledNoScan):
//                          cum[scan][0 .. n_tiles] = the slot's rows before every 256-row tile, the last entry their number
//                          (the layout masked_passes reads)
//   launch_labeled_fill    every slot's list of row ids at list + off[slot]: ascending for the slots that scan (placed by
//                          cum), in any order for the others (placed by a cursor per slot: cursor[n_slots], cleared here)
//   launch_labeled_samples sample[256 scan + i] = the i-th of every sample_stride(rows)-th id of a scanning slot's list by rank
//                          (scan_off[scan]: where its list starts)
constexpr uint32_t kLabeledMaxSlots = 2048;   // the queries of one device batch (kSideChunk)
constexpr uint32_t kLabeledMaxScan = 127;     // labels of more than max(1024, n / 128) rows: n / max(1024, n / 128) <= 128, strictly below
constexpr uint16_t kLabeledNoSlot = 0xFFFFu;
constexpr uint32_t kLabeledNoScan = 0xFFFFFFFFu;
hipError_t launch_labeled_count(const uint32_t* label_of, uint64_t n_rows, const uint32_t* table, uint32_t n_slots,
                                uint16_t* slot_of, uint32_t* count, hipStream_t st);
hipError_t launch_labeled_tiles(const uint16_t* slot_of, uint64_t n_rows, uint32_t n_tiles, const uint32_t* scan_of,
                                uint32_t n_scan, uint32_t* cum, hipStream_t st);
hipError_t launch_labeled_fill(const uint16_t* slot_of, uint64_t n_rows, uint32_t n_tiles, uint32_t n_slots,
                               const uint64_t* off, const uint32_t* scan_of, uint32_t n_scan, const uint32_t* cum,
                               uint32_t* cursor, uint64_t* list, hipStream_t st);
hipError_t launch_labeled_samples(const uint64_t* list, const uint64_t* scan_off, const uint32_t* cum, uint32_t n_scan,
                                  uint32_t n_tiles, uint64_t* sample, hipStream_t st);
// stored label columns (k_colindex.hip; ehx_columns.cpp): the index of a column over n < 2^32 rows, by a stable LSD radix
// sort of (label, row id) with 8-bit digits over tiles of kColIndexTile keys.
//   launch_colindex_digits  ghist[4][256] = the four digit histograms of keys[0, n) (cleared here)
//   launch_colindex_pass    ONE digit pass keys_in / vals_in -> keys_out / vals_out (vals_in nullptr: the positions); hist:
//                           scratch of 256 * colindex_blocks(n) words; ghist: launch_colindex_digits'
//   launch_colindex_bounds  sorted keys (vals nullptr: the identity) -> labels[L], start[L + 1], perm[n] (64-bit row ids);
//                           bbase: scratch of n / 256 + 2 words, its entry [ceil(n / 256)] = L when the launches have run
//   launch_colindex_heavy   run: [n_heavy] starts | [n_heavy] ends in perm of the labels that may scan (ascending row ids
//                           inside each) -> cum[n_heavy][n_tiles + 1] rows before every 256-row tile (rows_prefix_kernel's
//                           layout), sample[n_heavy][256] by rank
//   launch_column_scatter   col[dst_row[i]] = values[i] where dst_row[i] < cap (~0: skipped); launch_column_gather the reverse
constexpr uint32_t kColIndexTile = 4096;
inline uint32_t colindex_blocks(uint64_t n) { return (uint32_t)((n + kColIndexTile - 1) / kColIndexTile); }
hipError_t launch_colindex_digits(const uint32_t* keys, uint64_t n, uint32_t* ghist, hipStream_t st);
hipError_t launch_colindex_pass(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out, uint32_t* vals_out,
                                uint64_t n, uint32_t digit, const uint32_t* ghist, uint32_t* hist, hipStream_t st);
hipError_t launch_colindex_bounds(const uint32_t* keys, const uint32_t* vals, uint64_t n, uint32_t* bbase, uint32_t* labels,
                                  uint32_t* start, uint64_t* perm, hipStream_t st);
hipError_t launch_colindex_heavy(const uint64_t* perm, const uint64_t* run, uint32_t n_heavy, uint32_t n_tiles, uint32_t* cum,
                                 uint64_t* sample, hipStream_t st);
hipError_t launch_column_scatter(uint32_t* col, uint64_t cap, const uint64_t* dst_row, const uint32_t* values, size_t n,
                                 hipStream_t st);
hipError_t launch_column_gather(const uint32_t* col, uint64_t cap, const uint64_t* rows, uint32_t* out, size_t n, hipStream_t st);
// predicate filters on stored columns (k_where.hip; ehx_where.cpp): the bitmaps of n_preds <= kMaskedMaxMasks predicates over
// the rows [0, n_rows), n_rows < 2^32, bitmap p at dst + p * words, words = ceil(n_rows / 32) — launch_masked_count's dense
// layout; bits at or above n_rows in the last word are 0, no word at or above `words` is written.  cols.p[c]: column c's values,
// read iff bit c of cols.named is set (a column some predicate names AND that is live); every other column is the constant
// 0xFFFFFFFF.  preds: n_preds predicates in DEVICE memory, laid out as include/ehx.h's ehx_pred (ehx_where.cpp asserts it): a
// term holds iff lo <= value <= hi, unsigned, inverted by flag bit 0.
constexpr uint32_t kWhereMaxCols = 4, kWhereMaxTerms = 8;   // EHX_MAX_COLUMNS, EHX_PRED_MAX_TERMS
struct WhereTerm {
  uint32_t col, lo, hi, flags;
};
struct WherePred {
  uint32_t n_terms;
  WhereTerm terms[kWhereMaxTerms];
};
struct WhereCols {
  const uint32_t* p[kWhereMaxCols];
  uint32_t named;
};
constexpr uint32_t kWhereSpan = 1024;   // rows of one workgroup: four 256-row tiles, 32 words of every bitmap
hipError_t launch_where_bitmaps(const WhereCols& cols, const WherePred* preds, uint32_t n_preds, uint64_t n_rows, uint64_t words,
                                uint32_t* dst, hipStream_t st);
// Boolean filters on stored columns (k_filter.hip; ehx_filter.cpp): the same dense table for n_filters <= kMaskedMaxMasks
// filters, filter f the OR of the clauses [first, first + n) its run names, a clause a WherePred whose terms may carry
// kFilterTermIn: then lo is where the term's sorted, de-duplicated set starts among the values and hi how many it holds.
// expr, DEVICE memory, packed: n_clauses WherePreds | n_values values | n_filters x (first, n); every run lies inside the
// clauses and every set inside the values (ehx_filter.cpp checks and packs).  cols: as above, over every clause's terms.
constexpr uint32_t kFilterMaxClauses = 128, kFilterMaxValues = 4096, kFilterTermIn = 2u;   // EHX_FILTER_MAX_*, EHX_TERM_IN
constexpr uint32_t kFilterExprWords =
    kFilterMaxClauses * (uint32_t)(sizeof(WherePred) / sizeof(uint32_t)) + kFilterMaxValues + 2u * kMaskedMaxMasks;
hipError_t launch_filter_bitmaps(const WhereCols& cols, const uint32_t* expr, uint32_t n_clauses, uint32_t n_values,
                                 uint32_t n_filters, uint64_t n_rows, uint64_t words, uint32_t* dst, hipStream_t st);
// radius[q] = dist[q][k - 1] when cnt[q] >= k (result lists [nq][k]), else +Inf
hipError_t launch_masked_radius(const float* dist, const uint32_t* cnt, uint32_t nq, uint32_t k, float* radius, hipStream_t st);
// word w of a bitmap cut at n_bits (bits of the last word beyond n_bits and words beyond it read as 0)
__device__ __forceinline__ uint32_t mask_word(const uint32_t* __restrict__ mask, uint64_t w, uint64_t n_bits) {
  const uint64_t lo = w << 5;
  if (lo >= n_bits) return 0u;
  uint32_t v = mask[w];
  const uint64_t left = n_bits - lo;
  if (left < 32) v &= (1u << (uint32_t)left) - 1u;
  return v;
}
// The sample of a compacted filter: entry i is list[i * sample_stride(rows)] while that is below rows, at most 256.  Stated
// ONCE: the three sample kernels write it (256 lanes, one entry each), filtered_answer sizes the list scan over it.
__host__ __device__ inline uint64_t sample_stride(uint64_t rows) { return (rows + 255u) / 256u; }
__device__ __forceinline__ void write_sample(const uint64_t* __restrict__ list, uint64_t rows, uint64_t* __restrict__ sample) {
  const uint64_t i = threadIdx.x * sample_stride(rows);
  if (i < rows) sample[threadIdx.x] = list[i];
}

// exact kNN on the int8 radius scan under a radius that falls (k_radius.hip): the bitmap search's scan route (k <= 48) and
// the flat chain's route for EHX_MAX_K < k <= kLargeKMax
constexpr uint32_t kLargeKMax = 256;      // longest carried list: one key per thread of the re-rank's workgroup
constexpr uint32_t kLargeKSample = 1024;  // rows of a seed's sample, at most (>= 4 k for every served k)
enum { kRadiusPass = 0, kRadiusLast = 1, kRadiusSeed = 2 };   // RadiusRerankArgs::mode
// pool[q][i] = i * stride for i < n_sample <= kLargeKSample, pool_cnt[q] = n_sample; (n_sample - 1) * stride < n_rows
hipError_t launch_radius_seed(uint64_t* pool, uint32_t* pool_cnt, uint32_t nq, uint64_t n_rows, uint64_t stride,
                              uint32_t n_sample, hipStream_t st);
struct RadiusRerankArgs {
  const float* Q;            // prepared queries [*][ld]
  RowsView rows;             // stored rows, fp32 or binary16, plain layout
  float* radius;             // [nq] in: the radius the pass ran under; out: lowered to the k-th held distance (NaN: overflowed)
  const uint64_t* pool;      // [*][kPoolCap] the pass's hits (the seed: the sample), keys whose low halves are row ids
  uint32_t* pool_cnt;        // [*] in: keys in the pool; out: 0
  const uint32_t* ovf;       // [*] non-zero: the query is answered elsewhere, nothing is written for it (not read by the seed)
  uint64_t* top;             // [nq][kLargeKMax] the carried exact (distance, id) keys, ascending
  uint32_t* top_cnt;         // [nq] keys carried (the seed: set to 0; without a seed: zero before the first pass)
  uint32_t* work;            // [nq] rows re-ranked (the seed: set; a pass: +=; without a seed: zero before the first pass)
  uint64_t* out_ids;         // [nq][k]  written behind the last pass
  float* out_dist;
  uint32_t* out_count;       // [nq]
  uint32_t nq, k;
  uint32_t mode;             // kRadiusPass | kRadiusLast (write the page instead of carrying) | kRadiusSeed (the radius only)
};
hipError_t launch_radius_rerank(const RadiusRerankArgs& a, hipStream_t st);   // k <= kLargeKMax, rows.ld <= range_rerank_max_ld()

// grouped kNN (k_grouped.hip): the falling-radius re-rank with at most per_group rows of one label among the keys it carries,
// hands on and writes; every layout of stored rows
constexpr uint32_t kGroupNone = 0xFFFFFFFFu;   // EHX_GROUP_NONE: a row that is a group of its own
struct GroupedRerankArgs {
  RadiusRerankArgs r;        // (rows: any layout)
  const uint32_t* group_of;  // [>= r.rows.n_rows] the rows' labels
  uint32_t per_group;        // >= 1
};
uint32_t grouped_rerank_max_ld();   // longest row stride (floats): the pool, the cap's images and the prepared query share the LDS
hipError_t launch_grouped_rerank(const GroupedRerankArgs& g, hipStream_t st);   // r.k <= kLargeKMax, rows.ld <= grouped_rerank_max_ld()
// every query's pool filled from ITS OWN rows, query q's given as the range list[start[q], end[q]) — start, end: device
// arrays of nq entries, end[q] >= start[q], the range inside the list; list == nullptr: the identity list, entry i is row i
// (an empty range reads nothing, whatever list is).  Queries may name the same range, and any number of ranges fits one
// launch.  seed: pool[q][i] = entry i * stride of the range for i * stride < len, stride = ceil(len / kLargeKSample),
// pool_cnt[q] the number written.  slab: pool[q][0, n) = entries [slab * kPoolCap, ...) of the range, pool_cnt[q] = n = as
// many as remain, at most kPoolCap, possibly 0; first: radius[q] = +Inf, top_cnt[q] = work[q] = 0 besides (the state in front
// of the first slab)
hipError_t launch_grouped_range_seed(const uint64_t* list, const uint64_t* start, const uint64_t* end, uint64_t* pool,
                                     uint32_t* pool_cnt, uint32_t nq, hipStream_t st);
hipError_t launch_grouped_range_slab(const uint64_t* list, const uint64_t* start, const uint64_t* end, uint64_t slab,
                                     bool first, uint64_t* pool, uint32_t* pool_cnt, float* radius, uint32_t* top_cnt,
                                     uint32_t* work, uint32_t nq, hipStream_t st);

// per-row statistics for rows [row0, row0+n): inv_norm (cosine), rowp (a,b) for the scan epilogue;
// *max_sumsq (optional) is raised to the largest |x|^2 seen (the certification margin's norm bound)
// perm: the fp32 rows are stored block-permuted (single-copy graph spaces); the sums keep the logical order
hipError_t launch_row_stats(const void* X, int x_half, uint64_t row0, uint64_t n, uint32_t dims, uint32_t ld,
                            int metric, float* inv_norm, float2* rowp, float* max_sumsq, hipStream_t st, int perm = 0);
// single-copy graph spaces: rows [row0, row0 + n) (or rows ids[0..n)) into the search copy's block order, in place
hipError_t launch_permute_blocks(float* X, uint32_t ld, uint64_t row0, uint64_t n, const uint64_t* ids, hipStream_t st);
// rowp for padding rows [row0, row0+n): (0, +inf)
hipError_t launch_rowp_pad(float2* rowp, uint64_t row0, uint64_t n, hipStream_t st);
// graph mode: rows [row0, row0+n) of the search copy (16-float blocks permuted for the four SSE partial
// sums, cosine rows pre-normalised); must follow launch_row_stats (inv_norm)
hipError_t launch_make_search_copy(const void* X, bool x_half, const float* inv_norm, uint64_t row0, uint64_t n,
                                   uint32_t ld, int metric, float* Xs, hipStream_t st);

// fp16 storage: rows of an fp32 matrix (stride src_ld) rounded to nearest-even into rows ids[i] (or
// row0+i when ids == nullptr) of the fp16 matrix, and one fp16 row widened back for Get
hipError_t launch_store_rows_f16(const float* src, uint32_t src_ld, const uint64_t* ids, uint64_t row0, uint64_t n,
                                 uint32_t dims, uint32_t ld, __half* X, hipStream_t st);
hipError_t launch_load_row_f16(const __half* X, uint64_t row, uint32_t dims, uint32_t ld, float* out, hipStream_t st);

// EHX-GAUSS-1 rows row0, row0 + row_stride, ... generated straight into a [*, ld] matrix (optionally L2-normalised)
// latent != 0: EHX-MANIFOLD-1 rows on a `latent`-dimensional linear subspace + 5 % noise (include/ehx_datagen.h)
hipError_t launch_gen_rows(uint64_t seed, uint64_t row0, uint64_t n_rows, uint32_t dims, uint32_t ld,
                           int normalize, float* out, hipStream_t st, uint64_t row_stride = 1, uint32_t latent = 0);

// graph-mode search (k_graph.hip): one wave per query
constexpr uint32_t kGraphCounters = 12;  // n_dist, n_hops0, n_hops_up, n_prefetch_hit, [4..11] profile builds (wide walk: [4] = steps)
struct GraphArgs {
  const float* Q;           // prepared queries [nq][ld]
  const float* Xs;          // search copy [cap][ld] (launch_make_search_copy)
  const float* xscale = nullptr;  // single-copy graph spaces, cosine: Xs holds RAW permuted rows, scaled by inv_norm on the fly
  const uint32_t* adj0;     // [n][M0], pad 0xFFFFFFFF, stored order
  const uint32_t* up_start; // [n]: first upper list of the node (levels 1..L consecutive) or ~0
  const uint32_t* up_lists; // [*][M], pad 0xFFFFFFFF
  uint32_t* visited;        // [nq][vis_words], all-zero before the launch and again after it
  uint32_t* vislog;         // [nq][vislog_cap] rows a query marked (it clears their words when done)
  uint32_t vislog_cap;
  uint64_t* out_ids;        // [nq][k]
  float* out_dist;
  uint32_t* out_count;
  unsigned long long* counters;  // [kGraphCounters]
  uint32_t nq, k, ef, ef_cap, n, dims, ld, M, M0, vis_words, entry_point;
  int max_level, metric;
  // One query per call in ONE launch (round 5; the reference's request shape, server.cc:172-210): q_raw != nullptr — the
  // raw query is read from host-visible memory and prepared by the kernel itself into Q (device scratch, [ld]); out_*
  // then point into host-visible memory and the kernel publishes `seq` in done_flag (system scope) when they are written.
  const float* q_raw = nullptr;
  uint32_t* done_flag = nullptr;
  uint32_t seq = 0;
  // Expansions per step of the level-0 search (ehx_params.search_width): 1 = the strict walk (hnswlib's order, one node at
  // a time: graph_search_kernel); 2 / 4 = the wide walk (k_graphw.hip: the `width` closest unexpanded entries of the
  // result list are expanded together — same ef bound and termination, fewer dependent memory round trips per query).
  uint32_t width = 1;
  // The walk under a row bitmap (k_graphm.hip; launch_graph_search_masked only): row r is allowed iff r < allow_bits and
  // bit r & 31 of allow[r >> 5] is set (allow_bits already cut at the call's row count); ef_cap is then the walk list's
  // length cap >= ef, and *cap_hits counts the queries whose list reached it.  allow_of != nullptr: a bitmap PER QUERY —
  // allow is a table of bitmaps, query i's begins allow_of[i] words into it (every bitmap covers allow_bits rows).
  const uint32_t* allow = nullptr;
  uint32_t allow_bits = 0;
  unsigned long long* cap_hits = nullptr;
  const uint32_t* allow_of = nullptr;   // [nq] word offsets, or nullptr: ONE bitmap for the batch
};
size_t graph_lds_bytes(uint32_t ld, uint32_t ef_cap, uint32_t width = 1);
hipError_t launch_graph_search(const GraphArgs& a, hipStream_t st);
// the strict walk that carries a row bitmap, or with a.allow_of one per query: keys hold the row id in 30 bits
// (a.n <= 2^30), width is ignored
hipError_t launch_graph_search_masked(const GraphArgs& a, hipStream_t st);

// graph-mode insertion (k_insert.hip)
// hipFuncAttributeMaxDynamicSharedMemorySize is set per function AND per device (every device has its own loaded code
// object), and launches come from several host threads once a space is sharded over devices inside one process: the
// largest size set so far is kept per device, atomically.  `fns`: the kernel's instantiations.
struct DynLdsAttr {
  std::atomic<size_t> set[64] = {};
  template <class Fn>
  hipError_t ensure(const Fn* fns, int n_fns, size_t bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;  // (within the default limit)
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::atomic<size_t>& cur = set[dev & 63];
    if (cur.load(std::memory_order_acquire) >= bytes) return hipSuccess;
    for (int i = 0; i < n_fns; ++i) {
      e = hipFuncSetAttribute((const void*)fns[i], hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
      if (e != hipSuccess) return e;
    }
    size_t seen = cur.load(std::memory_order_relaxed);
    while (seen < bytes && !cur.compare_exchange_weak(seen, bytes, std::memory_order_release)) {
    }
    return hipSuccess;
  }
};

// The launch of a pool re-rank (pool_rerank_sorted: range_rerank_kernel, radius_rerank_kernel), one workgroup of `threads`
// per query: fns[half * 3 + metric], the kernel's instantiations; args_ok: what the kernel's own arguments must satisfy.
template <class Args>
hipError_t launch_pool_rerank(void (*const (&fns)[6])(const Args), DynLdsAttr& attr, const Args& a, bool args_ok,
                              uint32_t threads, hipStream_t st) {
  if (a.nq == 0) return hipSuccess;
  if (!args_ok || (a.rows.ld & 3u) || a.rows.ld > range_rerank_max_ld() || a.rows.metric < 0 || a.rows.metric > 2)
    return hipErrorInvalidValue;
  const size_t lds = pool_rerank_lds_bytes(a.rows.ld);
  hipError_t e = attr.ensure(fns, 6, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fns[(a.rows.x_half ? 3 : 0) + a.rows.metric], dim3(a.nq), dim3(threads), lds, st, a);
  return hipGetLastError();
}

struct InsertArgs {
  const float* Xs;         // search copy (launch_make_search_copy)
  const float* xscale;     // single-copy graph spaces, cosine: Xs holds RAW permuted rows, scaled by inv_norm on the fly (else nullptr)
  uint32_t* adj0;          // [cap][M0]
  uint32_t* up_start;      // [cap]
  uint32_t* up_lists;      // [*][M]
  uint32_t* visited;       // [P][vis_words], zero on entry (and on exit)
  uint32_t* vislog;        // [P][vislog_cap]
  const uint32_t* new_ids; // [P]
  const int32_t* new_levels;
  uint32_t* sel;           // [P][max_sel_levels][1+M]: per level (count, ids farthest first)
  uint32_t ef, dims, ld, M, M0, vis_words, vislog_cap, max_sel_levels, entry_point;
  int max_level, metric;
  uint32_t exclude_self;   // 1: repairConnectionsForUpdate (drop the node itself from the search results)
  // ---- bulk build: the link work items are made on the device (no host between the search and the link kernel) ----
  uint32_t id0;            // new_ids == nullptr: wave p inserts row id0 + p
  uint32_t head_rows;      // list id of (node t, level l): l == 0 ? t : head_rows + up_start[t] + l - 1
  uint32_t* link_head;     // [head_rows + upper lists], 0 = no incoming link this round; otherwise 1 + the pair
                           // (wave p, level, slot) = (p * max_sel_levels + level) * M + slot registered last on the list
  uint32_t* link_next;     // [P * max_sel_levels * M]: the pair registered before this one on the same list (same code)
  uint2* link_touched;     // (target, level) of every list that received a pair, in arrival order
  uint32_t* link_count;    // how many
};
size_t insert_lds_bytes(uint32_t ld, uint32_t ef);
hipError_t launch_insert_search(const InsertArgs& a, uint32_t n_new, hipStream_t st);
hipError_t launch_update_neigh(const InsertArgs& a, uint32_t n_items, const uint32_t* neigh, int level,
                               const uint32_t* cand_off, const uint32_t* cand_ids, hipStream_t st);
hipError_t launch_insert_link(const InsertArgs& a, uint32_t n_items, const uint32_t* tgt, const int32_t* tlevel,
                              const uint32_t* kind, const uint32_t* inc_off, const uint32_t* inc_ids, hipStream_t st);
hipError_t launch_insert_link_dev(const InsertArgs& a, uint32_t n_waves, hipStream_t st);

// k-way merge of per-shard (dist, id) result lists [n_lists][nq][k] -> [nq][k]; an id of list l enters as
// id * id_mul + l * id_step (row-sharded spaces: local row -> global row = local * G + shard)
hipError_t launch_merge_lists(const uint64_t* ids, const float* dist, const uint32_t* count, uint32_t nq,
                              uint32_t k, uint32_t n_lists, uint64_t* out_ids, float* out_dist,
                              uint32_t* out_count, hipStream_t st, size_t ids_stride, size_t dist_stride,
                              size_t count_stride, uint64_t id_mul = 1, uint64_t id_step = 0);

}  // namespace ehx
