// Stored label columns (ehx_columns.cpp): the index of one column over a prefix of n < 2^32 rows —
//   perm[n]      row ids ordered by (label, row id)
//   labels[L]    the distinct labels, ascending
//   start[L + 1] where every label's rows begin in perm
// built by a stable LSD radix sort of (label, row id), 8 bits per pass, least significant digit first, and what the scan
// route needs of the labels with many rows.  No sort library is linked; every step is its own launch, so no kernel waits for
// another workgroup (no flags, no look-back).
//   colindex_digits_kernel    the four digit histograms of the whole column, one read of it: LDS counters per workgroup, one
//                             device-scope add per occupied bucket and workgroup.  A digit whose histogram has ONE occupied
//                             bucket needs no pass (the host skips it): a column of fewer than 256 small tenant numbers sorts
//                             in one pass, a column of one label in none.
//   colindex_tilehist_kernel  per pass: the digit counts of every 4096-key tile, hist[digit][tile]
//   colindex_scan_kernel      per pass: a workgroup per digit, exclusive prefix (block_prefix, k_prefix.h) along its tiles on
//                             top of the digit's base
//                             (the sum of the smaller digits' totals, from the column's histogram): where every (digit, tile)
//                             begins in the output
//   colindex_scatter_kernel   per pass: the stable scatter.  A tile is 4 waves x 16 rounds x 64 keys, wave w's keys
//                             contiguous, a round 64 consecutive keys.  The rank of a key among the tile's keys of its digit
//                             = the earlier waves' count (LDS, after a barrier) + the wave's count in earlier rounds (the
//                             wave's own LDS row, updated by ONE lane per distinct digit) + the lower lanes of its round with
//                             the same digit (eight ballots, one per bit of the digit).  Equal digits keep their order by
//                             construction: row ids ascend inside a label.
//   colindex_bcount_kernel    sorted labels -> boundaries per 256-key tile (a key differs from the one before it)
//   (rows_prefix_kernel)      k_masked.hip's, ONE row: exclusive prefix of those counts, the total behind them
//   colindex_bfill_kernel     labels, start (boundary rank = tile prefix + waves before + ballot), perm widened to 64 bits
//   colindex_tiles_kernel     for every label with more than the cut's rows ("heavy", at most 127): its rows before every
//                             256-row tile of the id space — a lower bound in its ascending run of perm —
//                             rows_prefix_kernel's layout, cum[heavy][0 .. n_tiles]
//   colindex_sample_kernel    sample[heavy][i] = its run[i * sample_stride(rows)]
//   column_scatter_kernel / column_gather_kernel   values by row id (ehx_set_batch_cols, ehx_column_set / _get)
// Workgroup shape: 256 lanes (4 waves).  LDS: digits 4 KB, tilehist 1 KB, scatter 4 KB (the four waves' digit rows, turned in
// place into their output bases), nothing else; 16 keys and 16 ranks per lane stay in registers, no scratch.  Stores of the
// scatter are per-lane (up to 256 runs per tile): a pass is supposed to be bound by them (not measured).
#include "k_prefix.h"

namespace ehx {

namespace {
constexpr uint32_t kCiThreads = 256, kCiRounds = 16, kCiWaveSpan = 64 * kCiRounds;
static_assert(kColIndexTile == 4 * kCiWaveSpan, "a tile is four waves' spans");
constexpr uint32_t kCiGrid = 2048;   // workgroups of the grid-stride histogram, at most (8 per CU): chosen, not measured
}

__global__ __launch_bounds__(256) void colindex_digits_kernel(const uint32_t* __restrict__ keys, uint64_t n,
                                                              uint32_t* __restrict__ ghist) {
  __shared__ uint32_t h[4 * 256];
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < 1024u; i += kCiThreads) h[i] = 0u;
  __syncthreads();
  for (uint64_t i = (uint64_t)blockIdx.x * kCiThreads + tid; i < n; i += (uint64_t)gridDim.x * kCiThreads) {
    const uint32_t k = keys[i];
    atomicAdd(&h[k & 255u], 1u);
    atomicAdd(&h[256u + ((k >> 8) & 255u)], 1u);
    atomicAdd(&h[512u + ((k >> 16) & 255u)], 1u);
    atomicAdd(&h[768u + (k >> 24)], 1u);
  }
  __syncthreads();
  for (uint32_t i = tid; i < 1024u; i += kCiThreads)
    if (h[i]) atomicAdd(&ghist[i], h[i]);   // (device scope: workgroups of every XCD add here)
}

// one workgroup per tile
__global__ __launch_bounds__(256) void colindex_tilehist_kernel(const uint32_t* __restrict__ keys, uint64_t n, uint32_t shift,
                                                                uint32_t n_blocks, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  const uint32_t tid = threadIdx.x;
  h[tid] = 0u;
  __syncthreads();
  const uint64_t t0 = (uint64_t)blockIdx.x * kColIndexTile;
#pragma unroll 4
  for (uint32_t j = 0; j < kColIndexTile / kCiThreads; ++j) {
    const uint64_t e = t0 + (uint64_t)j * kCiThreads + tid;
    if (e < n) atomicAdd(&h[(keys[e] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[(size_t)tid * n_blocks + blockIdx.x] = h[tid];
}

// workgroup d: hist[d][0 .. n_blocks) counts -> where (d, tile) begins in the output
__global__ __launch_bounds__(256) void colindex_scan_kernel(uint32_t* __restrict__ hist, uint32_t n_blocks,
                                                            const uint32_t* __restrict__ ghist) {
  const uint32_t d = blockIdx.x;
  uint32_t base = 0;   // (lane 0's counts alone)
  for (uint32_t i = 0; threadIdx.x == 0 && i < d; ++i) base += ghist[i];
  block_prefix<kCiThreads>(hist + (size_t)d * n_blocks, n_blocks, base, false);
}

// one workgroup per tile; vals_in == nullptr: the values are the positions themselves (the first pass: row ids)
__global__ __launch_bounds__(256) void colindex_scatter_kernel(const uint32_t* __restrict__ keys_in,
                                                               const uint32_t* __restrict__ vals_in,
                                                               uint32_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out,
                                                               uint64_t n, uint32_t shift, uint32_t n_blocks,
                                                               const uint32_t* __restrict__ offs) {
  __shared__ uint32_t wcnt[4][256];   // [wave][digit]: the wave's keys so far; then where the wave's keys of the digit begin
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  for (uint32_t i = tid; i < 1024u; i += kCiThreads) (&wcnt[0][0])[i] = 0u;
  __syncthreads();
  volatile uint32_t* mine = wcnt[w];   // (touched by this wave alone until the barrier: the wave runs in lock step)
  const uint64_t e0 = (uint64_t)blockIdx.x * kColIndexTile + (uint64_t)w * kCiWaveSpan + lane;
  const uint64_t below = (1ull << lane) - 1ull;
  uint32_t key[kCiRounds], rank[kCiRounds];
#pragma unroll
  for (uint32_t j = 0; j < kCiRounds; ++j) {
    const uint64_t e = e0 + (uint64_t)j * 64u;
    const bool valid = e < n;
    const uint32_t k = valid ? keys_in[e] : 0u;
    const uint32_t d = (k >> shift) & 255u;
    uint64_t same = __ballot(valid);   // the valid lanes of the round with this lane's digit
#pragma unroll
    for (uint32_t b = 0; b < 8u; ++b) {
      const bool bit = (d >> b) & 1u;
      const uint64_t set = __ballot(bit);
      same &= bit ? set : ~set;
    }
    const uint32_t prior = mine[d];
    const uint32_t r = (uint32_t)__builtin_popcountll(same & below);
    __builtin_amdgcn_wave_barrier();
    if (valid && r == 0u) mine[d] = prior + (uint32_t)__builtin_popcountll(same);   // (one lane per distinct digit)
    __builtin_amdgcn_wave_barrier();
    key[j] = k;
    rank[j] = prior + r;
  }
  __syncthreads();
  {   // lane d of the workgroup: the waves' counts of digit d -> their bases in the output
    uint32_t run = offs[(size_t)tid * n_blocks + blockIdx.x];
    for (uint32_t i = 0; i < 4u; ++i) {
      const uint32_t c = wcnt[i][tid];
      wcnt[i][tid] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t j = 0; j < kCiRounds; ++j) {
    const uint64_t e = e0 + (uint64_t)j * 64u;
    if (e >= n) continue;
    const uint64_t dst = (uint64_t)wcnt[w][(key[j] >> shift) & 255u] + rank[j];
    if (dst >= n) continue;   // (never, while the histograms are this input's: no store leaves the arrays)
    keys_out[dst] = key[j];
    vals_out[dst] = vals_in ? vals_in[e] : (uint32_t)e;
  }
}

__device__ __forceinline__ bool colindex_boundary(const uint32_t* __restrict__ keys, uint64_t i, uint64_t n) {
  return i < n && (i == 0 || keys[i] != keys[i - 1]);
}

// one workgroup per 256-key tile: bcount[tile] = labels that begin in it
__global__ __launch_bounds__(256) void colindex_bcount_kernel(const uint32_t* __restrict__ keys, uint64_t n,
                                                              uint32_t* __restrict__ bcount) {
  __shared__ uint32_t wc[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  const uint64_t bal = __ballot(colindex_boundary(keys, (uint64_t)blockIdx.x * 256u + tid, n));
  if (lane == 0) wc[w] = (uint32_t)__builtin_popcountll(bal);
  __syncthreads();
  if (tid == 0) bcount[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// one workgroup per 256-key tile; vals == nullptr: no pass ran, perm is the identity
__global__ __launch_bounds__(256) void colindex_bfill_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                             uint64_t n, uint32_t n_tiles, const uint32_t* __restrict__ bbase,
                                                             uint32_t* __restrict__ labels, uint32_t* __restrict__ start,
                                                             uint64_t* __restrict__ perm) {
  __shared__ uint32_t wc[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  const uint64_t i = (uint64_t)blockIdx.x * 256u + tid;
  const bool flag = colindex_boundary(keys, i, n);
  const uint64_t bal = __ballot(flag);
  if (lane == 0) wc[w] = (uint32_t)__builtin_popcountll(bal);
  __syncthreads();
  if (i >= n) return;
  perm[i] = vals ? (uint64_t)vals[i] : i;
  const uint32_t total = bbase[n_tiles];   // L <= n
  if (flag) {
    uint32_t pos = bbase[blockIdx.x] + (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
    for (uint32_t j = 0; j < w; ++j) pos += wc[j];
    if (pos < total) {
      labels[pos] = keys[i];
      start[pos] = (uint32_t)i;
    }
  }
  if (i == n - 1) start[total] = (uint32_t)n;   // (n < 2^32)
}

// a lane per (heavy label, tile boundary): rows of the label below row 256 * tile
__global__ __launch_bounds__(256) void colindex_tiles_kernel(const uint64_t* __restrict__ perm, const uint64_t* __restrict__ run,
                                                             uint32_t n_heavy, uint32_t n_tiles, uint32_t* __restrict__ cum) {
  const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x, per = (uint64_t)n_tiles + 1u;
  if (g >= (uint64_t)n_heavy * per) return;
  const uint32_t h = (uint32_t)(g / per);
  const uint64_t bound = (g % per) * 256u, b = run[h];
  uint64_t lo = b, hi = run[n_heavy + h];   // the first entry of the run that is not below `bound`
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (perm[mid] < bound) lo = mid + 1u;
    else hi = mid;
  }
  cum[g] = (uint32_t)(lo - b);
}

// one workgroup per heavy label
__global__ __launch_bounds__(256) void colindex_sample_kernel(const uint64_t* __restrict__ perm, const uint64_t* __restrict__ run,
                                                              uint32_t n_heavy, uint64_t* __restrict__ sample) {
  const uint32_t h = blockIdx.x;
  write_sample(perm + run[h], run[n_heavy + h] - run[h], sample + (size_t)h * 256u);
}

__global__ __launch_bounds__(256) void column_scatter_kernel(uint32_t* __restrict__ col, uint64_t cap,
                                                             const uint64_t* __restrict__ dst_row,
                                                             const uint32_t* __restrict__ values, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint64_t r = dst_row[i];   // (~0: a later entry of the batch writes this row)
  if (r < cap) col[r] = values[i];
}

__global__ __launch_bounds__(256) void column_gather_kernel(const uint32_t* __restrict__ col, uint64_t cap,
                                                            const uint64_t* __restrict__ rows, uint32_t* __restrict__ out,
                                                            uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint64_t r = rows[i];
  out[i] = r < cap ? col[r] : 0xFFFFFFFFu;
}

hipError_t launch_colindex_digits(const uint32_t* keys, uint64_t n, uint32_t* ghist, hipStream_t st) {
  if (hipError_t e = hipMemsetAsync(ghist, 0, 1024 * sizeof(uint32_t), st); e != hipSuccess) return e;
  if (n == 0) return hipSuccess;
  if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
  const uint64_t groups = (n + kCiThreads - 1) / kCiThreads;
  hipLaunchKernelGGL(colindex_digits_kernel, dim3((uint32_t)std::min<uint64_t>(groups, kCiGrid)), dim3(kCiThreads), 0, st, keys, n,
                     ghist);
  return hipGetLastError();
}

hipError_t launch_colindex_pass(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out, uint32_t* vals_out,
                                uint64_t n, uint32_t digit, const uint32_t* ghist, uint32_t* hist, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (n > 0xFFFFFFFFull || digit > 3u) return hipErrorInvalidValue;
  const uint32_t n_blocks = colindex_blocks(n), shift = 8u * digit;
  hipLaunchKernelGGL(colindex_tilehist_kernel, dim3(n_blocks), dim3(kCiThreads), 0, st, keys_in, n, shift, n_blocks, hist);
  hipLaunchKernelGGL(colindex_scan_kernel, dim3(256), dim3(kCiThreads), 0, st, hist, n_blocks, ghist + 256u * digit);
  hipLaunchKernelGGL(colindex_scatter_kernel, dim3(n_blocks), dim3(kCiThreads), 0, st, keys_in, vals_in, keys_out, vals_out, n,
                     shift, n_blocks, hist);
  return hipGetLastError();
}

hipError_t launch_colindex_bounds(const uint32_t* keys, const uint32_t* vals, uint64_t n, uint32_t* bbase, uint32_t* labels,
                                  uint32_t* start, uint64_t* perm, hipStream_t st) {
  if (n == 0) return hipMemsetAsync(bbase, 0, sizeof(uint32_t), st);   // (no label: the total alone)
  if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
  const uint32_t n_tiles = (uint32_t)((n + 255u) / 256u);
  hipLaunchKernelGGL(colindex_bcount_kernel, dim3(n_tiles), dim3(256), 0, st, keys, n, bbase);
  if (hipError_t e = launch_rows_prefix(bbase, 1, n_tiles, st); e != hipSuccess) return e;
  hipLaunchKernelGGL(colindex_bfill_kernel, dim3(n_tiles), dim3(256), 0, st, keys, vals, n, n_tiles, bbase, labels, start, perm);
  return hipGetLastError();
}

hipError_t launch_colindex_heavy(const uint64_t* perm, const uint64_t* run, uint32_t n_heavy, uint32_t n_tiles, uint32_t* cum,
                                 uint64_t* sample, hipStream_t st) {
  if (n_heavy == 0) return hipSuccess;
  if (n_heavy > kLabeledMaxScan) return hipErrorInvalidValue;
  const uint64_t lanes = (uint64_t)n_heavy * ((uint64_t)n_tiles + 1u);
  hipLaunchKernelGGL(colindex_tiles_kernel, dim3((uint32_t)((lanes + 255u) / 256u)), dim3(256), 0, st, perm, run, n_heavy, n_tiles,
                     cum);
  hipLaunchKernelGGL(colindex_sample_kernel, dim3(n_heavy), dim3(256), 0, st, perm, run, n_heavy, sample);
  return hipGetLastError();
}

hipError_t launch_column_scatter(uint32_t* col, uint64_t cap, const uint64_t* dst_row, const uint32_t* values, size_t n,
                                 hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(column_scatter_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, st, col, cap, dst_row, values,
                     (uint32_t)n);
  return hipGetLastError();
}

hipError_t launch_column_gather(const uint32_t* col, uint64_t cap, const uint64_t* rows, uint32_t* out, size_t n, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(column_gather_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, st, col, cap, rows, out, (uint32_t)n);
  return hipGetLastError();
}

}  // namespace ehx
