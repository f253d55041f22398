// Profile search (ehx_knn_profile*, ehx_combine_rows_device; ehx_profile.cpp): the query is not a vector the caller holds but
// a weighted sum of rows the space already holds — "near what this user liked, weighted by recency, minus what they
// disliked".  combine_rows_kernel builds every query's target from the stored rows without a row copy ever existing: the
// rows stream from HBM through registers, once.  include/ehx.h has the definition; in short, per component c and in fp32,
//   strand s (0..7):  acc_s = +0; for e = s, s + 8, ... in list order, entries that name no row skipped:
//                     acc_s = fl(acc_s + fl(w_e * x_e[c]))
//   t[c] = fl(... fl(fl(acc_0 + acc_1) + acc_2) ... + acc_7)
// Every multiply and every add is rounded on its own: they are written as __fmul_rn / __fadd_rn, which the compiler may not
// contract (the project's -ffp-contract=off says the same for the whole library; this file does not rely on it).
//
// No matrix instructions: the kernel does ONE multiply-add per 4 bytes it fetches (2 bytes for binary16 rows) — three orders
// of magnitude below where an MFMA would matter — and the ORDER of a component's sum is the contract, which a matrix
// instruction's internal accumulation would not keep.  The bound is the HBM row gathers, sum of L_i x row bytes.
//
// Work split.  One workgroup per (query, slab of components), 8 waves; wave s owns strand s, so the eight strands are eight
// independent row streams and no order depends on data.
//   list      the query's list is staged ONCE in LDS as (32-bit row | weight) pairs — 32 KiB at 4096 entries; an id that names
//             no row becomes kNoRow there, and the block-wide OR of "names a row" is valid[q].
//   units     a row is cut into UNITS of 16 bytes as stored (4 floats; 8 binary16).  Lane l of every wave owns units
//             u0 + l, u0 + l + 64, ... (kUnits of them: 3 for fp32 — a 768-float row is one slab — 2 for binary16) and keeps
//             their components' partial sums in registers.  A row starts on a 128-byte boundary and is padded to its stride,
//             so every load is 16 bytes per lane, a wave reads 1 KiB of a row at a time, and dims % 4 != 0 needs no special
//             load: the padding is summed like any component and never stored.
//   flight    a wave walks its entries in groups of kGroup = 4 rows: the loads of the NEXT group are issued before the
//             multiply-adds of the current one (4 .. 8 rows x kUnits x 16 bytes per lane in flight), the ids and weights come
//             from LDS (one broadcast read per entry).
//   layouts   block-permuted rows (single-copy graph spaces) are summed IN STORED ORDER — components are independent, so
//             the sum of stored position p is the target's component at the logical position p stands for — and the 4 x 4
//             transpose is undone only where the target is stored (search_copy_pos, as gather_rows_kernel).  binary16 units
//             are widened (exact) to two float4.
//   meeting   the eight partials meet in LDS (the list's bytes, re-used behind a barrier) and are summed in strand order by
//             all 512 threads, one component each per step: coalesced 4-byte stores, so an output row of dims % 4 != 0 —
//             which starts on no 16-byte boundary — takes the same path (its "tail" is the whole row: the target is 1 / L of the
//             bytes the kernel moves).
//   slabs     components are independent, so grid.y cuts rows into slabs of 64 x units-per-lane units.  The bytes are the same
//             for every slab size (the list is re-staged per slab: 32 KiB against L rows); a batch too small to fill the
//             CUs with one workgroup per query takes fewer units per lane and more slabs (launch_combine_rows).
// Eight strands, four rows per group and three units per lane are choices, not measurements.
#include "ehx_kernels.h"

namespace ehx {

namespace {
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
constexpr uint32_t kThreads = 64 * kProfileStrands;
constexpr uint32_t kGroup = 4;                 // rows of one strand whose loads are issued together
constexpr uint32_t kNoRow = 0xFFFFFFFFu;       // a staged entry that names no row

__device__ __forceinline__ float4 madd4(float4 acc, float w, float4 x) {
  acc.x = __fadd_rn(acc.x, __fmul_rn(w, x.x));
  acc.y = __fadd_rn(acc.y, __fmul_rn(w, x.y));
  acc.z = __fadd_rn(acc.z, __fmul_rn(w, x.z));
  acc.w = __fadd_rn(acc.w, __fmul_rn(w, x.w));
  return acc;
}

// acc[0 .. kFloats / 4) += w * (the unit's components)
template <bool HALFX>
__device__ __forceinline__ void unit_madd(float4* acc, float w, const float4& raw) {
  if (HALFX) {
    const half8_t h = *(const half8_t*)&raw;
    acc[0] = madd4(acc[0], w, make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]));
    acc[1] = madd4(acc[1], w, make_float4((float)h[4], (float)h[5], (float)h[6], (float)h[7]));
  } else {
    acc[0] = madd4(acc[0], w, raw);
  }
}

// number of entries of the ascending global array a[0, n) that are < key
__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t* __restrict__ a, uint32_t n, uint32_t key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
}  // namespace

// SORTED (the centroid sums, ehx_assign.cpp): the list is a run of a label-sorted range and may have ANY length — it goes
// through LDS in pieces of kProfileMaxList entries, the lane accumulators staying in registers across the pieces (a piece is a
// multiple of 8 entries: an entry's strand by its place in the piece is its strand in the list); every weight is 1, and the
// run's length is written where the other form writes valid[q].  !SORTED runs the piece loop once: the code it always was.
template <bool HALFX, bool PERM, bool SORTED>
__global__ __launch_bounds__(kThreads) void combine_rows_kernel(CombineRowsArgs a, uint32_t n_units, uint32_t slab_units) {
  constexpr uint32_t kF = HALFX ? 8 : 4, kU = HALFX ? 2 : 3, kV = kF / 4;   // floats of a unit, units per lane at most, float4 of a unit
  // the list as (row, weight bits) pairs; behind the walk, the strands' partials [8][slab_units * kF]
  __shared__ uint2 lds[kProfileMaxList];
  static_assert(sizeof(uint2) * kProfileMaxList >= sizeof(float) * kProfileStrands * 64 * kU * kF, "the partials re-use the list's LDS");
  static_assert(kProfileMaxList % kProfileStrands == 0, "a piece keeps every entry's strand");
  const uint32_t tid = threadIdx.x, lane = tid & 63u, strand = tid >> 6, q = blockIdx.x;
  uint64_t e0, len;
  if (SORTED) {
    e0 = lower_bound_u32(a.sorted_key, a.n_sorted, q);
    len = lower_bound_u32(a.sorted_key, a.n_sorted, q + 1u) - e0;
    if (blockIdx.y == 0 && tid == 0) a.count[q] = (uint32_t)len;
  } else {
    e0 = a.off[q];
    len = a.off[q + 1] - e0;
    if (len > kProfileMaxList) len = kProfileMaxList;
  }

  // this lane's units of the slab (one beyond the row is clamped into it: read, summed, never stored)
  const uint32_t u0 = blockIdx.y * slab_units;
  uint32_t unit[kU];
#pragma unroll
  for (uint32_t j = 0; j < kU; ++j) unit[j] = min(u0 + min(lane + 64 * j, slab_units - 1), n_units - 1);
  const uint32_t upl = (slab_units + 63) >> 6;   // units per lane in use: a wave-uniform bound on j
  const char* __restrict__ X = (const char*)a.rows.X;
  const size_t row_bytes = (size_t)a.rows.ld * (HALFX ? 2 : 4);

  float4 acc[kU][kV];
#pragma unroll
  for (uint32_t j = 0; j < kU; ++j)
#pragma unroll
    for (uint32_t v = 0; v < kV; ++v) acc[j][v] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);

  uint64_t p0 = 0;   // where the piece begins in the list
  do {
    const uint32_t L = len - p0 < kProfileMaxList ? (uint32_t)(len - p0) : kProfileMaxList;
    if (SORTED) {
      if (p0) __syncthreads();   // (every wave is done with the last piece)
      for (uint32_t e = tid; e < L; e += kThreads) {
        const uint64_t id = a.row0 + a.sorted_pos[e0 + p0 + e];
        lds[e] = make_uint2(id < a.rows.n_rows ? (uint32_t)id : kNoRow, 0x3F800000u);
      }
      __syncthreads();
    } else {
      bool names = false;
      for (uint32_t e = tid; e < L; e += kThreads) {
        const uint64_t id = a.ids[e0 + e];
        const bool ok = id < a.rows.n_rows;
        names |= ok;
        lds[e] = make_uint2(ok ? (uint32_t)id : kNoRow, a.weights ? __float_as_uint(a.weights[e0 + e]) : 0x3F800000u);
      }
      const int any = __syncthreads_or(names ? 1 : 0);
      if (blockIdx.y == 0 && tid == 0) a.valid[q] = any ? 1u : 0u;
    }

    // strand `strand`: entries strand, strand + 8, ... in groups of kGroup; entry i of a group is list entry e + 8 i
    uint2 ent[kGroup], ent_next[kGroup];
    float4 raw[kGroup][kU], raw_next[kGroup][kU];
    auto fetch = [&](uint32_t e, uint2* en, float4 (*rw)[kU]) {
#pragma unroll
      for (uint32_t i = 0; i < kGroup; ++i) {
        const uint32_t ei = e + kProfileStrands * i;
        en[i] = ei < L ? lds[ei] : make_uint2(kNoRow, 0u);   // (wave-uniform: every lane reads the same entry)
        if (en[i].x != kNoRow) {
          const char* __restrict__ row = X + (size_t)en[i].x * row_bytes;
#pragma unroll
          for (uint32_t j = 0; j < kU; ++j)
            if (j < upl) rw[i][j] = *(const float4*)(row + (size_t)unit[j] * 16);
        }
      }
    };
    if (strand < L) fetch(strand, ent, raw);
    for (uint32_t e = strand; e < L; e += kProfileStrands * kGroup) {
      const uint32_t en = e + kProfileStrands * kGroup;
      if (en < L) fetch(en, ent_next, raw_next);
#pragma unroll
      for (uint32_t i = 0; i < kGroup; ++i) {
        if (ent[i].x == kNoRow) continue;
        const float w = __uint_as_float(ent[i].y);
#pragma unroll
        for (uint32_t j = 0; j < kU; ++j)
          if (j < upl) unit_madd<HALFX>(acc[j], w, raw[i][j]);
      }
#pragma unroll
      for (uint32_t i = 0; i < kGroup; ++i) {
        ent[i] = ent_next[i];
#pragma unroll
        for (uint32_t j = 0; j < kU; ++j) raw[i][j] = raw_next[i][j];
      }
    }
    p0 += kProfileMaxList;
  } while (SORTED && p0 < len);

  // the partials meet: part[strand][position in the slab, stored order]
  __syncthreads();   // (every wave is done with the list)
  float* part = (float*)lds;
  const uint32_t slab_floats = slab_units * kF;
#pragma unroll
  for (uint32_t j = 0; j < kU; ++j) {
    const uint32_t lu = lane + 64 * j;
    if (lu < slab_units) {
#pragma unroll
      for (uint32_t v = 0; v < kV; ++v) ((float4*)(part + (size_t)strand * slab_floats))[lu * kV + v] = acc[j][v];
    }
  }
  __syncthreads();
  // ... and are summed in strand order, one logical component per thread and step (a slab starts and ends on a 16-float
  // block boundary or at the row's end, so a block's permutation stays inside it)
  const uint32_t c0 = u0 * kF;
  float* __restrict__ out = a.out + (size_t)q * a.rows.dims;
  for (uint32_t m = tid; m < slab_floats; m += kThreads) {
    const uint32_t c = c0 + m;
    if (c >= a.rows.dims) break;
    const uint32_t p = (PERM ? search_copy_pos(c) : c) - c0;
    float t = part[p];
#pragma unroll
    for (uint32_t s = 1; s < kProfileStrands; ++s) t = __fadd_rn(t, part[(size_t)s * slab_floats + p]);
    out[c] = t;
  }
}

// Units per lane: the most (fewest slabs, the list staged fewest times) at which the grid still has a workgroup per CU; a
// batch that cannot reach that takes one unit per lane.
hipError_t launch_combine_rows(const CombineRowsArgs& a, int n_cus, hipStream_t st) {
  if (a.nq == 0) return hipSuccess;
  const bool half = a.rows.x_half != 0, perm = !half && a.rows.x_perm != 0;
  const uint32_t kF = half ? 8 : 4, kU = half ? 2 : 3;
  // the stored positions that hold the row's components: whole 16-float blocks of a permuted row (all inside the stride)
  const uint32_t n_units = (perm ? (a.rows.dims + 15u) / 16u * 16u : a.rows.dims + kF - 1) / kF;
  uint32_t upl = kU;
  while (upl > 1 && (uint64_t)a.nq * ((n_units + 64 * upl - 1) / (64 * upl)) < (uint64_t)n_cus) --upl;
  const uint32_t whole = (n_units + 3u) / 4u * 4u, slab_units = 64 * upl < whole ? 64 * upl : whole;   // (a short row: one partial slab, whole blocks)
  const dim3 grid(a.nq, (n_units + slab_units - 1) / slab_units), block(kThreads);
  if (a.sorted_key) {   // the centroid sums
    if (!a.sorted_pos || !a.count) return hipErrorInvalidValue;
    if (half) hipLaunchKernelGGL((combine_rows_kernel<true, false, true>), grid, block, 0, st, a, n_units, slab_units);
    else if (perm) hipLaunchKernelGGL((combine_rows_kernel<false, true, true>), grid, block, 0, st, a, n_units, slab_units);
    else hipLaunchKernelGGL((combine_rows_kernel<false, false, true>), grid, block, 0, st, a, n_units, slab_units);
    return hipGetLastError();
  }
  if (half) hipLaunchKernelGGL((combine_rows_kernel<true, false, false>), grid, block, 0, st, a, n_units, slab_units);
  else if (perm) hipLaunchKernelGGL((combine_rows_kernel<false, true, false>), grid, block, 0, st, a, n_units, slab_units);
  else hipLaunchKernelGGL((combine_rows_kernel<false, false, false>), grid, block, 0, st, a, n_units, slab_units);
  return hipGetLastError();
}

// One wave per query: a query whose list names no row gets count 0 and sentinels over whatever the search wrote for its
// all-zero target.
__global__ __launch_bounds__(256) void blank_invalid_kernel(const uint32_t* __restrict__ valid, uint32_t nq, uint32_t k,
                                                            uint64_t* __restrict__ out_ids, float* __restrict__ out_dist,
                                                            uint32_t* __restrict__ out_count) {
  const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (q >= nq || valid[q]) return;
  for (uint32_t j = lane; j < k; j += 64) {
    out_ids[(size_t)q * k + j] = ~0ull;
    out_dist[(size_t)q * k + j] = __builtin_inff();
  }
  if (lane == 0) out_count[q] = 0;
}

hipError_t launch_blank_invalid(const uint32_t* valid, uint32_t nq, uint32_t k, uint64_t* out_ids, float* out_dist,
                                uint32_t* out_count, hipStream_t st) {
  if (nq == 0) return hipSuccess;
  hipLaunchKernelGGL(blank_invalid_kernel, dim3((nq + 3) / 4), dim3(256), 0, st, valid, nq, k, out_ids, out_dist, out_count);
  return hipGetLastError();
}

}  // namespace ehx
