// Exact kNN under a label column (ehx_knn_labeled*): one 32-bit label per row, one wanted label per query; row r is allowed
// for query i iff label_of[r] == want[i].  This file compacts the column for the distinct wanted labels of ONE device batch —
// at most kLabeledMaxSlots = 2048 "slots", the host's ascending, de-duplicated table — into what the bitmap search's answer
// consumes (ehx_masked.cpp): per-slot row counts, every slot's list of row ids back to back, and for the slots that take the
// scan route (at most kLabeledMaxScan = 127: ehx_labeled.cpp has the argument) the rows before every 256-row tile, an
// ASCENDING list and the by-rank sample.
//   labeled_count_kernel    slot_of[r] = the slot of row r's label by binary search of the table in LDS (8 KB), counts
//                           reduced per workgroup in LDS: one global add per slot and workgroup, not one per row
//   labeled_tiles_kernel    the scanning slots' rows in every tile, cum[scan][tile] (a workgroup per tile, 127 LDS counters:
//                           never a slots x tiles table)
//   (rows_prefix_kernel)    k_masked.hip's: their exclusive prefix per scanning slot, cum[scan][0 .. n_tiles], the layout
//                           masked_passes reads
//   labeled_fill_kernel     the lists.  A scanning slot's row lands at off + cum[scan][tile] + its rank inside the tile (a
//                           ballot per distinct scanning slot of the wave, the waves' counts through LDS): ascending.  Every
//                           other slot's row takes the next free entry of its list from a cursor: any order, which
//                           ehx_knn_among_device's contract allows — the list scan orders by (distance, id), no answer
//                           depends on it.
//   labeled_sample_kernel   sample[scan][i] = the scanning slot's list[i * sample_stride(rows)]
// The offsets come from device arrays (2048 slots do not fit a kernel argument as MaskedOffsets' 64 do).
#include "ehx_kernels.h"

namespace ehx {

// grid-stride over 256-row tiles, one lane per row
__global__ __launch_bounds__(256) void labeled_count_kernel(const uint32_t* __restrict__ label_of, uint64_t n_rows,
                                                            uint32_t n_tiles, const uint32_t* __restrict__ table,
                                                            uint32_t n_slots, uint16_t* __restrict__ slot_of,
                                                            uint32_t* __restrict__ count) {
  __shared__ uint32_t tab[kLabeledMaxSlots], cnt[kLabeledMaxSlots];
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < n_slots; i += 256u) {
    tab[i] = table[i];
    cnt[i] = 0u;
  }
  __syncthreads();
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t r = (uint64_t)tile * 256u + tid;
    if (r >= n_rows) continue;
    const uint32_t lab = label_of[r];
    uint32_t lo = 0, hi = n_slots;   // the first slot whose label is not below lab
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (tab[mid] < lab) lo = mid + 1u;
      else hi = mid;
    }
    const bool hit = lo < n_slots && tab[lo] == lab;
    slot_of[r] = hit ? (uint16_t)lo : kLabeledNoSlot;
    if (hit) atomicAdd(&cnt[lo], 1u);
  }
  __syncthreads();
  for (uint32_t i = tid; i < n_slots; i += 256u)
    if (cnt[i]) atomicAdd(&count[i], cnt[i]);
}

// the scanning slot of row r (kLabeledNoScan: its slot does not scan, or nobody wants its label)
__device__ __forceinline__ uint32_t labeled_scan_of(const uint16_t* __restrict__ slot_of, const uint32_t* __restrict__ scan_of,
                                                    uint64_t r, uint64_t n_rows, uint32_t n_scan, uint32_t* slot) {
  *slot = r < n_rows ? (uint32_t)slot_of[r] : (uint32_t)kLabeledNoSlot;
  if (*slot == (uint32_t)kLabeledNoSlot) return kLabeledNoScan;
  const uint32_t sc = scan_of[*slot];
  return sc < n_scan ? sc : kLabeledNoScan;
}

// grid-stride over tiles: cum[scan][tile] = the scanning slot's rows in the tile
__global__ __launch_bounds__(256) void labeled_tiles_kernel(const uint16_t* __restrict__ slot_of, uint64_t n_rows,
                                                            uint32_t n_tiles, const uint32_t* __restrict__ scan_of,
                                                            uint32_t n_scan, uint32_t* __restrict__ cum) {
  __shared__ uint32_t c[kLabeledMaxScan + 1];
  const uint32_t tid = threadIdx.x;
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    if (tid <= kLabeledMaxScan) c[tid] = 0u;
    __syncthreads();
    uint32_t slot;
    const uint32_t sc = labeled_scan_of(slot_of, scan_of, (uint64_t)tile * 256u + tid, n_rows, n_scan, &slot);
    if (sc != kLabeledNoScan) atomicAdd(&c[sc], 1u);
    __syncthreads();
    if (tid < n_scan) cum[(size_t)tid * (n_tiles + 1u) + tile] = c[tid];
    __syncthreads();
  }
}

// one workgroup per tile, one lane per row
__global__ __launch_bounds__(256) void labeled_fill_kernel(const uint16_t* __restrict__ slot_of, uint64_t n_rows,
                                                           uint32_t n_tiles, const uint64_t* __restrict__ off,
                                                           const uint32_t* __restrict__ scan_of, uint32_t n_scan,
                                                           const uint32_t* __restrict__ cum, uint32_t* __restrict__ cursor,
                                                           uint64_t* __restrict__ list) {
  __shared__ uint32_t wc[4][kLabeledMaxScan + 1];   // [wave][scanning slot] rows of the wave
  const uint32_t tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  for (uint32_t i = tid; i < 4u * (kLabeledMaxScan + 1u); i += 256u) (&wc[0][0])[i] = 0u;
  __syncthreads();
  const uint64_t r = (uint64_t)tile * 256u + tid;
  uint32_t slot;
  const uint32_t sc = labeled_scan_of(slot_of, scan_of, r, n_rows, n_scan, &slot);
  if (slot != (uint32_t)kLabeledNoSlot && sc == kLabeledNoScan) list[off[slot] + atomicAdd(&cursor[slot], 1u)] = r;
  // the rank of a scanning slot's row among the wave's rows of that slot: one round per distinct scanning slot of the wave
  uint32_t rank = 0;
  for (uint64_t todo = __ballot(sc != kLabeledNoScan); todo;) {   // (wave-uniform)
    const int leader = __ffsll((unsigned long long)todo) - 1;
    const uint32_t lsc = (uint32_t)__shfl((int)sc, leader, 64);
    const uint64_t same = __ballot(sc == lsc);
    if (sc == lsc) rank = (uint32_t)__builtin_popcountll(same & ((1ull << lane) - 1ull));
    if ((int)lane == leader) wc[w][lsc] = (uint32_t)__builtin_popcountll(same);
    todo &= ~same;
  }
  __syncthreads();
  if (sc == kLabeledNoScan) return;
  uint32_t before = 0;
  for (uint32_t i = 0; i < w; ++i) before += wc[i][sc];
  list[off[slot] + cum[(size_t)sc * (n_tiles + 1u) + tile] + before + rank] = r;
}

// one workgroup per scanning slot: its sample (write_sample, ehx_kernels.h) at sample + 256 scan
__global__ __launch_bounds__(256) void labeled_sample_kernel(const uint64_t* __restrict__ list,
                                                             const uint64_t* __restrict__ scan_off,
                                                             const uint32_t* __restrict__ cum, uint32_t n_tiles,
                                                             uint64_t* __restrict__ sample) {
  const uint32_t sc = blockIdx.x;
  write_sample(list + scan_off[sc], cum[(size_t)sc * (n_tiles + 1u) + n_tiles], sample + (size_t)sc * 256u);
}

namespace {
constexpr uint32_t kLabeledGrid = 2048;   // workgroups of the grid-stride kernels, at most (8 per CU): chosen, not measured
}

hipError_t launch_labeled_count(const uint32_t* label_of, uint64_t n_rows, const uint32_t* table, uint32_t n_slots,
                                uint16_t* slot_of, uint32_t* count, hipStream_t st) {
  if (n_slots == 0) return hipSuccess;
  if (n_slots > kLabeledMaxSlots || n_rows > 0xFFFFFFFFull) return hipErrorInvalidValue;
  if (hipError_t e = hipMemsetAsync(count, 0, n_slots * sizeof(uint32_t), st); e != hipSuccess) return e;
  const uint32_t n_tiles = (uint32_t)((n_rows + 255u) / 256u);
  if (n_tiles == 0) return hipSuccess;
  hipLaunchKernelGGL(labeled_count_kernel, dim3(std::min(n_tiles, kLabeledGrid)), dim3(256), 0, st, label_of, n_rows, n_tiles,
                     table, n_slots, slot_of, count);
  return hipGetLastError();
}

hipError_t launch_labeled_tiles(const uint16_t* slot_of, uint64_t n_rows, uint32_t n_tiles, const uint32_t* scan_of,
                                uint32_t n_scan, uint32_t* cum, hipStream_t st) {
  if (n_tiles == 0 || n_scan == 0) return hipSuccess;
  if (n_scan > kLabeledMaxScan || (uint64_t)n_tiles * 256u < n_rows) return hipErrorInvalidValue;
  hipLaunchKernelGGL(labeled_tiles_kernel, dim3(std::min(n_tiles, kLabeledGrid)), dim3(256), 0, st, slot_of, n_rows, n_tiles,
                     scan_of, n_scan, cum);
  return launch_rows_prefix(cum, n_scan, n_tiles, st);
}

hipError_t launch_labeled_fill(const uint16_t* slot_of, uint64_t n_rows, uint32_t n_tiles, uint32_t n_slots,
                               const uint64_t* off, const uint32_t* scan_of, uint32_t n_scan, const uint32_t* cum,
                               uint32_t* cursor, uint64_t* list, hipStream_t st) {
  if (n_tiles == 0 || n_slots == 0) return hipSuccess;
  if (n_slots > kLabeledMaxSlots || n_scan > kLabeledMaxScan || (uint64_t)n_tiles * 256u < n_rows) return hipErrorInvalidValue;
  if (hipError_t e = hipMemsetAsync(cursor, 0, n_slots * sizeof(uint32_t), st); e != hipSuccess) return e;
  hipLaunchKernelGGL(labeled_fill_kernel, dim3(n_tiles), dim3(256), 0, st, slot_of, n_rows, n_tiles, off, scan_of, n_scan, cum,
                     cursor, list);
  return hipGetLastError();
}

hipError_t launch_labeled_samples(const uint64_t* list, const uint64_t* scan_off, const uint32_t* cum, uint32_t n_scan,
                                  uint32_t n_tiles, uint64_t* sample, hipStream_t st) {
  if (n_tiles == 0 || n_scan == 0) return hipSuccess;
  if (n_scan > kLabeledMaxScan) return hipErrorInvalidValue;
  hipLaunchKernelGGL(labeled_sample_kernel, dim3(n_scan), dim3(256), 0, st, list, scan_off, cum, n_tiles, sample);
  return hipGetLastError();
}

}  // namespace ehx
