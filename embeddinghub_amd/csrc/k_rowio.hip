// Rows written from device memory (ehx_set_batch_device): the mirror of gather_rows_kernel (k_bykey.hip).  The source is a
// dense [*][dims] matrix of fp32 or binary16 values in HBM; the destination the stored rows, fp32 or binary16.
#include "ehx_kernels.h"

namespace ehx {

namespace {
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
constexpr uint32_t kWavesPerBlock = 4;
}  // namespace

// One wave per source row: work item i reads source row src_idx[i] (nullptr: i) and writes columns [0, dims) of stored row
// dst_row[i] (nullptr: row0 + i); a destination of ~0 is skipped (a key given again later in the batch: the host marks every
// occurrence but the last, so no two waves write one row).  Columns [dims, ld) keep the zeroes grow put there.
//   fp32 -> fp32      the bits as they are
//   fp32 -> binary16  rounded to nearest-even, overflow to +-Inf (v_cvt_f16_f32 in the default mode: what F16C does on the host)
//   binary16 -> binary16  the bits as they are;  binary16 -> fp32  widened (exact)
// A stored row starts on a 128-byte boundary (ld % 32 == 0); a source row may start on any element boundary (a tensor view).
// 16-byte accesses where both sides allow them — the source row 16-byte aligned and dims % 4 == 0 (fp32 -> fp32) or
// dims % 8 == 0 (the paths with a binary16 side) — else element by element.
__global__ __launch_bounds__(64 * kWavesPerBlock) void scatter_rows_kernel(ScatterRowsArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (i >= a.n) return;
  const uint64_t r = a.dst_row ? a.dst_row[i] : a.row0 + i;
  if (r == ~0ull) return;
  const size_t sr = a.src_idx ? a.src_idx[i] : i;
  const uint32_t dims = a.dims;
  const char* __restrict__ sp = (const char*)a.src + sr * dims * (a.src_half ? sizeof(_Float16) : sizeof(float));
  const bool aligned = ((uintptr_t)sp & 15u) == 0;
  const uint32_t n8 = aligned && (dims & 7u) == 0 ? dims >> 3 : 0;
  if (a.x_half) {
    _Float16* __restrict__ x = (_Float16*)a.X + (size_t)r * a.ld;
    if (a.src_half) {
      const uint16_t* __restrict__ s = (const uint16_t*)sp;
      for (uint32_t c = lane; c < n8; c += 64) ((uint4*)x)[c] = ((const uint4*)s)[c];
      for (uint32_t c = n8 * 8 + lane; c < dims; c += 64) ((uint16_t*)x)[c] = s[c];
      return;
    }
    const float* __restrict__ s = (const float*)sp;
    for (uint32_t c = lane; c < n8; c += 64) {
      const float4 v0 = ((const float4*)s)[2 * c], v1 = ((const float4*)s)[2 * c + 1];
      half8_t h;
      h[0] = (_Float16)v0.x, h[1] = (_Float16)v0.y, h[2] = (_Float16)v0.z, h[3] = (_Float16)v0.w;
      h[4] = (_Float16)v1.x, h[5] = (_Float16)v1.y, h[6] = (_Float16)v1.z, h[7] = (_Float16)v1.w;
      ((half8_t*)x)[c] = h;
    }
    for (uint32_t c = n8 * 8 + lane; c < dims; c += 64) x[c] = (_Float16)s[c];
    return;
  }
  float* __restrict__ x = (float*)a.X + (size_t)r * a.ld;
  if (a.src_half) {
    const _Float16* __restrict__ s = (const _Float16*)sp;
    for (uint32_t c = lane; c < n8; c += 64) {
      const half8_t h = ((const half8_t*)s)[c];
      ((float4*)x)[2 * c] = make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
      ((float4*)x)[2 * c + 1] = make_float4((float)h[4], (float)h[5], (float)h[6], (float)h[7]);
    }
    for (uint32_t c = n8 * 8 + lane; c < dims; c += 64) x[c] = (float)s[c];
    return;
  }
  const uint32_t* __restrict__ s = (const uint32_t*)sp;
  const uint32_t n4 = aligned && (dims & 3u) == 0 ? dims >> 2 : 0;
  for (uint32_t c = lane; c < n4; c += 64) ((uint4*)x)[c] = ((const uint4*)s)[c];
  for (uint32_t c = n4 * 4 + lane; c < dims; c += 64) ((uint32_t*)x)[c] = s[c];
}

hipError_t launch_scatter_rows(const ScatterRowsArgs& a, hipStream_t st) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(scatter_rows_kernel, dim3((a.n + kWavesPerBlock - 1) / kWavesPerBlock), dim3(64 * kWavesPerBlock), 0,
                     st, a);
  return hipGetLastError();
}

}  // namespace ehx
