// Nearest neighbours of rows the space already holds (ehx_knn_by_keys / ehx_knn_by_ids_device): the query batch is
// gathered from the stored rows on the device, searched with k + 1 by the existing pipelines, and the row itself is
// removed from its own list on the device (server.cc:205-207: erase the key if present, else drop the last).
#include "ehx_kernels.h"

namespace ehx {

namespace {
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
constexpr uint32_t kWavesPerBlock = 4;
}  // namespace

// One wave per row: out[q][0, dims) = the bytes ehx_get_by_id returns for row row_ids[q] — fp32 rows as they are, binary16
// rows widened (exact), single-copy graph rows with the 4 x 4 block transpose undone (search_copy_pos).  A stored row starts
// on a 128-byte boundary (ld % 32 == 0), so the loads are 16 bytes per lane; the stores are when dims % 4 == 0 (every
// output row then starts on a 16-byte boundary), else the row goes element by element.  An id at or above n_rows writes a
// zero row and marks the query invalid (valid[q] = 0).  Row g of a sharded parent lives in shard g % G at local row g / G.
__global__ __launch_bounds__(64 * kWavesPerBlock) void gather_rows_kernel(GatherRowsArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t q = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (q >= a.n) return;
  const uint64_t g = a.row_ids[q];
  float* __restrict__ out = a.out + (size_t)q * a.rows.dims;
  const bool ok = g < a.rows.n_rows;
  if (lane == 0) a.valid[q] = ok ? 1u : 0u;
  if (!ok) {
    for (uint32_t c = lane; c < a.rows.dims; c += 64) out[c] = 0.0f;
    return;
  }
  const uint32_t g32 = (uint32_t)g, shard = a.G > 1 ? g32 % a.G : 0u, local = a.G > 1 ? g32 / a.G : g32;
  const char* __restrict__ base = (const char*)a.bases.p[shard];
  const bool vec = (a.rows.dims & 3u) == 0;
  if (a.rows.x_half) {
    const _Float16* __restrict__ x = (const _Float16*)base + (size_t)local * a.rows.ld;
    const uint32_t n8 = vec ? a.rows.dims >> 3 : 0;
    for (uint32_t c = lane; c < n8; c += 64) {
      const half8_t h = ((const half8_t*)x)[c];
      ((float4*)out)[2 * c] = make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
      ((float4*)out)[2 * c + 1] = make_float4((float)h[4], (float)h[5], (float)h[6], (float)h[7]);
    }
    for (uint32_t c = n8 * 8 + lane; c < a.rows.dims; c += 64) out[c] = (float)x[c];
    return;
  }
  const float* __restrict__ x = (const float*)base + (size_t)local * a.rows.ld;
  if (a.rows.x_perm) {
    const uint32_t n16 = vec ? a.rows.dims >> 4 : 0;   // whole 16-float blocks: four 16-byte loads, a transpose, four stores
    for (uint32_t b = lane; b < n16; b += 64) {
      const float4* s = (const float4*)(x + (size_t)b * 16);
      const float4 v0 = s[0], v1 = s[1], v2 = s[2], v3 = s[3];
      float4* d = (float4*)(out + (size_t)b * 16);
      d[0] = make_float4(v0.x, v1.x, v2.x, v3.x);
      d[1] = make_float4(v0.y, v1.y, v2.y, v3.y);
      d[2] = make_float4(v0.z, v1.z, v2.z, v3.z);
      d[3] = make_float4(v0.w, v1.w, v2.w, v3.w);
    }
    for (uint32_t c = n16 * 16 + lane; c < a.rows.dims; c += 64) out[c] = x[search_copy_pos(c)];
    return;
  }
  const uint32_t n4 = vec ? a.rows.dims >> 2 : 0;
  for (uint32_t c = lane; c < n4; c += 64) ((float4*)out)[c] = ((const float4*)x)[c];
  for (uint32_t c = n4 * 4 + lane; c < a.rows.dims; c += 64) out[c] = x[c];
}

hipError_t launch_gather_rows(const GatherRowsArgs& a, hipStream_t st) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((a.n + kWavesPerBlock - 1) / kWavesPerBlock), dim3(64 * kWavesPerBlock), 0,
                     st, a);
  return hipGetLastError();
}

// One wave per query: the (k + 1)-long list of query q without the first entry whose id is the query's own row, or
// without its last entry when the row is not in it, compacted into the k-long output (a ballot of the entries that stay
// and a prefix count per 64 entries).  out_count = min(count, k), or count - 1 when the row was removed from a list
// shorter than k + 1; a query the gather marked invalid gets count 0.  Entries beyond the count: id ~0, +Inf.
__global__ __launch_bounds__(64 * kWavesPerBlock) void drop_self_kernel(DropSelfArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t q = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (q >= a.n) return;
  const uint32_t L = a.k + 1;
  const uint64_t own = a.row_ids[q];
  uint32_t cnt = 0;
  if (a.valid[q]) {
    cnt = a.count[q];
    cnt = cnt < L ? cnt : L;
  }
  const uint64_t* __restrict__ ids = a.ids + (size_t)q * L;
  const float* __restrict__ dist = a.dist + (size_t)q * L;
  uint64_t* __restrict__ out_ids = a.out_ids + (size_t)q * a.k;
  float* __restrict__ out_dist = a.out_dist + (size_t)q * a.k;
  uint32_t kept = 0;
  bool removed = false;
  for (uint32_t j0 = 0; j0 < cnt; j0 += 64) {
    const uint32_t j = j0 + lane;
    const bool in = j < cnt;
    const uint64_t id = in ? ids[j] : ~0ull;
    const float d = in ? dist[j] : 0.0f;
    bool keep = in;
    if (!removed) {
      const unsigned long long mm = __ballot(in && id == own);
      if (mm) {
        removed = true;
        if (lane == (uint32_t)__builtin_ctzll(mm)) keep = false;
      }
    }
    const unsigned long long km = __ballot(keep);
    const uint32_t o = kept + (uint32_t)__builtin_popcountll(km & ((1ull << lane) - 1ull));
    if (keep && o < a.k) {
      out_ids[o] = id;
      out_dist[o] = d;
    }
    kept += (uint32_t)__builtin_popcountll(km);
  }
  const uint32_t oc = kept < a.k ? kept : a.k;
  for (uint32_t o = oc + lane; o < a.k; o += 64) {
    out_ids[o] = ~0ull;
    out_dist[o] = __builtin_inff();
  }
  if (lane == 0) a.out_count[q] = oc;
}

hipError_t launch_drop_self(const DropSelfArgs& a, hipStream_t st) {
  if (a.n == 0 || a.k == 0) return hipSuccess;
  hipLaunchKernelGGL(drop_self_kernel, dim3((a.n + kWavesPerBlock - 1) / kWavesPerBlock), dim3(64 * kWavesPerBlock), 0,
                     st, a);
  return hipGetLastError();
}

}  // namespace ehx
