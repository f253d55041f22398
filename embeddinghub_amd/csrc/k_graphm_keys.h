// What the walks under a filter (k_graphm.hip: a row bitmap, or one per query; k_graphx.hip: an exclusion list per query) share
// besides k_graph_common.h: the two flag bits of their keys — (ordered distance << 32) | (id << 2) | (allowed << 1) | expanded —
// and the scalar reads of the argument block and of per-query argument words.  The walk itself is k_graphm_walk.h.
#pragma once
#include "k_graph_common.h"

namespace ehx {
namespace {

constexpr uint64_t kKeyExpanded = 1ull, kKeyAllowed = 2ull;
__device__ __forceinline__ uint32_t mkey_id(uint64_t key) { return (uint32_t)(key & 0xFFFFFFFFull) >> 2; }

// the kernel's argument block where it lies in memory (scalar loads at the point of use; the empty asm keeps them there)
typedef const GraphArgs __attribute__((address_space(4)))* KernArgs;
__device__ __forceinline__ KernArgs late_args() {
  KernArgs p = (KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}
// query qi's entry of a [nq] argument array the host wrote before the launch: wave-uniform and constant while the kernel
// runs, so it is read with a scalar load (no vector-memory round trip in front of the load that depends on it)
typedef const uint32_t __attribute__((address_space(4)))* ConstWords;
__device__ __forceinline__ uint32_t uniform_word(const uint32_t* p, uint32_t qi) { return ((ConstWords)p)[qi]; }


// Where a query's exclusion list begins in the LDS of its wave (k_graphx.hip): behind everything GraphLds carves, aligned
// for the 16-byte copy.  The launcher adds the list region to it.
__host__ __device__ constexpr size_t graph_list_lds_offset(uint32_t ld, uint32_t ef_cap) {
  return (GraphLds::bytes(ld, ef_cap, 64) + 15) & ~(size_t)15;
}

// Whether the ascending array a[0, n) in LDS holds id; n is wave-uniform, id is the lane's own.  A lower bound by halving:
// ceil(log2 n) steps, the same number in every lane, each a read inside [0, n) and a select — no branch depends on what a
// lane holds — then one read for the answer.  An empty list reads nothing.
__device__ __forceinline__ bool lds_list_holds(const uint32_t* a, uint32_t n, uint32_t id) {
  if (n == 0) return false;
  uint32_t base = 0;
  for (uint32_t len = n; len > 1;) {
    const uint32_t half = len >> 1;
    base = a[base + half] <= id ? base + half : base;
    len -= half;
  }
  return a[base] == id;
}

}  // namespace

}  // namespace ehx
