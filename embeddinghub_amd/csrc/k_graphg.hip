// Graph-mode GROUPED search (ehx_graph_knn_grouped*, ehx_graphg.cpp): "the k nearest rows, at most per_group of a group",
// walked.  The walk is the bitmap walk's (k_graphm_walk.h; its model is tests/filtered_walk_model.py) with "allowed" replaced
// by ELIGIBLE, which is a fact about the list R and not about a row alone (the model: tests/grouped_walk_model.py):
//   * row r is labelled iff r < a.allow_bits (= n_eff, the prefix that has labels); a row that is not is walked through and
//     never returned, never eligible and counted toward no cap — kKeyAllowed in a key means "labelled";
//   * an entry of R is eligible iff it is labelled and its label is EHX_GROUP_NONE or fewer than per_group labelled entries
//     of R with its label lie in front of it;
//   * R is trimmed behind its ef-th ELIGIBLE entry and never grows beyond a.ef_cap; the answer is its first k eligible ones.
// A closer row of a group makes a farther one ineligible, so eligibility is state, and it is kept where R is, in LDS:
//   tag[ef_cap] u32   the label of every slot of R, behind GraphLds' carve (graph_list_lds_offset)
//   bit 1 of F[]      the slot's entry is eligible (bit 0 is the merge's landing mark, zero outside a merge)
// Both move with their key (merge_sorted_into_R's payload form).  Four bytes a slot: at ef 100 (a list of 1200) and rows of
// 768 floats the wave's LDS is 20160 bytes, eight waves a CU — what the bitmap walk's registers allow it.
// Per step, beside the bitmap walk's work:
//   * the label of a fresh labelled neighbour is loaded where that walk loads the word of its bitmap, in flight beside the
//     row fetches; nothing else goes to global memory;
//   * behind the merge, for every labelled key of a real group that went in (a wave-uniform loop; keys the walk dropped in
//     front of the merge and EHX_GROUP_NONE keys are not in it): one lane-parallel pass over R in chunks of 64 — ballot of
//     "labelled and of this group", popcount in front of the lane — gives every entry of the group its rank and sets its
//     flag to rank < per_group.  A fresh key of a real group goes in with the flag clear, so the pass is what makes it
//     eligible, and it ends as soon as per_group + 64 entries of the group are behind it: at most 64 keys went in, so
//     entries farther back had rank >= per_group before and have it now;
//   * the trim counts flags as the bitmap walk counts allowed bits, and is skipped when no flag changed, no EHX_GROUP_NONE
//     key went in and the list does not end at cap: the eligible entries are then the ones counted last time.
// One wavefront per query, no matrix instructions: a pointer chase, a 64-lane distance per neighbour row and integer
// bookkeeping.  The descent, wave_group_dists, the visited bitmap and its log, the adjacency prefetch and the page write are
// the shared pieces; the level-0 loop is written out here, not a fourth TABLE of k_graphm_walk.h: that text is kept
// instruction-identical for its three users, and this merge carries a payload and this trim counts what an insertion changes.
#include "k_graphm_keys.h"

namespace ehx {
namespace {

constexpr uint8_t kSlotEligible = 2;   // bit 1 of a slot's byte of F

struct GroupPayload {
  static constexpr bool kHas = true;
  uint32_t* tag;     // [ef_cap] the label of every slot of R
  uint32_t* stage;   // [64] the fresh labels in the fresh keys' order
  uint32_t mine;     // the label of the lane's fresh key
  // a fresh key: eligible at once iff labelled and a group of its own; a real group's pass decides behind the merge
  __device__ __forceinline__ uint8_t first(uint64_t key, uint32_t label) const {
    return (key & kKeyAllowed) && label == kGroupNone ? kSlotEligible : (uint8_t)0;
  }
};

}  // namespace

template <int METRIC01>
__global__ __launch_bounds__(64) void graph_search_grouped_kernel(const GraphArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const uint32_t qi = blockIdx.x;
  GraphLds L;
  L.carve(smem, a.ld, a.ef_cap, 64);
  uint64_t* R = L.R;
  uint64_t* batch = L.batch;
  uint32_t* ids_l = L.ids;
  uint32_t* labs = (uint32_t*)L.S;   // a step's fresh labels by slot; S is the merge's, which runs behind their last read
  // (the labels' LDS address is worked out where a merge needs it, not held in a scalar register across the step)
  auto tags = [&]() {
    const KernArgs p = late_args();
    return (uint32_t*)(smem + graph_list_lds_offset(p->ld, p->ef_cap));
  };
  uint32_t n_logged = 0;  // rows marked visited so far (wave-uniform)
  for (uint32_t i = lane; i < a.ef_cap; i += 64) L.F[i] = 0;
  load_query<1>(a, L.qs, qi, 0, lane);

  WalkCounters ctr;
  const Descent top = greedy_descent<METRIC01>(a, L, lane, ctr);
  const uint32_t cur = top.cur;
  // (scalar registers are what the level-0 loop runs out of: k_graphm_walk.h says what is done about it, and so it is here)
  if (lane == 0) {
    atomicAdd(&a.counters[0], ctr.n_dist);
    atomicAdd(&a.counters[2], ctr.n_hops_up);
    L.ctrl[0] = 0u;
  }
  uint32_t n_hops0 = 0;

  const KernArgs al = late_args();
  const uint32_t ef = al->ef, cap = al->ef_cap, M0 = al->M0;
  const uint32_t* adj0 = al->adj0;
  uint32_t* vis = al->visited + (size_t)qi * al->vis_words;
  const uint64_t lt_lane = (1ull << lane) - 1ull;
  // eligible entries of R: exact at the head of every step; trimmed: R holds exactly ef of them and ends with one
  uint32_t n_elig = cur < al->allow_bits ? 1u : 0u;
  uint32_t nR = 1;
  if (lane == 0) {
    uint32_t* vlog = al->vislog + (size_t)qi * al->vislog_cap;
    R[0] = ((uint64_t)(top.nan_seed ? kOrdNaN : f32_to_ordered(top.curdist)) << 32) | ((uint64_t)cur << 2) |
           (n_elig ? kKeyAllowed : 0ull);
    tags()[0] = n_elig ? al->group_of[cur] : kGroupNone;
    L.F[0] = n_elig ? kSlotEligible : (uint8_t)0;   // (nothing lies in front of it; per_group >= 1)
    atomicOr(&vis[cur >> 5], 1u << (cur & 31));
    if (al->vislog_cap) vlog[0] = cur;
  }
  n_logged = 1;
  wave_lds_sync();
  uint32_t scan_from = 0;  // every entry of R before this index is expanded
  uint32_t pf_node = kNoNode, pf_nb = kNoNode, pf_word = 0;
  GraphProf prof;
  for (;;) {
    // closest unexpanded entry (and the one after it), as k_graph.hip picks them
    uint32_t idx = kNoNode, idx2 = kNoNode;
    uint64_t kidx = 0, kidx2 = kKeyInf;
    for (uint32_t base = scan_from & ~63u; base < nR && idx2 == kNoNode; base += 128) {
      const uint32_t i0 = base + lane, i1 = i0 + 64;
      const uint64_t v0 = i0 < nR ? R[i0] : kKeyExpanded;  // beyond nR: "expanded"
      const uint64_t v1 = i1 < nR ? R[i1] : kKeyExpanded;
      uint64_t m0 = __ballot(!(v0 & kKeyExpanded)), m1 = __ballot(!(v1 & kKeyExpanded));
#pragma unroll
      for (int pick = 0; pick < 2; ++pick) {
        if (pick == 0 ? idx != kNoNode : (idx == kNoNode || idx2 != kNoNode)) continue;
        uint32_t at = kNoNode;
        uint64_t key = 0;
        if (m0) {
          const int l = __builtin_ctzll(m0);
          m0 &= m0 - 1;
          at = base + (uint32_t)l;
          key = readlane64(v0, l);
        } else if (m1) {
          const int l = __builtin_ctzll(m1);
          m1 &= m1 - 1;
          at = base + 64 + (uint32_t)l;
          key = readlane64(v1, l);
        }
        if (at == kNoNode) continue;
        if (pick == 0) {
          idx = at;
          kidx = key;
        } else {
          idx2 = at;
          kidx2 = key;
        }
      }
    }
    if (idx == kNoNode) break;
    const uint32_t c = mkey_id(kidx);
    const uint32_t c2 = idx2 != kNoNode ? mkey_id(kidx2) : kNoNode;
    wave_lds_sync();
    if (lane == 0) R[idx] |= kKeyExpanded;
    n_hops0 += 1;
    // neighbours (stored order) and their visited words
    uint32_t nb = kNoNode, word = 0;
    if (c == pf_node) {
      nb = pf_nb;
      word = pf_word;
    } else {  // the first expansion, and a pick the trim moved away from what was requested
      if (lane < (int)M0) nb = adj0[(size_t)c * M0 + lane];
      if (nb != kNoNode) word = __hip_atomic_load(&vis[nb >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const bool fresh = nb != kNoNode && !(word & (1u << (nb & 31)));
    if (fresh) (void)__hip_atomic_fetch_or(&vis[nb >> 5], 1u << (nb & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the label of a fresh labelled id, in flight beside the row fetches (kNoNode lies above every prefix)
    const KernArgs ap = late_args();
    const bool labelled = nb < ap->allow_bits;
    uint32_t lab = kGroupNone;
    if (fresh && labelled) lab = load_here(ap->group_of + nb);
    pf_node = c2;
    pf_nb = kNoNode;
    if (c2 != kNoNode && lane < (int)M0) pf_nb = load_here(adj0 + (size_t)c2 * M0 + lane);
    const uint64_t fmask = __ballot(fresh);
    const uint32_t nfresh = __builtin_popcountll(fmask);
    const uint32_t slot = (uint32_t)__builtin_popcountll(fmask & lt_lane);
    if (fresh) {
      ids_l[slot] = nb;
      batch[slot] = labelled ? kKeyAllowed : 0ull;   // (lane slot takes both back behind the distances)
      labs[slot] = lab;
      const uint32_t vislog_cap = ap->vislog_cap;
      if (n_logged + slot < vislog_cap) ap->vislog[(size_t)qi * vislog_cap + n_logged + slot] = nb;
    }
    n_logged += nfresh;
    wave_lds_sync();
    // distances: lane p (< nfresh) owns fresh neighbour p; a NaN distance keeps +inf and never enters R
    uint64_t mykey = kKeyInf;
    uint32_t mylab = kGroupNone;
    if (nfresh) {
      const float d = wave_group_dists<METRIC01>(L.qs, a.Xs, a.ld, a.dims, ids_l, nfresh, lane, a.xscale);
      if ((uint32_t)lane < nfresh && d == d) {
        mykey = ((uint64_t)f32_to_ordered(d) << 32) | ((uint64_t)ids_l[lane] << 2) | batch[lane];
        mylab = labs[lane];
      }
    }
    // a key behind R's last entry while R is trimmed or at cap would be deleted by this step's trim, and changes no
    // entry's eligibility in front of it: dropped here
    const bool trimmed = n_elig >= ef;
    if ((trimmed || nR == cap) && mykey > R[nR - 1]) mykey = kKeyInf;
    wave_lds_sync();
    const uint32_t nin = (uint32_t)__builtin_popcountll(__ballot(mykey != kKeyInf));
    scan_from = idx2 != kNoNode ? idx2 : nR;  // entries before idx2 are all expanded now (positions only grow)
    const bool do_merge = nin != 0;
    uint64_t minkey = kKeyInf;
    uint32_t rank = 0;
    if (do_merge) {
      batch[lane] = mykey;
      wave_lds_sync();
      rank = rank_by_counting(batch, nfresh, mykey);  // (batch[nfresh..64) = +inf never counts)
      const uint64_t first = __ballot(mykey != kKeyInf && rank == 0);
      minkey = readlane64(mykey, (int)__builtin_ctzll(first));
    }
    // the node expanded next, unless the trim deletes it (then the pick above does not match): requested before the merge
    bool pf_have_word;
    if (minkey < kidx2) {
      pf_node = mkey_id(minkey);
      pf_nb = kNoNode;
      if (lane < (int)M0) pf_nb = load_here(adj0 + (size_t)pf_node * M0 + lane);
      pf_have_word = false;
    } else {
      pf_word = 0;
      if (pf_nb != kNoNode) pf_word = __hip_atomic_load(&vis[pf_nb >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      pf_have_word = true;
    }
    if (do_merge) {
      uint32_t* tag = tags();
      const GroupPayload pay = {tag, ids_l, mylab};   // (ids_l: the distances have read it)
      merge_sorted_into_R<5, 6>(L, cap, mykey, mykey != kKeyInf, rank, nin, nR, scan_from, lane, prof, pay);
      // re-rank the groups the merge touched.  (A list that ends at cap may have lost eligible entries behind it: counted
      // anew, as the bitmap walk does for a merge that cut at cap)
      const uint32_t per_group = late_args()->per_group;
      const bool came = mykey != kKeyInf && (mykey & kKeyAllowed);   // labelled keys of this merge
      uint32_t recount = nR == cap || __ballot(came && mylab == kGroupNone) != 0ull ? 1u : 0u;
      uint64_t todo = __ballot(came && mylab != kGroupNone);
      while (todo) {
        const uint32_t g = (uint32_t)__builtin_amdgcn_readlane((int)mylab, (int)__builtin_ctzll(todo));
        todo &= todo - 1;   // (two keys of one group: the second pass finds every flag as it wants it)
        const uint32_t enough = per_group + 64u;   // (at most 64 keys went in; per_group <= ef_cap: the launcher's)
        uint32_t seen = 0;
        for (uint32_t base = 0; base < nR && seen < enough; base += 64) {
          const uint32_t i = base + (uint32_t)lane;
          const bool of_g = i < nR && (R[i] & kKeyAllowed) && tag[i] == g;
          const uint64_t m = __ballot(of_g);
          bool flip = false;
          if (of_g) {
            const uint8_t want = seen + (uint32_t)__builtin_popcountll(m & lt_lane) < per_group ? kSlotEligible : (uint8_t)0;
            flip = L.F[i] != want;
            if (flip) L.F[i] = want;
          }
          recount |= __ballot(flip) != 0ull ? 1u : 0u;
          seen += (uint32_t)__builtin_popcountll(m);
        }
      }
      wave_lds_sync();
      // the trim: the ef-th eligible entry of R ends it
      if (recount) {
        uint32_t seen = 0, cut = kNoNode;
        for (uint32_t base = 0; base < nR && cut == kNoNode; base += 64) {
          const uint32_t i = base + (uint32_t)lane;
          const uint64_t m = __ballot(i < nR && (L.F[i] & kSlotEligible) != 0);
          const uint32_t cnt = (uint32_t)__builtin_popcountll(m);
          if (seen + cnt >= ef) {
            const uint32_t want = ef - seen - 1u;   // eligible entries of this chunk in front of the one looked for
            const uint64_t hit = __ballot(((m >> lane) & 1ull) && (uint32_t)__builtin_popcountll(m & lt_lane) == want);
            cut = base + (uint32_t)__builtin_ctzll(hit);
          } else {
            seen += cnt;
          }
        }
        n_elig = cut != kNoNode ? ef : seen;
        if (cut != kNoNode) nR = cut + 1u;
      }
      if (nR == cap && lane == 0) L.ctrl[0] = 1u;
    }
    if (!pf_have_word) {
      pf_word = 0;
      if (pf_nb != kNoNode) pf_word = __hip_atomic_load(&vis[pf_nb >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }

  // ---- the visited bitmap back to all-zero, the first k eligible entries of R, the counters ----
  const KernArgs ap = late_args();
  clear_visited(ap->vislog_cap, ap->vis_words, lane, vis, ap->vislog + (size_t)qi * ap->vislog_cap, n_logged);
  const uint32_t k = ap->k;
  uint64_t* out_ids = ap->out_ids + (size_t)qi * k;
  float* out_dist = ap->out_dist + (size_t)qi * k;
  uint32_t cnt = 0;
  for (uint32_t base = 0; base < nR && cnt < k; base += 64) {
    const uint32_t i = base + (uint32_t)lane;
    const uint64_t v = i < nR ? R[i] : 0ull;
    const bool ok = i < nR && (L.F[i] & kSlotEligible) != 0 && (uint32_t)(v >> 32) != kOrdNaN;
    const uint64_t m = __ballot(ok);
    const uint32_t pos = cnt + (uint32_t)__builtin_popcountll(m & lt_lane);
    if (ok && pos < k) {
      out_ids[pos] = (uint64_t)mkey_id(v);
      out_dist[pos] = ordered_to_f32((uint32_t)(v >> 32));
    }
    cnt += (uint32_t)__builtin_popcountll(m);
  }
  if (cnt > k) cnt = k;
  for (uint32_t j = cnt + (uint32_t)lane; j < k; j += 64) {
    out_ids[j] = ~0ull;
    out_dist[j] = __builtin_inff();
  }
  if (lane == 0) {
    ap->out_count[qi] = cnt;
    unsigned long long* counters = ap->counters;
    atomicAdd(&counters[0], (unsigned long long)(n_logged - 1u));
    atomicAdd(&counters[1], (unsigned long long)n_hops0);
    if (L.ctrl[0]) atomicAdd(ap->cap_hits, 1ull);
  }
}

size_t graph_grouped_lds_bytes(uint32_t ld, uint32_t ef_cap) {
  return graph_list_lds_offset(ld, ef_cap) + (size_t)ef_cap * sizeof(uint32_t);
}

hipError_t launch_graph_search_grouped(const GraphArgs& a, hipStream_t st) {
  if (a.n > (1u << 30) || a.ef_cap < a.ef || a.M0 > 64 || !a.cap_hits || (a.allow_bits && !a.group_of) || a.per_group == 0 ||
      a.per_group > a.ef_cap || a.allow_bits > a.n || a.q_raw)
    return hipErrorInvalidValue;
  const size_t lds = graph_grouped_lds_bytes(a.ld, a.ef_cap);
  if (lds > kMaxLds) return hipErrorInvalidValue;
  static DynLdsAttr attr;
  static const GraphKernel kGrouped[2] = {graph_search_grouped_kernel<0>, graph_search_grouped_kernel<1>};   // [metric != L2]
  if (hipError_t e = attr.ensure(kGrouped, 2, lds); e != hipSuccess) return e;
  hipLaunchKernelGGL(kGrouped[a.metric != 0], dim3(a.nq), dim3(64), lds, st, a);
  return hipGetLastError();
}

}  // namespace ehx
