// The body of the walk kernels of k_graphm.hip — included INSIDE each of them, not a header of declarations: with
//   METRIC01   0: L2, 1: the dot-product metrics
//   TABLE      0: ONE bitmap for the batch; 1: a bitmap PER QUERY (ehx_graph_knn_masked_multi*) — a.allow is a table of bitmaps
//              and query qi's begins a.allow_of[qi] words into it.  The offset is wave-uniform and is read where a bit is
//              tested (one scalar load beside the ones late_args() already issues there), never held across the level-0 loop
//   a          the kernel's GraphArgs
// in scope.  Text, not a __device__ function: a function inlined into the kernels is optimised on its own first (without
// the kernel's launch bounds) and came out as other code for the one-bitmap pair than the kernel written out — 2 % or so
// slower on the 768-dimension bench — while this text with TABLE = 0 is that kernel, instruction for instruction.
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const uint32_t qi = blockIdx.x;
  GraphLds L;
  L.carve(smem, a.ld, a.ef_cap, 64);
  uint64_t* R = L.R;
  uint64_t* batch = L.batch;
  uint32_t* ids_l = L.ids;
  uint32_t n_logged = 0;  // rows marked visited so far (wave-uniform)
  for (uint32_t i = lane; i < a.ef_cap; i += 64) L.F[i] = 0;
  load_query<1>(a, L.qs, qi, 0, lane);

  WalkCounters ctr;
  const Descent top = greedy_descent<METRIC01>(a, L, lane, ctr);
  const uint32_t cur = top.cur;
  // Scalar registers are what the level-0 loop runs out of (the shared pieces hold the argument block in them): the
  // descent's counts go out now, level 0 counts in 32 bits (its rows fetched are n_logged - 1), the flag "the list
  // reached cap" lives in LDS (ctrl: the wide walk's word, free here), and arguments used once per step or only by the
  // epilogue are read where they are used (late_args).
  if (lane == 0) {
    atomicAdd(&a.counters[0], ctr.n_dist);
    atomicAdd(&a.counters[2], ctr.n_hops_up);
    L.ctrl[0] = 0u;
  }
  uint32_t n_hops0 = 0;   // (prefetch hits, counters[3], are not counted by this walk)

  // (what the level-0 loop needs and the descent does not: read behind the descent)
  const KernArgs al = late_args();
  const uint32_t ef = al->ef, cap = al->ef_cap, M0 = al->M0;
  const uint32_t* adj0 = al->adj0;
  uint32_t* vis = al->visited + (size_t)qi * al->vis_words;
  const uint64_t lt_lane = (1ull << lane) - 1ull;
  // allowed entries of R: exact behind every trim, an upper bound in between (entries the merge dropped behind cap are
  // not taken off); trimmed: R holds exactly ef of them and ends with one
  uint32_t n_allow = cur < al->allow_bits && ((al->allow[(TABLE ? uniform_word(al->allow_of, qi) : 0u) + (cur >> 5)] >> (cur & 31)) & 1u) ? 1u : 0u;
  n_allow = wave_uniform(n_allow);   // (>= ef at the head of a step: R is trimmed, and then it is ef exactly)
  uint32_t nR = 1;
  if (lane == 0) {
    uint32_t* vlog = al->vislog + (size_t)qi * al->vislog_cap;
    R[0] = ((uint64_t)(top.nan_seed ? kOrdNaN : f32_to_ordered(top.curdist)) << 32) | ((uint64_t)cur << 2) |
           (n_allow ? kKeyAllowed : 0ull);
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
    // the allowed bit of a fresh id: its word of the bitmap, in flight beside the row fetches
    const KernArgs ap = late_args();
    uint32_t aword = 0;
    if (fresh && nb < ap->allow_bits) aword = ap->allow[(TABLE ? uniform_word(ap->allow_of, qi) : 0u) + (nb >> 5)];
    pf_node = c2;
    pf_nb = kNoNode;
    if (c2 != kNoNode && lane < (int)M0) pf_nb = load_here(adj0 + (size_t)c2 * M0 + lane);
    const uint64_t fmask = __ballot(fresh);
    const uint32_t nfresh = __builtin_popcountll(fmask);
    const uint32_t slot = (uint32_t)__builtin_popcountll(fmask & lt_lane);
    if (fresh) {
      ids_l[slot] = nb;
      batch[slot] = (aword >> (nb & 31)) & 1u ? kKeyAllowed : 0ull;   // (lane slot takes it back behind the distances)
      const uint32_t vislog_cap = ap->vislog_cap;
      if (n_logged + slot < vislog_cap) ap->vislog[(size_t)qi * vislog_cap + n_logged + slot] = nb;
    }
    n_logged += nfresh;
    wave_lds_sync();
    // distances: lane p (< nfresh) owns fresh neighbour p; a NaN distance keeps +inf and never enters R
    uint64_t mykey = kKeyInf;
    if (nfresh) {
      const float d = wave_group_dists<METRIC01>(L.qs, a.Xs, a.ld, a.dims, ids_l, nfresh, lane, a.xscale);
      if ((uint32_t)lane < nfresh && d == d)
        mykey = ((uint64_t)f32_to_ordered(d) << 32) | ((uint64_t)ids_l[lane] << 2) | batch[lane];
    }
    // a key behind R's last entry while R is trimmed or at cap would be deleted by this step's trim: dropped here
    const bool trimmed = n_allow >= ef;
    if ((trimmed || nR == cap) && mykey > R[nR - 1]) mykey = kKeyInf;
    wave_lds_sync();
    const uint32_t nin = (uint32_t)__builtin_popcountll(__ballot(mykey != kKeyInf));
    const uint32_t nin_allowed = (uint32_t)__builtin_popcountll(__ballot(mykey != kKeyInf && (mykey & kKeyAllowed)));
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
      const bool cut_at_cap = nR + nin > cap;   // the merge drops R's tail behind cap: allowed entries may leave with it
      merge_sorted_into_R<5, 6>(L, cap, mykey, mykey != kKeyInf, rank, nin, nR, scan_from, lane, prof);
      n_allow += nin_allowed;
      // the trim: the ef-th allowed entry of R ends it
      if (n_allow >= ef && !(trimmed && !cut_at_cap && nin_allowed == 0)) {
        uint32_t seen = 0, cut = kNoNode;
        for (uint32_t base = 0; base < nR && cut == kNoNode; base += 64) {
          const uint32_t i = base + (uint32_t)lane;
          const uint64_t v = i < nR ? R[i] : 0ull;
          const uint64_t m = __ballot((v & kKeyAllowed) != 0);
          const uint32_t cnt = (uint32_t)__builtin_popcountll(m);
          if (seen + cnt >= ef) {
            const uint32_t want = ef - seen - 1u;   // allowed entries of this chunk in front of the one looked for
            const uint64_t hit = __ballot(((m >> lane) & 1ull) && (uint32_t)__builtin_popcountll(m & lt_lane) == want);
            cut = base + (uint32_t)__builtin_ctzll(hit);
          } else {
            seen += cnt;
          }
        }
        n_allow = cut != kNoNode ? ef : seen;
        if (cut != kNoNode) nR = cut + 1u;
      }
      if (nR == cap && lane == 0) L.ctrl[0] = 1u;
    }
    if (!pf_have_word) {
      pf_word = 0;
      if (pf_nb != kNoNode) pf_word = __hip_atomic_load(&vis[pf_nb >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }

  // ---- the visited bitmap back to all-zero, the first k allowed entries of R, the counters ----
  const KernArgs ap = late_args();
  clear_visited(ap->vislog_cap, ap->vis_words, lane, vis, ap->vislog + (size_t)qi * ap->vislog_cap, n_logged);
  const uint32_t k = ap->k;
  uint64_t* out_ids = ap->out_ids + (size_t)qi * k;
  float* out_dist = ap->out_dist + (size_t)qi * k;
  uint32_t cnt = 0;
  for (uint32_t base = 0; base < nR && cnt < k; base += 64) {
    const uint32_t i = base + (uint32_t)lane;
    const uint64_t v = i < nR ? R[i] : 0ull;
    const bool ok = (v & kKeyAllowed) != 0 && (uint32_t)(v >> 32) != kOrdNaN;
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
