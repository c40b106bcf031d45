// pm_propose.inc — neighbour rows (included by pm_kernels.hip inside namespace pm): a wave keeps the 64 nearest
// candidates of a seed sorted across its lanes (NearRow), over the whole list or over the spatial index's cells around
// the seed; carve_propose_kernel is the batch pipeline's launch of it.  Reference: sort_nodes_by_proximity, mod.rs:206-255.
// Proposal generator: one wave per located live slot of the prepared configuration.  The wave sweeps the whole
// candidate list and keeps its 64 smallest keys SORTED ACROSS ITS LANES (lane i = the i-th nearest so far).  A
// candidate enters only if it beats lane 63 (one compare against a wave-uniform threshold; after the first few
// hundred slots almost nothing does: 64 (1 + ln(n / 64)) insertions over a list of n), and an insertion is a
// wave-wide shift by one lane (DPP wave_shr) from the insertion point — so the sweep's inner loop is the key
// arithmetic alone, and the finished register IS the row: no per-lane queues, no pop rounds, no re-sweeps.
struct NearRow {
  uint64_t key;     // ascending over the lanes; ~0 = empty
  uint64_t tau;     // lane 63's key (wave-uniform): what a candidate has to beat
  uint64_t tau_hi;  // keys in (tau, tau_hi) may end up within the certificate band of the row's last entry
  // the unlisted candidates that came that close (rejected at the threshold, or pushed out of lane 63 later):
  // the smallest key and its site, and the smallest key at any OTHER site — enough to answer, at the end, "is
  // there an unlisted candidate within the band of the last entry that does not sit at that entry's site?"
  uint64_t m1, m2;
  uint32_t s1;
  NEAR_ROW_PROF_FIELDS  // (a measuring build: the row's anatomy — NR_T0 / NR_ADD / NR_CNT / NR_SEG below book into these)
};
__device__ __forceinline__ uint64_t wave_shr1_u64(uint64_t v) {  // lane i <- lane i - 1, lane 0 <- 0
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, 0x138, 0xF, 0xF, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), 0x138, 0xF, 0xF, false);
  return ((uint64_t)hi << 32) | lo;
}
// Upper end of the window behind the threshold.  The row's last entry (the K-th nearest, K <= 63) never lies
// beyond lane 63, and lane 63 only ever moves inwards, so a candidate that finishes within the band
// (a <= a_last (1 + 4 band) + 1e-300) of the last entry is, whenever it is looked at, fewer than 4 band 2^53 ulps
// above the threshold's `a` (or below 1e-290): in integer terms — keys are the bit patterns of positive doubles —
// below tau + ulps.  `ulps` = 2^20 / 2^25 (twice what the band needs; the key truncation is 2^13 / 2^18).
// Location-less thresholds, and a row that is not full yet, have no window.
__device__ __forceinline__ uint64_t near_window(uint64_t tau, uint32_t SB, uint64_t ulps) {
  if (tau >= ((PM_KEY_NOLOC >> SB) << SB)) return tau;
  const uint64_t hi = tau + ulps, floor_bits = 0x03B8F2B061AEA073ull;  // bits of 1e-290, rounded up
  return (hi > floor_bits ? hi : floor_bits) | ((1ull << SB) - 1ull);
}
__device__ __forceinline__ void near_track(NearRow& r, uint64_t k, uint32_t site, bool cand) {
  uint64_t chg = __ballot(cand && (k < r.m1 || (site != r.s1 && k < r.m2)));
  NR_T0;
  NR_CNT(r.p_trk_n, (uint32_t)__popcll(chg));
  while (chg) {  // (a city of co-located workers: the first one sets m1 / s1, the others change nothing)
    const uint32_t l = (uint32_t)__builtin_ctzll(chg);
    chg &= chg - 1ull;
    const uint64_t kk = readlane_u64(k, l);
    const uint32_t ss = (uint32_t)__builtin_amdgcn_readlane((int)site, (int)l);
    if (kk < r.m1) {
      if (ss != r.s1) r.m2 = r.m1;
      r.m1 = kk;
      r.s1 = ss;
    } else if (ss != r.s1 && kk < r.m2) {
      r.m2 = kk;
    }
  }
  NR_ADD(r.p_trk_t);
}
// the candidates of one 64-slot stride (k = ~0 where the lane has none; site = the candidate's site) against the row
template <typename SP>
__device__ __forceinline__ void near_row_offer(NearRow& r, uint64_t k, uint32_t site, SP cc_site, uint32_t SB, uint64_t ulps) {
  NR_CNT(r.p_strides, 1u);
  if (!__ballot(k < r.tau_hi)) return;
  uint64_t m = __ballot(k < r.tau);
  if (m) {
    const uint64_t old = r.key;
    NR_T0;
    NR_CNT(r.p_ins_n, (uint32_t)__popcll(m));
    do {
      const uint32_t l = (uint32_t)__builtin_ctzll(m);
      m &= m - 1ull;
      const uint64_t kk = readlane_u64(k, l);  // wave-uniform
      const uint64_t prev = wave_shr1_u64(r.key);
      const bool gt = r.key > kk, pgt = prev > kk;  // keys are distinct (the slot is in the low bits)
      r.key = gt ? (pgt ? prev : kk) : r.key;     // (a key that no longer beats lane 63 changes nothing)
    } while (m);
    NR_ADD(r.p_ins_t);
    r.tau = readlane_u64(r.key, 63u);
    r.tau_hi = near_window(r.tau, SB, ulps);
    const bool ev = old > r.tau && old < r.tau_hi;  // pushed out of the row, still near
    if (__ballot(ev)) {
      NR_CNT(r.p_ev_n, 1u);
      const uint32_t es = ev ? cc_site[(uint32_t)(old & ((1ull << SB) - 1ull))] : 0u;
      near_track(r, old, es, ev);
    }
  }
  const bool nm = k > r.tau && k < r.tau_hi;  // not (or no longer) in the row, but near
  if (__ballot(nm)) near_track(r, k, site, nm);
}

// ---- several strides at once (the streaming carve's rows, round 5).  The insertion above is a serial loop — one
// readlane, one shift, two compares per entrant, each waiting for the one before: a lone wave gets through an
// instruction every 8 cycles — and while a row fills up and settles nearly every candidate is an entrant (64 (1 + ln(n / 64))
// of n: 227 of 740, 45 % of a row's time at 10 k workers, profiles/r05_row_anatomy_10k.txt).  Here S strides are sorted
// across the lanes by S independent bitonic networks (21 compare-exchanges each: their instructions interleave, nothing
// waits), the lower halves are merged pairwise (a list reversed against the other: the 64 smaller ones are the lane-wise
// minima, a bitonic sequence six exchanges sort) and the result with the row.  Same row — the 64 smallest keys in order
// are what they are — and the same tracker semantics: what is unlisted BEHIND the call and within the window of the
// threshold as it stands then is tracked (a subset of what the insertion tracks, a superset of what the end needs:
// the threshold only moves inwards).
template <uint32_t J>
__device__ __forceinline__ uint32_t lane_xor_u32(uint32_t v, uint32_t addr32) {  // lane i <- lane i ^ J
  if constexpr (J == 1u) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);  // quad_perm [1, 0, 3, 2]
  } else if constexpr (J == 2u) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true);  // quad_perm [2, 3, 0, 1]
  } else if constexpr (J == 4u) {
    const int a = __builtin_amdgcn_update_dpp((int)v, (int)v, 0x104, 0xF, 0x5, false);  // row_shl:4 into banks 0, 2: i <- i + 4
    return (uint32_t)__builtin_amdgcn_update_dpp(a, (int)v, 0x114, 0xF, 0xA, false);    // row_shr:4 into banks 1, 3: i <- i - 4
  } else if constexpr (J == 8u) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xF, 0xF, true);  // row_ror:8
  } else if constexpr (J == 16u) {
    return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x401F);  // bit mode: xor 16 within 32 lanes
  } else {
    return (uint32_t)__builtin_amdgcn_ds_bpermute((int)addr32, (int)v);
  }
}
#ifndef NET_SERIAL_MAX
#define NET_SERIAL_MAX 16u  // entrants of four strides up to which they are inserted one by one (near_row_bulk4; 3 / 6 / 12 / 16 / 24 / 40 measured)
#endif
#define NET_PACK_KEYS 128u  // keys of LDS a wave packs entrants into (near_row_bulk4: one list or two)
struct LaneNet {  // what the networks need of the lane: computed once per wave
  uint32_t lane, a_x32, a_rev;  // byte addresses of lane ^ 32 and of 63 - lane for ds_bpermute
  uint64_t* pack;               // NET_PACK_KEYS keys of LDS of the wave's own (entrants of several strides packed into one list or two)
};
__device__ __forceinline__ LaneNet lane_net(uint32_t lane, uint64_t* pack) {
  return LaneNet{lane, (lane ^ 32u) << 2, (63u - lane) << 2, pack};
}
// one compare-exchange of a network on S lists: partner lane ^ J; a lane keeps the smaller of the two where bit J and
// bit KK of its number agree (KK = 64: everywhere ascending — the last pass of a sort, and every pass of a merge)
template <uint32_t S, uint32_t KK, uint32_t J>
__device__ __forceinline__ void net_exchange(uint64_t (&w)[S], const LaneNet& ln) {
  const bool want_min = ((ln.lane & J) == 0u) == ((ln.lane & KK) == 0u);
  // (list by list in three rounds, not exchange by exchange: the lists' instructions alternate and none waits for the one before)
  uint64_t pv[S];
  bool keep[S];
#pragma unroll
  for (uint32_t s = 0; s < S; ++s)
    pv[s] = ((uint64_t)lane_xor_u32<J>((uint32_t)(w[s] >> 32), ln.a_x32) << 32) | lane_xor_u32<J>((uint32_t)w[s], ln.a_x32);
#pragma unroll
  for (uint32_t s = 0; s < S; ++s) keep[s] = (w[s] < pv[s]) == want_min;
#pragma unroll
  for (uint32_t s = 0; s < S; ++s) w[s] = keep[s] ? w[s] : pv[s];
}
template <uint32_t S, uint32_t KK>
__device__ __forceinline__ void net_merge_pass(uint64_t (&w)[S], const LaneNet& ln) {  // a bitonic sequence of KK -> sorted
  if constexpr (KK >= 64u) net_exchange<S, KK, 32u>(w, ln);
  if constexpr (KK >= 32u) net_exchange<S, KK, 16u>(w, ln);
  if constexpr (KK >= 16u) net_exchange<S, KK, 8u>(w, ln);
  if constexpr (KK >= 8u) net_exchange<S, KK, 4u>(w, ln);
  if constexpr (KK >= 4u) net_exchange<S, KK, 2u>(w, ln);
  net_exchange<S, KK, 1u>(w, ln);
}
template <uint32_t S>
__device__ __forceinline__ void net_sort(uint64_t (&w)[S], const LaneNet& ln) {  // every list ascending over the lanes
  net_merge_pass<S, 2u>(w, ln);
  net_merge_pass<S, 4u>(w, ln);
  net_merge_pass<S, 8u>(w, ln);
  net_merge_pass<S, 16u>(w, ln);
  net_merge_pass<S, 32u>(w, ln);
  net_merge_pass<S, 64u>(w, ln);
}
// a, b ascending -> the 64 smallest of both, ascending
__device__ __forceinline__ uint64_t net_lower(uint64_t a, uint64_t b, const LaneNet& ln) {
  const uint64_t rb = ((uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute((int)ln.a_rev, (int)(uint32_t)(b >> 32)) << 32) |
                      (uint32_t)__builtin_amdgcn_ds_bpermute((int)ln.a_rev, (int)(uint32_t)b);
  uint64_t m[1] = {a < rb ? a : rb};
  net_merge_pass<1u, 64u>(m, ln);
  return m[0];
}
__device__ __forceinline__ NearRow near_row_bulk4_body(NearRow r, uint64_t k0, uint64_t k1, uint64_t k2, uint64_t k3, uint32_t s0, uint32_t s1,
                                                     uint32_t s2, uint32_t s3, const uint32_t* cc_site_, uint32_t SB, uint64_t ulps,
                                                     uint32_t lane, uint64_t* pack) {
  constexpr uint32_t S = 4u;
  const LaneNet ln = lane_net(lane, pack);
  const auto cc_site = G(cc_site_);
  const uint64_t k[S] = {k0, k1, k2, k3};
  const uint32_t site[S] = {s0, s1, s2, s3};
  NR_CNT(r.p_strides, S);
  NR_SEG0(sg_t);
  uint64_t ent[S];
  uint32_t n_ent = 0u;
#pragma unroll
  for (uint32_t s = 0; s < S; ++s) {
    ent[s] = __ballot(k[s] < r.tau);
    n_ent += (uint32_t)__popcll(ent[s]);
  }
  if (n_ent) {
    NR_T0;
    NR_CNT(r.p_ins_n, n_ent);
    uint64_t low;  // the (at most 64) smallest of the entrants, ascending
    const uint64_t old0 = r.key;
    if (n_ent <= NET_SERIAL_MAX) {
      // A handful of entrants (the usual case once a row has seen a thousand candidates): inserted one by one — a readlane, a
      // shift by one lane and two compares each — under the bulk path's bookkeeping: ONE look at the threshold in front of four
      // strides, one update of it behind them, one look at what was pushed out, where the stride-by-stride insertion
      // (near_row_offer) pays each of them per stride (round 6, tools/row_bench.py: a tenth of a row's time was the look at
      // what a stride pushed out)
#pragma unroll
      for (uint32_t s = 0; s < S; ++s) {
        uint64_t m = ent[s];
        while (m) {
          const uint32_t l = (uint32_t)__builtin_ctzll(m);
          m &= m - 1ull;
          const uint64_t kk = readlane_u64(k[s], l);  // wave-uniform
          const uint64_t prev = wave_shr1_u64(r.key);
          const bool gt = r.key > kk, pgt = prev > kk;  // keys are distinct (the slot is in the low bits)
          r.key = gt ? (pgt ? prev : kk) : r.key;     // (a key that no longer beats lane 63 changes nothing)
        }
      }
      low = 0ull;
    } else if (n_ent <= NET_PACK_KEYS) {
      // Once the row is full a stride has few entrants (64 ln(n' / n) of the candidates n .. n'): packed through LDS into
      // one list, or two, they cost that many networks instead of four
      uint32_t base = 0u;
#pragma unroll
      for (uint32_t s = 0; s < S; ++s) {
        if (k[s] < r.tau) ln.pack[base + __builtin_amdgcn_mbcnt_hi((uint32_t)(ent[s] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ent[s], 0u))] = k[s];
        base += (uint32_t)__popcll(ent[s]);
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // (the lanes read what other lanes of the wave packed)
      NR_SEG(r, 0, sg_t);
      if (n_ent <= 64u) {
        uint64_t one[1] = {ln.lane < n_ent ? ln.pack[ln.lane] : ~0ull};
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        net_sort<1u>(one, ln);
        low = one[0];
      } else {
        uint64_t two[2] = {ln.pack[ln.lane], 64u + ln.lane < n_ent ? ln.pack[64u + ln.lane] : ~0ull};
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        net_sort<2u>(two, ln);
        low = net_lower(two[0], two[1], ln);
      }
    } else {
      uint64_t w[S];
#pragma unroll
      for (uint32_t s = 0; s < S; ++s) w[s] = k[s];
      net_sort<S>(w, ln);
      // (0, 1) and (2, 3) side by side, then their results
      const uint64_t r1 = ((uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute((int)ln.a_rev, (int)(uint32_t)(w[1] >> 32)) << 32) |
                          (uint32_t)__builtin_amdgcn_ds_bpermute((int)ln.a_rev, (int)(uint32_t)w[1]);
      const uint64_t r3 = ((uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute((int)ln.a_rev, (int)(uint32_t)(w[3] >> 32)) << 32) |
                          (uint32_t)__builtin_amdgcn_ds_bpermute((int)ln.a_rev, (int)(uint32_t)w[3]);
      uint64_t m[2] = {w[0] < r1 ? w[0] : r1, w[2] < r3 ? w[2] : r3};
      net_merge_pass<2u, 64u>(m, ln);
      low = net_lower(m[0], m[1], ln);
    }
    const uint64_t old = old0;
    if (n_ent > NET_SERIAL_MAX) r.key = net_lower(old, low, ln);
    NR_ADD(r.p_ins_t);
    NR_SEG(r, 1, sg_t);
    r.tau = readlane_u64(r.key, 63u);
    r.tau_hi = near_window(r.tau, SB, ulps);
    const bool ev = old > r.tau && old < r.tau_hi;  // pushed out of the row, still near
    if (__ballot(ev)) {
      NR_CNT(r.p_ev_n, 1u);
      const uint32_t es = ev ? cc_site[(uint32_t)(old & ((1ull << SB) - 1ull))] : 0u;
      near_track(r, old, es, ev);
    }
    NR_SEG(r, 2, sg_t);
  }
#pragma unroll
  for (uint32_t s = 0; s < S; ++s) {
    const bool nm = k[s] > r.tau && k[s] < r.tau_hi;  // not (or no longer) in the row, but near
    if (__ballot(nm)) near_track(r, k[s], site[s], nm);
  }
  NR_SEG(r, 3, sg_t);
  return r;
}
// (the walk's copy, out of line: the networks are two thousand instructions and the walk offers candidates in six places.  A
// call waits for every load in flight, so the bitmap sweep — whose next gathers are in flight while a batch is evaluated —
// has the networks inline, in its one place)
__device__ __noinline__ NearRow near_row_bulk4(NearRow r, uint64_t k0, uint64_t k1, uint64_t k2, uint64_t k3, uint32_t s0, uint32_t s1,
                                               uint32_t s2, uint32_t s3, const uint32_t* cc_site_, uint32_t SB, uint64_t ulps,
                                               uint32_t lane, uint64_t* pack) {
  return near_row_bulk4_body(r, k0, k1, k2, k3, s0, s1, s2, s3, cc_site_, SB, ulps, lane, pack);
}
template <uint32_t S, bool INLINE = false>
__device__ __forceinline__ void near_row_offer_bulk(NearRow& r, const uint64_t (&k)[S], const uint32_t (&site)[S], const uint32_t* cc_site,
                                                    uint32_t SB, uint64_t ulps, const LaneNet& ln) {
  static_assert(S == 4u, "four strides a call");
  uint64_t any_hi = 0ull;
#pragma unroll
  for (uint32_t s = 0; s < S; ++s) any_hi |= __ballot(k[s] < r.tau_hi);
  if (!any_hi) {
    NR_CNT(r.p_strides, S);
    return;
  }
  NR_SEG0(call_t);
  if constexpr (INLINE) r = near_row_bulk4_body(r, k[0], k[1], k[2], k[3], site[0], site[1], site[2], site[3], cc_site, SB, ulps, ln.lane, ln.pack);
  else r = near_row_bulk4(r, k[0], k[1], k[2], k[3], site[0], site[1], site[2], site[3], cc_site, SB, ulps, ln.lane, ln.pack);
  NR_SEG(r, 5, call_t);
  NR_CNT(r.p_seg[4], 1u);
}

// The candidate columns of a tile of PROP_TILE slots, staged in LDS and shared by the four waves (= four seeds) of a
// workgroup: the sweep of a seed is then a chain of LDS reads (~64 cycles) instead of L2 round trips (~500), the
// next tile's global loads are in flight while the current one is consumed (two buffers), and every candidate
// row is fetched once per workgroup instead of once per seed.
#ifndef PROP_TILE
#define PROP_TILE 512u  // (256 / 512 / 1024 measure the same at 10 k and 100 k candidates)
#endif
#define PROP_TILE_PER_THREAD (PROP_TILE / 256u)
#define PROP_TILE_WORDS (PROP_TILE / 64u)
struct TileBuf {
  double x[PROP_TILE], y[PROP_TILE], z[PROP_TILE];  // unit vectors
  uint32_t site[PROP_TILE];
  uint64_t alive[PROP_TILE_WORDS], loc[PROP_TILE_WORDS];
};
struct TileRegs {  // one thread's share of a tile on its way from HBM/L2 to LDS: slots tid, tid + 256, ...
  double x[PROP_TILE_PER_THREAD], y[PROP_TILE_PER_THREAD], z[PROP_TILE_PER_THREAD];
  uint32_t site[PROP_TILE_PER_THREAD];
  uint64_t bm;
};
template <typename BP>
__device__ __forceinline__ void tile_fetch(const CarveArgs& p, BP alive, BP loc, uint32_t lw, uint32_t n_list,
                                           uint32_t tile, uint32_t tid, TileRegs& r) {
#pragma unroll
  for (uint32_t h = 0; h < PROP_TILE_PER_THREAD; ++h) {
    const uint32_t t = tile * PROP_TILE + h * 256u + tid;
    const uint32_t tc = t < n_list ? t : n_list - 1u;  // unconditional loads; the bitmaps are zero beyond the list
    r.x[h] = G(p.cc_ux)[tc];
    r.y[h] = G(p.cc_uy)[tc];
    r.z[h] = G(p.cc_uz)[tc];
    r.site[h] = G(p.cc_site)[tc];
  }
  const uint32_t j = tile * PROP_TILE_WORDS + (tid % PROP_TILE_WORDS);
  r.bm = (tid < 2u * PROP_TILE_WORDS && j < lw) ? (tid < PROP_TILE_WORDS ? alive[j] : loc[j]) : 0ull;
}
__device__ __forceinline__ void tile_store(TileBuf& tb, uint32_t tid, const TileRegs& r) {
#pragma unroll
  for (uint32_t h = 0; h < PROP_TILE_PER_THREAD; ++h) {
    const uint32_t o = h * 256u + tid;
    tb.x[o] = r.x[h];
    tb.y[o] = r.y[h];
    tb.z[o] = r.z[h];
    tb.site[o] = r.site[h];
  }
  if (tid < PROP_TILE_WORDS) tb.alive[tid] = r.bm;
  else if (tid < 2u * PROP_TILE_WORDS) tb.loc[tid - PROP_TILE_WORDS] = r.bm;
}
// keys of one seed against a staged tile: lane l owns the slots t = l (mod 64), as everywhere in this kernel.
// Straight-line code: every LDS read of four strides is issued up front, the chord key is computed for every lane,
// and a slot that does not count (dead, the seed itself, same shared site) becomes the key ~0, which never beats
// the row's threshold — a `continue` per condition would put an LDS round trip and a branch between each of them.
__device__ __forceinline__ void tile_keys(const CarveArgs& p, const TileBuf& tb, uint32_t tile, uint32_t lane, uint32_t s,
                                          bool shared, uint32_t ssite, const SeedGeo& sg, uint32_t SB, uint64_t ulps,
                                          NearRow& q, uint32_t& n_mine) {
  const bool form = UNI(p.mode) != CARVE_MODE_MERGE;
#pragma unroll 1
  for (uint32_t h = 0; h < PROP_TILE / 256u; ++h) {
    double x[4], y[4], z[4];
    uint32_t si[4];
    uint64_t aw[4], lwd[4];
#pragma unroll
    for (uint32_t v = 0; v < 4u; ++v) {
      const uint32_t u = h * 4u + v, o = u * 64u + lane;
      aw[v] = tb.alive[u];
      lwd[v] = tb.loc[u];
      x[v] = tb.x[o];
      y[v] = tb.y[o];
      z[v] = tb.z[o];
      si[v] = tb.site[o];
    }
#pragma unroll
    for (uint32_t v = 0; v < 4u; ++v) {
      const uint32_t u = h * 4u + v, t = tile * PROP_TILE + u * 64u + lane;
      const bool located = (lwd[v] >> lane) & 1ull;
      // FORM: a located candidate in front of the seed is dead by the time it is a seed (a live located slot in front
      // of it would be the seed instead, mod.rs:526-530) and would only fill the row — wherever it sits.  Location-less
      // ones in front stay in: they sort behind every located one and may well be alive at the seed's turn.  MERGE
      // keeps the rule for the seed's own (shared) site only, where candidates are at distance 0 (key = their slot)
      // and the ones behind the seed head its row in slot order: a merge batch can be refused with its seed still in
      // the list.
      const bool counts = ((aw[v] >> lane) & 1ull) && t != s && !(located && t < s && (form || (shared && si[v] == ssite)));
      const double dx = x[v] - sg.ux, dy = y[v] - sg.uy, dz = z[v] - sg.uz;
      double a = 0.25 * fma(dx, dx, fma(dy, dy, dz * dz));
      // (see prox_a: the sine form below ~14.5 km.  A candidate at the seed's own site — identical coordinates — has the
      // Haversine term 0 in either form, exactly: sin(0) = 0; a city of co-located workers would otherwise send
      // nearly every stride of its seeds' sweeps through the sine polynomials)
      const bool same_site = located && si[v] == ssite;
      const bool near = counts && located && a < PM_A_CHORD_MIN && !same_site;
      a = same_site ? 0.0 : a;
      if (__ballot(near)) {
        if (near) a = hav_a(sg.lat, sg.lon, sg.cos, G(p.cc_lat)[t], G(p.cc_lon)[t], G(p.cc_cos)[t]);
      }
      const uint64_t kl = pack_key(located ? (uint64_t)__double_as_longlong(a) : PM_KEY_NOLOC, t, SB);
      near_row_offer(q, counts ? kl : ~0ull, si[v], G(p.cc_site), SB, ulps);
      n_mine += counts ? 1u : 0u;
    }
  }
}

// ---- Proposals from the spatial index (cell_*_kernel below).  The whole-list sweep above evaluates every candidate
// for every seed: 13,500 keys to pick 63 at 1M x 100k.  When the list is long and most of the indexed positions are
// still candidates, a seed instead walks the grid cells around its own cell, ring by ring (Chebyshev distance r in
// cell coordinates), and stops in front of the first ring that cannot hold anything of interest: every point of a
// cell at distance r is at least (r - 1) h away in one coordinate, hence in chord length, and what matters to a row
// is only what lies below its window (near_window: the threshold plus the certificate band).  Inside a ring each lane
// owns one run of cells along x — a contiguous range of the cell-sorted entries — and skips it when the box of the
// run is already out of reach of the seed's exact coordinates.  The row, its flags and the near-miss tracker come
// out bit for bit as the whole-list sweep produces them: both are functions of the SET of candidates below the final
// window, and the walk sees all of those.
__device__ __forceinline__ uint32_t cell_g_for(uint32_t n) {
  return n >= PM_CELL_BIG_N ? PM_CELL_G_MAX : n >= PM_CELL_MIN_N ? PM_CELL_G_MAX / 2u : 0u;
}
__device__ __forceinline__ uint32_t cell_coord(double v, uint32_t g) {  // v in [-1, 1]
  const double t = fmax((v + 1.0) * (double)(g >> 1), 0.0);  // (g / 2 is a power of two: the product is exact)
  const uint32_t c = (uint32_t)t;
  return c < g ? c : g - 1u;
}
// Lower bound of the key of anything at least `gx, gy, gz` away from the seed along the axes.  The gaps come from cell
// boundaries, which hold for the stored coordinates up to one rounding of (v + 1); 1e-9 (6 mm) per axis and 1e-6 of
// the result are far beyond that and beyond the difference between the chord form and the sine form of the key
// (relative 2^-31 at worst, the certificate band), and nothing next to a cell of 200 km.
__device__ __forceinline__ uint64_t cell_bound_key(double gx, double gy, double gz, uint32_t SB) {
  gx = fmax(gx - 1e-9, 0.0);
  gy = fmax(gy - 1e-9, 0.0);
  gz = fmax(gz - 1e-9, 0.0);
  const double a = 0.25 * (gx * gx + gy * gy + gz * gz) * (1.0 - 1e-6);
  return pack_key((uint64_t)__double_as_longlong(a), 0u, SB);
}
// one candidate per lane: its key (the key arithmetic of tile_keys, operands in registers; ~0 where the lane has none)
__device__ __forceinline__ uint64_t candidate_key(const CarveArgs& p, const SeedGeo& sg, uint32_t ssite, double x, double y, double z,
                                                  uint32_t si, uint32_t t, bool located, bool counts, uint32_t SB, NearRow& q) {
  const double dx = x - sg.ux, dy = y - sg.uy, dz = z - sg.uz;
  double a = 0.25 * fma(dx, dx, fma(dy, dy, dz * dz));
  const bool same_site = located && si == ssite;
  const bool near = counts && located && a < PM_A_CHORD_MIN && !same_site;
  a = same_site ? 0.0 : a;
  if (__ballot(near)) {
    NR_T0;
    NR_CNT(q.p_hav_n, 1u);
    if (near) a = hav_a(sg.lat, sg.lon, sg.cos, G(p.cc_lat)[t], G(p.cc_lon)[t], G(p.cc_cos)[t]);
    NR_ADD(q.p_hav_t);
  }
  const uint64_t kl = pack_key(located ? (uint64_t)__double_as_longlong(a) : PM_KEY_NOLOC, t, SB);
  return counts ? kl : ~0ull;
}
// ... against the row
__device__ __forceinline__ void offer_candidate(const CarveArgs& p, const SeedGeo& sg, uint32_t ssite, double x, double y,
                                                double z, uint32_t si, uint32_t t, bool located, bool counts, uint32_t SB,
                                                uint64_t ulps, NearRow& q, uint32_t& n_mine) {
  const uint64_t kl = candidate_key(p, sg, ssite, x, y, z, si, t, located, counts, SB, q);
  near_row_offer(q, kl, si, G(p.cc_site), SB, ulps);
  n_mine += counts ? 1u : 0u;
}
// The entries of up to 64 runs — lane l holds run l: first entry b, length len (0 = none) — against the row.  The runs
// are short (a few cells of a few dozen positions), so they are laid end to end and cut into strides of 64: lane l of a
// stride finds its run by bisecting the running totals held across the lanes (6 ds_bpermute).  Most entries are not
// candidates of THIS list (another configuration's, or gone), and the walk of one seed is a chain of memory round trips,
// not a stream: so the first pass reads only the entries' slot words, four strides per trip, and packs the candidates
// it finds into the wave's LDS buffer; their coordinates are fetched in a second pass, over full strides.
#define CELL_BUF 768u  // candidates a wave collects before it drains them (2 words each)
#ifndef STREAM_BULK_UPTO
#define STREAM_BULK_UPTO 0x40000000u  // candidates of a row that go four strides at a time (near_row_offer_bulk: networks for many entrants,
                                      // one by one for a few): all of them since round 6 — it was the first 1,024, the rest stride by stride
#endif
struct BulkCtx {  // the streaming carve's rows: how many candidates the row has seen, the lane's network constants
  uint32_t seen;
  LaneNet ln;
  BULK_REC_FIELDS  // (a measuring build: when the sweep's first pass was packed, when the first batch's keys were there)
};
template <bool STREAM = false>
__device__ __forceinline__ void cell_drain(const CarveArgs& p, uint32_t* wl, uint32_t& nb, uint32_t lane, uint32_t s, bool shared,
                                           uint32_t ssite, const SeedGeo& sg, uint32_t SB, uint64_t ulps, NearRow& q,
                                           uint32_t& n_mine, BulkCtx* bulk = nullptr) {
  const auto cs_site = G((const uint32_t*)p.cs_site);
  const auto cs_x = G((const double*)p.cs_ux);
  const auto cs_y = G((const double*)p.cs_uy);
  const auto cs_z = G((const double*)p.cs_uz);
  const double* const pack = p.cs_pack;  // (streaming carve: one 32-byte record per entry instead of four columns)
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // (the lanes read what other lanes of the wave packed)
  constexpr uint32_t NV = STREAM ? 4u : 2u;  // strides per trip
  for (uint32_t k0 = 0; k0 < nb; k0 += NV * 64u) {
    uint32_t t[NV], si[NV];
    double x[NV], y[NV], z[NV];
    bool in[NV];
#pragma unroll
    for (uint32_t v = 0; v < NV; ++v) {
      const uint32_t k = k0 + v * 64u + lane;
      in[v] = k < nb;
      const uint32_t kc = in[v] ? k : 0u;
      const uint32_t ic = wl[kc];
      t[v] = wl[CELL_BUF + kc];
      if (STREAM) {
        const pm_d4 r = pack_load(pack, ic);
        x[v] = r.x;
        y[v] = r.y;
        z[v] = r.z;
        si[v] = pack_site(r);
      } else {
        x[v] = cs_x[ic];
        y[v] = cs_y[ic];
        z[v] = cs_z[ic];
        si[v] = cs_site[ic];
      }
    }
    if constexpr (STREAM) {  // (the keys first, then the row: see stream_drain)
      uint64_t kk[NV];
#pragma unroll
      for (uint32_t v = 0; v < NV; ++v) {
        const bool counts = in[v] && t[v] != s && !(shared && si[v] == ssite && t[v] < s);
        kk[v] = candidate_key(p, sg, ssite, x[v], y[v], z[v], si[v], in[v] ? t[v] : 0u, true, counts, SB, q);
        n_mine += counts ? 1u : 0u;
      }
      const uint32_t n_in = nb - k0 < NV * 64u ? nb - k0 : NV * 64u;
      if (bulk && UNI(bulk->seen) < STREAM_BULK_UPTO) {
        near_row_offer_bulk<NV>(q, kk, si, p.cc_site, SB, ulps, bulk->ln);
      } else {
#pragma unroll
        for (uint32_t v = 0; v < NV; ++v) {
          if (v * 64u >= n_in) continue;
          near_row_offer(q, kk[v], si[v], G(p.cc_site), SB, ulps);
        }
      }
      if (bulk) bulk->seen += n_in;
    } else {
#pragma unroll
      for (uint32_t v = 0; v < NV; ++v) {
        if (!__ballot(in[v])) continue;
        // (every indexed position has a location; the slots in front of the seed at its own shared site: see tile_keys.
        // The walk leaves out no other candidate in front of the seed, though none of them can be alive at its turn:
        // a walk stops where its row's window closes, and with the few hundred candidates of the look-ahead window
        // gone from around a late seed the rings go further out and give up twice as often — measured at 1M x 100k,
        // 6.5 - 7.0 ms a match with this rule as it stands against 6.9 - 7.4 with the general one, DESIGN.md 4.2)
        const bool counts = in[v] && t[v] != s && !(shared && si[v] == ssite && t[v] < s);
        offer_candidate(p, sg, ssite, x[v], y[v], z[v], si[v], in[v] ? t[v] : 0u, true, counts, SB, ulps, q, n_mine);
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  nb = 0;
}
template <bool STREAM = false>
__device__ __forceinline__ void cell_offer_runs(const CarveArgs& p, uint32_t* wl, uint32_t b, uint32_t len, uint32_t lane, uint32_t s,
                                                bool shared, uint32_t ssite, const SeedGeo& sg, uint32_t SB, uint64_t ulps,
                                                NearRow& q, uint32_t& n_mine,
                                                const uint32_t* cfg32 = nullptr, BulkCtx* bulk = nullptr) {
  const uint32_t incl = wave_incl_scan_u32(len);
  const uint32_t excl = incl - len;
  const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
  const auto cs_slot = G((const uint32_t*)p.cs_slot);
  uint32_t nb = 0;
  for (uint32_t f0 = 0; f0 < total; f0 += 256u) {
    uint32_t t[4], ic[4];
    bool in[4];
#pragma unroll
    for (uint32_t v = 0; v < 4u; ++v) {
      const uint32_t f = f0 + v * 64u + lane;
      in[v] = f < total;
      uint32_t j = 0;
#pragma unroll
      for (uint32_t step = 32u; step; step >>= 1) {
        const uint32_t pv = __shfl(incl, (int)(j + step - 1u), 64);
        j += pv <= f ? step : 0u;
      }
      j = j > 63u ? 63u : j;
      const uint32_t idx = __shfl(b, (int)j, 64) + (f - __shfl(excl, (int)j, 64));
      ic[v] = in[v] ? idx : 0u;
      t[v] = cs_slot[ic[v]];
    }
    // (streaming carve: an entry's slot is its position for the whole carve; whether it is a candidate of the
    // configuration being carved, and still free, is one bit of the validator's published bitmap)
    uint32_t cw[4] = {~0u, ~0u, ~0u, ~0u};
    if (STREAM) {  // free (the validator's published bitmap, a little behind) and compatible with the configuration
      const auto freeg = G((const uint32_t*)p.bits_scratch);
      const auto cfgb = G(cfg32);
#pragma unroll
      for (uint32_t v = 0; v < 4u; ++v) {
        const uint32_t wi = (in[v] ? t[v] : 0u) >> 5;
        cw[v] = __hip_atomic_load(&freeg[wi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & cfgb[wi];
      }
    }
#pragma unroll
    for (uint32_t v = 0; v < 4u; ++v) {
      const bool cand = in[v] && t[v] != 0xFFFFFFFFu && (!STREAM || ((cw[v] >> (t[v] & 31u)) & 1u) != 0u);
      const uint64_t m = __ballot(cand);
      if (cand) {
        const uint32_t at = nb + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        wl[at] = ic[v];
        wl[CELL_BUF + at] = t[v];
      }
      nb += (uint32_t)__popcll(m);
    }
    if (nb > CELL_BUF - 256u) cell_drain<STREAM>(p, wl, nb, lane, s, shared, ssite, sg, SB, ulps, q, n_mine, bulk);
  }
  if (nb) cell_drain<STREAM>(p, wl, nb, lane, s, shared, ssite, sg, SB, ulps, q, n_mine, bulk);
}
// run qi of ring r around cell (cx, cy, cz): where its entries begin and end in cell_start, and the lower bound of
// the keys in its box.  false = the run lies outside the grid.
__device__ __forceinline__ bool cell_run(uint32_t r, uint32_t qi, int cx, int cy, int cz, uint32_t g, double h, const SeedGeo& sg,
                                         uint32_t SB, uint32_t* lin_b, uint32_t* lin_e, uint64_t* lbk) {
  const int G1 = (int)g;
  int dy = 0, dz = 0, x0 = cx, x1 = cx;
  if (r > 0u) {
    const uint32_t side = 2u * r, n_full = 8u * r, inner = 2u * r - 1u;
    if (qi < n_full) {  // the rim of the (2r + 1)^2 square of (dy, dz): whole runs -r .. r along x
      const uint32_t sd = qi / side, t = qi - sd * side;
      const int R = (int)r, T = (int)t;
      dy = sd == 0u ? -R + T : sd == 1u ? R : sd == 2u ? R - T : -R;
      dz = sd == 0u ? -R : sd == 1u ? -R + T : sd == 2u ? R : R - T;
      x0 = cx - R;
      x1 = cx + R;
    } else {  // the inside of the square: the two end cells x = -r and x = r
      const uint32_t m = (qi - n_full) >> 1;
      dy = (int)(m % inner) - (int)(r - 1u);
      dz = (int)(m / inner) - (int)(r - 1u);
      x0 = x1 = ((qi - n_full) & 1u) ? cx + (int)r : cx - (int)r;
    }
  }
  const int y = cy + dy, z = cz + dz;
  const bool ok = y >= 0 && y < G1 && z >= 0 && z < G1 && x1 >= 0 && x0 < G1;
  x0 = x0 < 0 ? 0 : x0;
  x1 = x1 >= G1 ? G1 - 1 : x1;
  // the box of the run against the seed's own coordinates
  const double xlo = (double)x0 * h - 1.0, xhi = (double)(x1 + 1) * h - 1.0;
  const double ylo = (double)y * h - 1.0, yhi = ylo + h, zlo = (double)z * h - 1.0, zhi = zlo + h;
  const double gx = fmax(fmax(xlo - sg.ux, sg.ux - xhi), 0.0), gy = fmax(fmax(ylo - sg.uy, sg.uy - yhi), 0.0),
               gz = fmax(fmax(zlo - sg.uz, sg.uz - zhi), 0.0);
  *lbk = cell_bound_key(gx, gy, gz, SB);
  const uint32_t row = ok ? ((uint32_t)z * g + (uint32_t)y) * g : 0u;
  *lin_b = row + (uint32_t)(ok ? x0 : 0);
  *lin_e = row + (uint32_t)(ok ? x1 : 0) + 1u;
  return ok;
}
__device__ __forceinline__ uint32_t ring_runs(uint32_t r) { return r ? 8u * r + 2u * (2u * r - 1u) * (2u * r - 1u) : 1u; }
// The walk.  Returns the ring in front of which it stopped (>= 2), or 0 = the rings ran out before the row's window
// closed (a seed far from everything else, or fewer located candidates than a row holds): the caller starts over on
// the whole list.
template <bool STREAM = false>
__device__ __forceinline__ uint32_t cell_walk(const CarveArgs& p, uint32_t* wl, uint32_t g, uint32_t r_max, uint32_t lane, uint32_t s,
                                          bool shared, uint32_t ssite, const SeedGeo& sg, uint32_t SB, uint64_t ulps, NearRow& q,
                                          uint32_t& n_mine,
                                          const uint32_t* cfg32 = nullptr, BulkCtx* bulk = nullptr) {
  const double h = 2.0 / (double)g;
  const int cx = (int)cell_coord(sg.ux, g), cy = (int)cell_coord(sg.uy, g), cz = (int)cell_coord(sg.uz, g);
  const auto cstart = G((const uint32_t*)p.cell_start);
  {
    // rings 0, 1 and 2 are 1 + 10 + 34 runs: one trip to cell_start for all of them.  Ring 1 always counts (a cell
    // next door can hold a point a hair away); ring 2 only if the window is still open behind ring 1.
    static_assert(1u + 10u + 34u <= 64u, "three rings in one wave");
    const uint32_t r = lane == 0u ? 0u : lane <= 10u ? 1u : 2u, qi = lane == 0u ? 0u : lane <= 10u ? lane - 1u : lane - 11u;
    uint32_t lb, le;
    uint64_t lbk;
    const bool ok = lane < 45u && (r < g) && cell_run(r, qi, cx, cy, cz, g, h, sg, SB, &lb, &le, &lbk);
    uint32_t b = 0, e = 0;
    if (ok) {
      b = cstart[lb];
      e = cstart[le];
    }
    cell_offer_runs<STREAM>(p, wl, b, (ok && lane <= 10u) ? e - b : 0u, lane, s, shared, ssite, sg, SB, ulps, q, n_mine, cfg32, bulk);
    if (cell_bound_key(h, 0.0, 0.0, SB) > q.tau_hi) return 2u;
    if (r_max < 2u || g <= 2u) return 0u;
    cell_offer_runs<STREAM>(p, wl, b, (ok && lane > 10u && !(lbk > q.tau_hi)) ? e - b : 0u, lane, s, shared, ssite, sg, SB, ulps, q, n_mine, cfg32, bulk);
  }
  for (uint32_t r = 3u;; ++r) {
    if (cell_bound_key((double)(r - 1u) * h, 0.0, 0.0, SB) > q.tau_hi) return r;  // nothing of interest from this ring on
    if (r > r_max || r >= g) return 0u;
    const uint32_t n_runs = ring_runs(r);
    for (uint32_t q0 = 0; q0 < n_runs; q0 += 64u) {
      const uint32_t qi = q0 + lane;
      uint32_t lb, le;
      uint64_t lbk;
      bool ok = qi < n_runs && cell_run(r, qi < n_runs ? qi : 0u, cx, cy, cz, g, h, sg, SB, &lb, &le, &lbk);
      ok = ok && !(lbk > q.tau_hi);
      uint32_t b = 0, e = 0;
      if (ok) {
        b = cstart[lb];
        e = cstart[le];
      }
      if (!__ballot(ok && e > b)) continue;
      cell_offer_runs<STREAM>(p, wl, b, ok ? e - b : 0u, lane, s, shared, ssite, sg, SB, ulps, q, n_mine, cfg32, bulk);
    }
  }
}
// the whole list by one wave, from L2/HBM (the fallback of cell_walk; four strides per trip for the loads to overlap)
template <bool STREAM = false>
__device__ __forceinline__ void list_sweep_solo(const CarveArgs& p, uint32_t n_list, uint32_t lane, uint32_t s, bool shared,
                                             uint32_t ssite, const SeedGeo& sg, uint32_t SB, uint64_t ulps, NearRow& q,
                                             uint32_t& n_mine,
                                             const uint64_t* cfg64 = nullptr) {
  const auto alive = G((const uint64_t*)p.bits_scratch);
  const auto loc = G((const uint64_t*)p.bits_scratch) + p.bits_stride;
  const bool form = UNI(p.mode) != CARVE_MODE_MERGE;  // (see tile_keys)
  for (uint32_t t0 = 0; t0 < n_list; t0 += 256u) {
    double x[4], y[4], z[4];
    uint32_t si[4];
    uint64_t aw[4], lw[4];
#pragma unroll
    for (uint32_t v = 0; v < 4u; ++v) {
      const uint32_t tb = t0 + v * 64u, t = tb + lane, tc = t < n_list ? t : n_list - 1u;
      const bool w_in = tb < n_list;
      // (the bitmaps are zero beyond the list; streaming carve: the validator clears bits while this runs)
      aw[v] = !w_in ? 0ull : STREAM ? (__hip_atomic_load(&alive[tb >> 6], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & G(cfg64)[tb >> 6]) : alive[tb >> 6];
      lw[v] = w_in ? loc[tb >> 6] : 0ull;
      x[v] = G(p.cc_ux)[tc];
      y[v] = G(p.cc_uy)[tc];
      z[v] = G(p.cc_uz)[tc];
      si[v] = G(p.cc_site)[tc];
    }
#pragma unroll
    for (uint32_t v = 0; v < 4u; ++v) {
      const uint32_t t = t0 + v * 64u + lane;
      const bool located = (lw[v] >> lane) & 1ull;
      const bool counts = ((aw[v] >> lane) & 1ull) && t != s && !(located && t < s && (form || (shared && si[v] == ssite)));
      offer_candidate(p, sg, ssite, x[v], y[v], z[v], si[v], counts ? t : 0u, located, counts, SB, ulps, q, n_mine);
    }
  }
}

// The finished register of a seed's sweep -> its row: *mine_out = this lane's entry (~0 beyond the row's K entries);
// returns the flags word (PM_ROW_*, entries in bits 0..7, first entry within the band of the last one in bits 8..15).
__device__ __forceinline__ uint32_t near_row_finish(const CarveArgs& p, const NearRow& q, bool valid, uint32_t K, uint32_t SB,
                                                    double TIE_BAND, uint32_t lane, uint64_t* mine_out) {
  // ---- the K nearest in (key, slot) order are lanes 0 .. K-1 of the row; lane K holds the first unlisted one
  const uint32_t n_tot = valid ? (uint32_t)__popcll(__ballot(q.key != ~0ull)) : 0u;
  const uint32_t n_k = n_tot < K ? n_tot : K;
  const uint64_t beyond = n_tot > K ? readlane_u64(q.key, K) : ~0ull;
  const uint64_t mine = lane < n_k ? q.key : ~0ull;
  const uint64_t noloc_kb = (PM_KEY_NOLOC >> SB) << SB;
  // row certificates the validator can rely on instead of re-deriving them at every step:
  //  clean      — no two neighbouring entries within the band of each other sit at different sites (entries in
  //               between are within the band too, so this covers every pair of the row)
  //  tail_clear — the first candidate NOT in the row is further than the band from the last entry
  //  tail_ok    — otherwise: everything unlisted within the band of the last entry sits at that entry's site
  uint32_t clean = 1, tail_clear = 0, tail_ok = 0;
  int tail_bad = 0;
  uint64_t e_last = 0;
  double a_last = 0.0, band2 = 0.0;
  uint32_t site_last = 0;
  if (valid) {
    const uint64_t kb = (mine >> SB) << SB;
    const uint32_t my_site = (lane < n_k && kb != noloc_kb) ? G(p.cc_site)[(uint32_t)(mine & ((1ull << SB) - 1ull))] : 0u;
    const uint64_t nkb_lo = __shfl_down((uint32_t)kb, 1, 64), nkb_hi = __shfl_down((uint32_t)(kb >> 32), 1, 64);
    const uint64_t nkb = (nkb_hi << 32) | nkb_lo;
    const uint32_t nsite = __shfl_down(my_site, 1, 64);
    int bad = 0;
    if (lane + 1u < n_k && kb != noloc_kb && nkb != noloc_kb) {
      const double a0 = __longlong_as_double((long long)kb), a1 = __longlong_as_double((long long)nkb);
      if (a1 - a0 <= a1 * (4.0 * TIE_BAND) + 1e-300 && nsite != my_site) bad = 1;
    }
    clean = __ballot(bad) == 0ull;
  }
  if (valid && n_k == K) {
    e_last = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(mine >> 32), (int)K - 1) << 32) |
             (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)mine, (int)K - 1);
    const uint64_t kb_last = (e_last >> SB) << SB;
    const uint64_t kb_beyond = (beyond >> SB) << SB;
    if (beyond == ~0ull || kb_last == noloc_kb) {
      tail_clear = 1;  // nothing unlisted, or only location-less candidates (exact ties, larger slots)
    } else if (kb_beyond == noloc_kb) {
      tail_clear = 1;
    } else {
      a_last = __longlong_as_double((long long)kb_last);
      const double a_b = __longlong_as_double((long long)kb_beyond);
      if (a_b - a_last > a_b * (4.0 * TIE_BAND) + 1e-300) {
        tail_clear = 1;
      } else {
        site_last = G(p.cc_site)[(uint32_t)(e_last & ((1ull << SB) - 1ull))];
        band2 = a_last * (4.0 * TIE_BAND) + 1e-300;
        // The unlisted candidates closest to the last entry are lanes K .. 63 of the sorted register; whatever
        // else came near the row during the sweep is summarised in the tracker (see NearRow): of those, only
        // the nearest one that does NOT sit at the last entry's site can break the certificate.
        if (lane >= K && lane < n_tot) {
          const uint64_t kb2 = (q.key >> SB) << SB;
          if (kb2 != noloc_kb && __longlong_as_double((long long)kb2) - a_last <= band2 &&
              G(p.cc_site)[(uint32_t)(q.key & ((1ull << SB) - 1ull))] != site_last)
            tail_bad = 1;
        }
        const uint64_t other = q.s1 != site_last ? q.m1 : q.m2;
        const uint64_t kb_o = (other >> SB) << SB;
        if (other != ~0ull && kb_o != noloc_kb && __longlong_as_double((long long)kb_o) - a_last <= band2) tail_bad = 1;
        tail_ok = __ballot(tail_bad) == 0ull;
      }
    }
  }
  // what the validator's chain needs to settle a step from the flags alone: is any listed term near the antipode,
  // and from which entry on does the row lie within the certificate band of its LAST entry (a selection that ends
  // in front of that entry has nothing to do with the row's tail) — the validator's own band expression
  uint32_t safe, j_tail = n_k;
  {
    const uint64_t kb = (mine >> SB) << SB;
    const bool located = lane < n_k && kb != noloc_kb;
    const double a_l = __longlong_as_double((long long)kb);
    safe = __ballot(located && a_l > PM_A_MAX_SAFE) == 0ull;
    if (n_k > 0u) {
      const uint64_t kb_le = (readlane_u64(mine, n_k - 1u) >> SB) << SB;
      if (kb_le != noloc_kb) {
        const double a_le = __longlong_as_double((long long)kb_le);
        const uint64_t within = __ballot(located && (a_le - a_l) <= a_l * TIE_BAND + 1e-300);
        j_tail = within ? (uint32_t)__builtin_ctzll(within) : n_k;
      }
    }
  }
  const uint32_t meta = n_k | (j_tail << 8) | (safe ? PM_ROW_SAFE : 0u) | ((n_k < K) ? PM_ROW_COMPLETE : 0u) |
                        (tail_ok ? PM_ROW_TAIL_OK : 0u) | (clean ? PM_ROW_CLEAN : 0u) | (tail_clear ? PM_ROW_TAIL_CLEAR : 0u);
  *mine_out = mine;
  return meta;
}

__global__ __launch_bounds__(256) void carve_propose_kernel(const CarveArgs* __restrict__ pa) {
  const CarveArgs& p = *pa;  // argument block in device memory: read through the scalar cache, never copied
  const auto st = G((const CarveStatus*)p.status);
  if (st->state != CARVE_STATE_RUNNING) return;
  const auto D = G((const BatchDesc*)p.desc);
  if (!D->planned || !D->valid) return;
  const uint32_t K = D->prop_k, n_list = D->n_list;
  const auto prop_out = G(p.prop);
  if (K == 0 || n_list > PM_CARVE_BIG_SLOTS) return;
  const uint32_t SB = n_list > PM_CARVE_SLOTS ? PM_CARVE_SLOT_BITS_BIG : PM_CARVE_SLOT_BITS;
  const double TIE_BAND = n_list > PM_CARVE_SLOTS ? PM_TIE_BAND_BIG : PM_TIE_BAND;
  const uint64_t WINDOW_ULPS = n_list > PM_CARVE_SLOTS ? (1ull << 25) : (1ull << 20);  // 8 band 2^53 (see near_window)
  const uint32_t lane = threadIdx.x & 63u;
  const auto alive = G((const uint64_t*)p.bits_scratch);
  const auto loc = G((const uint64_t*)p.bits_scratch) + p.bits_stride;
  const uint32_t lw = (n_list + 63u) >> 6;
  // ---- the neighbour rows.  Four seeds per workgroup (one per wave) sweep the candidate list together,
  // tile by tile through LDS.
  __shared__ TileBuf tiles[2];
  const uint32_t tid = threadIdx.x, wave = tid >> 6;
  const uint32_t n_seeds = D->n_seeds, cell_g = D->cell_g;
  const uint32_t n_tiles = (n_list + PROP_TILE - 1u) / PROP_TILE;
  const auto seed_slots = G((const uint32_t*)p.seed_slots);
  for (uint32_t k0 = blockIdx.x * 4u; k0 < n_seeds; k0 += gridDim.x * 4u) {
    const uint32_t out_row = k0 + wave;  // seed number = row
    const bool valid = out_row < n_seeds;
    const uint32_t s = valid ? seed_slots[out_row] : 0u;
    const uint32_t ssite = G(p.cc_site)[s];
    const SeedGeo sg = {G(p.cc_lat)[s], G(p.cc_lon)[s], G(p.cc_cos)[s], G(p.cc_ux)[s], G(p.cc_uy)[s], G(p.cc_uz)[s]};
    const bool shared = (ssite & 0x80000000u) != 0u;
    NearRow q = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull, 0xFFFFFFFFu};
    uint32_t n_mine = 0;
    if (cell_g) {  // (the same for every workgroup of the launch: no barrier on this side)
      if (valid) {
        // (the tiles' LDS is free on this side: a candidate buffer per wave)
        static_assert(4u * 2u * CELL_BUF * sizeof(uint32_t) <= sizeof(tiles), "four candidate buffers in the tiles' LDS");
        uint32_t* wl = reinterpret_cast<uint32_t*>(tiles) + wave * (2u * CELL_BUF);
        PM_BLOG(const uint64_t wt0 = PM_TICKS();)
        const uint32_t stop_r = p.prune_mode != 3u ? cell_walk(p, wl, cell_g, PM_CELL_RMAX, lane, s, shared, ssite, sg, SB, WINDOW_ULPS, q, n_mine) : 0u;
        BLOG_WALK(wt0, n_mine, stop_r);  // where the walk stopped, what it cost
        if (!stop_r) {
          q = NearRow{~0ull, ~0ull, ~0ull, ~0ull, ~0ull, 0xFFFFFFFFu};
          n_mine = 0;
          list_sweep_solo(p, n_list, lane, s, shared, ssite, sg, SB, WINDOW_ULPS, q, n_mine);
          if (lane == 0) atomicAdd(&p.status->prune_fallbacks, 1u);
        }
      }
    } else {
      TileRegs tr;
      tile_fetch(p, alive, loc, lw, n_list, 0u, tid, tr);
      tile_store(tiles[0], tid, tr);
      __syncthreads();
      for (uint32_t t = 0; t < n_tiles; ++t) {
        const bool more = t + 1u < n_tiles;
        if (more) tile_fetch(p, alive, loc, lw, n_list, t + 1u, tid, tr);  // in flight while this tile is consumed
        if (valid) tile_keys(p, tiles[t & 1u], t, lane, s, shared, ssite, sg, SB, WINDOW_ULPS, q, n_mine);
        if (more) tile_store(tiles[(t + 1u) & 1u], tid, tr);
        __syncthreads();
      }
    }
    uint64_t mine;
    const uint32_t meta = near_row_finish(p, q, valid, K, SB, TIE_BAND, lane, &mine);
    if (!valid) continue;  // (the workgroup's last seeds may be fewer than four)
    if (p.count_keys) {  // bookkeeping for the roofline of this kernel (bench only): keys this sweep evaluated
      const uint32_t swept = wave_sum(n_mine);
      if (lane == 0) {
        atomicAdd((unsigned long long*)&p.status->prop_keys, (unsigned long long)swept);
        atomicAdd(&p.status->n_props, 1u);
      }
    }
    // the row: the flags word, then the K sorted entries
    prop_out[(size_t)out_row * PM_PROP_ROW + ((lane + 1u) & 63u)] = lane == 63u ? (uint64_t)meta : mine;
    // ... and the same once more as 32-bit words (flags, slot of entry 0, slot of entry 1, ...): what a lane of
    // the chain's producer reads — 256 coalesced bytes per row
    reinterpret_cast<__attribute__((address_space(1))) uint32_t*>(prop_out + (size_t)out_row * PM_PROP_ROW + PM_PROP_SLOTS)[(lane + 1u) & 63u] =
        lane == 63u ? meta : (uint32_t)(mine & ((1ull << SB) - 1ull));
  }
}

#ifndef PM_PROP_CAP_DIV_WALK
#define PM_PROP_CAP_DIV_WALK 10u
#endif
#ifndef PM_PROP_CAP_DIV_BIG
#define PM_PROP_CAP_DIV_BIG 10u
#endif
#ifndef PM_PROP_CAP_DIV
#define PM_PROP_CAP_DIV 5u
#endif
// One proposal per located slot, at most PM_PROP_MAX_SEEDS per batch.  Returns the slot after the word in which
// the cap-th located slot falls (a later batch covers the rest), or n_list; *n_seeds = the located live slots
// below it (the batch's seeds).  Also records, per bitmap word below the limit, the seed bitmap and the number of
// seeds in front of the word (seed_map / seed_prefix): the rank of a slot among the seeds is the row its
// proposal is stored in (proposer and validator derive it from these two words).
// (one wave; the results are valid in every lane)
__device__ __forceinline__ void prop_limit_scan(const CarveArgs& p, uint32_t n_list, uint32_t lane, uint32_t* limit_out,
                                                uint32_t* n_seeds_out, bool walk = false) {
  // The configuration is re-prepared (and re-proposed) once half of its list is dead; by then the seed
  // pointer has advanced through roughly the first eighth of the slots (each group removes max_s slots
  // spread over the whole list), so later slots never consume this round's proposals: cap the batch.
  // (big lists: a tenth; measured again with the sorted-lane proposer at 1M x 100k, carve through the stepwise
  // tick: 1/6 26.3 ms, 1/8 22.5, 1/10 22.0, 1/14 22.7; small lists 1/3 .. 1/7 all within 1 %)
  // (a batch whose seeds walk the spatial index pays per seed, not per seed and candidate: it can afford more of them)
  uint32_t cap = walk ? n_list / (p.walk_cap_div ? p.walk_cap_div : PM_PROP_CAP_DIV_WALK) : n_list > PM_CARVE_SLOTS ? n_list / PM_PROP_CAP_DIV_BIG : n_list / PM_PROP_CAP_DIV;
  if (cap < 512u) cap = 512u;
  if (cap > PM_PROP_MAX_SEEDS) cap = PM_PROP_MAX_SEEDS;
  const auto g_al = G((const uint64_t*)p.bits_scratch);
  const auto g_lc = G((const uint64_t*)p.bits_scratch) + p.bits_stride;
  const auto seed_map = G(p.seed_map);
  const auto seed_prefix = G(p.seed_prefix);
  const uint32_t lwp = (n_list + 63u) >> 6;
  uint32_t acc = 0, limit = n_list;
  for (uint32_t j0 = 0; j0 < lwp; j0 += 64u) {
    const uint32_t j = j0 + lane;
    const uint64_t m = j < lwp ? (g_al[j] & g_lc[j]) : 0ull;  // bits beyond n_list are zero in both bitmaps
    const uint32_t cnt = (uint32_t)__popcll(m);
    const uint32_t incl = wave_incl_scan_u32(cnt);
    const uint64_t over = __ballot(acc + incl >= cap);
    const uint32_t last = over ? (uint32_t)__builtin_ctzll(over) : 63u;  // last word of this pass inside the batch
    if (j < lwp && lane <= last) {
      seed_map[j] = m;
      seed_prefix[j] = acc + incl - cnt;
    }
    acc += __shfl(incl, (int)last, 64);
    if (over) {
      limit = (j0 + last + 1u) * 64u;
      break;
    }
  }
  *limit_out = limit < n_list ? limit : n_list;
  *n_seeds_out = acc;
}

// seed number -> slot (the proposer takes its seeds from this dense list): every thread of the workgroup expands
// the bitmap words it owns, after prop_limit_scan (and a barrier) have produced seed_map / seed_prefix
__device__ __forceinline__ void prop_seed_slots(const CarveArgs& p, uint32_t limit, uint32_t tid, uint32_t n_threads) {
  const auto seed_map = G((const uint64_t*)p.seed_map);
  const auto seed_prefix = G((const uint32_t*)p.seed_prefix);
  const auto seed_slots = G(p.seed_slots);
  const uint32_t words = (limit + 63u) >> 6;
  for (uint32_t j = tid; j < words; j += n_threads) {
    uint32_t o = seed_prefix[j];
    for (uint64_t mm = seed_map[j]; mm; mm &= mm - 1ull) seed_slots[o++] = j * 64u + (uint32_t)__builtin_ctzll(mm);
  }
}

__device__ __noinline__ uint32_t carve_prop_limit(const CarveArgs& p, BlockRed& red, uint32_t n_list, uint32_t* n_seeds) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (wave == 0) {
    uint32_t limit, acc;
    prop_limit_scan(p, n_list, lane, &limit, &acc);
    if (lane == 0) {
      red.b[0] = limit;
      red.b[1] = acc;
    }
  }
  __syncthreads();
  const uint32_t r = red.b[0];
  *n_seeds = red.b[1];
  prop_seed_slots(p, r, threadIdx.x, CARVE_THREADS);
  __syncthreads();
  return r;
}


// debug (pm_debug_row_certificates): what a finished row is and what near_row_finish makes of it, for the host to hold to a
// reference of its own.  Per wave and row: the 64 keys; tau, tau_hi, m1, m2, s1; and for every K = 1 .. PM_PROP_KMAX the flags
// word and the lanes' entries.  `p` is all zeros but the site table: near_row_finish reads nothing else of it.
// The slot width reaches near_row_finish and the networks' inline copy as the product's kernels hand it over — one of the two
// constants rows run at (row_cert_sb; the entry point refuses any other) — and not as a free kernel argument: the compiler
// carries an argument's range into a function all of whose callers agree on it, and with a third caller that knows nothing of
// the width carve_stream_kernel and carve_propose_kernel came out as other code, with more registers spilled.  With this the two
// have the parent's instructions (the propose kernel up to register numbers).
__device__ __forceinline__ uint32_t row_cert_sb(uint32_t SB) { return SB > PM_CARVE_SLOT_BITS ? PM_CARVE_SLOT_BITS_BIG : PM_CARVE_SLOT_BITS; }
struct RowCertOut {
  uint64_t* rows;   // [n_waves][3][64]
  uint64_t* track;  // [n_waves][3][5]
  uint32_t* flags;  // [n_waves][3][PM_PROP_KMAX]
  uint64_t* mine;   // [n_waves][3][PM_PROP_KMAX][64]
};
__device__ __noinline__ void row_cert_emit(const NearRow q, const uint32_t* sites, uint32_t SB, double tie_band, uint32_t lane, size_t at,
                                           const RowCertOut o) {
  CarveArgs p = {};
  p.cc_site = const_cast<uint32_t*>(sites);
  o.rows[at * 64u + lane] = q.key;
  if (lane < 5u) o.track[at * 5u + lane] = lane == 0u ? q.tau : lane == 1u ? q.tau_hi : lane == 2u ? q.m1 : lane == 3u ? q.m2 : (uint64_t)q.s1;
#pragma unroll 1
  for (uint32_t K = 1u; K <= PM_PROP_KMAX; ++K) {
    uint64_t mine;
    const uint32_t meta = near_row_finish(p, q, true, K, row_cert_sb(SB), tie_band, lane, &mine);
    o.mine[(at * PM_PROP_KMAX + (K - 1u)) * 64u + lane] = mine;
    if (lane == 0u) o.flags[at * PM_PROP_KMAX + (K - 1u)] = meta;
  }
}
// debug (pm_debug_row_networks): one wave per block builds the row of its n_per_wave keys twice — stride by stride
// through the insertion, and four strides at a time through the networks for the first `upto` keys — and compares the
// registers lane by lane and what the trackers answer at the end (for every site the last entry could have).  rows_out
// gets the second row (the host compares it with a sort of its own).  With `cert` (pm_debug_row_certificates) a third row goes
// through the networks' inline copy, as the streaming carve's sweep has it, and all three are written out (row_cert_emit).
__global__ __launch_bounds__(256) void row_network_test_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ sites,
                                                              uint32_t n_per_wave, uint32_t SB, uint64_t ulps, uint32_t upto,
                                                              uint64_t* __restrict__ rows_out, uint32_t* __restrict__ mismatches,
                                                              double tie_band, RowCertOut cert) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, w = blockIdx.x * 4u + wave;  // (n_waves is a multiple of four)
  const uint64_t* kw = keys + (size_t)w * n_per_wave;
  NearRow a = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull, 0xFFFFFFFFu}, b = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull, 0xFFFFFFFFu};
  NearRow c = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull, 0xFFFFFFFFu};
  const bool with_cert = cert.rows != nullptr;  // (the same for every wave of the launch)
  __shared__ uint64_t pack_lds[4u * NET_PACK_KEYS];  // (side by side, as in the row-making workgroups)
  const LaneNet ln = lane_net(lane, pack_lds + wave * NET_PACK_KEYS);
  const auto cs = G(sites);
  const uint64_t slot_mask = (1ull << SB) - 1ull;
  for (uint32_t k0 = 0; k0 < n_per_wave; k0 += 256u) {
    uint64_t kk[4];
    uint32_t ss[4];
#pragma unroll
    for (uint32_t v = 0; v < 4u; ++v) {
      const uint32_t i = k0 + v * 64u + lane;
      kk[v] = i < n_per_wave ? kw[i] : ~0ull;
      ss[v] = kk[v] != ~0ull ? cs[(uint32_t)(kk[v] & slot_mask)] : 0u;
    }
#pragma unroll
    for (uint32_t v = 0; v < 4u; ++v) near_row_offer(a, kk[v], ss[v], cs, SB, ulps);
    if (k0 < upto) {
      near_row_offer_bulk<4u>(b, kk, ss, sites, SB, ulps, ln);
    } else {
#pragma unroll
      for (uint32_t v = 0; v < 4u; ++v) near_row_offer(b, kk[v], ss[v], cs, SB, ulps);
    }
    if (with_cert) {
      if (k0 < upto) {
        near_row_offer_bulk<4u, true>(c, kk, ss, sites, row_cert_sb(SB), ulps, ln);
      } else {
#pragma unroll
        for (uint32_t v = 0; v < 4u; ++v) near_row_offer(c, kk[v], ss[v], cs, SB, ulps);
      }
    }
  }
  if (with_cert) {
    row_cert_emit(a, sites, SB, tie_band, lane, (size_t)w * 3u, cert);
    row_cert_emit(b, sites, SB, tie_band, lane, (size_t)w * 3u + 1u, cert);
    row_cert_emit(c, sites, SB, tie_band, lane, (size_t)w * 3u + 2u, cert);
  }
  uint32_t bad = __ballot(a.key != b.key) ? 1u : 0u;
  if (a.tau != b.tau || a.tau_hi != b.tau_hi) bad |= 2u;
  const uint32_t try_sites[3] = {a.s1, b.s1, 0xFFFFFFFEu};
#pragma unroll
  for (uint32_t i = 0; i < 3u; ++i) {  // the nearest tracked key that is not at the last entry's site, if within the window
    uint64_t oa = a.s1 != try_sites[i] ? a.m1 : a.m2, ob = b.s1 != try_sites[i] ? b.m1 : b.m2;
    oa = oa < a.tau_hi ? oa : ~0ull;
    ob = ob < b.tau_hi ? ob : ~0ull;
    if (oa != ob) bad |= 4u;
  }
  rows_out[(size_t)w * 64u + lane] = b.key;
  if (lane == 0u && bad) atomicOr(&mismatches[0], bad), atomicAdd(&mismatches[1], 1u);
}

// debug (pm_debug_distance_keys): the carve's distance key of n pairs through the device functions the carve runs.  in: lat[2n]
// (first points, then second points), lon[2n], slot[n] (as f64); geo: what geo_kernel made of those 2n points (cos(lat), ux,
// uy, uz: 2n each).  Per pair out[PM_DK_WORDS]: see include/pm_engine_debug.h.  mode 1: out[i] = sin_band(in[i]).
struct DkNanCol {  // a coordinate column that is NaN everywhere: prox_a answers NaN iff it fell back to the sine form
  __device__ double operator[](uint32_t) const { return __builtin_nan(""); }
};
__global__ __launch_bounds__(256) void distance_key_test_kernel(const double* __restrict__ in, const double* __restrict__ geo,
                                                               uint32_t n, uint32_t mode, double* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (mode == 1u) {
    if (i < n) out[i] = sin_band(in[i]);
    return;
  }
  const uint32_t j = i < n ? i : 0u, k = n + j;  // (every lane takes part: candidate_key ballots)
  const double *lat = in, *lon = in + 2u * (size_t)n, *cs = geo, *ux = cs + 2u * (size_t)n, *uy = ux + 2u * (size_t)n,
               *uz = uy + 2u * (size_t)n;
  const uint32_t slot = (uint32_t)in[4u * (size_t)n + j];
  const SeedGeo sg = {lat[j], lon[j], cs[j], ux[j], uy[j], uz[j]};
  const double h = hav_a(sg.lat, sg.lon, sg.cos, lat[k], lon[k], cs[k]);
  const double pa = prox_a(sg, ux[k], uy[k], uz[k], lat, lon, cs, k);
  const double pn = prox_a(sg, ux[k], uy[k], uz[k], DkNanCol{}, DkNanCol{}, DkNanCol{}, k);
  // candidate_key with the candidate's columns based at it (t = 0) and no slot bits: the unpacked key, at another site
  CarveArgs p = {};
  p.cc_lat = (double*)lat + k;
  p.cc_lon = (double*)lon + k;
  p.cc_cos = (double*)cs + k;
  NearRow q{};
  const uint64_t ck = candidate_key(p, sg, 0u, ux[k], uy[k], uz[k], 1u, 0u, true, true, 0u, q);
  if (i >= n) return;
  double* o = out + (size_t)i * PM_DK_WORDS;
  o[0] = sin_band((lat[k] - lat[j]) * PM_RAD * 0.5);
  o[1] = sin_band((lon[k] - lon[j]) * PM_RAD * 0.5);
  o[2] = cs[j], o[3] = ux[j], o[4] = uy[j], o[5] = uz[j];
  o[6] = cs[k], o[7] = ux[k], o[8] = uy[k], o[9] = uz[k];
  o[10] = h;
  o[11] = pa;
  o[12] = pn == pn ? 1.0 : 0.0;
  o[13] = __longlong_as_double((long long)ck);
  const uint32_t widths[3] = {PM_CARVE_SLOT_BITS, PM_CARVE_SLOT_BITS_BIG, PM_CARVE_SLOT_BITS_MEM};
#pragma unroll
  for (uint32_t w = 0; w < 3u; ++w) {
    const uint32_t sl = slot & ((1u << widths[w]) - 1u);
    o[14 + w] = __longlong_as_double((long long)pack_key((uint64_t)__double_as_longlong(pa), sl, widths[w]));
    o[17 + w] = __longlong_as_double((long long)pack_key((uint64_t)__double_as_longlong(h), sl, widths[w]));
  }
}
