// pm_stream.inc — the streaming carve (carve_variant 0): ONE launch forms every group of a try_form_new_groups pass
// (reference: crates/orchestrator/src/plugins/node_groups/mod.rs:478-628).  Included by pm_kernels.hip behind the
// validator's building blocks (carve_chain, carve_fast_steps, carve_exact_step, the proposer's row builders).
//
// The batch pipeline (carve_variant 3) alternates four launches per batch — prepare a compact candidate list,
// propose a neighbour row for a fifth of its seeds, validate — and every batch and every configuration starts cold.
// Here nothing is compacted and nothing is batched:
//   * slot == position.  The eligible list's positions ARE the candidate slots of every configuration; the candidate
//     set of configuration c is the bitmap  free & compatible_c  (cfgbits, built once by carve_elig_place_kernel), and
//     removals are bit clears.  The validator keeps the current configuration's candidate bitmap in LDS and publishes
//     ONE bitmap for the whole carve — `free`, p.bits_scratch: the positions no group holds yet — which its collector
//     wave keeps a few commits behind the truth.  A copy that only ever lags is a superset of the truth at any later
//     moment, and that is all a neighbour row needs (rows are validated against the live bitmap; a row made from a
//     superset minus its dead entries is the reference's sorted remaining list, see carve_chain).  The superset need
//     not hold what is certainly dead at the seed's turn: the located candidates in front of the seed (a live one would
//     be the seed instead) are masked out of a swept row before anything is fetched — stream_bitmap_sweep.
//   * workgroup 0 is the validator (the same three-wave chain as the batch pipeline).  Its producer wave walks the
//     candidate bitmap in front of the chain and hands every live located candidate a TICKET — an 8-byte granule
//     {tag, position | configuration | how to make the row} in a ring — at most a look-ahead of `la` tickets in front
//     of what it has handed to the chain; once the configuration being carved has no candidate without a ticket left,
//     it goes on with the first candidates of the configuration that comes next (they are candidates of it whatever
//     the rest of this one removes, unless it removes them), so a configuration does not start cold.
//   * every other workgroup is eight independent proposer waves: take the next ticket number (one atomicAdd), wait
//     for that ticket to be issued, build the seed's row — a walk over the spatial index, or a sweep of the bitmap
//     free & compatible: set bits -> positions, packed into LDS, evaluated in full strides — and write it to a ring
//     of rows as granules {tag, half of a packed key}.  The producer wave polls the rows of its tickets IN ORDER and
//     parks them, digested, in the chain's LDS ring.
//   * granules ({tag, value} in one aligned 8-byte agent-scope store) need no fence and no flag: the data is the flag
//     (cdna_hip_programming.md, Guideline 16, form R2).  Every wait is bounded: a row that does not arrive is a step
//     for the exact sweep, a proposer that is never asked anything leaves, and a lost hand-shake ends the launch with
//     CARVE_STATE_ABORTED (what was committed stands; the engine continues on the batch pipeline).
// Staleness is bounded by the look-ahead instead of by a batch, and what the look-ahead wastes — rows for seeds that a
// group absorbs before their turn — is work of CUs that have nothing else to do, off the chain's path.

// words of the validator's ticket state in LDS (behind the carve kernel's regions; survives exact steps)
enum { SLW_TREQ = PM_STREAM_TP,  // tickets issued so far (read by carve_fast_steps<STREAM>: where its walk over the tickets ends)
       SLW_PAY,                  // bits 18.. of a ticket's payload: configuration, row mode (carve_fast_steps reads the configuration)
       SLW_TISSUED,              // the same count, as the ticketer left it
       SLW_SCANW, SLW_SCANLO, SLW_SCANHI,  // the ticketer's cursor over the candidate bitmap: word, bits left in it
       SLW_TIMEOUTS,             // rows given up on
       SLW_LA,                   // look-ahead for this configuration
       SLW_TEND,                 // PM_NONE until the configuration has no candidate without a ticket, then the count at that moment
       SLW_ACKT, SLW_ACKP0, SLW_ACKP1, SLW_ACKP2, SLW_ACKP3, SLW_ACKP4,  // acknowledgements of the ticketer and the parkers
       SLW_NCAND,                // candidates alive (published by the chain with every batch of steps)
       // two configurations expected behind this one get their first tickets ahead of their turn (a ticket carries its
       // configuration, so the streams interleave): per slot the configuration (PM_NONE = free), payload bits, how many
       // to issue, the first ticket, how many have been issued, the cursor over ITS candidates
       SLW_P_CI, SLW_P_CI1, SLW_P_PAY, SLW_P_PAY1, SLW_P_MAX, SLW_P_MAX1, SLW_P_T0, SLW_P_T01, SLW_P_CNT, SLW_P_CNT1,
       SLW_P_SCANW, SLW_P_SCANW1, SLW_P_SCANLO, SLW_P_SCANLO1, SLW_P_SCANHI, SLW_P_SCANHI1,
       SLW_WORDS };
static_assert(SLW_TREQ == PM_STREAM_SLW_TREQ && SLW_PAY == PM_STREAM_SLW_PAY, "the words carve_fast_steps reads");
static_assert(SLW_WORDS <= PM_STREAM_TP + 32u, "ticket state fits its LDS region");
#ifndef STREAM_NPARK
#define STREAM_NPARK 5u  // parker waves: 1, 5, 6, 7 and — the fifth — wave 4, the chain's SIMD partner (a parker mostly waits for
                        // memory: what it takes from the chain's issue slots, +6 % per step, is less than what the chain
                        // waited for rows with four: -2 % per match at every size, profiles/r04_stream_anatomy_*.txt)
#endif
#ifndef STREAM_PARK_NB
#define STREAM_PARK_NB 16u    // tickets a parker takes up at a time
#endif
// naps of the validator's feeding waves between two looks at an LDS word (s_sleep units of 64 clocks): the ticketer with nothing to hand
// out, a parker waiting for its block's tickets or rows, a parker waiting for its turn or for room in the ring
#ifndef STREAM_NAP_TICKETER
#define STREAM_NAP_TICKETER 4
#endif
#ifndef STREAM_NAP_PARK
#define STREAM_NAP_PARK 2
#endif
#ifndef STREAM_NAP_TURN
#define STREAM_NAP_TURN 1
#endif
#ifndef STREAM_TICKETER_WAVE  // 3, or 4: the chain's SIMD partner (waves w and w + 4 share a SIMD) — then wave 3 is the fifth parker
#define STREAM_TICKETER_WAVE 3u
#endif
#ifndef STREAM_BATCH_N
#define STREAM_BATCH_N 16u    // entries the chain takes up at a time (<= 31: their live ones are a mask with a guard bit behind)
#endif
static_assert(STREAM_BATCH_N >= 1u && STREAM_BATCH_N <= 31u, "a batch's live mask and its guard bit fit 32 bits");
#define STREAM_SMALL_CPL 2u   // located candidates a lane holds when a configuration's located phase ends in registers
#define STREAM_SMALL (64u * STREAM_SMALL_CPL)
#ifndef STREAM_SMALL_AT  // located candidates left at which the chain hands a configuration over to stream_small
#define STREAM_SMALL_AT 16u
#endif
#ifndef STREAM_NAP_LONG  // the longest nap of a row maker between two looks at its ticket slot (s_sleep units of 64 clocks)
#define STREAM_NAP_LONG 32
#endif
#ifndef STREAM_SMALL_START  // located candidates up to which a configuration (or what is left of one) is carved in registers from the start
#define STREAM_SMALL_START STREAM_SMALL
#endif
static_assert(STREAM_SMALL_START >= STREAM_SMALL_AT && STREAM_SMALL_START <= STREAM_SMALL, "what the chain hands over fits, and is taken");
#define STREAM_LATE_ROW_TICKS 240000ull  // s_memtime ticks (~100 us) after which a finished row checks that its slot is still its own
// (the three below can be set from the command line of a variant build: tools/variant_bench.py, PM_EXP_DEFINES)
#ifndef STREAM_PRE_EARLY
#define STREAM_PRE_EARLY 192u  // tickets a configuration expected next gets while the current one is still handing out its own
#endif
#ifndef STREAM_PRE_NEAR
#define STREAM_PRE_NEAR 1024u  // ... once the current one is down to this many candidates
#endif
#ifndef STREAM_LA_SMALL_NUM  // ... quarters of them, that is (4: all)
#define STREAM_LA_SMALL_NUM 4u
#endif
#if STREAM_LA_SMALL_NUM == 4u
#define STREAM_LA_SMALL(n) (n)
#else
#define STREAM_LA_SMALL(n) ((n) / 4u * STREAM_LA_SMALL_NUM)
#endif
// STREAM_NO_DROP is 0 or 1 — a variant build's switch, not a tuning knob.  1 (what a bare -DSTREAM_NO_DROP gives): no ticket is
// ever dropped, STREAM_DROPPED is false.  0, the product: the tickets a configuration has no use for any more are let be.
#ifndef STREAM_NO_DROP
#define STREAM_NO_DROP 0
#endif
static_assert(STREAM_NO_DROP == 0 || STREAM_NO_DROP == 1, "STREAM_NO_DROP is 0 or 1");
#ifndef STREAM_LA_ALL
#define STREAM_LA_ALL 1536u  // candidates up to which a configuration's seeds all get their tickets at once
#endif
#ifndef PM_STREAM_ROW_SPINS
#define PM_STREAM_ROW_SPINS 4096u       // polls (about 0.5 us each) before the validator gives a row up
#endif
#ifndef PM_STREAM_IDLE_SPINS
#define PM_STREAM_IDLE_SPINS (1u << 21) // polls (about 1 us each) before an unasked proposer wave leaves
#endif
#ifndef STREAM_SMALL_WINDOW  // live candidates in front of a candidate of stream_small_rows whose row is being made (settable in a variant build)
#define STREAM_SMALL_WINDOW 8u
#endif
// located candidates alive (cand & loc), counted by one wave from the LDS bitmaps
__device__ __forceinline__ uint32_t stream_count_located(const uint64_t* l_alive, const uint64_t* l_loc, uint32_t lw, uint32_t lane) {
  uint32_t cnt = 0u;
  for (uint32_t j = lane; j < lw; j += 64u) cnt += (uint32_t)__popcll(l_alive[j] & l_loc[j]);
  return wave_sum(cnt);
}

// SC_DROP: what the validator publishes when a configuration's outstanding tickets lose their purpose, and what a row maker
// asks of it (ticket numbers count from zero in every launch and stay far below 2^25)
#define STREAM_DROP_WORD(ci, t) (((uint32_t)(ci) << 26) | ((uint32_t)(t) & 0x03FFFFFFu))
#define STREAM_DROPPED(word, ci, t) (!STREAM_NO_DROP && ((word) >> 26) == (uint32_t)(ci) && ((((uint32_t)(t) - (word)) & 0x03FFFFFFu) >= 0x02000000u))
typedef __attribute__((address_space(1))) unsigned long long stream_gu64;
typedef __attribute__((address_space(1))) uint32_t stream_gu32;
__device__ __forceinline__ unsigned long long ld_ag(const stream_gu64* q) {
  return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_ag(stream_gu64* q, unsigned long long v) {
  __hip_atomic_store(q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t ld_ag32(const stream_gu32* q) {
  return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_ag32(stream_gu32* q, uint32_t v) {
  __hip_atomic_store(q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// control words of the chain's block beyond carve_chain's: the parkers take ring positions in ticket order —
// CC_CUMSEQ: the block of tickets whose turn it is, CC_CUM: entries parked (or being parked) in front of it
enum { CC_CUMSEQ = 11, CC_CUM = 12 };
static_assert(CC_CUM < 16u && CC_M0 < CC_CUMSEQ, "the parkers' words fit the control block");

// The row source of the chain, on the validator's otherwise idle waves:
//   the ticketer (one wave)    walks the candidate bitmap in front of the chain and hands every live located candidate a
//                              ticket — at most `la` of them in front of what the parkers have taken up — then the
//                              first candidates of the configuration expected next;
//   five parkers (a wave each) parker i takes the blocks of sixteen tickets i, i + 5, ... of the run: waits for the
//                              block's tickets (or the end of the configuration's), requests the rows of the seeds that
//                              are alive at that moment, takes its turn for their ring positions (entries are dense: a
//                              dead seed takes none), waits for room, polls the rows and parks them, digested — per lane
//                              the LDS address of the entry's bitmap word and its bit — each entry stamped with its
//                              sequence number when it is complete.
// One wave doing all of it needed 0.6 us per row against the chain's 0.28 (profiles/r04_stream_anatomy_*.txt).
template <bool BIG>
__device__ __noinline__ void stream_ticket(const CarveArgs& p, const StepCtx& c, uint64_t* l_alive, const uint64_t* l_loc,
                                           uint32_t* l_buf, uint32_t* sl_words) {
  const uint32_t lane = threadIdx.x & 63u;
  const chain_lds_u64* const A64 = lds_pin<const chain_lds_u64*>(l_alive);
  const chain_lds_u64* const LOC64 = lds_pin<const chain_lds_u64*>(l_loc);
  chain_lds_u32* const SL = lds_pin<chain_lds_u32*>(sl_words);
  const ChainLds L = chain_lds(l_buf);
  const auto sq = G(p.stream_sq);
  const uint32_t tag0 = UNI(p.stream_tag0);
  const uint32_t lw = (UNI(c.n_list) + 63u) >> 6;
  const bool need_rows = UNI(c.max_s) > 1u;  // (a group of one node needs no neighbours)
  uint32_t t_req = UNI(cc_ld(&SL[SLW_TISSUED])), scan_w = UNI(cc_ld(&SL[SLW_SCANW]));
  uint32_t scan_lo = UNI(cc_ld(&SL[SLW_SCANLO])), scan_hi = UNI(cc_ld(&SL[SLW_SCANHI]));
  const uint32_t la_cap = UNI(cc_ld(&SL[SLW_LA])), pay_hi = UNI(cc_ld(&SL[SLW_PAY]));
  uint32_t la = la_cap + 4u * STREAM_PARK_NB;
  // the configurations expected behind this one: once this one has no candidate without a ticket left, their first
  // candidates get theirs — from what is free right now: (master & ~compatible_this) | candidates_this — so that they
  // do not start cold
  const uint32_t this_ci = (pay_hi >> 18) & 63u;
  uint32_t p_ci[2], p_pay[2], p_max[2], p_t0[2], p_cnt[2], p_w[2], p_lo[2], p_hi[2];
#pragma unroll
  for (uint32_t k = 0; k < 2u; ++k) {
    p_ci[k] = UNI(cc_ld(&SL[SLW_P_CI + k]));
    p_pay[k] = UNI(cc_ld(&SL[SLW_P_PAY + k]));
    p_max[k] = UNI(cc_ld(&SL[SLW_P_MAX + k]));
    p_t0[k] = UNI(cc_ld(&SL[SLW_P_T0 + k]));
    p_cnt[k] = UNI(cc_ld(&SL[SLW_P_CNT + k]));
    p_w[k] = UNI(cc_ld(&SL[SLW_P_SCANW + k]));
    p_lo[k] = UNI(cc_ld(&SL[SLW_P_SCANLO + k]));
    p_hi[k] = UNI(cc_ld(&SL[SLW_P_SCANHI + k]));
  }
  uint32_t t_end = UNI(cc_ld(&SL[SLW_TEND]));
  if (lane == 0u) STREAM_TRACE(17, p_ci[0] & 0xFFu | (p_ci[1] & 0xFFu) << 8 | this_ci << 16, p_cnt[0] | p_cnt[1] << 16);  // slots as the ticketer finds them
  const auto master = G((const uint64_t*)p.alive_g);
  const auto cfgbits_all = G((const uint64_t*)p.cfgbits);  // (the argument block is read here, not inside the loops)
  const size_t bits_stride = p.bits_stride;
  const auto cfg_this = cfgbits_all + (size_t)this_ci * bits_stride;
  uint32_t seen = 0u;  // last command word acted on
  auto publish = [&]() {  // what the parkers and carve_fast_steps go by
    if (scan_w >= lw && t_end == PM_NONE) t_end = t_req;  // this configuration's tickets are complete: all below here
    if (lane == 0u) {
      cc_st(&SL[SLW_TREQ], t_req);
      cc_st(&SL[SLW_TEND], t_end);  // (behind the count)
    }
  };
  auto save = [&]() {
    publish();
    if (lane == 0u) STREAM_TRACE(18, p_ci[0] & 0xFFu | (p_ci[1] & 0xFFu) << 8 | this_ci << 16, p_cnt[0] | p_cnt[1] << 16);  // ... and leaves them
    if (lane == 0u) {
      cc_st(&SL[SLW_TISSUED], t_req);
#pragma unroll
      for (uint32_t k = 0; k < 2u; ++k) {
        cc_st(&SL[SLW_P_T0 + k], p_t0[k]);
        cc_st(&SL[SLW_P_CNT + k], p_cnt[k]);
        cc_st(&SL[SLW_P_SCANW + k], p_w[k]);
        cc_st(&SL[SLW_P_SCANLO + k], p_lo[k]);
        cc_st(&SL[SLW_P_SCANHI + k], p_hi[k]);
      }
      cc_st(&SL[SLW_SCANW], scan_w);
      cc_st(&SL[SLW_SCANLO], scan_lo);
      cc_st(&SL[SLW_SCANHI], scan_hi);
    }
  };
  // one word of candidates -> tickets (at most `room`): which bits of it are left
  auto hand_out = [&](uint64_t w, uint32_t wj, uint32_t room, uint32_t pay) -> uint64_t {
    const uint32_t rk = __builtin_amdgcn_mbcnt_hi((uint32_t)(w >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)w, 0u));
    const bool mine = ((w >> lane) & 1ull) && rk < room;
    const uint64_t tk_m = __ballot(mine);
    if (mine) {
      const uint32_t pos = wj * 64u + lane, t = t_req + rk;
      cc_st(&SL[t & (PM_STREAM_TP - 1u)], (pay & 0x00FC0000u) | pos);  // (position | configuration << 18)
      if (need_rows) st_ag(&sq[t & (PM_STREAM_SQ - 1u)], ((unsigned long long)(tag0 + t) << 32) | pay | pos);
    }
    t_req += (uint32_t)__popcll(tk_m);
    return w & ~tk_m;
  };
  for (;;) {
    uint32_t cmd = chain_wait_cmd(L, seen);
    if (cmd == 0u) break;
    seen = cmd;
    if ((cmd & 3u) == CH_QUIT) break;
    if ((cmd & 3u) != CH_RUN) {  // (a STOP without a RUN in between)
      save();
      cc_st(&SL[SLW_ACKT], cmd);
      continue;
    }
    const uint32_t t0_run = UNI(cc_ld(&L.CC[CC_START]));
    uint32_t idle = 0u;
    for (;;) {
      if (cc_ld(&L.CC[CC_CMD]) != seen) break;
      const uint32_t t_front = t0_run + UNI(cc_ld(&L.CC[CC_CUMSEQ])) * STREAM_PARK_NB;  // the tickets the parkers have taken up
      const uint32_t before = t_req;
      {  // the window follows what is left of the configuration (see look_ahead in carve_stream_kernel)
        const uint32_t n_now = UNI(cc_ld(&SL[SLW_NCAND]));
        uint32_t l = n_now <= STREAM_LA_ALL ? STREAM_LA_SMALL(n_now) : n_now / 4u;
        l = l < 24u ? 24u : l;
        la = (l < la_cap ? l : la_cap) + 4u * STREAM_PARK_NB;
      }
      // (tickets of the configurations behind this one that the parkers have not passed yet do not count against this
      // one's window: a slot whose first ticket is still in front of them is so as a whole)
      uint32_t pre_ahead = 0u;
#pragma unroll
      for (uint32_t k = 0; k < 2u; ++k)
        if (p_ci[k] != PM_NONE && p_cnt[k] != 0u && p_t0[k] - t_front < 0x80000000u) pre_ahead += p_cnt[k];
      // ---- this configuration's candidates
      while (t_req - t_front - pre_ahead < la && scan_w < lw) {
        const uint32_t j = scan_w + lane;
        unsigned long long ll = j < lw ? (A64[j] & LOC64[j]) : 0ull;
        if (lane == 0u) ll &= ((unsigned long long)scan_hi << 32) | scan_lo;
        const uint64_t nz = __ballot(ll != 0ull);
        if (!nz) {
          scan_w += 64u;
          scan_lo = scan_hi = 0xFFFFFFFFu;
          continue;
        }
        {  // all 64 words at once when their candidates fit the window: a lane per word
          const uint32_t cw = (uint32_t)__popcll(ll);
          const uint32_t incl = wave_incl_scan_u32(cw);
          const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
          if (tot <= la - (t_req - t_front - pre_ahead)) {
            uint32_t t = t_req + incl - cw;
            for (unsigned long long b = ll; b; b &= b - 1ull, ++t) {
              const uint32_t pos = j * 64u + (uint32_t)__builtin_ctzll(b);
              cc_st(&SL[t & (PM_STREAM_TP - 1u)], (pay_hi & 0x00FC0000u) | pos);
              if (need_rows) st_ag(&sq[t & (PM_STREAM_SQ - 1u)], ((unsigned long long)(tag0 + t) << 32) | pay_hi | pos);
            }
            t_req += tot;
            scan_w += 64u;
            scan_lo = scan_hi = 0xFFFFFFFFu;
            publish();  // (the parkers take a block of tickets up as soon as it is complete)
            continue;
          }
        }
        const uint32_t src = (uint32_t)__builtin_ctzll(nz);
        const uint32_t wj = scan_w + src;
        const uint64_t rest = hand_out(readlane_u64(ll, src), wj, la - (t_req - t_front - pre_ahead), pay_hi);
        scan_w = rest ? wj : wj + 1u;
        scan_lo = rest ? (uint32_t)rest : 0xFFFFFFFFu;
        scan_hi = rest ? (uint32_t)(rest >> 32) : 0xFFFFFFFFu;
      }
      // ---- they all have their tickets — or this configuration is within a few hundred candidates of its end: on to the
      // configurations expected behind this one.  Early, a slot gets STREAM_PRE_EARLY tickets whatever the window says
      // (a cold start costs the chain a ticket round trip and a row, 40 - 60 us, at every configuration boundary; the
      // rows are the work of CUs that have nothing else to do); once this configuration's scan is through, the window's
      // worth.  (Only near the end: a configuration that issues thousands of tickets of its own afterwards overwrites
      // them in the ticket ring — see in_reach in carve_stream_kernel.)
      publish();  // (this configuration's tickets first: the parkers are waiting for them)
      const bool scan_done = scan_w >= lw;
      if ((scan_done || UNI(cc_ld(&SL[SLW_NCAND])) <= STREAM_PRE_NEAR) && need_rows) {
#pragma unroll
        for (uint32_t k = 0; k < 2u; ++k) {
          if (p_ci[k] == PM_NONE) continue;
          const auto cfg_next = cfgbits_all + (size_t)p_ci[k] * bits_stride;
          const uint32_t cap_k = scan_done ? p_max[k] : (p_max[k] < STREAM_PRE_EARLY ? p_max[k] : STREAM_PRE_EARLY);
          const uint32_t win = scan_done ? la : la + 4u * STREAM_PRE_EARLY;
          // (tickets issued and not yet taken up.  Once the parkers have taken this configuration's last, partly filled
          // block their front stands BEHIND the last ticket issued — t_front counts whole blocks — and the difference
          // wraps: nothing outstanding then, not four billion)
          auto outst = [&]() -> uint32_t { return t_req - t_front < 0x80000000u ? t_req - t_front : 0u; };
          while (outst() < win && p_cnt[k] < cap_k && p_w[k] < lw) {
            // 64 words a look (three reads of HBM-resident bitmaps: not one look per word), their tickets from registers
            const uint32_t jb = p_w[k], j = jb + lane;
            unsigned long long ll = 0ull;
            if (j < lw) ll = ((master[j] & ~cfg_this[j]) | A64[j]) & cfg_next[j] & LOC64[j];
            if (lane == 0u) ll &= ((unsigned long long)p_hi[k] << 32) | p_lo[k];
            uint64_t nz = __ballot(ll != 0ull);
            uint32_t nw = jb + 64u, nlo = 0xFFFFFFFFu, nhi = 0xFFFFFFFFu;  // where the scan stands behind this look
            while (nz) {
              const uint32_t src = (uint32_t)__builtin_ctzll(nz), wj = jb + src;
              const uint64_t w = readlane_u64(ll, src);
              uint32_t room = outst() < win ? win - outst() : 0u;
              room = room < cap_k - p_cnt[k] ? room : cap_k - p_cnt[k];
              if (room == 0u) {  // (its candidates as of now are the ones still to get a ticket)
                nw = wj;
                nlo = (uint32_t)w;
                nhi = (uint32_t)(w >> 32);
                break;
              }
              if (p_cnt[k] == 0u) p_t0[k] = t_req;
              const uint32_t t_before = t_req;
              const uint64_t rest = hand_out(w, wj, room, p_pay[k]);
              p_cnt[k] += t_req - t_before;
              if (rest) {
                nw = wj;
                nlo = (uint32_t)rest;
                nhi = (uint32_t)(rest >> 32);
                break;
              }
              nz &= nz - 1ull;
            }
            p_w[k] = nw;
            p_lo[k] = nlo;
            p_hi[k] = nhi;
          }
        }
      }
      publish();
      if (t_req != before && lane == 0u) STREAM_TRACE(4, t_req, before);
      if (t_req == before) {  // nothing to hand out right now
        __builtin_amdgcn_s_sleep(STREAM_NAP_TICKETER);
        if (++idle > CHAIN_SPIN_LIMIT || cc_ld(&L.CC[CC_ABORT])) {
          cc_st(&L.CC[CC_ABORT], 1u);
          break;
        }
      } else {
        idle = 0u;
      }
    }
    cmd = chain_wait_cmd(L, seen);
    if (cmd == 0u) break;
    seen = cmd;
    save();  // (before the acknowledgement: carve_fast_steps reads the ticket count)
    if ((cmd & 3u) == CH_QUIT) return;
    cc_st(&SL[SLW_ACKT], cmd);  // STOP
  }
  save();
}

template <bool BIG>
__device__ __noinline__ void stream_park(const CarveArgs& p, const StepCtx& c, uint64_t* l_alive, uint32_t* l_buf,
                                         uint32_t* sl_words, uint32_t pi) {
  // (blocks of sixteen tickets: most tickets of a configuration of large groups are dead at their turn — a block of
  // eight yielded three entries, and four parkers at a block per 3.5 us fed the chain no faster than it ate)
  constexpr uint32_t NB = STREAM_PARK_NB, R = CHAIN_RING;
  static_assert(NB <= 32u && R >= 2u * NB && (R & (R - 1u)) == 0u, "a block's entries fit the ring twice over");
  constexpr uint32_t SB = BIG ? PM_CARVE_SLOT_BITS_BIG : PM_CARVE_SLOT_BITS;
  const uint32_t lane = threadIdx.x & 63u;
  chain_lds_u32* const A = lds_pin<chain_lds_u32*>(l_alive);
  chain_lds_u32* const SL = lds_pin<chain_lds_u32*>(sl_words);
  const ChainLds L = chain_lds(l_buf);
  const uint32_t a_base = (uint32_t)(uintptr_t)A;
  const auto row_lo = G((const unsigned long long*)p.stream_row_lo);
  const uint32_t tag0 = UNI(p.stream_tag0);
  const bool need_rows = UNI(c.max_s) > 1u;
  const uint32_t this_ci = (UNI(cc_ld(&SL[SLW_PAY])) >> 18) & 63u;
  // (rows that do not arrive mean the proposers are not running beside this workgroup — a GPU shared with other work:
  // after a few of them stop waiting long)
  const uint32_t spin_rows = UNI(cc_ld(&SL[SLW_TIMEOUTS])) > 8u ? 64u
                             : UNI(p.stream_row_spins) ? UNI(p.stream_row_spins) : PM_STREAM_ROW_SPINS;
  uint32_t timeouts = 0u;
  uint32_t seen = 0u;
  SP_DECL;
  for (;;) {
    uint32_t cmd = chain_wait_cmd(L, seen);
    SP_MARK(pt_idle);
    if (cmd == 0u) break;
    seen = cmd;
    if ((cmd & 3u) == CH_QUIT) break;
    if ((cmd & 3u) != CH_RUN) {
      cc_st(&SL[SLW_ACKP0 + pi], cmd);
      continue;
    }
    const uint32_t t0_run = UNI(cc_ld(&L.CC[CC_START]));
    bool stopped = false;
    for (uint32_t b = pi;; b += STREAM_NPARK) {
      const uint32_t q0 = b * NB, t0 = t0_run + q0;
      // ---- the block's tickets: all eight issued, or the configuration's tickets complete (the rest is void)
      uint32_t n_real = 0u;
      for (uint32_t sp_n = 0u;;) {
        const uint32_t t_end = UNI(cc_ld(&SL[SLW_TEND])), t_lim = UNI(cc_ld(&SL[SLW_TREQ]));  // (the end first: it is set behind the count)
        if (t_end != PM_NONE) {
          n_real = t_end > t0 ? (t_end - t0 < NB ? t_end - t0 : NB) : 0u;
          // (n_real == 0: the run ended in front of this block — it still takes its turn, to say where)
          break;
        }
        if (t_lim >= t0 + NB && t_lim - t0 < 0x80000000u) {
          n_real = NB;
          break;
        }
        __builtin_amdgcn_s_sleep(STREAM_NAP_PARK);
        if (cc_ld(&L.CC[CC_CMD]) != seen) {
          stopped = true;
          break;
        }
        if (++sp_n > CHAIN_SPIN_LIMIT || cc_ld(&L.CC[CC_ABORT])) {
          cc_st(&L.CC[CC_ABORT], 1u);
          stopped = true;
          break;
        }
      }
      if (stopped) break;
      SP_MARK(pt_tick);
      PM_PROF(const uint64_t rw0 = PM_TICKS();)
      // ---- the seeds (lane k: ticket t0 + k) and the rows of the ones that are alive (lane = granule of the row)
      // (a ticket of another configuration, issued ahead of its turn, is not this run's business)
      const uint32_t tp_k = lane < n_real ? cc_ld(&SL[(t0 + lane) & (PM_STREAM_TP - 1u)]) : 0u;
      const bool mine_k = lane < n_real && (tp_k >> 18) == this_ci;
      const uint32_t pos_k = mine_k ? tp_k & 0x3FFFFu : 0u;
      const uint32_t w_k = A[pos_k >> 5];
      uint32_t live_m = (uint32_t)__ballot(mine_k && ((w_k >> (pos_k & 31u)) & 1u) != 0u);
      uint32_t n_live = (uint32_t)__builtin_popcount(live_m);
      unsigned long long prow[NB];
#pragma unroll
      for (uint32_t k = 0; k < NB; ++k)
        prow[k] = (need_rows && ((live_m >> k) & 1u)) ? ld_ag(&row_lo[(size_t)((t0 + k) & (PM_STREAM_RQ - 1u)) * 64u + lane]) : 0ull;
      SP_COUNT(pn_rows, n_live);
      PARK_REC_OPEN(t0, live_m, n_real);  // the block's record: which tickets' rows were asked for, and when
      // one row -> its ring entry q (digested: per lane the LDS address of the entry's bitmap word and its bit), stamped
      auto park_one = [&](uint32_t k, unsigned long long row, uint32_t q) {
        const uint32_t v = (uint32_t)row;  // granule 0: the flags word; granule g: the low half of entry g - 1's key
        const uint32_t meta = UNI(v);
        const uint32_t sp = (uint32_t)__builtin_amdgcn_readlane((int)pos_k, (int)k);
        const uint32_t e = lane == 0u ? sp : (v & ((1u << SB) - 1u));
        const uint32_t r = q & (R - 1u), o = r * 64u + lane;
        // (bits 16..23: the row's last valid lane — what the chain needs to rebuild a flagged row's bits from RE)
        const uint32_t m2 = (((meta & PM_ROW_CLEAN) && (meta & PM_ROW_SAFE)) ? 1u : 0u) |
                            ((meta & (PM_ROW_COMPLETE | PM_ROW_TAIL_CLEAR | PM_ROW_TAIL_OK)) ? 2u : 0u) | (meta & 0xFF00u) | ((meta & 0xFFu) << 16);
        // A row whose flags do not settle the certificate wholesale takes the chain's second look whatever is alive: it is
        // parked with its NEIGHBOURS' bits absent, so the chain's one test — "the seed and group_n - 1 more are alive" — fails
        // for it without a look at the flags (the second look rebuilds the bits from RE).  The high half is the bit's
        // COMPLEMENT: the chain tests with one and-not and kills with ds_and, no v_not in between.
        const bool flagged = need_rows && (m2 & 3u) != 3u;
        const uint32_t bit = (lane <= (meta & 0xFFu) && (lane == 0u || !flagged)) ? 1u << (e & 31u) : 0u;
        L.RAB[o] = ((unsigned long long)(~bit) << 32) | (a_base + ((e >> 5) << 2));
        L.RE[o] = e;
        if (lane == 0u) {
          L.RI[r] = t0 + k;
          L.RM[r] = m2;
          cc_st(&L.RS[r], q + 1u);  // (LDS operations of a wave execute in order: the entry is there before its stamp)
        }
      };
      if (need_rows && live_m) {  // every granule of a row carries the ticket's tag once the row is there
        for (uint32_t sp_r = 0u;;) {
          uint32_t not_ready = 0u;
#pragma unroll
          for (uint32_t k = 0; k < NB; ++k) {
            if ((live_m >> k) & 1u) {
              if (__ballot((uint32_t)(prow[k] >> 32) != tag0 + t0 + k)) {
                not_ready |= 1u << k;
                prow[k] = ld_ag(&row_lo[(size_t)((t0 + k) & (PM_STREAM_RQ - 1u)) * 64u + lane]);
              }
            }
          }
          if (!not_ready) break;
          SP_COUNT(pn_polls, 1u);
          SP_COUNT(pn_late, sp_r == 0u ? (uint32_t)__builtin_popcount(not_ready) : 0u);
          __builtin_amdgcn_s_sleep(STREAM_NAP_PARK);
          if (cc_ld(&L.CC[CC_CMD]) != seen) {
            stopped = true;
            break;
          }
          if (++sp_r > spin_rows) {  // give those rows up: a seed without a row is a step for the exact sweep
#pragma unroll
            for (uint32_t k = 0; k < NB; ++k)
              if ((not_ready >> k) & 1u) {
                STREAM_TIMEOUT_DUMP(t0 + k, prow[k]);  // what was there instead
                prow[k] = 0ull;
                ++timeouts;
              }
            break;
          }
        }
        if (stopped) break;
      }
      SP_MARK(pt_rows);
      PARK_REC_STAMP(2);  // the rows are all there
      PM_PROF(if (lane == 0u) STREAM_TRACE(16, b, (uint32_t)(PM_TICKS() - rw0));)  // (the block's rows: asked for -> all there)
      // ---- who is still alive now that the rows are there (a dead seed takes no ring entry: the later this is looked
      // at, the fewer entries the chain finds dead at their turn)
      {
        const uint32_t w2 = A[pos_k >> 5];
        live_m &= (uint32_t)__ballot(mine_k && ((w2 >> (pos_k & 31u)) & 1u) != 0u);
        n_live = (uint32_t)__builtin_popcount(live_m);
      }
      // ---- this block's turn: its entries go behind those of the blocks in front of it
      uint32_t q_b = 0u;
      for (uint32_t sp_n = 0u;;) {
        if (UNI(cc_ld(&L.CC[CC_CUMSEQ])) == b) {
          q_b = UNI(cc_ld(&L.CC[CC_CUM]));
          break;
        }
        __builtin_amdgcn_s_sleep(STREAM_NAP_TURN);
        if (cc_ld(&L.CC[CC_CMD]) != seen) {
          stopped = true;
          break;
        }
        if (++sp_n > CHAIN_SPIN_LIMIT || cc_ld(&L.CC[CC_ABORT])) {
          cc_st(&L.CC[CC_ABORT], 1u);
          stopped = true;
          break;
        }
      }
      if (stopped) break;
      PARK_REC_STAMP(3);  // the block has its turn
      if (lane == 0u) {
        cc_st(&L.CC[CC_CUM], q_b + n_live);
        if (n_real < NB) cc_st(&L.CC[CC_DONE], q_b + n_live + 1u);  // (the run's last block: its last entry is known)
        cc_st(&L.CC[CC_CUMSEQ], b + 1u);
      }
      SP_MARK(pt_tick);
      // ---- room: everything up to R entries in front of the last one of this block has been released by the collector
      for (uint32_t sp_n = 0u; q_b + n_live - cc_ld(&L.CC[CC_TAIL]) > R && q_b + n_live > cc_ld(&L.CC[CC_TAIL]);) {
        __builtin_amdgcn_s_sleep(STREAM_NAP_TURN);
        if (cc_ld(&L.CC[CC_CMD]) != seen) {
          stopped = true;
          break;
        }
        if (++sp_n > CHAIN_SPIN_LIMIT) {
          cc_st(&L.CC[CC_ABORT], 1u);
          stopped = true;
          break;
        }
      }
      if (stopped) break;
      PARK_REC_STAMP(4);  // it has room
      SP_MARK(pt_room);
      // ---- park the live ones
#pragma unroll
      for (uint32_t k = 0; k < NB; ++k)
        if ((live_m >> k) & 1u) park_one(k, prow[k], q_b + (uint32_t)__builtin_popcount(live_m & ((1u << k) - 1u)));
      SP_MARK(pt_write);
      if (lane == 0u) STREAM_TRACE_NOT_REC(5, b, q_b | (n_live << 24));  // (the PM_ROW_REC build has the record's last words instead)
      PARK_REC_CLOSE(q_b, live_m, b);  // it is parked: when, where and which
      if (n_real < NB) break;  // the run's last block
    }
    cmd = chain_wait_cmd(L, seen);
    SP_MARK(pt_idle);
    if (cmd == 0u) break;
    seen = cmd;
    if ((cmd & 3u) == CH_QUIT) break;
    cc_st(&SL[SLW_ACKP0 + pi], cmd);  // STOP
  }
  if (lane == 0u && timeouts) __hip_atomic_fetch_add(&SL[SLW_TIMEOUTS], timeouts, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  SP_BOOK();
}

// ---- the chain (wave 0 of the validator).  carve_chain's loop, with the ring fed by the parkers: entry q of a run is
// there when RS[q % R] == q + 1, and the run is used up at entry CC_DONE - 1.  seed_cur: the ticket to resume at.
template <bool BIG>
__device__ __noinline__ int stream_chain(const CarveArgs& p, StepCtx& c_ref, uint32_t* l_buf, uint32_t* sl_words,
                                         const uint64_t* l_alive, const uint64_t* l_loc, uint32_t steps_before,
                                         uint32_t& seed_cur, uint32_t& cmd_seq) {
  StepCtx c = c_ref;
  constexpr uint32_t R = CHAIN_RING;
  const uint32_t lane = threadIdx.x & 63u;
  typedef chain_lds_u32 lds_u32;
  const ChainLds L = chain_lds(l_buf);
  chain_lds_u32* const SL = lds_pin<chain_lds_u32*>(sl_words);
  const uint32_t dbg_abort = UNI(p.debug_abort_after);  // (test hook: pm_debug_stream_abort_after)
  const uint32_t n_seeds = PM_NONE;
  const ChainRun run = chain_run(p, c, steps_before);
  const uint32_t group_n = run.group_n, want = group_n - 1u;
  const uint32_t step0 = run.step0, base_cand = run.base_cand;
  uint32_t n_cand = base_cand, commits = 0;
  int action = FAST_SEQ;
  uint32_t exit_cur = n_seeds;  // where carve_fast_steps resumes its search for the first live seed
  const uint32_t lw_bits = (run.n_list + 63u) >> 6;
  uint32_t n_loc = UNI(stream_count_located(l_alive, l_loc, lw_bits, lane));  // located candidates alive (as of the last count)
  // chain_budget, and what only this chain stops for: the abort hook and the hand-over to stream_small
  auto budget_now = [&]() -> uint32_t {
    uint32_t b = chain_budget(run, n_cand, commits);
    if (dbg_abort) {
      const uint32_t r = dbg_abort > step0 + commits ? dbg_abort - (step0 + commits) : 0u;
      b = b < r ? b : r;
    }
    // (the last STREAM_SMALL located candidates of a configuration are carved in registers, stream_small: a commit takes
    // at most group_n of them, so this many commits are safe; the count is taken again when they are used up)
    const uint32_t t = n_loc > STREAM_SMALL_AT ? (n_loc - STREAM_SMALL_AT + group_n - 1u) / group_n : 0u;
    return b < t ? b : t;
  };
  CH_DECL_FINE;

  // ---- start the ticketer, the parkers and the collector: the run begins at ticket T0 — the one to resume at, or
  // behind the last one issued for this configuration when nothing issued so far is of use any more
  uint32_t t0_run = UNI(seed_cur);
  {
    const uint32_t t_lim = UNI(cc_ld(&SL[SLW_TREQ]));
    if (t0_run == PM_NONE || t0_run > t_lim) t0_run = t_lim;
  }
  if (lane < R) cc_st(&L.RS[lane], 0u);  // (stamps of the run before this one)
  if (lane == 0u) {
    cc_st(&L.CC[CC_HEAD], 0u);
    cc_st(&L.CC[CC_CRIT], 0u);
    cc_st(&L.CC[CC_TAIL], 0u);
    cc_st(&L.CC[CC_DONE], 0u);
    cc_st(&L.CC[CC_CUMSEQ], 0u);
    cc_st(&L.CC[CC_CUM], 0u);
    cc_st(&L.CC[CC_START], t0_run);
    cc_st(&L.CC[CC_G0], run.base_groups);
    cc_st(&L.CC[CC_M0], run.base_mem);
  }
  cmd_seq += 4u;
  if (lane == 0u) cc_st(&L.CC[CC_CMD], cmd_seq | CH_RUN);
  if (lane == 0u) STREAM_TRACE(6, t0_run, base_cand);
  uint32_t tail = 0u, budget = 0u;
  bool aborted = false;
  PM_REC(uint32_t rec_batches = UNI(p.stream_ctl[SC_BATCHES]);)  // (the runs of a launch share the region)
  // entries parked from `tail` on, as far as their stamps say (at most the next 16 matter): one LDS read, one ballot
  auto head_now = [&](uint32_t tl) -> uint32_t {
    const uint32_t q = tl + lane;
    const uint64_t there = __ballot(lane < STREAM_BATCH_N && cc_ld(&L.RS[q & (R - 1u)]) == q + 1u);
    return tl + (uint32_t)__builtin_ctzll(~there);
  };
  {
    for (;;) {
      CH_COUNT(cn_outer);
      PM_REC(const uint64_t rec_top = STREAM_CLOCK();)
      tail = UNI(tail);
      // ---- rows parked and not yet looked at
      uint32_t head = head_now(tail);
      if (head == tail) {
        uint32_t sp_n = 0u;
        bool used_up = false;
        if (lane == 0u) STREAM_TRACE(2, tail, commits);
        for (;;) {
          const uint32_t done = UNI(cc_ld(&L.CC[CC_DONE]));  // (the run's last entry + 1, once that is known)
          head = head_now(tail);
          if (head != tail) break;
          if (done && tail + 1u >= done) {
            used_up = true;
            break;
          }
          __builtin_amdgcn_s_sleep(1);
          if (++sp_n > CHAIN_SPIN_LIMIT || UNI(cc_ld(&L.CC[CC_ABORT]))) {
            aborted = true;
            break;
          }
        }
        CH_COUNT(cn_wait);
        if (lane == 0u) STREAM_TRACE(3, head, used_up ? 1u : 0u);
        if (aborted) break;
        if (used_up) {  // the list is used up
          action = FAST_SEQ;
          exit_cur = PM_NONE;
          break;
        }
      }
      CH_MARK(ct_wait);
      uint32_t n_steps = head - tail;
      n_steps = n_steps < STREAM_BATCH_N ? n_steps : STREAM_BATCH_N;
      n_steps = n_steps < R - (tail & (R - 1u)) ? n_steps : R - (tail & (R - 1u));  // (a batch does not wrap around the ring: see rabT)
      bool stop = false;
      // ---- which of these entries' seeds are alive right now: one gather and a ballot.  (A ring of 64 rows is a fifth of
      // a second of commits: between its parking and its turn a good fifth of the seeds has been absorbed by a group —
      // more where the groups are large — and an entry found dead the slow way costs a step like any other.)  The steps
      // below visit the live ones only; a seed that dies DURING the batch is still a step that selects nothing.
      // An entry's word for the collector — the live mask of a committed step, 0 for a step that selected nothing — goes
      // where the entry's row was (lane 0's slot of RAB): the row is in registers by then and nobody else reads it.
      const uint32_t tail0 = tail;
      uint32_t lm;
      {
        const uint32_t qe = (tail0 + lane) & (R - 1u);
        const unsigned long long sab = L.RAB[qe * 64u];  // (lane 0's word of the entry: the seed itself; 0 once marked dead)
        const uint32_t sw = *(lds_u32*)(uintptr_t)(uint32_t)sab;
        const bool al = lane < n_steps && sab != 0ull && (sw & ~(uint32_t)(sab >> 32)) != 0u;
        lm = (uint32_t)__ballot(al);
        if (lane < n_steps && !al) L.RAB[qe * 64u] = 0ull;
        PM_PROF(cn_dead += n_steps - (uint32_t)__builtin_popcount(lm);)
        CHAIN_REC_BATCH(rec_top, tail0, n_steps, __builtin_popcount(lm), step0 + commits);  // the batch's record: its entries seen and looked at
      }
      // ---- the budget, looked at in FRONT of a batch (the steps below do not test it: a batch takes no more entries than
      // the budget has commits left)
      if (lm != 0u && budget == 0u) {
        const uint32_t r0 = (tail0 + (uint32_t)__builtin_ctz(lm)) & (R - 1u);
        tail = tail0 + (uint32_t)__builtin_ctz(lm);  // (where the chain stops if it does: the dead entries in front are done)
        exit_cur = UNI(L.RI[r0]);
        n_cand = base_cand - commits * group_n;
        if (dbg_abort && step0 + commits >= dbg_abort) {  // test hook: the launch gives up here, as a lost hand-shake would
          action = FAST_ABORT;
          stop = true;
        } else {
          n_loc = UNI(stream_count_located(l_alive, l_loc, lw_bits, lane));
          const int why = n_loc <= STREAM_SMALL_AT ? FAST_TINY : chain_stop_reason(run, n_cand, commits);
          if (why != FAST_AGAIN) {
            if (why == FAST_REPROPOSE && lane == 0u) p.status->why[0] += 1u;
            action = why;
            stop = true;
          } else {
            budget = budget_now();
          }
        }
      }
      if (!stop) {
        if (budget != 0u && n_steps > budget) {  // (budget is 0 here only when the whole batch is dead)
          n_steps = budget;
          lm &= (1u << budget) - 1u;  // (budget < n_steps <= 16)
        }
        const uint32_t commits0 = commits;
        CH_MARK(ct_head);  // (the batch's head: parked entries counted, their seeds' liveness, the budget)
        // (an entry's row by its LDS byte address: the address the row is read from is the one the entry's word is written to.
        // rabT: this lane's slot of the batch's FIRST entry — a batch does not wrap around the ring, so entry tail0 + j is
        // 512 j bytes behind it)
        const uint32_t rabT = (uint32_t)(uintptr_t)L.RAB + lane * 8u + ((tail0 & (R - 1u)) << 9);
        uint32_t s = n_steps;  // this entry's offset in the batch
        if (lm != 0u) {
          // ---- the steps.  What a plain step costs was measured alone on a CU (round 6, tools/microbench/chain_step.hip,
          // profiles/r06_chain_step_microbench.txt): a look at the bitmap is 75 cycles, the 37 instructions the run used to be
          // 276 a step, and of those 62 were the five SCALAR instructions of the "does this step need attention" test standing
          // between the vector ones (a scalar instruction that reads what a vector one has just written waits the vector
          // pipeline out, and everything behind it waits with it), 45 the wait for "everything in flight" where only the look
          // was needed — the row after next, asked for behind the collector's word and the counters, came back that much later —
          // and 40 the register rotation, the exec mask set and restored around the kill, and a taken branch a step.  So:
          //   * two steps a trip, the two register sets (current / next row) changing roles instead of being moved;
          //   * the entry after next is found (its offset depends on the batch's live mask only) in the shadow of the look that
          //     is on its way, and its row is asked for right behind the next look; the wait is for the look alone
          //     (lgkmcnt(1): LDS answers in order; the read behind it stays on its way);
          //   * the vector chain — alive? rank among the alive, rank <= want — runs through, the scalar test reads its result
          //     when it is through, and the kill goes to all 64 lanes with all-ones where a lane does not take part (no exec
          //     games: and-ing with all-ones changes nothing; a dead lane that ranks low clears a bit that is clear);
          //   * a step's word for the collector — its live mask — goes into lane `offset` of a register pair (v_writelane) and
          //     the batch's words go out together behind it; a row — address and bit — is ONE read: three LDS operations a step
          //     (the look, the kill, the row after next) where there were five.
          // The run ends when the batch is used up (status 0) or in FRONT of a step that needs attention — fewer than group_n
          // alive, or a seed that died (status 1 / 3: the current entry's row is in the first / the second register set; `a`
          // is its live mask).  sc / sn: the offsets of the current and the next live entry (-1: none); lm: the live entries
          // behind the current one.
          uint32_t ra, nrb, adr, ra_n, nrb_n, adr_n, r, m2, status;
          uint32_t acl = 0u, ach = 0u;  // lane j: entry tail0 + j's word for the collector (0: it selected nothing)
          uint64_t a;
          // prologue: the first live entry becomes the current one, the row behind it is asked for
          uint32_t sc = UNI((uint32_t)__builtin_ctz(lm));
          lm = UNI(lm & (lm - 1u));
          uint32_t sn = UNI(lm ? (uint32_t)__builtin_ctz(lm) : 0xFFFFFFFFu);
          adr = rabT + (sc << 9);
          adr_n = rabT + (sn << 9);  // (no next entry: the row in front of the batch's first — read, never used)
          ra = *(lds_u32*)(uintptr_t)adr;
          nrb = *(lds_u32*)(uintptr_t)(adr + 4u);
          ra_n = *(lds_u32*)(uintptr_t)adr_n;
          nrb_n = *(lds_u32*)(uintptr_t)(adr_n + 4u);
          for (;;) {
            {
              uint32_t w, vt, vk, adr2, st, su, sn2;
              uint64_t sx;
#define PM_CHAIN_STEP(XRA, XNRB, XPAIR, YRA, LBL_ATT, LBL_LAST)                                                             \
                  "s_mov_b32 m0, %[sc]\n\t"                           /* (the lane of this step's word for the collector) */ \
                  "s_bitset0_b32 %[lm], %[sn]\n\t"                    /* lm: the live entries behind the NEXT one */         \
                  "s_ff1_i32_b32 %[sn2], %[lm]\n\t"                   /* the entry after next (-1: none) ... */              \
                  "v_lshl_add_u32 %[adr2], %[sn2], 9, %[rabT]\n\t"    /* ... and its row */                                  \
                  "s_waitcnt lgkmcnt(1)\n\t"                          /* the look is back */                                 \
                  "v_bfi_b32 %[vt], " XNRB ", 0, %[w]\n\t"            /* w & ~nrb: my entry alive? */                        \
                  "v_cmp_ne_u32_e32 vcc, 0, %[vt]\n\t"                /* the live mask */                                    \
                  "s_nop 0\n\t"                                       /* (VCC written by its alias, read by its number below: one wait state — without it the ranks are the step before's) */ \
                  "v_mbcnt_lo_u32_b32 %[vt], vcc_lo, 0\n\t"           /* my rank among the live lanes */                     \
                  "v_mbcnt_hi_u32_b32 %[vt], vcc_hi, %[vt]\n\t"                                                              \
                  "v_cmp_ge_u32_e64 %[sx], %[want], %[vt]\n\t"        /* the seed and its `want` nearest live neighbours */  \
                  "s_bcnt1_i32_b64 %[st], vcc\n\t"                                                                           \
                  "s_bfe_i32 %[su], vcc_lo, 0x10000\n\t"              /* -1 when the seed is alive, else 0: then no count is enough */ \
                  "v_cndmask_b32_e64 %[vk], -1, " XNRB ", %[sx]\n\t"                                                         \
                  "s_and_b32 %[st], %[st], %[su]\n\t"                                                                        \
                  "s_cmp_lt_u32 %[st], %[gn]\n\t"                                                                            \
                  "s_cbranch_scc1 " LBL_ATT "\n\t"                    /* -> needs attention */                               \
                  "ds_and_b32 " XRA ", %[vk]\n\t"                     /* the kill (healthy_nodes.retain, mod.rs:585) */      \
                  "s_cmp_eq_u32 %[sn], -1\n\t"                                                                               \
                  "s_cbranch_scc1 " LBL_LAST "\n\t"                   /* -> that was the batch's last live entry */          \
                  "s_waitcnt lgkmcnt(1)\n\t"                          /* (the next row: asked for a step ago) */             \
                  "ds_read_b32 %[w], " YRA "\n\t"                     /* the NEXT step's look, behind the kill */            \
                  "ds_read_b64 " XPAIR ", %[adr2]\n\t"                /* the row after next — address and bit in one read — into the set the kill has freed */ \
                  "v_writelane_b32 %[acl], vcc_lo, m0\n\t"            /* this step's word for the collector: lane sc of a register */ \
                  "v_writelane_b32 %[ach], vcc_hi, m0\n\t"            /* pair, written out behind the batch */                \
                  "s_add_u32 %[cm], %[cm], 1\n\t"                                                                            \
                  "s_mov_b32 %[sc], %[sn]\n\t"                                                                               \
                  "s_mov_b32 %[sn], %[sn2]\n\t"
              // (the two register sets by their NUMBERS — v20 / v21: address and bit of one row, v22 / v23 of the other — so that a
              // row can be read as the pair it is in LDS and used as its halves: inline assembly has no name for half an operand)
              asm volatile(
                  "ds_read_b32 %[w], v20\n\t"                        // the current step's look at the bitmap
                  "s_waitcnt lgkmcnt(0)\n\t"
                  "1:\n\t"
                  PM_CHAIN_STEP("v20", "v21", "v[20:21]", "v22", "3f", "2f")
                  PM_CHAIN_STEP("v22", "v23", "v[22:23]", "v20", "5f", "6f")
                  "s_branch 1b\n\t"
                  "2:\n\t"
                  "6:\n\t"
                  "v_writelane_b32 %[acl], vcc_lo, m0\n\t"
                  "v_writelane_b32 %[ach], vcc_hi, m0\n\t"
                  "s_add_u32 %[cm], %[cm], 1\n\t"
                  "s_mov_b32 %[status], 0\n\t"
                  "s_branch 4f\n\t"
                  "3:\n\t"
                  "s_mov_b32 %[status], 1\n\t"
                  "s_branch 4f\n\t"
                  "5:\n\t"
                  "s_mov_b32 %[status], 3\n\t"
                  "4:\n\t"
                  "s_mov_b64 %[a], vcc\n\t"
                  "s_waitcnt lgkmcnt(0)"
                  : [w] "=&v"(w), [vt] "=&v"(vt), [vk] "=&v"(vk), [adr2] "=&v"(adr2), [acl] "+v"(acl), [ach] "+v"(ach), [st] "=&s"(st), [su] "=&s"(su),
                    [sx] "=&s"(sx), [sn2] "=&s"(sn2), [a] "=&s"(a), [status] "=&s"(status), "+{v20}"(ra), "+{v21}"(nrb), "+{v22}"(ra_n),
                    "+{v23}"(nrb_n), [lm] "+s"(lm), [sc] "+s"(sc), [sn] "+s"(sn), [cm] "+s"(commits)
                  : [gn] "s"(group_n), [want] "s"(want), [rabT] "v"(rabT)
                  : "vcc", "scc", "m0", "memory");
              // (m0 — v_writelane's lane select beside an SGPR operand has to be m0 — is a register the compiler reserves and says so in
              // a note; nothing else in this code object reads or writes it: tools/kernel_resources.sh's disassembly, grep m0)
#undef PM_CHAIN_STEP
              static_assert(R == 64u && STREAM_BATCH_N <= 31u, "the run's ring arithmetic (512 bytes an entry, a batch inside the ring; bit 31 of the live mask stays free)");
            }
            s = sc;
            if (status == 0u) break;  // the batch is used up
            CH_MARK(ct_plain);
            CH_COUNT(cn_att);
            if (status == 3u) {  // (the current entry's row is in the second set: the sets change names)
              uint32_t t_;
              t_ = ra, ra = ra_n, ra_n = t_;
              t_ = nrb, nrb = nrb_n, nrb_n = t_;
            }
            // (here: lm — the live entries behind the NEXT one; sn — the next one's offset, -1: none)
            r = (tail0 + s) & (R - 1u);
            if ((a & 1ull) == 0ull) {  // the seed is dead at its turn: a step that selects nothing (its word stays 0)
              PM_PROF(cn_dead += 1u;)
            } else {
              // ---- a live seed that needs a second look
              m2 = UNI(L.RM[r]);
              if (want != 0u && (m2 & 3u) != 3u) {  // parked without its neighbours' bits: here they are
                const uint32_t e = L.RE[r * 64u + lane];
                ra = (uint32_t)(uintptr_t)lds_pin<lds_u32*>(const_cast<uint64_t*>(l_alive)) + ((e >> 5) << 2);
                nrb = lane <= ((m2 >> 16) & 0xFFu) ? ~(1u << (e & 31u)) : ~0u;
                const uint32_t w2 = *(lds_u32*)(uintptr_t)ra;
                a = __ballot((w2 & ~nrb) != 0u);
              }
              const uint32_t rk = __builtin_amdgcn_mbcnt_hi((uint32_t)(a >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)a, 0u));
              const uint64_t selm = a & __ballot(rk <= want);
              // enough live entries, and a row whose flags settle the certificate: no two entries near each other at
              // different sites, nothing near the antipode, and a tail that is complete / clear / at one site — or a
              // selection that ends in front of the tail's band
              bool ok = (uint32_t)__popcll(selm) == group_n;
              if (want != 0u && (m2 & 3u) != 3u)
                ok = ok && (m2 & 1u) && 62u - (uint32_t)__builtin_clzll(selm | 2ull) < ((m2 >> 8) & 0xFFu);
              if (!ok) {
                exit_cur = UNI(L.RI[r]);
                // (a row that has run out of live entries is known for what it is right here — the parked row lists every
                // entry of the row in HBM, and what is alive is what carve_fast_steps would find alive: no second look at
                // the row through memory to learn the same)
                action = ((uint32_t)__popcll(a) < group_n && UNI(c.mode) != CARVE_MODE_MERGE) ? FAST_RANOUT : FAST_SLOW;  // (merge: an exact step's business)
                stop = true;  // (s: this entry — the chain stops in front of it)
                CH_MARK(ct_att);
                break;
              }
              if ((selm >> lane) & 1ull)
                __hip_atomic_fetch_and((lds_u32*)(uintptr_t)ra, nrb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              acl = lane == s ? (uint32_t)a : acl;
              ach = lane == s ? (uint32_t)(a >> 32) : ach;
              commits += 1u;
            }
            CH_MARK(ct_att);
            if (sn == 0xFFFFFFFFu) break;
            // the next live entry becomes the current one, the one behind it — the first of lm, which the run takes out itself — the next
            sc = UNI(sn);
            ra = ra_n;
            nrb = nrb_n;
            lm = UNI(lm);
            sn = UNI(lm ? (uint32_t)__builtin_ctz(lm) : 0xFFFFFFFFu);
            adr_n = rabT + (sn << 9);
            ra_n = *(lds_u32*)(uintptr_t)adr_n;
            nrb_n = *(lds_u32*)(uintptr_t)(adr_n + 4u);
          }
          // the words of the entries that are through, for the collector (lane j: entry tail0 + j's, into its row's first slot)
          if (lane < (stop ? s : n_steps))
            *(chain_lds_u64*)(uintptr_t)(rabT - lane * 8u + (lane << 9)) = ((unsigned long long)ach << 32) | acl;
          CH_MARK(ct_plain);
        }
        tail = tail0 + (stop ? s : n_steps);
        budget -= commits - commits0;
        n_cand = base_cand - commits * group_n;
      }
      CHAIN_REC_BATCH_END();  // ... and the clock behind its steps
      if (lane == 0u) {
        cc_st(&L.CC[CC_CRIT], tail);  // for the collector
        cc_st(&SL[SLW_NCAND], n_cand);  // for the ticketer: its window follows what is left
      }
      CH_MARK(ct_steps);
      if (stop) break;
    }
  }
  // ---- stop the other two (they must be off the key array before it is used again; the collector writes out first)
  cmd_seq += 4u;
  if (lane == 0u) cc_st(&L.CC[CC_CMD], cmd_seq | CH_STOP);
  STREAM_TRACE_ACKS(L, SL, cmd_seq | CH_STOP);  // when each of the seven acknowledges
  {
    uint32_t sp_n = 0u;
    const uint32_t want_ack = cmd_seq | CH_STOP;
    while (UNI(cc_ld(&L.CC[CC_ACK2])) != want_ack || UNI(cc_ld(&SL[SLW_ACKT])) != want_ack ||
           UNI(cc_ld(&SL[SLW_ACKP0])) != want_ack || UNI(cc_ld(&SL[SLW_ACKP0 + 1u])) != want_ack ||
           UNI(cc_ld(&SL[SLW_ACKP0 + 2u])) != want_ack || UNI(cc_ld(&SL[SLW_ACKP0 + 3u])) != want_ack ||
           (STREAM_NPARK > 4u && UNI(cc_ld(&SL[SLW_ACKP0 + 4u])) != want_ack)) {
      __builtin_amdgcn_s_sleep(1);
      if (++sp_n > CHAIN_SPIN_LIMIT || UNI(cc_ld(&L.CC[CC_ABORT]))) {
        aborted = true;
        break;
      }
    }
  }
  CH_MARK(ct_stop);
  if (aborted) {
    if (lane == 0u) cc_st(&L.CC[CC_ABORT], 1u);
    action = FAST_ABORT;  // a hand-shake inside the workgroup timed out: reported as CARVE_STATE_ABORTED (never seen)
  }
  chain_book(c, run, commits, n_cand);
  CH_BOOK(CH_FINE_WORDS);
  PM_REC(if (lane == 0u) p.stream_ctl[SC_BATCHES] = rec_batches;)
  if (lane == 0u) STREAM_TRACE(7, action, commits);
  c_ref = c;
  seed_cur = exit_cur;
  return action;
}


// The positions of the set bits of the candidate bitmap, ascending, into `cl` (LDS); returns how many.  The whole workgroup.
#define STREAM_SPARSE_MAX 2048u
#define STREAM_TAIL_MAX 8192u  // candidates a first-come tail may hold to be drained in one go
static_assert(3u * STREAM_SPARSE_MAX <= PM_CARVE_SLOTS * 2u, "keys and positions of a sparse exact step fit the key array's LDS");
__device__ __noinline__ uint32_t stream_compact_candidates(BlockRed& red, const uint64_t* l_alive_, uint32_t lw, uint32_t* cl_,
                                                           const uint64_t* l_and_ = nullptr, uint32_t place_max = 0xFFFFFFFFu) {
  // (LDS, said so: through a generic pointer every access is a FLAT one, waited for on both counters)
  typedef __attribute__((address_space(3))) uint64_t lds_u64;
  typedef __attribute__((address_space(3))) uint32_t lds_u32;
  const lds_u64* const l_alive = lds_pin<const lds_u64*>(l_alive_);
  const lds_u64* const l_and = l_and_ ? lds_pin<const lds_u64*>(l_and_) : nullptr;
  lds_u32* const cl = lds_pin<lds_u32*>(cl_);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t wpw = (lw + CARVE_WAVES - 1u) / CARVE_WAVES;
  const uint32_t j0 = wave * wpw, j1 = min(lw, j0 + wpw);
  uint32_t cnt = 0;
  for (uint32_t j = j0 + lane; j < j1; j += 64u) cnt += (uint32_t)__popcll(l_alive[j] & (l_and ? l_and[j] : ~0ull));
  cnt = wave_sum(cnt);
  __syncthreads();
  if (lane == 0) red.a[wave] = cnt;
  __syncthreads();
  uint32_t off = 0, total = 0;
  for (uint32_t k = 0; k < CARVE_WAVES; ++k) {
    off += k < wave ? red.a[k] : 0u;
    total += red.a[k];
  }
  if (total > place_max) {  // (only the count was wanted: more than the caller has a use for as a list)
    __syncthreads();
    return total;
  }
  for (uint32_t jb = j0; jb < j1; jb += 64u) {
    const uint32_t j = jb + lane;
    uint64_t w = j < j1 ? (l_alive[j] & (l_and ? l_and[j] : ~0ull)) : 0ull;
    const uint32_t cw = (uint32_t)__popcll(w);
    const uint32_t incl = wave_incl_scan_u32(cw);
    uint32_t o = off + incl - cw;
    for (; w; w &= w - 1ull)
      if (o < STREAM_SPARSE_MAX) cl[o++] = j * 64u + (uint32_t)__builtin_ctzll(w);
    off += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
  }
  __syncthreads();
  return total < STREAM_SPARSE_MAX ? total : STREAM_SPARSE_MAX;
}

// The first-come tail of a configuration (no located candidate left, or proximity off): the groups are the remaining
// candidates in input order, max at a time, as long as at least min are left (mod.rs:507, 517-519, 545-561) — nothing
// depends on anything, so the whole workgroup writes them at once instead of a wave walking the bitmap group by group.
// Returns FAST_DONE, FAST_OVERFLOW, or FAST_AGAIN when the tail is longer than STREAM_TAIL_MAX (the serial drain).
__device__ __noinline__ int stream_first_come(const CarveArgs& p, BlockRed& red, StepCtx& c, uint64_t* l_alive_, uint32_t* cl_,
                                              const uint64_t* l_loc_ = nullptr) {
  typedef __attribute__((address_space(3))) uint64_t lds_u64;
  typedef __attribute__((address_space(3))) uint32_t lds_u32;
  lds_u64* const l_alive = lds_pin<lds_u64*>(l_alive_);  // (LDS, said so: see stream_compact_candidates)
  lds_u32* const cl = lds_pin<lds_u32*>(cl_);
  const uint32_t tid = threadIdx.x;
  // (everything this needs from the argument block and the step context is asked for HERE, in one go, and waited for
  // once: left to their uses, each read is a round trip to L2 of its own between two barriers — and a wait for the
  // member stores of the step before on top)
  const uint32_t n_cand0 = UNI(c.n_cand), n_list0 = UNI(c.n_list), max_s = UNI(c.max_s), min_s = UNI(c.min_s);
  const uint32_t g0 = UNI(c.n_groups), m0 = UNI(c.mem_off), cfg_id = UNI(c.cfg);
  const uint32_t cap_g = UNI(p.cap_groups), cap_m = UNI(p.cap_members);
  const auto members = G(p.members);
  const auto freeg = G((unsigned long long*)p.bits_scratch);
  const auto gcfg_g = G(p.g_cfg);
  const auto gn_g = G(p.g_n);
  const auto goff_g = G(p.g_off);
  asm volatile("" ::"v"(members), "v"(freeg), "v"(gcfg_g), "v"(gn_g), "v"(goff_g));
  if (n_cand0 > STREAM_TAIL_MAX) return FAST_AGAIN;
  static_assert(STREAM_TAIL_MAX <= PM_CARVE_SLOTS * 2u, "the tail's positions fit the key array's LDS");
  const uint32_t lw = (n_list0 + 63u) >> 6;
  // (stream_compact_candidates caps at STREAM_SPARSE_MAX: the same compaction with the tail's bound)
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  const uint32_t wpw = (lw + CARVE_WAVES - 1u) / CARVE_WAVES;
  const uint32_t j0 = wave * wpw, j1 = min(lw, j0 + wpw);
  // (l_loc_ given — groups of ONE node with proximity on: the seed is the first located candidate while there is one
  // (mod.rs:526-530) and the group is the seed, so the groups are the located candidates in input order, then the
  // others: the list in two parts)
  const lds_u64* const l_loc = l_loc_ ? lds_pin<const lds_u64*>(l_loc_) : nullptr;
  uint32_t n = 0;
  for (uint32_t part = 0; part < (l_loc ? 2u : 1u); ++part) {
    auto word = [&](uint32_t j) -> uint64_t { return l_alive[j] & (l_loc ? (part == 0u ? l_loc[j] : ~l_loc[j]) : ~0ull); };
    uint32_t cnt = 0;
    for (uint32_t j = j0 + lane; j < j1; j += 64u) cnt += (uint32_t)__popcll(word(j));
    cnt = wave_sum(cnt);
    __syncthreads();
    if (lane == 0) red.a[wave] = cnt;
    __syncthreads();
    uint32_t off = n, n_part = 0;
    for (uint32_t k = 0; k < CARVE_WAVES; ++k) {
      off += k < wave ? red.a[k] : 0u;
      n_part += red.a[k];
    }
    __syncthreads();
    n += n_part;
    if (n > STREAM_TAIL_MAX) return FAST_AGAIN;
    for (uint32_t jb = j0; jb < j1; jb += 64u) {
      const uint32_t j = jb + lane;
      uint64_t w = j < j1 ? word(j) : 0ull;
      const uint32_t cw = (uint32_t)__popcll(w);
      const uint32_t incl = wave_incl_scan_u32(cw);
      uint32_t o = off + incl - cw;
      for (; w; w &= w - 1ull) cl[o++] = j * 64u + (uint32_t)__builtin_ctzll(w);
      off += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
  }
  __syncthreads();
  // how many groups: full ones while max fit, then the rest if it is at least min (and the loop would still be entered)
  uint32_t n_full = n / max_s;
  // (`while total_available >= min`: candidates are a subset of what is available, so n_rem >= min implies it)
  const uint32_t rest = n - n_full * max_s;
  const uint32_t n_groups = n_full + ((rest >= min_s && rest > 0u) ? 1u : 0u);
  const uint32_t taken = rest >= min_s ? n : n_full * max_s;
  if (n_groups == 0u) return FAST_DONE;
  if (g0 + n_groups > cap_g || m0 + taken > cap_m) return FAST_OVERFLOW;
  for (uint32_t i = tid; i < taken; i += CARVE_THREADS) {
    const uint32_t s = cl[i];
    members[m0 + i] = s;  // (positions: carve_finish_kernel turns them into worker ids)
    __hip_atomic_fetch_and(&l_alive[s >> 6], ~(1ull << (s & 63u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_and(&freeg[s >> 6], ~(1ull << (s & 63u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  for (uint32_t g = tid; g < n_groups; g += CARVE_THREADS) {
    gcfg_g[g0 + g] = cfg_id;
    gn_g[g0 + g] = g < n_full ? max_s : rest;
    goff_g[g0 + g] = m0 + g * max_s;
  }
  // sum over the steps of the candidates before each: n, n - max, ...
  c.cand_sum += (unsigned long long)n_groups * n - (unsigned long long)max_s * ((unsigned long long)n_groups * (n_groups - 1u) / 2ull);
  c.n_groups = g0 + n_groups;
  c.mem_off = m0 + taken;
  c.n_cand = n_cand0 - taken;
  c.total_available -= taken;
  c.steps += n_groups;
  c.fast_steps += n_groups;
  __syncthreads();
  return FAST_DONE;
}

// STEP_AGAIN (stream_small_n with two candidates a lane): a wave's worth is left — the caller takes the list afresh and
// finishes on rows
#define STEP_AGAIN 5
// The end of a configuration's located phase in registers: at most STREAM_SMALL LOCATED candidates are left — up to four
// a lane (cl: their positions, ascending) — the location-less ones stay in the bitmap.  Every step is the reference's
// filter + sort + take evaluated as it stands (carve_exact_step's rule, mod.rs:511-561): the seed is the first located
// candidate, its keys in registers, up to `want` rounds of wave-wide argmin; when the located candidates run out before
// the group is full the rest are location-less ones in input order (their distance is f64::MAX: they sort behind every
// located one, ties by position), and then nothing is left to certify.  One wave, no barrier, no row: where neighbour
// rows run out of live entries nothing needs them any more.  Returns STEP_BREAK (configuration exhausted), STEP_CONTINUE
// (no located candidate left, the first-come tail remains), STEP_UNCERTAIN, STEP_OVERFLOW.
template <bool BIG, uint32_t CPL>
__device__ __noinline__ int stream_small_n(const CarveArgs& p, StepCtx& c_ref, uint64_t* l_alive_, const uint64_t* l_loc_,
                                           const uint32_t* cl, uint32_t n_cl, uint32_t steps_before) {
  static_assert(CPL >= 1u && CPL <= STREAM_SMALL_CPL, "candidates a lane");
  typedef __attribute__((address_space(3))) uint64_t lds_u64;
  lds_u64* const l_alive = lds_pin<lds_u64*>(l_alive_);  // (LDS, said so: a generic pointer makes every access a FLAT one)
  const lds_u64* const l_loc = lds_pin<const lds_u64*>(l_loc_);
  StepCtx c = c_ref;
  const uint32_t lane = threadIdx.x & 63u;
  constexpr uint32_t SB = BIG ? PM_CARVE_SLOT_BITS_BIG : PM_CARVE_SLOT_BITS;
  constexpr uint64_t SLOT_MASK = (1ull << SB) - 1ull;
  constexpr double band_rel = BIG ? PM_TIE_BAND_BIG : PM_TIE_BAND;
  // (everything the loop reads from the argument block is read HERE: behind a store the compiler re-reads whatever it
  // cannot prove unaliased, and a read of the argument block is a round trip to L2 in the middle of a selection round)
  const auto freeg = G((unsigned long long*)p.bits_scratch);
  const auto mem_g = G(p.members);
  const auto gcfg_g = G(p.g_cfg);
  const auto gn_g = G(p.g_n);
  const auto goff_g = G(p.g_off);
  const uint32_t cap_g = UNI(p.cap_groups), cap_m = UNI(p.cap_members), dbg_every = UNI(p.debug_uncertain_every);
  ctx_uniform(c);
  const bool prox = UNI(c.proximity) != 0u;
  n_cl = UNI(n_cl);
  steps_before = UNI(steps_before);
  const uint32_t lw = (c.n_list + 63u) >> 6;
  uint32_t s[CPL];
  double lat[CPL], lon[CPL], cs[CPL];
  uint64_t alive[CPL];  // (wave-uniform: candidate lane + 64 j is alive)
#pragma unroll
  for (uint32_t j = 0; j < CPL; ++j) {
    const uint32_t i = lane + 64u * j;
    const bool in = i < n_cl;
    s[j] = in ? cl[i] : 0xFFFFFFFFu;
    const uint32_t sc = in ? s[j] : 0u;
    lat[j] = G(p.cc_lat)[sc];
    lon[j] = G(p.cc_lon)[sc];
    cs[j] = G(p.cc_cos)[sc];
    alive[j] = __ballot(in);
  }
  // (the coordinates are waited for HERE.  Left to their first use inside the loop, the wait sits there as "at most N
  // memory operations outstanding" — and from the second group on what is outstanding are the loop's own stores and
  // atomics: every group then waited a store's round trip to memory, four times what the selection takes.)
#pragma unroll
  for (uint32_t j = 0; j < CPL; ++j) asm volatile("" ::"v"(lat[j]), "v"(lon[j]), "v"(cs[j]), "v"(s[j]));
  uint32_t n_loc = n_cl;  // located candidates alive
  uint32_t uw = 0u;       // first bitmap word that may still hold a live location-less candidate
  int rc = STEP_BREAK;
  if (lane == 0u) STREAM_TRACE(15, n_cl, c.n_cand);
  SM_DECL;
  for (;;) {
    if (!step_open(c)) break;
    if (!(prox && n_loc > 0u)) {  // first-come from here on: the whole workgroup's business
      rc = STEP_CONTINUE;
      break;
    }
    if (n_loc <= 64u) {  // (a wave's worth: the rest on rows, stream_small_rows)
      rc = STEP_AGAIN;
      break;
    }
    const uint32_t want = step_want(c);
    const bool room = step_room(c, want + 1u, cap_g, cap_m);
    // ---- the seed: the first candidate WITH a location
    uint32_t smin = 0xFFFFFFFFu;
#pragma unroll
    for (uint32_t j = 0; j < CPL; ++j) smin = ((alive[j] >> lane) & 1ull) && s[j] < smin ? s[j] : smin;
    const uint32_t seed = wave_min_u32(smin);
    double slat = 0.0, slon = 0.0, scos = 0.0;
#pragma unroll
    for (uint32_t j = 0; j < CPL; ++j) {
      const uint64_t m = __ballot(s[j] == seed);
      if (m) {
        const uint32_t l = (uint32_t)__builtin_ctzll(m);
        slat = __longlong_as_double((long long)readlane_u64((uint64_t)__double_as_longlong(lat[j]), l));
        slon = __longlong_as_double((long long)readlane_u64((uint64_t)__double_as_longlong(lon[j]), l));
        scos = __longlong_as_double((long long)readlane_u64((uint64_t)__double_as_longlong(cs[j]), l));
      }
    }
    SM_MARK(0);
    uint64_t k[CPL], kk[CPL];
#pragma unroll
    for (uint32_t j = 0; j < CPL; ++j) {
      k[j] = ~0ull;
      if (((alive[j] >> lane) & 1ull) && s[j] != seed)
        k[j] = pack_key((uint64_t)__double_as_longlong(hav_a(slat, slon, scos, lat[j], lon[j], cs[j])), s[j], SB);
      kk[j] = k[j];
    }
    SM_MARK(1);
    // ---- the nearest located ones, in key order
    const uint32_t want_loc = want < n_loc - 1u ? want : n_loc - 1u;
    uint64_t last = 0ull;
    uint32_t n_sel = 0u;
    uint64_t selm[CPL];
#pragma unroll
    for (uint32_t j = 0; j < CPL; ++j) selm[j] = 0ull;
    while (n_sel < want_loc) {
      uint64_t mine = kk[0];
#pragma unroll
      for (uint32_t j = 1; j < CPL; ++j) mine = kk[j] < mine ? kk[j] : mine;
      const uint64_t v = wave_min_u64(mine);
      if (v == ~0ull) break;
#pragma unroll
      for (uint32_t j = 0; j < CPL; ++j) {
        const uint64_t m = __ballot(kk[j] == v);
        selm[j] |= m;
        if (kk[j] == v) {
          kk[j] = ~0ull;
          if (room) mem_g[c.mem_off + 1u + n_sel] = (uint32_t)(v & SLOT_MASK);  // (positions: see carve_finish_kernel)
        }
      }
      last = v;
      ++n_sel;
    }
    SM_MARK(2);
    // ---- not enough of them: location-less candidates in input order fill the group (they sort behind every located one)
    const uint32_t n_unl_alive = c.n_cand - n_loc;
    uint32_t need_unl = want - n_sel < n_unl_alive ? want - n_sel : n_unl_alive;
    if (n_sel < want_loc) need_unl = 0u;  // (never: every live located candidate has a key)
    const uint32_t total = 1u + n_sel + need_unl;
    if (total < c.min_s) break;  // mod.rs:564-566
    // ---- exactness certificate for the distance-ordered part (see carve_exact_step): only when the LAST selected
    // candidate has a location — otherwise every located one is in, and nothing is left to decide
    bool uncertain = step_forced(dbg_every, steps_before + c.steps);
    if (n_sel > 0u && need_unl == 0u) {
      const uint64_t last_key = (last >> SB) << SB;
      const double a_m = __longlong_as_double((long long)last_key);
      bool unsafe;
      const double band = cert_band(a_m, band_rel, unsafe);
      const uint32_t last_s = (uint32_t)(last & SLOT_MASK);
      double mlat = 0.0, mlon = 0.0;
#pragma unroll
      for (uint32_t j = 0; j < CPL; ++j) {
        const uint64_t m = __ballot(s[j] == last_s);
        if (m) {
          const uint32_t l = (uint32_t)__builtin_ctzll(m);
          mlat = __longlong_as_double((long long)readlane_u64((uint64_t)__double_as_longlong(lat[j]), l));
          mlon = __longlong_as_double((long long)readlane_u64((uint64_t)__double_as_longlong(lon[j]), l));
        }
      }
      if (unsafe) uncertain = true;
      bool bad = false;
#pragma unroll
      for (uint32_t j = 0; j < CPL; ++j) {
        const uint64_t kb = (k[j] >> SB) << SB;
        const bool near = k[j] != ~0ull && fabs(__longlong_as_double((long long)kb) - a_m) <= band;
        bad = bad || (near && (lat[j] != mlat || lon[j] != mlon));
      }
      if (__ballot(bad)) uncertain = true;
    }
    if (uncertain) {
      rc = STEP_UNCERTAIN;
      break;
    }
    if (!room) {
      rc = STEP_OVERFLOW;
      break;
    }
    SM_MARK(3);
    // ---- commit
#pragma unroll
    for (uint32_t j = 0; j < CPL; ++j) {
      const uint64_t kill = selm[j] | __ballot(s[j] == seed);
      if ((kill >> lane) & 1ull) {
        __hip_atomic_fetch_and(&l_alive[s[j] >> 6], ~(1ull << (s[j] & 63u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_and(&freeg[s[j] >> 6], ~(1ull << (s[j] & 63u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      alive[j] &= ~kill;
    }
    if (need_unl) fill_location_less(l_alive, l_loc, freeg, mem_g, c.mem_off + 1u + n_sel, need_unl, lw, lane, uw);
    if (lane == 0u) {
      mem_g[c.mem_off] = seed;
      step_record(gcfg_g, gn_g, goff_g, c.n_groups, c.cfg, total, c.mem_off);
    }
    n_loc -= 1u + n_sel;
    step_book(c, total);
    c.fast_steps += 1u;  // (not an exact sweep of the workgroup: counted with the steps that came from rows)
    SM_MARK(4);
    PM_PROF(++sm_n;)
  }
  SM_BOOK();
  c_ref = c;
  return rc;
}

// ---- A wave's worth of located candidates or fewer: the chain in miniature (round 5).  stream_small_n pays for every
// group what the streaming carve takes OFF the chain — the seed's keys, `want` rounds of a wave-wide minimum, ≈2 us a
// group on a lone wave — while seven waves of the workgroup wait at a barrier.  Here six of them make sorted neighbour
// rows ahead of wave 0: a candidate's keys to the others (the candidate's index in the key's low bits — the list is
// ascending, so index order is position order), a bitonic network across the lanes, the row and its inverse (where in
// row i candidate c stands) into the idle key array, a bit in a ready mask behind them.  They take the candidates in
// ascending order — the order seeds come in — and pass over the ones wave 0 has killed by then.  A step of wave 0 is
// what a step of the chain is: one LDS read (the seed's row and its inverse), one ballot of who is alive, the first
// `want` live entries, the certificate on the row's keys — and the live mask stays in two scalar registers.  (All the
// rows first, then the steps: 2.3 us per pair of rows in front of every configuration's end — the steps got four
// times cheaper and the match 1 % faster; made on demand the rows are off wave 0's path but for the first.)
//   l_stage words [0, 128): the candidates' positions (stream_compact_candidates); [192, 198): control words;
//   [ROWS_AT, + 8192): 64 rows of 64 keys; behind them 64 x 64 bytes: the inverses.
#define STREAM_ROWS_AT 256u
#define STREAM_ROWS_INV_AT (STREAM_ROWS_AT + 64u * 64u * 2u)
static_assert(STREAM_ROWS_INV_AT + 64u * 64u / 4u <= 3u * CHAIN_RING * 64u, "the rows end in front of the chain's control block");
// control words of the phase (u32 index into l_stage): the next candidate a helper takes, the end of the phase, the rows
// that are there (a 64-bit mask), who is alive as wave 0 sees it (published behind every step)
enum { SRW_NEXT = 192, SRW_QUIT = 193, SRW_READY = 194, SRW_ALIVE = 196 };
static_assert(SRW_ALIVE + 2u <= STREAM_ROWS_AT && STREAM_SMALL <= SRW_NEXT, "the control words lie between the list and the rows");
struct SmallRowGeo {  // a wave's view of the candidates: candidate `lane`'s coordinates
  double lat, lon, cs;
  bool in;
};
// candidate i's row and its inverse -> LDS, its bit in the ready mask behind them (LDS operations of a wave execute in order)
template <bool BIG>
__device__ __forceinline__ void stream_small_make_row(uint32_t* l_stage, const SmallRowGeo& g, uint32_t i, uint32_t lane) {
  typedef __attribute__((address_space(3))) uint64_t lds_u64;
  typedef __attribute__((address_space(3))) unsigned char lds_u8;
  constexpr uint32_t SB = BIG ? PM_CARVE_SLOT_BITS_BIG : PM_CARVE_SLOT_BITS;
  lds_u64* const rows = lds_pin<lds_u64*>(reinterpret_cast<uint64_t*>(l_stage + STREAM_ROWS_AT));
  lds_u8* const inv = lds_pin<lds_u8*>(reinterpret_cast<unsigned char*>(l_stage + STREAM_ROWS_INV_AT));
  lds_u64* const ready = lds_pin<lds_u64*>(reinterpret_cast<uint64_t*>(l_stage + SRW_READY));
  const double slat = __longlong_as_double((long long)readlane_u64((uint64_t)__double_as_longlong(g.lat), i));
  const double slon = __longlong_as_double((long long)readlane_u64((uint64_t)__double_as_longlong(g.lon), i));
  const double scos = __longlong_as_double((long long)readlane_u64((uint64_t)__double_as_longlong(g.cs), i));
  uint64_t w[1] = {(g.in && lane != i) ? pack_key((uint64_t)__double_as_longlong(hav_a(slat, slon, scos, g.lat, g.lon, g.cs)), lane, SB)
                                       : ~0ull};
  const LaneNet ln = lane_net(lane, nullptr);
  net_sort<1u>(w, ln);
  rows[i * 64u + lane] = w[0];
  if (w[0] != ~0ull) inv[i * 64u + ((uint32_t)w[0] & 63u)] = (unsigned char)lane;
  if (lane == 0u) __hip_atomic_fetch_or(ready, 1ull << i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// (the helper waves: candidates in ascending order — the order seeds come in —, the ones that are dead by now passed over:
// a dead candidate is never a seed)
template <bool BIG>
__device__ __forceinline__ void stream_small_rows_help(const CarveArgs& p, uint32_t* l_stage, uint32_t n_cl) {
  typedef __attribute__((address_space(3))) uint64_t lds_u64;
  typedef __attribute__((address_space(3))) uint32_t lds_u32;
  const uint32_t lane = threadIdx.x & 63u;
  const lds_u32* const cl = lds_pin<const lds_u32*>(l_stage);
  lds_u32* const ctl = lds_pin<lds_u32*>(l_stage);
  const lds_u64* const alive_pub = lds_pin<const lds_u64*>(reinterpret_cast<uint64_t*>(l_stage + SRW_ALIVE));
  n_cl = UNI(n_cl);
  SmallRowGeo g;
  g.in = lane < n_cl;
  const uint32_t sc = g.in ? cl[lane] : 0u;
  g.lat = G(p.cc_lat)[sc];
  g.lon = G(p.cc_lon)[sc];
  g.cs = G(p.cc_cos)[sc];
  for (;;) {
    if (UNI(cc_ld(&ctl[SRW_QUIT]))) break;
    uint32_t i = 0u;
    if (lane == 0u) i = __hip_atomic_fetch_add(&ctl[SRW_NEXT], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    i = UNI(i);
    if (i >= n_cl) break;
    // (not too far ahead of wave 0: every step takes max - 1 candidates that are no seeds, and a row made for one of
    // them is a row the next seed waits behind — a candidate's row is made once fewer than STREAM_SMALL_WINDOW live ones
    // stand in front of it.  The lowest live candidate has none in front of it: its row is never waited for in vain.)
    bool dead = false;
    for (uint32_t sp_n = 0u;; ++sp_n) {
      const uint64_t al = __hip_atomic_load(alive_pub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      const uint64_t alu = ((uint64_t)UNI((uint32_t)(al >> 32)) << 32) | UNI((uint32_t)al);
      dead = !((alu >> i) & 1ull);
      if (dead || (uint32_t)__popcll(alu & ((1ull << i) - 1ull)) < STREAM_SMALL_WINDOW) break;
      if (UNI(cc_ld(&ctl[SRW_QUIT])) || sp_n > CHAIN_SPIN_LIMIT) {
        dead = true;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    if (dead) continue;
    stream_small_make_row<BIG>(l_stage, g, i, lane);
  }
}

// (wave 0, behind the barrier.  Statement for statement stream_small_n's loop — the same conditions in the same order,
// the same keys: hav_a of the same arguments, packed with an index that orders like the position — except that the
// selection is read off the seed's row.)
template <bool BIG>
__device__ __noinline__ int stream_small_rows(const CarveArgs& p, StepCtx& c_ref, uint64_t* l_alive_, const uint64_t* l_loc_,
                                              uint32_t* l_stage, uint32_t n_cl, uint32_t steps_before) {
  typedef __attribute__((address_space(3))) uint64_t lds_u64;
  typedef __attribute__((address_space(3))) uint32_t lds_u32;
  typedef __attribute__((address_space(3))) unsigned char lds_u8;
  lds_u64* const l_alive = lds_pin<lds_u64*>(l_alive_);
  const lds_u64* const l_loc = lds_pin<const lds_u64*>(l_loc_);
  const lds_u32* const cl = lds_pin<const lds_u32*>(l_stage);
  const lds_u64* const rows = lds_pin<const lds_u64*>(reinterpret_cast<uint64_t*>(l_stage + STREAM_ROWS_AT));
  const lds_u8* const inv = lds_pin<const lds_u8*>(reinterpret_cast<unsigned char*>(l_stage + STREAM_ROWS_INV_AT));
  StepCtx c = c_ref;
  const uint32_t lane = threadIdx.x & 63u;
  constexpr uint32_t SB = BIG ? PM_CARVE_SLOT_BITS_BIG : PM_CARVE_SLOT_BITS;
  constexpr double band_rel = BIG ? PM_TIE_BAND_BIG : PM_TIE_BAND;
  const auto freeg = G((unsigned long long*)p.bits_scratch);
  const auto mem_g = G(p.members);
  const auto gcfg_g = G(p.g_cfg);
  const auto gn_g = G(p.g_n);
  const auto goff_g = G(p.g_off);
  const uint32_t cap_g = UNI(p.cap_groups), cap_m = UNI(p.cap_members), dbg_every = UNI(p.debug_uncertain_every);
  ctx_uniform(c);
  const bool prox = UNI(c.proximity) != 0u;
  n_cl = UNI(n_cl);
  steps_before = UNI(steps_before);
  const uint32_t lw = (c.n_list + 63u) >> 6;
  const bool in = lane < n_cl;
  const uint32_t s = in ? cl[lane] : 0xFFFFFFFFu;  // candidate `lane`'s position
  const uint32_t sc = in ? s : 0u;
  SmallRowGeo geo;  // (the certificate's rare second look compares coordinates; a row nobody has made yet is made here)
  geo.in = in;
  geo.lat = G(p.cc_lat)[sc];
  geo.lon = G(p.cc_lon)[sc];
  geo.cs = G(p.cc_cos)[sc];
  const double lat = geo.lat, lon = geo.lon;
  asm volatile("" ::"v"(geo.lat), "v"(geo.lon), "v"(geo.cs), "v"(s));  // (waited for here, not behind the loop's own stores: see stream_small_n)
  lds_u32* const ctl = lds_pin<lds_u32*>(l_stage);
  lds_u64* const ready_w = lds_pin<lds_u64*>(reinterpret_cast<uint64_t*>(l_stage + SRW_READY));
  lds_u64* const alive_pub = lds_pin<lds_u64*>(reinterpret_cast<uint64_t*>(l_stage + SRW_ALIVE));
  uint64_t alive = n_cl >= 64u ? ~0ull : ((1ull << n_cl) - 1ull);  // candidate i is alive (wave-uniform)
  uint32_t n_loc = n_cl;
  uint32_t uw = 0u;
  int rc = STEP_BREAK;
  if (lane == 0u) STREAM_TRACE(15, n_cl, c.n_cand);
  PM_PROF(const uint64_t sr_t0 = PM_TICKS(); const uint32_t sr_g0 = c.n_groups;)  // (the steps on rows are booked as selection time)
  for (;;) {
    if (!step_open(c)) break;
    if (!(prox && n_loc > 0u)) {  // first-come from here on: the whole workgroup's business
      rc = STEP_CONTINUE;
      break;
    }
    const uint32_t want = step_want(c);
    const bool room = step_room(c, want + 1u, cap_g, cap_m);
    // ---- the seed: the first candidate WITH a location = the lowest live index; its row
    const uint32_t si = (uint32_t)__builtin_ctzll(alive);
    {  // its row: made by a helper wave a step or two ago — or on its way, or (never seen) by nobody: then here
      uint32_t sp_n = 0u;
      for (;;) {
        const uint64_t rd = __hip_atomic_load(ready_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const uint64_t rdu = ((uint64_t)UNI((uint32_t)(rd >> 32)) << 32) | UNI((uint32_t)rd);
        if ((rdu >> si) & 1ull) break;
        __builtin_amdgcn_s_sleep(1);
        if (++sp_n > 4096u) {
          stream_small_make_row<BIG>(l_stage, geo, si, lane);
          break;
        }
      }
    }
    const uint64_t rk = rows[si * 64u + lane];
    const uint32_t iv = inv[si * 64u + lane];
    const uint32_t seed = (uint32_t)__builtin_amdgcn_readlane((int)s, (int)si);
    const uint32_t idx = (uint32_t)rk & 63u;
    const bool live = rk != ~0ull && ((alive >> idx) & 1ull);
    const uint64_t am = __ballot(live);
    // ---- the nearest located ones, in key order
    const uint32_t want_loc = want < n_loc - 1u ? want : n_loc - 1u;
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(am >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)am, 0u));
    const bool sel = live && rank < want_loc;
    const uint64_t selm = __ballot(sel);
    const uint32_t n_sel = (uint32_t)__popcll(selm);
    if (sel && room) mem_g[c.mem_off + 1u + rank] = cl[idx];  // (positions: see carve_finish_kernel)
    // ---- not enough of them: location-less candidates in input order fill the group (they sort behind every located one)
    const uint32_t n_unl_alive = c.n_cand - n_loc;
    uint32_t need_unl = want - n_sel < n_unl_alive ? want - n_sel : n_unl_alive;
    if (n_sel < want_loc) need_unl = 0u;  // (never: every live located candidate is in the row)
    const uint32_t total = 1u + n_sel + need_unl;
    if (total < c.min_s) break;  // mod.rs:564-566
    // ---- exactness certificate for the distance-ordered part (see carve_exact_step): only when the LAST selected
    // candidate has a location — otherwise every located one is in, and nothing is left to decide
    bool uncertain = step_forced(dbg_every, steps_before + c.steps);
    if (n_sel > 0u && need_unl == 0u) {
      const uint32_t lane_m = 63u - (uint32_t)__builtin_clzll(selm);  // (ascending row: the last selected is the highest)
      const uint64_t last = readlane_u64(rk, lane_m);
      const double a_m = __longlong_as_double((long long)((last >> SB) << SB));
      bool unsafe;
      const double band = cert_band(a_m, band_rel, unsafe);
      if (unsafe) uncertain = true;
      const bool near = live && fabs(__longlong_as_double((long long)((rk >> SB) << SB)) - a_m) <= band;
      if (__ballot(near) & ~(1ull << lane_m)) {  // someone beside it within the band: at its coordinates?
        const uint32_t im = (uint32_t)last & 63u;
        const double mlat = __longlong_as_double((long long)readlane_u64((uint64_t)__double_as_longlong(lat), im));
        const double mlon = __longlong_as_double((long long)readlane_u64((uint64_t)__double_as_longlong(lon), im));
        const uint64_t latb = (uint64_t)__double_as_longlong(lat), lonb = (uint64_t)__double_as_longlong(lon);
        const uint64_t elat = ((uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute((int)(idx << 2), (int)(uint32_t)(latb >> 32)) << 32) |
                              (uint32_t)__builtin_amdgcn_ds_bpermute((int)(idx << 2), (int)(uint32_t)latb);
        const uint64_t elon = ((uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute((int)(idx << 2), (int)(uint32_t)(lonb >> 32)) << 32) |
                              (uint32_t)__builtin_amdgcn_ds_bpermute((int)(idx << 2), (int)(uint32_t)lonb);
        const bool bad = near && (__longlong_as_double((long long)elat) != mlat || __longlong_as_double((long long)elon) != mlon);
        if (__ballot(bad)) uncertain = true;
      }
    }
    if (uncertain) {
      rc = STEP_UNCERTAIN;
      break;
    }
    if (!room) {
      rc = STEP_OVERFLOW;
      break;
    }
    // ---- commit: candidate c goes when its place
    // in the row is among the selected, and the seed
    const uint64_t kill = __ballot(in && lane != si && ((selm >> iv) & 1ull)) | (1ull << si);
    if ((kill >> lane) & 1ull) {
      __hip_atomic_fetch_and(&l_alive[s >> 6], ~(1ull << (s & 63u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_and(&freeg[s >> 6], ~(1ull << (s & 63u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    alive &= ~kill;
    if (lane == 0u) __hip_atomic_store(alive_pub, alive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // (for the helpers)
    if (need_unl) fill_location_less(l_alive, l_loc, freeg, mem_g, c.mem_off + 1u + n_sel, need_unl, lw, lane, uw);
    if (lane == 0u) {
      mem_g[c.mem_off] = seed;
      step_record(gcfg_g, gn_g, goff_g, c.n_groups, c.cfg, total, c.mem_off);
    }
    n_loc -= 1u + n_sel;
    step_book(c, total);
    c.fast_steps += 1u;  // (not an exact sweep of the workgroup: counted with the steps that came from rows)
  }
  if (lane == 0u) cc_st(&ctl[SRW_QUIT], 1u);  // (the helpers leave: on to the caller's barrier)
  SR_BOOK(sr_t0, c.n_groups - sr_g0);
  c_ref = c;
  return rc;
}

// A first-come tail too long for the key array's LDS (more than STREAM_TAIL_MAX candidates): wave 0 walks the bitmap,
// group by group (carve_fast_steps' loop).  The whole workgroup calls; returns STEP_BREAK or STEP_OVERFLOW.
template <bool BIG>
__device__ __noinline__ int stream_tail_serial(const CarveArgs& p, BlockRed& red, StepCtx& c, const uint32_t* l_site,
                                               uint64_t* l_alive, const uint64_t* l_loc, uint32_t steps_before) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (wave == 0) {
    uint32_t dummy = 0u;
    const uint32_t prox = c.proximity;
    c.proximity = 0u;  // (no located candidate is left: straight to the first-come loop, whatever the seed list says)
    const int a2 = carve_fast_steps<BIG, false>(p, c, l_site, l_alive, l_loc, steps_before, dummy, 0xFFFFFFFFu);
    c.proximity = prox;
    if (lane == 0) {
      red.f_action = (uint32_t)a2;
      red.f_n_cand = c.n_cand;
      red.f_total_available = c.total_available;
      red.f_n_groups = c.n_groups;
      red.f_mem_off = c.mem_off;
      red.f_steps = c.steps;
      red.f_fast = c.fast_steps;
      red.f_cand_sum = c.cand_sum;
    }
  }
  lds_barrier();
  const uint32_t a2 = red.f_action;
  c.n_cand = red.f_n_cand;
  c.total_available = red.f_total_available;
  c.n_groups = red.f_n_groups;
  c.mem_off = red.f_mem_off;
  c.steps = red.f_steps;
  c.fast_steps = red.f_fast;
  c.cand_sum = red.f_cand_sum;
  lds_barrier();
  return a2 == FAST_OVERFLOW ? STEP_OVERFLOW : STEP_BREAK;
}

// One configuration of the streaming carve, from its candidate bitmap to "exhausted": the chain with its producer and
// collector, what the chain hands over (carve_fast_steps), exact steps for what no row can serve.
template <bool BIG>
__device__ __noinline__ int stream_run_config(const CarveArgs& p, BlockRed& red, StepCtx& c, const uint32_t* l_site,
                                              uint64_t* l_key, uint64_t* l_alive, const uint64_t* l_loc, uint64_t* part,
                                              uint32_t* sel_out, uint32_t* l_stage, uint32_t* sl_words, uint32_t steps_before,
                                              uint32_t seed_cur0) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const ChainLds CL = chain_lds(l_stage);
  uint32_t seed_cur = seed_cur0;  // the ticket the chain resumes at (PM_NONE: behind the last one issued)
  const bool chain = c.prop_k != 0u;
  const uint32_t lw_all = (c.n_list + 63u) >> 6;
  uint32_t refresh_at = c.steps;  // steps when this configuration's tickets were last issued afresh
  // The merge pass (try_merge_solo_groups, mod.rs:631-971: the candidates are the nodes of the compatible solo groups in
  // group-id order) through the same launch: a group of the seed and its max - 1 nearest LOCATED candidates is what the
  // chain commits in either mode (the rows of a merge list no location-less candidate: stream_drain); everything the
  // modes differ in — too few located candidates (mod.rs:824-848: a group of what there is if that is min, else first
  // come), the end of the list (`n_rem >= min`, mod.rs:695; fewer than two: mod.rs:868-870) — is an exact step's
  // business (carve_exact_step knows both modes), not stream_small's / stream_first_come's / carve_fast_steps'.
  const bool merge = c.mode == CARVE_MODE_MERGE;
  auto exact_step = [&]() -> int {
    // With few candidates left (the tail of a configuration: where rows run out) it runs over their compacted
    // positions, staged with the keys in the (now idle) ring's LDS; else over every position.
    int rc;
    if (c.n_cand <= STREAM_SPARSE_MAX) {
      uint64_t* ck = reinterpret_cast<uint64_t*>(l_stage);                       // [STREAM_SPARSE_MAX] keys
      uint32_t* cl = l_stage + 2u * STREAM_SPARSE_MAX;                            // [STREAM_SPARSE_MAX] positions
      const uint32_t n_cl = stream_compact_candidates(red, l_alive, (c.n_list + 63u) >> 6, cl);
      rc = carve_exact_step<BIG, true>(p, red, c, p.slot_wid, ck, l_alive, l_loc, part, sel_out, steps_before,
                                       (unsigned long long*)p.bits_scratch, cl, n_cl);
    } else {
      rc = carve_exact_step<BIG>(p, red, c, p.slot_wid, l_key, l_alive, l_loc, part, sel_out, steps_before,
                                 (unsigned long long*)p.bits_scratch);
    }
    if (tid == 0) STREAM_TRACE(9, c.n_cand, c.steps);
    return rc;
  };
  // ---- groups of one node (max = 1): nothing to choose, nothing depends on anything — every candidate is a group, the
  // located ones first (the seed is the first located candidate while there is one); the whole workgroup in one go
  if (!merge && c.max_s == 1u && c.proximity && c.n_cand > 0u && c.n_cand <= STREAM_TAIL_MAX && !p.debug_uncertain_every &&
      !p.debug_abort_after) {  // (the test hooks count steps of the chain)
    const int ta = stream_first_come(p, red, c, l_alive, l_stage, l_loc);
    if (tid == 0) STREAM_TRACE(12, (uint32_t)ta, c.steps);
    if (ta == FAST_DONE) return STEP_BREAK;
    if (ta == FAST_OVERFLOW) return STEP_OVERFLOW;
  }
  for (;;) {
    // ---- few enough located candidates are left to finish the located phase in registers (stream_small)?
    uint32_t n_loc_now = 0u;
    // (count and list in one: the positions are placed only when they are few enough for stream_small)
    if (chain && c.proximity && c.n_cand > 0u)
      n_loc_now = stream_compact_candidates(red, l_alive, lw_all, l_stage, l_loc, merge ? 0u : STREAM_SMALL_START);
    if (merge && !(chain && c.proximity && c.n_cand > 0u && n_loc_now > STREAM_SMALL_START)) {
      for (;;) {  // the rest of the list, step by step
        const int rc = exact_step();
        if (rc != STEP_CONTINUE) return rc;
      }
    }
    if (chain && c.proximity && c.n_cand > 0u && n_loc_now <= STREAM_SMALL_START) {
      int rt = STEP_CONTINUE;
      if (n_loc_now > 0u) {
        uint32_t* cl = l_stage;
        const uint32_t n_cl = n_loc_now;
        const bool on_rows = n_cl <= 64u;
        if (on_rows) {  // the phase's control words; then wave 0 carves and six waves make rows ahead of it
          if (tid < 4u) l_stage[SRW_NEXT + tid] = 0u;
          if (tid == 8u)
            *reinterpret_cast<uint64_t*>(l_stage + SRW_ALIVE) = n_cl >= 64u ? ~0ull : ((1ull << n_cl) - 1ull);
          lds_barrier();
          // (wave 4 shares wave 0's SIMD and its issue slots: it stays idle)
          if (wave != 0u && wave != 4u) stream_small_rows_help<BIG>(p, l_stage, n_cl);
        }
        if (wave == 0) {
          const int r0 = on_rows ? stream_small_rows<BIG>(p, c, l_alive, l_loc, l_stage, n_cl, steps_before)
                                 : stream_small_n<BIG, STREAM_SMALL_CPL>(p, c, l_alive, l_loc, cl, n_cl, steps_before);
          if (lane == 0) {
            red.f_action = (uint32_t)r0;
            red.f_n_cand = c.n_cand;
            red.f_total_available = c.total_available;
            red.f_n_groups = c.n_groups;
            red.f_mem_off = c.mem_off;
            red.f_steps = c.steps;
            red.f_fast = c.fast_steps;
            red.f_cand_sum = c.cand_sum;
            STREAM_TRACE(13, (uint32_t)r0, c.steps);
          }
        }
        lds_barrier();
        rt = (int)red.f_action;
        c.n_cand = red.f_n_cand;
        c.total_available = red.f_total_available;
        c.n_groups = red.f_n_groups;
        c.mem_off = red.f_mem_off;
        c.steps = red.f_steps;
        c.fast_steps = red.f_fast;
        c.cand_sum = red.f_cand_sum;
        lds_barrier();
        if (rt == STEP_AGAIN) continue;  // (a wave's worth is left: listed afresh at the top, finished on rows)
        if (rt != STEP_CONTINUE) return rt;
      }
      // no located candidate is left: the first-come tail, in one go
      if (!step_open(c)) return STEP_BREAK;
      const int ta = stream_first_come(p, red, c, l_alive, l_stage);
      if (tid == 0) STREAM_TRACE(12, (uint32_t)ta, c.steps);
      if (ta == FAST_DONE) return STEP_BREAK;
      if (ta == FAST_OVERFLOW) return STEP_OVERFLOW;
      return stream_tail_serial<BIG>(p, red, c, l_site, l_alive, l_loc, steps_before);
    }
    if (chain) {  // the control block of the chain (an exact step in between has used the key array it lives in)
      if (tid < 16u) cc_st(&CL.CC[tid], 0u);
      if (tid >= 16u && tid < 22u) sl_words[SLW_ACKT + (tid - 16u)] = 0u;
      lds_barrier();
    }
    if (wave == 0) {
      PROF_DECL;
      int act = FAST_SEQ;
      uint32_t cmd_seq = 0u;
      for (;;) {
        if (chain) {
          act = stream_chain<BIG>(p, c, l_stage, sl_words, l_alive, l_loc, steps_before, seed_cur, cmd_seq);
          PROF_MARK(0);
          if (act == FAST_OVERFLOW || act == FAST_REPROPOSE || act == FAST_ABORT || act == FAST_TINY || act == FAST_RANOUT) break;
          if (merge) {  // (a step the chain cannot settle: one exact step; the end of its list: exact steps to the end)
            if (act != FAST_SLOW) act = FAST_TAIL;
            break;
          }
        }
        act = carve_fast_steps<BIG, true>(p, c, l_site, l_alive, l_loc, steps_before, seed_cur,
                                          (chain && act == FAST_SLOW) ? 1u : 0xFFFFFFFFu, sl_words);
        if (lane == 0) STREAM_TRACE(10, act, c.steps);
        if (act != FAST_AGAIN) break;
      }
      if (chain && lane == 0) cc_st(&CL.CC[CC_CMD], (cmd_seq + 4u) | CH_QUIT);  // waves 1 and 2 come to the barrier
      if (lane == 0) {
        red.f_action = (uint32_t)act;
        red.f_n_cand = c.n_cand;
        red.f_total_available = c.total_available;
        red.f_n_groups = c.n_groups;
        red.f_mem_off = c.mem_off;
        red.f_steps = c.steps;
        red.f_fast = c.fast_steps;
        red.f_cand_sum = c.cand_sum;
        red._spare1 = seed_cur;
      }
      PROF_MARK(11);
    } else if (wave == 2 && chain) {
      carve_chain_collect<BIG, true>(p, c, l_stage);
    } else if (wave == STREAM_TICKETER_WAVE && chain) {
      stream_ticket<BIG>(p, c, l_alive, l_loc, l_stage, sl_words);
    } else if (chain && (wave == 1 || wave >= 5 || (STREAM_NPARK > 4u && wave == (STREAM_TICKETER_WAVE == 4u ? 3u : 4u)))) {
      // (waves w and w + 4 share a SIMD and its issue slots: the chain's partner, wave 4, stays idle)
      stream_park<BIG>(p, c, l_alive, l_stage, sl_words, wave == 1 ? 0u : wave < 5u ? 4u : wave - 4u);
    }
    lds_barrier();
    const uint32_t act = red.f_action;
    c.n_cand = red.f_n_cand;
    c.total_available = red.f_total_available;
    c.n_groups = red.f_n_groups;
    c.mem_off = red.f_mem_off;
    c.steps = red.f_steps;
    c.fast_steps = red.f_fast;
    c.cand_sum = red.f_cand_sum;
    seed_cur = red._spare1;
    lds_barrier();  // the mailbox is rewritten after the next slow step
    if (act == FAST_TINY) continue;  // (few enough candidates are left to finish in registers: the top of the loop)
    if (act == FAST_TAIL && merge) {
      for (;;) {
        const int rc = exact_step();
        if (rc != STEP_CONTINUE) return rc;
      }
    }
    if (act == FAST_TAIL) {  // no located candidate left: the rest of the configuration in one go
      const int ta = stream_first_come(p, red, c, l_alive, l_stage);
      if (tid == 0) STREAM_TRACE(12, (uint32_t)ta, c.steps);
      if (ta == FAST_DONE) return STEP_BREAK;
      if (ta == FAST_OVERFLOW) return STEP_OVERFLOW;
      return stream_tail_serial<BIG>(p, red, c, l_site, l_alive, l_loc, steps_before);
    }
    if (act == FAST_DONE) return STEP_BREAK;
    if (act == FAST_OVERFLOW) return STEP_OVERFLOW;
    if (act == FAST_ABORT) return STEP_ABORT;
    if (act == FAST_REPROPOSE) {
      // The configuration was entered walking the spatial index and has thinned out below what a walk is good for:
      // from here on its rows come from a sweep of its candidate bitmap (tickets already issued stay as they are).
      if (tid == 0) {
        typedef __attribute__((address_space(3))) uint32_t sl_u32;
        sl_u32* const SL = (sl_u32*)sl_words;
        SL[SLW_PAY] = (SL[SLW_PAY] & 0x00FC0000u) | ((uint32_t)SROW_BITMAP << 24);
        p.status->stream_switches += 1u;
      }
      c.n_start = 0u;  // (no second switch)
      __syncthreads();
      continue;
    }
    if (act == FAST_RANOUT && c.steps - refresh_at >= 8u) {
      // The row of this seed had run out of live entries, and the rows requested along with it are as old (a
      // configuration of up to STREAM_LA_ALL candidates gets all its tickets at once): what has been issued is
      // dropped, and the candidates that are left get new tickets — rows against what is free now, this seed's first.
      // (The batch pipeline's re-proposal, triggered by the evidence instead of a threshold.  No exact step: the seed
      // waits for its new row like the others; only a seed whose FRESH row cannot serve it takes the sweep below.)
      if (tid == 0) {
        typedef __attribute__((address_space(3))) uint32_t sl_u32;
        sl_u32* const SL = (sl_u32*)sl_words;
        SL[SLW_SCANW] = 0u;
        SL[SLW_SCANLO] = SL[SLW_SCANHI] = 0xFFFFFFFFu;
        SL[SLW_TEND] = PM_NONE;
        SL[SLW_TREQ] = SL[SLW_TISSUED];
        SL[SLW_NCAND] = c.n_cand;
        p.status->stream_refreshes += 1u;
        // (the row makers that still work on the tickets dropped here let them be: the new rows find free waves)
        __hip_atomic_store(&p.stream_ctl[SC_DROP], STREAM_DROP_WORD((SL[SLW_PAY] >> 18) & 63u, SL[SLW_TISSUED]), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      }
      seed_cur = PM_NONE;
      refresh_at = c.steps;
      __syncthreads();
      continue;
    }
    // ---- an exact step
    const int rc = exact_step();
    if (rc != STEP_CONTINUE) return rc;
    if (merge && c.steps - refresh_at >= 8u) {
      // (merge: a row that cannot serve its seed is an exact step at once, and its neighbours' rows are as old — every
      // few such steps the candidates that are left get new tickets)
      if (tid == 0) {
        typedef __attribute__((address_space(3))) uint32_t sl_u32;
        sl_u32* const SL = (sl_u32*)sl_words;
        SL[SLW_SCANW] = 0u;
        SL[SLW_SCANLO] = SL[SLW_SCANHI] = 0xFFFFFFFFu;
        SL[SLW_TEND] = PM_NONE;
        SL[SLW_TREQ] = SL[SLW_TISSUED];
        SL[SLW_NCAND] = c.n_cand;
        p.status->stream_refreshes += 1u;
        // (the row makers that still work on the tickets dropped here let them be: the new rows find free waves)
        __hip_atomic_store(&p.stream_ctl[SC_DROP], STREAM_DROP_WORD((SL[SLW_PAY] >> 18) & 63u, SL[SLW_TISSUED]), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      }
      seed_cur = PM_NONE;
      refresh_at = c.steps;
      __syncthreads();
    }
  }
}

// ---- the sweep of a configuration's candidate bitmap (SROW_BITMAP): free & compatible, 64 words a pass — the set
// bits become positions, packed into the wave's LDS buffer, and are evaluated in full strides (a candidate costs what
// a candidate costs; a position that is none costs a sixty-fourth of a popcount)
#define STREAM_WL_WORDS 4608u  // a pass adds up to 4096 positions to at most 511 left over
// (returns true when the ticket was dropped in the meantime — SC_DROP, asked once per batch, the answer read behind the
// batch's evaluation: the row is let be)
// (PM_ROWB: what carve_row_bench_kernel leaves out of a row — 1 the row: the keys are made, the row is not; 2 the key
// arithmetic: a key out of the position; 4 the gathers: every candidate the record of position `lane`; 8 everything but the
// passes over the bitmap.  false in every build but the row bench's.)
__device__ __forceinline__ bool stream_drain(const CarveArgs& p, const uint32_t* wl, uint32_t nb, uint32_t lane, uint32_t s, bool shared,
                                             uint32_t ssite, const SeedGeo& sg, uint32_t SB, uint64_t ulps, NearRow& q, uint32_t& n_mine,
                                             BulkCtx& bulk, uint32_t ci, uint32_t ticket) {
  // two batches of four strides: the next batch's gathers are in flight while this one is evaluated.  A candidate is
  // ONE 32-byte record (c_pack: unit vector, site, located bit) — one memory line per candidate where the separate
  // columns were five, and a row is a chain of exactly these gathers
  const double* const pack = p.c_pack;
  const bool located_only = UNI(p.mode) == CARVE_MODE_MERGE;  // (read here, once: not inside the strides)
  const bool form = !located_only;  // (FORM: no located candidate in front of the seed can be alive at its turn, see tile_keys)
  // The next batch's gathers are in flight while this one is evaluated; the evaluation stands in ONE place (it has the
  // sorting networks inline) and the batches change places in registers.
  struct Batch {
    uint32_t t[4];
    pm_d4 rec[4];
  };
  auto fetch = [&](Batch& bt, uint32_t k0) {
#pragma unroll
    for (uint32_t v = 0; v < 4u; ++v) {
      const uint32_t k = k0 + v * 64u + lane;
      const uint32_t tc = wl[k < nb ? k : 0u];
      bt.t[v] = k < nb ? tc : 0xFFFFFFFFu;
      bt.rec[v] = pack_load(pack, PM_ROWB(4u) ? lane : tc);
    }
  };
  auto eval = [&](const Batch& bt, uint32_t n_in_batch) {
    // the four strides' keys first (one copy of the key arithmetic), then the row: its first candidates go through the
    // networks four strides at once (near_row_offer_bulk), the later ones — few of which enter — stride by stride
    uint64_t kk[4];
    uint32_t ss[4];
    const uint32_t n_in = n_in_batch;  // (how many of the batch's 256 places hold a candidate: the caller's arithmetic, not four ballots)
    PM_PROF(const uint64_t ek0 = PM_TICKS();)
#pragma unroll
    for (uint32_t v = 0; v < 4u; ++v) {
      const bool in = bt.t[v] != 0xFFFFFFFFu;
      const uint32_t tv = in ? bt.t[v] : 0u;
      const bool located = pack_located(bt.rec[v]);
      ss[v] = pack_site(bt.rec[v]);
      // (merge pass: the neighbours of a seed are the LOCATED candidates only, mod.rs:792-804)
      const bool counts = in && tv != s && !(located && tv < s && (form || (shared && ss[v] == ssite))) && (located || !located_only);
      kk[v] = PM_ROWB(2u) ? (counts ? (((uint64_t)(tv * 2654435761u) << SB) | tv) : ~0ull)
                          : candidate_key(p, sg, ssite, bt.rec[v].x, bt.rec[v].y, bt.rec[v].z, ss[v], counts ? tv : 0u, located, counts, SB, q);
      n_mine += counts ? 1u : 0u;
    }
    PM_PROF(const uint64_t ek1 = PM_TICKS(); q.p_key_t += ek1 - ek0;)
    PM_REC(if (bulk.rec_keys == 0) bulk.rec_keys = STREAM_CLOCK();)
    if (PM_ROWB(1u)) {
      q.m1 ^= kk[0] ^ kk[1] ^ kk[2] ^ kk[3];
    } else if (UNI(bulk.seen) < STREAM_BULK_UPTO) {
      near_row_offer_bulk<4u, true>(q, kk, ss, p.cc_site, SB, ulps, bulk.ln);
    } else {
#pragma unroll
      for (uint32_t v = 0; v < 4u; ++v) {
        if (v * 64u >= n_in) continue;
        near_row_offer(q, kk[v], ss[v], G(p.cc_site), SB, ulps);
      }
    }
    PM_PROF(q.p_off_t += PM_TICKS() - ek1;)
    bulk.seen += n_in;
  };
  if (nb == 0u) return false;
  if (PM_ROWB(8u)) {
    n_mine += nb / 64u;
    return false;
  }
  const auto drop_w = G(p.stream_ctl) + SC_DROP;
  Batch cur, nxt;
  fetch(cur, 0u);
  for (uint32_t k0 = 0; k0 < nb; k0 += 256u) {
    const bool more = k0 + 256u < nb;
    const uint32_t dropw = ld_ag32(drop_w);
    if (more) fetch(nxt, k0 + 256u);
    DRAIN_PROF_WAIT(more);  // (a measuring build waits for this batch's gathers HERE, to tell the wait from the evaluation)
    eval(cur, nb - k0 < 256u ? nb - k0 : 256u);
    DRAIN_PROF_BOOK(q);
    if (STREAM_DROPPED(UNI(dropw), ci, ticket)) return true;
    if (more) cur = nxt;
  }
  return false;
}
__device__ __forceinline__ bool stream_bitmap_sweep(const CarveArgs& p, const uint64_t* cfg64, uint32_t n, uint32_t* wl, uint32_t lane,
                                                    uint32_t s, bool shared, uint32_t ssite, const SeedGeo& sg, uint32_t SB,
                                                    uint64_t ulps, NearRow& q, uint32_t& n_mine, BulkCtx& bulk, uint32_t ci, uint32_t ticket) {
  const auto freeg = G((const unsigned long long*)p.bits_scratch);
  const auto cfgb = G(cfg64);
  const uint32_t lw = (n + 63u) >> 6;
  uint32_t nb = 0u;
  SWEEP_PROF_DECL;
  // FORM: the located candidates in front of the seed are masked out right here — every one of them is in a group by
  // the seed's turn (a live one would be the seed instead, mod.rs:526-530), so they take no place in the buffer, no
  // gather and no key.  One more load per word up to the seed's; the words behind it are untouched.  (The merge pass
  // keeps its candidates: a merge batch can be refused with its seed still in the list.)
  const auto locg = G((const unsigned long long*)p.loc_g);
  const uint32_t sw = UNI(p.mode) != CARVE_MODE_MERGE ? s >> 6 : 0u;  // words up to here have located positions in front of the seed
  const unsigned long long s_below = UNI(p.mode) != CARVE_MODE_MERGE ? (1ull << (s & 63u)) - 1ull : 0ull;
  auto word = [&](uint32_t j) -> unsigned long long {
    if (j >= lw) return 0ull;
    unsigned long long a = ld_ag(&freeg[j]) & cfgb[j];
    if (j <= sw) a &= ~(locg[j] & (j < sw ? ~0ull : s_below));
    return a;
  };
  unsigned long long a_n = word(lane);  // (the next pass's words, one pass early)
  for (uint32_t j0 = 0; j0 < lw; j0 += 64u) {
    unsigned long long a = a_n;
    a_n = word(j0 + 64u + lane);
    const uint32_t cw = (uint32_t)__popcll(a);
    const uint32_t incl = wave_incl_scan_u32(cw);
    uint32_t o = nb + incl - cw;
    const uint32_t base = (j0 + lane) * 64u;
    for (; a; a &= a - 1ull) wl[o++] = base + (uint32_t)__builtin_ctzll(a);
    nb += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    PM_REC(if (bulk.rec_pass == 0) bulk.rec_pass = STREAM_CLOCK();)
    SWEEP_PROF_MARK(bp_pass, bp_np, 1u);
    if (nb >= 512u || j0 + 64u >= lw) {  // whole batches of 256 while the sweep goes on, everything at its end
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // (the lanes read what other lanes of the wave packed)
      const uint32_t take = j0 + 64u >= lw ? nb : (nb & ~255u);
      if (stream_drain(p, wl, take, lane, s, shared, ssite, sg, SB, ulps, q, n_mine, bulk, ci, ticket)) return true;
      SWEEP_PROF_MARK(bp_drain, bp_nd, (take + 255u) >> 8);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      const uint32_t left = nb - take;  // (< 256: moved to the front)
      uint32_t mv[4];
#pragma unroll
      for (uint32_t v = 0; v < 4u; ++v) mv[v] = v * 64u + lane < left ? wl[take + v * 64u + lane] : 0u;
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
      for (uint32_t v = 0; v < 4u; ++v)
        if (v * 64u + lane < left) wl[v * 64u + lane] = mv[v];
      nb = left;
    }
  }
  SWEEP_PROF_BOOK(q);
  return false;
}

// ---- a proposer workgroup: eight independent waves, each serving one ticket at a time
__device__ __forceinline__ void stream_proposer(const CarveArgs& p, unsigned char* s_raw) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  // A row is a chain of ~6000 dependent instructions, and what the carve waits for is its LATENCY: one wave per SIMD
  // issues twice as fast as two that share it (waves w and w + 4 of a workgroup do), so half the waves leave at once.
  if (wave >= PM_STREAM_PROP_WAVES) return;
  const auto st = G((const CarveStatus*)p.status);
  if (st->state != CARVE_STATE_RUNNING) return;
  const uint32_t n = st->n_eligible;
  if (n == 0u || n > PM_CARVE_BIG_SLOTS) return;
  const uint32_t SB = n > PM_CARVE_SLOTS ? PM_CARVE_SLOT_BITS_BIG : PM_CARVE_SLOT_BITS;
  const double TIE_BAND = n > PM_CARVE_SLOTS ? PM_TIE_BAND_BIG : PM_TIE_BAND;
  const uint64_t WINDOW_ULPS = n > PM_CARVE_SLOTS ? (1ull << 25) : (1ull << 20);
  const uint32_t cell_g = st->cell_g;
  static_assert(STREAM_WL_WORDS >= 2u * CELL_BUF, "the walk's buffer fits the sweep's");
  static_assert(size_t(CARVE_WAVES) * STREAM_WL_WORDS * 4u <= PM_STREAM_LDS_BYTES, "one candidate buffer per wave");
  uint32_t* wl = reinterpret_cast<uint32_t*>(s_raw) + wave * STREAM_WL_WORDS;  // this wave's candidate buffer
  const auto ctl = G(p.stream_ctl);
  const auto sq = G((const unsigned long long*)p.stream_sq);
  const auto row_lo = G(p.stream_row_lo);
  const auto row_hi = G(p.stream_row_hi);
  const uint32_t tag0 = UNI(p.stream_tag0);
  static_assert(size_t(CARVE_WAVES) * STREAM_WL_WORDS * 4u + size_t(CARVE_WAVES) * NET_PACK_KEYS * 8u <= PM_STREAM_LDS_BYTES,
                "a packing list per wave behind the buffers");
  BulkCtx bulk = {0u, lane_net(lane, reinterpret_cast<uint64_t*>(s_raw + size_t(CARVE_WAVES) * STREAM_WL_WORDS * 4u) + wave * NET_PACK_KEYS)};
  for (;;) {
    uint32_t t = 0u;
    if (lane == 0u) t = atomicAdd(&p.stream_ctl[SC_CLAIM], 1u);
    t = UNI(t);
    unsigned long long g;
    // The ticket has not been issued yet: wait for it — polling its own slot only, ever more patiently.  (A thousand
    // waves asking ONE word "is it over?" every microsecond kept the memory channel of that word, and everything else
    // on it, busy: at the end the validator hands every waiting wave a ticket that says so instead.)
    uint32_t nap = 8u;
    for (uint32_t spins = 0u;;) {
      g = ld_ag(&sq[t & (PM_STREAM_SQ - 1u)]);
      if (UNI((uint32_t)(g >> 32)) == tag0 + t) break;
      if ((spins & 255u) == 255u && UNI(ld_ag32(&ctl[SC_QUIT]))) return;  // (a backstop)
      if (nap >= 32u) __builtin_amdgcn_s_sleep(STREAM_NAP_LONG);
      else if (nap >= 16u) __builtin_amdgcn_s_sleep(STREAM_NAP_LONG < 32 ? STREAM_NAP_LONG : 32);
      else __builtin_amdgcn_s_sleep(STREAM_NAP_LONG < 16 ? STREAM_NAP_LONG : 16);
      nap = nap < 32u ? nap << 1 : nap;
      if (++spins > PM_STREAM_IDLE_SPINS) {
        if (lane == 0u) atomicAdd(&p.stream_ctl[SC_GAVE_UP], 1u);
        return;
      }
    }
    if (UNI((uint32_t)g) == 0xFFFFFFFFu) return;  // the carve is over
    const uint64_t t_seen = __builtin_amdgcn_s_memtime();
    PM_PROF(const uint64_t bt0 = t_seen;)
    const uint32_t pay = UNI((uint32_t)g);
    const uint32_t s = pay & 0x3FFFFu, mode = (pay >> 24) & 3u, ci = (pay >> 18) & 63u;
    if (s >= n) continue;  // (never: a ticket names a position)
    if (STREAM_DROPPED(UNI(ld_ag32(&ctl[SC_DROP])), ci, t)) continue;  // a ticket its configuration has no use for any more
    const uint64_t* cfg64 = p.cfgbits + (size_t)ci * p.bits_stride;  // the configuration's compatible positions
    const uint32_t ssite = G(p.cc_site)[s];
    const SeedGeo sg = {G(p.cc_lat)[s], G(p.cc_lon)[s], G(p.cc_cos)[s], G(p.cc_ux)[s], G(p.cc_uy)[s], G(p.cc_uz)[s]};
    const bool shared = (ssite & 0x80000000u) != 0u;
    NearRow q = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull, 0xFFFFFFFFu};
    uint32_t n_mine = 0;
    bulk.seen = 0u;
    PM_REC(bulk.rec_pass = bulk.rec_keys = 0; const uint64_t rec_seen = STREAM_CLOCK();)
    PM_PROF(asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); const uint64_t bt_geo = PM_TICKS();)  // (the seed's own columns are there)
    bool sweep = true;  // (the bitmap sweep stands in one place: it has the sorting networks inline)
    if (mode == SROW_WALK && cell_g) {
      const uint32_t stop_r = p.prune_mode != 3u ? cell_walk<true>(p, wl, cell_g, PM_CELL_RMAX, lane, s, shared, ssite, sg, SB, WINDOW_ULPS, q, n_mine, (const uint32_t*)cfg64, &bulk) : 0u;
      sweep = !stop_r;
      if (sweep) {  // the rings ran out before the row's window closed: every position, the slow way
        q = NearRow{~0ull, ~0ull, ~0ull, ~0ull, ~0ull, 0xFFFFFFFFu};
        n_mine = 0;
        bulk.seen = 0u;
        if (lane == 0) atomicAdd(&p.status->prune_fallbacks, 1u);
      }
    } else if (mode == SROW_SWEEP) {  // (kept as the plain form of the sweep: every position, a stride at a time)
      list_sweep_solo<true>(p, n, lane, s, shared, ssite, sg, SB, WINDOW_ULPS, q, n_mine, cfg64);
      sweep = false;
    }
    if (UNI(sweep) && stream_bitmap_sweep(p, cfg64, n, wl, lane, s, shared, ssite, sg, SB, WINDOW_ULPS, q, n_mine, bulk, ci, t)) {
      if (lane == 0u) atomicAdd(&p.stream_ctl[SC_LET_BE], 1u);
      continue;
    }
    PM_PROF(const uint64_t bt1 = PM_TICKS();)
    PM_REC(const uint64_t rec_swept = STREAM_CLOCK();)
    uint64_t mine;
    const uint32_t meta = near_row_finish(p, q, true, PM_PROP_KMAX, SB, TIE_BAND, lane, &mine);
    PM_REC(const uint64_t rec_fin = STREAM_CLOCK() + (meta & 0u);)  // (behind the flags word)
    if (p.count_keys) {  // bookkeeping for the bench: keys this row evaluated
      const uint32_t swept = wave_sum(n_mine);
      if (lane == 0) {
        atomicAdd((unsigned long long*)&p.status->prop_keys, (unsigned long long)swept);
        atomicAdd(&p.status->n_props, 1u);
      }
    }
    // A row that took long (a walk that gave up and swept a 40,000-candidate configuration: a millisecond and more when
    // the launch is busy) may be a whole ring late: tickets t and t + PM_STREAM_RQ share a row slot, and at 6 tickets per
    // microsecond the ring turns over in 1.3 ms.  Written now it would REPLACE the newer ticket's row — whose parker then
    // waits for a row that was there and is gone, until it times out 10 ms later (what made one 1M x 100k match in four
    // twice as slow with a longer look-ahead).  The ticket ring has the same length: if this ticket's granule has been
    // overwritten, nobody waits for this row any more.
    static_assert(PM_STREAM_SQ == PM_STREAM_RQ, "the ticket ring tells when a row slot has a newer owner");
    if (__builtin_amdgcn_s_memtime() - t_seen > STREAM_LATE_ROW_TICKS) {
      const unsigned long long g2 = ld_ag(&sq[t & (PM_STREAM_SQ - 1u)]);
      if (UNI((uint32_t)(g2 >> 32)) != tag0 + t) continue;
    }
    // the row: granule (lane + 1) & 63 of the ticket's slot in both rings — the high halves first, so that the low
    // halves (what the validator's producer polls) are the last thing to arrive
    const size_t rb = (size_t)(t & (PM_STREAM_RQ - 1u)) * 64u + ((lane + 1u) & 63u);
    const unsigned long long tagw = (unsigned long long)(tag0 + t) << 32;
    st_ag(&row_hi[rb], tagw | (lane == 63u ? 0ull : (unsigned long long)(uint32_t)(mine >> 32)));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    st_ag(&row_lo[rb], tagw | (lane == 63u ? (unsigned long long)meta : (unsigned long long)(uint32_t)mine));
    PROP_REC_ROW(t, mode, n_mine, rec_seen, bulk, rec_swept, rec_fin);  // the row's record: its stamps, how it was made, where
    PROP_PROF_ROW(t, mode, q, n_mine, bt0, bt_geo, bt1);  // what the row cost, by the way it was made
  }
}

// ---- the kernel: workgroup 0 validates, the others propose
__global__ __launch_bounds__(CARVE_THREADS) void carve_stream_kernel(const CarveArgs* __restrict__ pa, uint32_t start_ci) {
  const CarveArgs& p = *pa;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  if (blockIdx.x != 0u) {
    stream_proposer(p, s_raw);
    return;
  }
  uint64_t* part = reinterpret_cast<uint64_t*>(s_raw);                       // [16 * PART]
  uint64_t* lds_alive = part + CARVE_WAVES * PM_CARVE_PART;                  // [SLOTS / 64]
  uint64_t* lds_loc = lds_alive + PM_CARVE_SLOTS / 64;                       // [SLOTS / 64]
  uint32_t* lds_wid = reinterpret_cast<uint32_t*>(lds_loc + PM_CARVE_SLOTS / 64);  // [SLOTS] more than 8192 positions: the candidate bitmap
  uint32_t* lds_site = lds_wid + PM_CARVE_SLOTS;                             // [SLOTS] site ids / more than 8192 positions: the loc bitmap
  uint64_t* lds_key = reinterpret_cast<uint64_t*>(lds_site + PM_CARVE_SLOTS);  // [SLOTS] keys of an exact step / the chain's rings
  uint32_t* sel_out = reinterpret_cast<uint32_t*>(lds_key + PM_CARVE_SLOTS);  // [SEL_CAP]
  BlockRed& red = *reinterpret_cast<BlockRed*>(sel_out + PM_CARVE_SEL_CAP);
  uint32_t* sl_words = reinterpret_cast<uint32_t*>(s_raw + PM_CARVE_LDS_BYTES);  // ticket state (StreamLds words)

  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const auto st = G(p.status);
  const auto ctl = G(p.stream_ctl);
  if (st->state != CARVE_STATE_RUNNING) {
    if (tid == 0) st_ag32(&ctl[SC_QUIT], 1u);
    return;
  }
  const uint32_t n = st->n_eligible;
  const uint32_t lw = (n + 63u) >> 6;
  uint32_t exit_state = CARVE_STATE_DONE, stop_ci = p.n_avail;
  StepCtx c;
  c.mode = p.mode;  // (FORM; MERGE: one configuration, the eligible list supplied — see stream_run_config)
  c.proximity = p.proximity;
  c.use_props = true;
  c.steps = 0;
  c.fast_steps = 0;
  c.cand_sum = 0;
  c.total_available = st->total_available;
  c.n_groups = st->n_groups;
  c.mem_off = st->n_members;
  c.n_list = n;
  c.n_cand = 0;
  c.min_s = c.max_s = 1;
  c.cfg = 0;
  ctx_set_geometry(c);
  const uint32_t groups_at_entry = c.n_groups;
  const uint32_t steps_before = st->steps_total;
  const bool big = c.big;
  uint64_t* r_alive = big ? reinterpret_cast<uint64_t*>(lds_wid) : lds_alive;
  uint64_t* r_loc = big ? reinterpret_cast<uint64_t*>(lds_site) : lds_loc;
  uint32_t ci = start_ci;
  if (n > PM_CARVE_BIG_SLOTS) {  // (the engine sends such swarms through the batch pipeline; never seen)
    exit_state = CARVE_STATE_ABORTED;
    stop_ci = ci;
  } else if (n > 0u) {
    // ---- what stays put for the whole carve: the loc bitmap, the site ids (small swarms), the ticket state
    for (uint32_t j = tid; j < lw; j += CARVE_THREADS) r_loc[j] = G(p.loc_g)[j];
    if (!big)
      for (uint32_t sl = tid; sl < n; sl += CARVE_THREADS) lds_site[sl] = G(p.cc_site)[sl];
    for (uint32_t k = tid; k < (uint32_t)SLW_WORDS; k += CARVE_THREADS) sl_words[k] = (k == SLW_P_CI || k == SLW_P_CI1 || k == SLW_TEND) ? PM_NONE : 0u;
    __syncthreads();
    const auto master = G(p.alive_g);
    const auto cfgbits = G((const uint64_t*)p.cfgbits);
    const uint32_t cell_g = st->cell_g, n_indexed = st->n_indexed;
    // candidates of a configuration as of now: free & compatible, counted by the whole workgroup
    auto count_candidates = [&](uint32_t cx) -> uint32_t {
      uint32_t cnt = 0;
      for (uint32_t j = tid; j < lw; j += CARVE_THREADS) cnt += (uint32_t)__popcll(master[j] & cfgbits[(size_t)cx * p.bits_stride + j]);
      cnt = wave_sum(cnt);
      __syncthreads();
      if (lane == 0) red.a[wave] = cnt;
      __syncthreads();
      uint32_t tot = 0;
#pragma unroll
      for (uint32_t k = 0; k < CARVE_WAVES; ++k) tot += red.a[k];
      __syncthreads();
      return tot;
    };
    // how a configuration's rows are made: a walk over the spatial index while its candidates are many (n^2 >=
    // prune_factor x indexed positions, the batch pipeline's measured crossover), else a sweep of its candidate bitmap
    auto row_mode = [&](uint32_t n_cand, uint32_t* switch_at) -> uint32_t {
      *switch_at = 0u;
      if (!cell_g || !p.prune_mode) return SROW_BITMAP;
      if (p.prune_mode >= 2u) return SROW_WALK;
      if ((uint64_t)n_cand * n_cand < (uint64_t)p.prune_factor * n_indexed) return SROW_BITMAP;
      *switch_at = (uint32_t)sqrt((double)p.prune_factor * (double)n_indexed);
      return SROW_WALK;
    };
    // look-ahead.  What it wastes — rows for seeds that a group absorbs before their turn, about (max - 1) x outstanding
    // tickets / candidates of the rows — is work of CUs with nothing else to do; what it has to do is cover a row's
    // latency (10 - 35 us) at the chain's pace (3 - 4 rows per us).  A configuration of a thousand candidates or so gets
    // all its tickets at once (a row lists 63 neighbours: by the time most of them are gone the configuration is nearly
    // through); a bigger one a window that keeps rows young — the co-located workers of a city share their neighbours,
    // every seed of the city takes max - 1 of them, and a row that has run out of live entries is an exact step.
    auto look_ahead = [&](uint32_t n_cand, uint32_t max_s) -> uint32_t {
      // (re-measured with the faster chain, 896 / 1,024 / 1,150: within the run-to-run noise of one another.  A longer
      // look-ahead had shown one 1M x 100k match in four twice as slow: rows a whole ring late replacing newer ones — see
      // STREAM_LATE_ROW_TICKS in stream_proposer; fixed there, not here.)
      const uint32_t la_max = p.stream_la ? p.stream_la : 896u;
      const uint32_t small = p.stream_la_div ? p.stream_la_div * 256u : 1536u;
      // (the window is counted in tickets, and most tickets of a configuration of large groups are dead at their turn —
      // every commit takes max - 1 candidates that held one: a quarter of the candidates is a tenth of the commits)
      uint32_t la = n_cand <= small ? STREAM_LA_SMALL(n_cand) : n_cand / 4u;
      (void)max_s;
      la = la < 24u ? 24u : la;
      return la > la_max ? la_max : la;
    };
    uint32_t prev_ci = PM_NONE;  // the configuration whose removals are still to be folded into the master bitmap
    // (the statistics a boundary used to add into the status block in memory — a load, an add, a store by one thread,
    // and the next barrier waits for it — are kept in registers of thread 0 until the launch ends.  Counting the
    // candidates of the configurations ahead on the entry pass, so that empty configurations are skipped by an upper
    // bound and the choice of the configurations that get tickets early reads counts instead of making a pass each, was
    // built and measured in round 5: +37 us per configs[1] match — eight more loads per word and eight wave reductions
    // at every entry cost more than the passes they save; profiles/r05_kernel_bisect.txt.)
    uint32_t acc_pre_used = 0u, acc_pre_lost = 0u, acc_listed = 0u, acc_pruned = 0u, acc_done = 0u;  // (thread 0)
    for (; ci < p.n_avail; ++ci) {
      c.min_s = p.min_size[ci];
      c.max_s = p.max_size[ci];
      if (tid == 0) STREAM_TRACE(11, ci, c.total_available);
      if (c.total_available < c.min_s) continue;  // `while` never entered (mod.rs:507)
      // ---- the candidate bitmap of this configuration: free & compatible (mod.rs:511-515 evaluated once; removals
      // are bit clears).  The removals of the configuration before it reach the master bitmap on the way: what it
      // took is what its candidate bitmap lost.
      uint32_t cnt = 0;
      PROF_DECL;
      for (uint32_t j = tid; j < lw; j += CARVE_THREADS) {
        uint64_t m = master[j];
        if (prev_ci != PM_NONE) m = (m & ~cfgbits[(size_t)prev_ci * p.bits_stride + j]) | r_alive[j];
        const uint64_t nc = m & cfgbits[(size_t)ci * p.bits_stride + j];
        master[j] = m;
        r_alive[j] = nc;
        cnt += (uint32_t)__popcll(nc);
      }
      prev_ci = ci;
      cnt = wave_sum(cnt);
      __syncthreads();
      if (lane == 0) red.a[wave] = cnt;
      __syncthreads();
      uint32_t n_cand = 0;
#pragma unroll
      for (uint32_t k = 0; k < CARVE_WAVES; ++k) n_cand += red.a[k];
      __syncthreads();
      PROF_MARK(32);
      if (n_cand < c.min_s || n_cand == 0u) continue;  // mod.rs:517-519
      c.cfg = p.avail_cfg[ci];
      c.n_cand = n_cand;
      c.prop_k = (p.proximity && c.max_s - 1u < PM_PROP_KMAX) ? PM_PROP_KMAX : 0u;
      c.prop_limit = n;
      c.n_seeds = PM_NONE;  // (carve_chain: "the list is used up" = no ticket)
      uint32_t switch_at = 0u;
      const uint32_t mode = c.prop_k ? row_mode(n_cand, &switch_at) : SROW_BITMAP;
      // (carve_chain leaves with FAST_REPROPOSE once n_cand * PM_THIN_DIV < n_start: the walk -> sweep switch)
      c.n_start = switch_at > 256u / PM_THIN_DIV ? switch_at * PM_THIN_DIV : 0u;
      // ---- this configuration's ticket state: the tickets issued ahead of its turn, if it has a slot; the slots of
      // configurations that were passed over are freed (their tickets are never looked at: a ticket names its configuration)
      uint32_t seed_cur0 = PM_NONE;
      if (tid == 0) {
        red._spare2 = PM_NONE;
        sl_words[SLW_SCANW] = 0u;
        sl_words[SLW_SCANLO] = sl_words[SLW_SCANHI] = 0xFFFFFFFFu;
        for (uint32_t k = 0; k < 2u; ++k) {
          const uint32_t pc = sl_words[SLW_P_CI + k];
          if (pc == PM_NONE) continue;
          // (its tickets must still be within the rings' reach: a configuration that issued thousands of its own in
          // between has overwritten their seeds in the ticket table and their rows — then they are as good as never issued)
          const bool in_reach = sl_words[SLW_TISSUED] - sl_words[SLW_P_T0 + k] + 1280u < PM_STREAM_TP;
          STREAM_TRACE(19, ci | pc << 8 | (in_reach ? 1u : 0u) << 16, sl_words[SLW_P_CNT + k]);  // a slot at a configuration's entry
          if (pc == ci && sl_words[SLW_P_CNT + k] > 0u && c.prop_k && c.max_s > 1u && in_reach) {
            red._spare2 = sl_words[SLW_P_T0 + k];
            sl_words[SLW_SCANW] = sl_words[SLW_P_SCANW + k];
            sl_words[SLW_SCANLO] = sl_words[SLW_P_SCANLO + k];
            sl_words[SLW_SCANHI] = sl_words[SLW_P_SCANHI + k];
            acc_pre_used += 1u;
          } else if (pc <= ci) {
            acc_pre_lost += sl_words[SLW_P_CNT + k];
          }
          if (pc <= ci) sl_words[SLW_P_CI + k] = PM_NONE;
        }
        sl_words[SLW_TEND] = PM_NONE;
        sl_words[SLW_NCAND] = n_cand;
        sl_words[SLW_TREQ] = sl_words[SLW_TISSUED];
        sl_words[SLW_LA] = look_ahead(n_cand, c.max_s);
        sl_words[SLW_PAY] = (ci << 18) | (mode << 24);
        if (mode == SROW_BITMAP) acc_listed += 1u;
        else acc_pruned += 1u;  // (configurations whose rows walk the spatial index: the batch pipeline counts batches)
      }
      __syncthreads();
      // ---- the configurations expected behind this one: the next two whose loop could still be entered — counts and
      // total_available only shrink, so what cannot be entered by today's numbers never will be; what can, may or may
      // not be when its turn comes.  Their first candidates get their tickets while this one is finishing (stream_ticket).
      if (c.prop_k && c.max_s > 1u) {
        uint32_t have = 0u;
        for (uint32_t cx = ci + 1u; cx < p.n_avail && have < 2u; ++cx) {
          if (c.total_available < p.min_size[cx]) continue;
          const bool slotted = sl_words[SLW_P_CI] == cx || sl_words[SLW_P_CI1] == cx;  // (it keeps its slot and its cursor)
          uint32_t nx = 0u;
          if (!slotted) {
            nx = count_candidates(cx);
            if (nx < p.min_size[cx] || nx == 0u) continue;
          }
          ++have;
          if (slotted || !(p.max_size[cx] > 1u && p.max_size[cx] - 1u < PM_PROP_KMAX)) continue;
          if (tid == 0) {
            const uint32_t k = sl_words[SLW_P_CI] == PM_NONE ? 0u : sl_words[SLW_P_CI1] == PM_NONE ? 1u : 2u;
            if (k < 2u) {
              uint32_t sw_next = 0u;
              sl_words[SLW_P_CI + k] = cx;
              sl_words[SLW_P_PAY + k] = (cx << 18) | (row_mode(nx, &sw_next) << 24);
              sl_words[SLW_P_MAX + k] = look_ahead(nx, p.max_size[cx]);
              sl_words[SLW_P_CNT + k] = 0u;
              sl_words[SLW_P_T0 + k] = 0u;
              sl_words[SLW_P_SCANW + k] = 0u;
              sl_words[SLW_P_SCANLO + k] = sl_words[SLW_P_SCANHI + k] = 0xFFFFFFFFu;
            }
          }
          __syncthreads();
        }
      }
      __syncthreads();
      seed_cur0 = red._spare2;
      __syncthreads();
      if (tid == 0) STREAM_TRACE(1, ci, n_cand);
      PROF_MARK(33);
      int rc;
      if (!big)
        rc = stream_run_config<false>(p, red, c, lds_site, lds_key, r_alive, r_loc, part, sel_out,
                                      reinterpret_cast<uint32_t*>(lds_key), sl_words, steps_before, seed_cur0);
      else
        rc = stream_run_config<true>(p, red, c, p.cc_site, p.keys, r_alive, r_loc, part, sel_out,
                                     reinterpret_cast<uint32_t*>(lds_key), sl_words, steps_before, seed_cur0);
      __syncthreads();
      // (this configuration is over: whoever still makes a row for it lets it be)
      if (tid == 0) st_ag32(&ctl[SC_DROP], STREAM_DROP_WORD(ci, sl_words[SLW_TISSUED]));
      PROF_MARK(34);
      if (rc == STEP_UNCERTAIN || rc == STEP_OVERFLOW || rc == STEP_ABORT) {
        exit_state = rc == STEP_UNCERTAIN ? CARVE_STATE_UNCERTAIN : rc == STEP_ABORT ? CARVE_STATE_ABORTED : CARVE_STATE_OVERFLOW;
        stop_ci = ci;
        break;
      }
      if (tid == 0) acc_done += 1u;
    }
    if (tid == 0) {
      st->why[3] += acc_done;
      st->stream_pre_used += acc_pre_used;
      st->stream_pre_lost += acc_pre_lost;
      st->stream_listed += acc_listed;
      st->pruned_batches += acc_pruned;
    }
  }
  // ---- the proposers leave; the records are complete (members hold POSITIONS: carve_finish_kernel turns them into
  // worker ids and writes group_of on every CU)
  if (tid == 0) {
    st_ag32(&ctl[SC_QUIT], 1u);
    ctl[SC_FINISH] = 1u;  // (for carve_finish_kernel, behind this launch)
  }
  if (n > 0u && n <= PM_CARVE_BIG_SLOTS) {
    // every wave that holds (or is about to take) a ticket number beyond the last one issued gets a ticket that says
    // "over": each proposer wave takes at most one more number
    const uint32_t q_lo = sl_words[SLW_TISSUED];
    const uint32_t q_hi = ld_ag32(&ctl[SC_CLAIM]) + (gridDim.x - 1u) * PM_STREAM_PROP_WAVES + 64u;
    const auto sq = G(p.stream_sq);
    const uint32_t tag0 = p.stream_tag0;
    for (uint32_t t = q_lo + tid; t < q_hi && t - q_lo < PM_STREAM_SQ; t += CARVE_THREADS)
      st_ag(&sq[t & (PM_STREAM_SQ - 1u)], ((unsigned long long)(tag0 + t) << 32) | 0xFFFFFFFFull);
  }
  __syncthreads();
  if (tid == 0) {
    st->state = exit_state;
    st->n_groups = c.n_groups;
    st->n_members = c.mem_off;
    st->steps_total = steps_before + c.steps;
    st->stop_ci = stop_ci;
    st->cand_sum += c.cand_sum;
    st->cur_ci = exit_state == CARVE_STATE_DONE ? p.n_avail : ci;
    st->n_list = n;
    st->total_available = c.total_available;
    st->g_lo = groups_at_entry;
    st->g_hi = c.n_groups;
    st->fast_steps += c.fast_steps;
    st->slow_steps += c.steps - c.fast_steps;
    st->n_batches += 1u;
    if (n > 0u && n <= PM_CARVE_BIG_SLOTS) {
      st->stream_timeouts += sl_words[SLW_TIMEOUTS];
      st->stream_tickets += sl_words[SLW_TISSUED];
    }
  }
}

// ---- behind the streaming carve, on every CU: the members of the groups it appended are positions of the eligible
// list -> worker ids; group_of for them; single-node groups counted (the merge pass only runs when there are two)
__global__ __launch_bounds__(256) void carve_finish_kernel(const CarveArgs* __restrict__ pa) {
  const CarveArgs& p = *pa;
  const auto st = G(p.status);
  const auto ctl = G(p.stream_ctl);
  __shared__ uint32_t s_last;
  if (ctl[SC_FINISH]) {  // (else the carve launch in front returned at once: nothing new)
    const uint32_t g_lo = st->g_lo, g_hi = st->g_hi;
    const uint32_t total = gridDim.x * 256u;
    const uint32_t id_g0 = p.id_g0, m0 = p.stage_m0, cap_g = p.stage_cap_g, cap_m = p.stage_cap_m;
    const bool stage = p.stage_cfg != nullptr;
    uint32_t solo = 0;
    for (uint32_t g = g_lo + blockIdx.x * 256u + threadIdx.x; g < g_hi; g += total) {
      const uint32_t off = G(p.g_off)[g], gn = G(p.g_n)[g];
      const uint32_t k = g - id_g0;
      for (uint32_t j = 0; j < gn; ++j) {
        const uint32_t w = G(p.order)[G(p.members)[off + j]];
        G(p.members)[off + j] = w;
        if (p.mode == CARVE_MODE_FORM) G(p.group_of)[w] = (int32_t)g;  // (a merge batch is the host's to apply)
        if (stage && off + j - m0 < cap_m) p.stage_mem[off + j - m0] = w;  // (pinned host memory)
      }
      if (p.g_id_out) {  // generate_group_id (mod.rs:1489-1493, injected): output k + 1 of the splitmix64 stream
        unsigned long long z = p.id_state + (unsigned long long)(k + 1u) * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        p.g_id_out[g] = z ^ (z >> 31);
        p.g_task_out[g] = PM_NONE;
      }
      if (stage && k < cap_g) {
        p.stage_cfg[k] = G(p.g_cfg)[g];
        p.stage_n[k] = gn;
        p.stage_off[k] = off;
      }
      solo += gn == 1u ? 1u : 0u;
    }
    solo = wave_sum(solo);
    if ((threadIdx.x & 63u) == 0u && solo) atomicAdd(&p.status->n_solo, solo);
  }
  // ---- the block that is through last mirrors the status block to the host (n_solo is complete then)
  if (!p.h_status) return;
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    s_last = atomicAdd(&p.stream_ctl[SC_FINISH_TICKET], 1u);
  }
  __syncthreads();
  if (s_last != gridDim.x - 1u) return;
  const auto src = G((const uint32_t*)p.status);
  uint32_t* dst = (uint32_t*)p.h_status;
  for (uint32_t k = threadIdx.x; k < (uint32_t)(sizeof(CarveStatus) / 4u); k += 256u) dst[k] = ld_ag32((const stream_gu32*)(src + k));
}

// eligible list [+ spatial index] -> carve_stream_kernel -> carve_finish_kernel.  n_prop_wgs: proposer workgroups
// (one per CU: the kernel's LDS fills a CU).
hipError_t launch_carve_stream(const CarveArgs* d_args, uint32_t start_ci, uint32_t n_prop_wgs, hipStream_t s) {
  // (the control words are zeroed by carve_elig_count_kernel, the first launch of every sequence that ends here)
  hipLaunchKernelGGL(carve_stream_kernel, dim3(1u + n_prop_wgs), dim3(CARVE_THREADS), PM_STREAM_LDS_BYTES, s, d_args, start_ci);
  hipLaunchKernelGGL(carve_finish_kernel, dim3(128), dim3(256), 0, s, d_args);
  return hipGetLastError();
}

// ---- measuring builds only (-DPM_ROW_BENCH; everything else that measures lives in pm_measure.inc, this calls the row maker)
#ifdef PM_ROW_BENCH
// A measuring build's kernel (tools/row_bench.py): ONE wave alone on a CU makes the row of seed `s` in configuration `ci` `reps`
// times over — the bitmap sweep exactly as a row maker runs it (every position of free & compatible; the caller hands in a free
// bitmap of all ones) — and reports s_memtime ticks: out[0] ticks in all, [1] rows, [2] candidates evaluated in the last one,
// [3] a checksum of the last row (so that what is taken out of the row maker in a variant build shows), [4..7] ticks of the
// seed's columns, the sweep, the finish.
__global__ __launch_bounds__(CARVE_THREADS) void carve_row_bench_kernel(const CarveArgs* __restrict__ pa, uint32_t s, uint32_t ci, uint32_t reps,
                                                                        unsigned long long* __restrict__ out) {
  const CarveArgs& p = *pa;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (wave != 0u) return;
  const auto st = G((const CarveStatus*)p.status);
  const uint32_t n = st->n_eligible;
  if (n == 0u || n > PM_CARVE_BIG_SLOTS || s >= n) return;
  const uint32_t SB = n > PM_CARVE_SLOTS ? PM_CARVE_SLOT_BITS_BIG : PM_CARVE_SLOT_BITS;
  const double TIE_BAND = n > PM_CARVE_SLOTS ? PM_TIE_BAND_BIG : PM_TIE_BAND;
  const uint64_t WINDOW_ULPS = n > PM_CARVE_SLOTS ? (1ull << 25) : (1ull << 20);
  uint32_t* wl = reinterpret_cast<uint32_t*>(s_raw);
  BulkCtx bulk = {0u, lane_net(lane, reinterpret_cast<uint64_t*>(s_raw + size_t(CARVE_WAVES) * STREAM_WL_WORDS * 4u))};
  const uint64_t* cfg64 = p.cfgbits + (size_t)ci * p.bits_stride;
  unsigned long long t_all = 0, t_geo = 0, t_sweep = 0, t_fin = 0, check = 0;
  uint32_t swept = 0;
  for (uint32_t rep = 0; rep < reps; ++rep) {
    const uint64_t t0 = __builtin_amdgcn_s_memtime();
    const uint32_t ssite = G(p.cc_site)[s];
    const SeedGeo sg = {G(p.cc_lat)[s], G(p.cc_lon)[s], G(p.cc_cos)[s], G(p.cc_ux)[s], G(p.cc_uy)[s], G(p.cc_uz)[s]};
    const bool shared = (ssite & 0x80000000u) != 0u;
    NearRow q = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull, 0xFFFFFFFFu};
    uint32_t n_mine = 0;
    bulk.seen = 0u;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint64_t t1 = __builtin_amdgcn_s_memtime();
    (void)stream_bitmap_sweep(p, cfg64, n, wl, lane, s, shared, ssite, sg, SB, WINDOW_ULPS, q, n_mine, bulk, ci, 0x01FFFFF0u);
    const uint64_t t2 = __builtin_amdgcn_s_memtime();
    uint64_t mine = q.m1;
    const uint32_t meta = PM_ROWB(1u) ? 0u : near_row_finish(p, q, true, PM_PROP_KMAX, SB, TIE_BAND, lane, &mine);
    const uint64_t t3 = __builtin_amdgcn_s_memtime() + (meta & 0u);
    t_all += t3 - t0;
    t_geo += t1 - t0;
    t_sweep += t2 - t1;
    t_fin += t3 - t2;
    swept = wave_sum(n_mine);
    check = mine * (lane + 1u) + meta;
  }
  unsigned long long cs = check;
  for (uint32_t o = 32u; o; o >>= 1) cs += __shfl_xor(cs, o, 64);
  if (lane == 0u) {
    out[0] = t_all;
    out[1] = reps;
    out[2] = swept;
    out[3] = cs;
    out[4] = t_geo;
    out[5] = t_sweep;
    out[6] = t_fin;
  }
}
#endif
