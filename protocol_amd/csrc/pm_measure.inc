// pm_measure.inc — everything the measuring builds add to the carve kernels (included by pm_kernels.hip in front of them).
// The product build defines none of the switches below, and every name in this file then expands to nothing (PM_ROWB: to
// false): the kernels read straight, and the product library is the same with or without a measuring line.
//   -DPM_CARVE_PROF       s_memtime ticks and counts per phase in status->prof[64], a timeline of the streaming carve in
//                         p.stream_trace (tools/stream_prof.py, stream_trace.py, carve_prof.py)
//     + PM_CHAIN_FINE     the chain's steps taken apart, in the parkers' prof slots (PM_CHAIN_FINE=1 tools/stream_prof.py)
//     + PM_CARVE_PROF_FINE  the batch pipeline's fast steps counted by kind (PM_PROF_FINE=1 tools/carve_prof.py)
//   -DPM_ROW_REC          every stamp the real-time counter, plain stores: a record per ticket, per block of the parkers, per
//                         batch of the chain (tools/row_rec.py, pipeline_probe.py, stream_trace.py)
//   -DPM_ROW_BENCH        carve_row_bench_kernel (at the end of pm_stream.inc): one wave alone makes a row, with pieces
//                         left out by g_rowb_mode (tools/row_bench.py)
//   -DPM_BATCH_LOG        what every preparation of the batch pipeline produced, and what it cost (tools/prune_probe.py)
//   -DPM_TIMEOUT_DIAG     what a parker found instead of a row it gave up on
// The vocabulary of the kernel bodies: PM_PROF(...), PM_REC(...), PM_BLOG(...) expand to their arguments
// in the matching build; PM_ROWB(bit) asks for a mode of the row bench.  Anything longer than a line is a named piece
// below, built from those.  The pieces are macros, not functions: they stand in front of the types they touch.  Every piece
// reads `p` (the CarveArgs) and, where one lane books, `lane` / `tid`; what else it reads of the function it is used in — beyond
// its parameters and the counters its own *_DECL declares — its comment lists under "reads".  (A rename of such a local shows
// in the measuring builds only: `tools/build_variants.py` builds them all in two minutes.)
#ifdef PM_CARVE_PROF
#define PM_PROF(...) __VA_ARGS__
#else
#define PM_PROF(...)
#endif
#ifdef PM_ROW_REC
#define PM_REC(...) __VA_ARGS__
#else
#define PM_REC(...)
#endif
#ifdef PM_BATCH_LOG
#define PM_BLOG(...) __VA_ARGS__
#else
#define PM_BLOG(...)
#endif
#ifdef PM_ROW_BENCH
__device__ uint32_t g_rowb_mode = 0u;  // measuring modes: set by pm_debug_row_bench around its launch only
#define PM_ROWB(bit) ((g_rowb_mode & (bit)) != 0u)
#else
#define PM_ROWB(bit) false
#endif
#define PM_TICKS() __builtin_amdgcn_s_memtime()

// ---- phase marks of a whole workgroup (thread 0 books): ticks since the last mark into prof[slot]
#define PROF_DECL PM_PROF(uint64_t prof_t0 = PM_TICKS())
#define PROF_MARK(slot) PM_PROF(do { const uint64_t t_ = PM_TICKS(); if (threadIdx.x == 0) G(p.status)->prof[slot] += t_ - prof_t0; prof_t0 = t_; } while (0))
#ifdef PM_CARVE_PROF_FINE
#define PROF_COUNT(slot) do { if (lane == 0) G(p.status)->prof[slot] += 1; } while (0)
#else
#define PROF_COUNT(slot)
#endif
// why a step went to the exact sweep: 20 no proposal, 21 debug hook, 25 row exhausted, 31 certificate
#ifdef PM_CARVE_PROF
#define SLOW_RETURN(why) do { if (lane == 0) G(p.status)->prof[why] += 1; FAST_RETURN(FAST_SLOW); } while (0)
#else
#define SLOW_RETURN(why) FAST_RETURN(FAST_SLOW)
#endif

// ---- a row's anatomy (NearRow): ticks and counts of the sorted insertions, the near-miss tracker, the exact (sine form)
// keys, evictions that needed a site looked up; p_seg — near_row_bulk4: count + pack, networks, threshold + evictions,
// near misses; calls; whole calls
#define NEAR_ROW_PROF_FIELDS PM_PROF(uint64_t p_ins_t = 0, p_trk_t = 0, p_hav_t = 0, p_wait_t = 0, p_eval_t = 0, p_key_t = 0, p_off_t = 0; \
                                     uint32_t p_ins_n = 0, p_trk_n = 0, p_hav_n = 0, p_ev_n = 0, p_strides = 0;                              \
                                     uint64_t p_seg[6] = {0, 0, 0, 0, 0, 0};)
#define NR_SEG(r, i, t0) PM_PROF(do { const uint64_t t_ = PM_TICKS(); (r).p_seg[i] += t_ - (t0); (t0) = t_; } while (0))
#define NR_SEG0(var) PM_PROF(uint64_t var = PM_TICKS())
#define NR_T0 PM_PROF(const uint64_t nr_t0_ = PM_TICKS())
#define NR_ADD(field) PM_PROF((field) += PM_TICKS() - nr_t0_)
#define NR_CNT(field, n) PM_PROF((field) += (n))
// (BulkCtx: when the sweep's first pass was packed, when the first batch's keys were there)
#define BULK_REC_FIELDS PM_REC(uint64_t rec_pass = 0, rec_keys = 0;)

// ---- the streaming carve's timeline (one lane calls): 1 configuration entered (ci, candidates), 2 chain waits (entry), 3 chain
// goes on (entry), 4 tickets issued (count), 5 block parked (block, first entry), 6 run starts (ticket), 7 run ends (action,
// commits), 8 row written (ticket, ticks it took), 9 exact step, 14 a row that ran out, 16 a block's rows asked for -> all
// there, 20-25 where a swept row's time went, 26 who acknowledged a STOP after how many ticks
// (PM_ROW_REC: the row makers' records fill the first half of the buffer, the validator's events the second; every stamp
// of it is the REAL-TIME counter — 100 MHz, one clock for all CUs — so that a ticket's way from the ticketer through a row
// maker and a parker to the chain can be laid on one axis: tools/pipeline_probe.py)
#ifdef PM_ROW_REC
#define STREAM_TRACE_AT size_t(PM_STREAM_TRACE_CAP)
#define STREAM_TRACE_MAX (PM_STREAM_TRACE_CAP / 8u)
#define STREAM_PARK_AT (size_t(PM_STREAM_TRACE_CAP) + PM_STREAM_TRACE_CAP / 4u)  // the parkers' blocks: eight words each, plain stores, by ticket / 16
#define STREAM_PARK_MAX (PM_STREAM_TRACE_CAP / 32u)
#define STREAM_BATCH_AT (size_t(PM_STREAM_TRACE_CAP) + PM_STREAM_TRACE_CAP / 2u)  // the chain's batches: {clock, what it took up}, plain stores
#define STREAM_BATCH_MAX (PM_STREAM_TRACE_CAP / 8u)  // (four words each)
#define STREAM_CLOCK() __builtin_amdgcn_s_memrealtime()
#else
#define STREAM_TRACE_AT size_t(0)
#define STREAM_TRACE_MAX PM_STREAM_TRACE_CAP
#define STREAM_CLOCK() __builtin_amdgcn_s_memtime()
#endif
#if defined(PM_CARVE_PROF) || defined(PM_ROW_REC)
#define PM_PROF_OR_REC(...) __VA_ARGS__
#define STREAM_TRACE(type, a, b)                                                                                   \
  do {                                                                                                             \
    if (p.stream_trace) {                                                                                          \
      const uint32_t ti_ = atomicAdd(&p.stream_ctl[SC_TRACE], 1u);                                                 \
      if (ti_ < STREAM_TRACE_MAX) {                                                                                \
        p.stream_trace[STREAM_TRACE_AT + 2u * ti_] = STREAM_CLOCK();                                               \
        p.stream_trace[STREAM_TRACE_AT + 2u * ti_ + 1u] = (unsigned long long)(type) | ((unsigned long long)((a) & 0xFFFFFFu) << 8) | \
                                        ((unsigned long long)(b) << 32);                                           \
      }                                                                                                            \
    }                                                                                                              \
  } while (0)
#ifdef PM_ROW_REC  // (an event that is an atomic with its return value in a path the records time: they have plain stores instead)
#define STREAM_TRACE_NOT_REC(type, a, b)
#else
#define STREAM_TRACE_NOT_REC(type, a, b) STREAM_TRACE(type, a, b)
#endif
#else
#define PM_PROF_OR_REC(...)
#define STREAM_TRACE(type, a, b)
#define STREAM_TRACE_NOT_REC(type, a, b)
#endif
// event 26, behind the chain's STOP: when each of the seven — collector, ticketer, five parkers — acknowledges (who, ticks)
// reads: lane; the control words CC_ACK2, SLW_ACKT, SLW_ACKP0.. of the L and SL it is given
#define STREAM_TRACE_ACKS(L, SL, want_ack)                                                                         \
  PM_PROF_OR_REC({                                                                                                 \
    const uint64_t st0 = PM_TICKS();                                                                               \
    const uint32_t want_ack_ = (want_ack);                                                                         \
    uint32_t got = 0u, sp_n = 0u;                                                                                  \
    uint32_t dt[7] = {0, 0, 0, 0, 0, 0, 0};                                                                        \
    while (got != 0x7Fu && ++sp_n < (1u << 16)) {                                                                  \
      _Pragma("unroll") for (uint32_t i = 0; i < 7u; ++i) {                                                        \
        const uint32_t v = i == 0u ? UNI(cc_ld(&L.CC[CC_ACK2])) : i == 1u ? UNI(cc_ld(&SL[SLW_ACKT])) : UNI(cc_ld(&SL[SLW_ACKP0 + (i - 2u)])); \
        if (!((got >> i) & 1u) && v == want_ack_) {                                                                \
          got |= 1u << i;                                                                                          \
          dt[i] = (uint32_t)(PM_TICKS() - st0);                                                                    \
        }                                                                                                          \
      }                                                                                                            \
    }                                                                                                              \
    if (lane == 0u) {                                                                                              \
      _Pragma("unroll") for (uint32_t i = 0; i < 7u; ++i) STREAM_TRACE(26, i, dt[i]);                              \
    }                                                                                                              \
  })

// ---- a parker's anatomy (stream_park): ticks waiting for tickets, for room, for rows, digesting; SP_BOOK at its end
// SP_MARK, SP_COUNT, SP_BOOK read: SP_DECL's pt, pt_*, pn_*; SP_BOOK also lane
// (with PM_CHAIN_FINE the chain's counters take the parkers' slots — every prof word has an owner — and these are not read)
#define SP_DECL PM_PROF([[maybe_unused]] uint64_t pt = PM_TICKS(), pt_tick = 0, pt_room = 0, pt_rows = 0, pt_write = 0, pt_idle = 0; \
                        [[maybe_unused]] uint32_t pn_polls = 0, pn_late = 0, pn_rows = 0)
#define SP_MARK(var) PM_PROF(do { const uint64_t t_ = PM_TICKS(); var += t_ - pt; pt = t_; } while (0))
#define SP_COUNT(var, n) PM_PROF((var += (n)))
#ifndef PM_CHAIN_FINE
#define SP_BOOK()                                                                                                  \
  PM_PROF(if (lane == 0u) {                                                                                        \
    unsigned long long* pr = (unsigned long long*)p.status->prof;                                                  \
    atomicAdd(&pr[5], (unsigned long long)pt_tick);                                                                \
    atomicAdd(&pr[6], (unsigned long long)pt_room);                                                                \
    atomicAdd(&pr[7], (unsigned long long)pt_rows);                                                                \
    atomicAdd(&pr[8], (unsigned long long)pt_write);                                                               \
    atomicAdd(&pr[9], (unsigned long long)pt_idle);                                                                \
    atomicAdd(&pr[26], (unsigned long long)pn_polls);                                                              \
    atomicAdd(&pr[27], (unsigned long long)pn_late);                                                               \
    atomicAdd(&pr[28], (unsigned long long)pn_rows);                                                               \
  })
#define CH_FINE_WORDS
#else
#define SP_BOOK()
// of the steps' time: the batches' heads, the plain runs, the steps that needed attention (a dead seed, a second look), how
// many of those (ct_steps, pr[18]: what is left — the batch's tail: counters, the hand-over words)
#define CH_FINE_WORDS pr[5] += ct_head; pr[6] += ct_plain; pr[7] += ct_att; pr[8] += cn_att;
#endif
// ... and a record per block (PM_ROW_REC, plain stores: which tickets' rows were asked for and when; when they were all there;
// when the block had its turn; when it had room; when it was parked, where and which)
// PARK_REC_OPEN declares `prec`, the block's record, for PARK_REC_STAMP and PARK_REC_CLOSE behind it in the same scope; all read lane
#define PARK_REC_OPEN(t0, live_m, n_real)                                                                          \
  PM_REC(unsigned long long* const prec = p.stream_trace ? p.stream_trace + STREAM_PARK_AT + size_t(((t0) >> 4) & (STREAM_PARK_MAX - 1u)) * 8u : nullptr; \
         if (lane == 0u && prec) {                                                                                 \
           prec[0] = (unsigned long long)(t0) | ((unsigned long long)(live_m) << 32) | ((unsigned long long)(n_real) << 48) | (1ull << 63); \
           prec[1] = STREAM_CLOCK();                                                                               \
         })
#define PARK_REC_STAMP(i) PM_REC(if (lane == 0u && prec) prec[i] = STREAM_CLOCK())
#define PARK_REC_CLOSE(q_b, live_m, b)                                                                             \
  PM_REC(if (lane == 0u && prec) {                                                                                 \
    prec[5] = STREAM_CLOCK();                                                                                      \
    prec[6] = (unsigned long long)(q_b) | ((unsigned long long)(live_m) << 32) | ((unsigned long long)(b) << 48);  \
  })
// what a parker found instead of a row it gave up on (first time-outs of the launch): status->prof[8 n .. 8 n + 7]
// reads of stream_park: lane, tag0, t0_run (the run's first ticket), SL (the ticket state: SLW_TREQ, SLW_TISSUED)
#ifdef PM_TIMEOUT_DIAG
#define STREAM_TIMEOUT_DUMP(t, row)                                                                                \
  {                                                                                                                \
    const unsigned long long sqv2 = ld_ag(&G((const unsigned long long*)p.stream_sq)[(t) & (PM_STREAM_SQ - 1u)]);  \
    const uint32_t claim2 = ld_ag32(&G(p.stream_ctl)[SC_CLAIM]);                                                   \
    const uint32_t rtag2 = UNI((uint32_t)((row) >> 32));                                                           \
    if (lane == 0u) {                                                                                              \
      unsigned long long* pr = (unsigned long long*)p.status->prof;                                                \
      const unsigned long long slot = atomicAdd(&pr[47], 1ull);                                                    \
      if (slot < 5ull) {                                                                                           \
        pr[8 * slot + 0] = (t);                                                                                    \
        pr[8 * slot + 1] = rtag2 - tag0;                                                                           \
        pr[8 * slot + 2] = (uint32_t)(sqv2 >> 32) - tag0;                                                          \
        pr[8 * slot + 3] = (uint32_t)sqv2;                                                                         \
        pr[8 * slot + 4] = claim2;                                                                                 \
        pr[8 * slot + 5] = UNI(cc_ld(&SL[SLW_TREQ]));                                                              \
        pr[8 * slot + 6] = t0_run;                                                                                 \
        pr[8 * slot + 7] = UNI(cc_ld(&SL[SLW_TISSUED]));                                                           \
      }                                                                                                            \
    }                                                                                                              \
  }
#else
#define STREAM_TIMEOUT_DUMP(t, row)
#endif

// ---- the chain's anatomy (carve_chain, stream_chain): ticks waiting for rows, in steps, stopping the others; trips of the
// loop, seeds found dead, waits.  CH_DECL_FINE (stream_chain): with the steps' time taken apart — the batches' heads, the
// plain runs, the steps that needed attention — which the PM_CHAIN_FINE build alone reads
// CH_MARK, CH_COUNT, CH_BOOK (and CH_FINE_WORDS inside it) read: CH_DECL's ct, ct_*, cn_*; CH_BOOK also lane and the chain's
// `commits` and `action` as it leaves
#define CH_DECL PM_PROF(uint64_t ct = PM_TICKS(), ct_wait = 0, ct_steps = 0, ct_stop = 0; uint32_t cn_outer = 0, cn_dead = 0, cn_wait = 0)
#define CH_DECL_FINE PM_PROF(uint64_t ct = PM_TICKS(), ct_wait = 0, ct_steps = 0, ct_stop = 0; [[maybe_unused]] uint64_t ct_head = 0, ct_plain = 0, ct_att = 0; \
                             uint32_t cn_outer = 0, cn_dead = 0, cn_wait = 0; [[maybe_unused]] uint32_t cn_att = 0)
#define CH_MARK(var) PM_PROF(do { const uint64_t t_ = PM_TICKS(); var += t_ - ct; ct = t_; } while (0))
#define CH_COUNT(var) PM_PROF((++var))
#define CH_BOOK(...)                                                                                               \
  PM_PROF(if (lane == 0u) {                                                                                        \
    unsigned long long* pr = (unsigned long long*)p.status->prof;                                                  \
    pr[1] += 1u; /* calls */                                                                                       \
    pr[2] += commits;                                                                                              \
    pr[4] += action == FAST_SLOW ? 1u : 0u;                                                                        \
    pr[16] += ct_wait;                                                                                             \
    pr[17] += ct_stop;                                                                                             \
    pr[18] += ct_steps;                                                                                            \
    pr[19] += cn_outer;                                                                                            \
    pr[23] += cn_dead;                                                                                             \
    pr[24] += cn_wait;                                                                                             \
    __VA_ARGS__                                                                                                    \
  })
// ... and a record per batch (PM_ROW_REC, plain stores: clock at the loop's top; first entry | entries << 24 | live ones << 32 |
// commits so far << 40; clock here — the entries seen and looked at; clock behind the steps).
// both read: lane, and `rec_batches` of stream_chain (batches recorded so far: the runs of a launch share the region — loaded
// from SC_BATCHES at the run's start, stored back at its end); CHAIN_REC_BATCH_END counts it up
#define CHAIN_REC_BATCH(rec_top, first, n, live, done)                                                             \
  PM_REC(if (lane == 0u && p.stream_trace && rec_batches < STREAM_BATCH_MAX) {                                     \
    p.stream_trace[STREAM_BATCH_AT + 4u * rec_batches] = (rec_top);                                                \
    p.stream_trace[STREAM_BATCH_AT + 4u * rec_batches + 1u] = (unsigned long long)((first) & 0xFFFFFFu) | ((unsigned long long)(n) << 24) | \
                                                              ((unsigned long long)(live) << 32) | ((unsigned long long)(done) << 40); \
    p.stream_trace[STREAM_BATCH_AT + 4u * rec_batches + 2u] = STREAM_CLOCK();                                      \
  })
#define CHAIN_REC_BATCH_END()                                                                                      \
  PM_REC(if (lane == 0u && p.stream_trace && rec_batches < STREAM_BATCH_MAX) p.stream_trace[STREAM_BATCH_AT + 4u * rec_batches + 3u] = STREAM_CLOCK(); \
         rec_batches += 1u)

// ---- stream_small_n: ticks of a group's five phases (prof[42..46]) and the groups (47); stream_small_rows: booked as
// selection time (44) — the anatomy's stream_small line
// SM_MARK, SM_BOOK read: SM_DECL's sm_t, sm_a, sm_n; SM_BOOK and SR_BOOK also lane
#define SM_DECL PM_PROF(uint64_t sm_t = PM_TICKS(), sm_a[5] = {0, 0, 0, 0, 0}; uint32_t sm_n = 0)
#define SM_MARK(k) PM_PROF(do { const uint64_t t_ = PM_TICKS(); sm_a[k] += t_ - sm_t; sm_t = t_; } while (0))
#define SM_BOOK()                                                                                                  \
  PM_PROF(if (lane == 0u) {                                                                                        \
    unsigned long long* pr = (unsigned long long*)p.status->prof;                                                  \
    for (int q = 0; q < 5; ++q) pr[42 + q] += sm_a[q];                                                             \
    pr[47] += sm_n;                                                                                                \
  })
#define SR_BOOK(t0, groups)                                                                                        \
  PM_PROF(if (lane == 0u) {                                                                                        \
    unsigned long long* pr = (unsigned long long*)p.status->prof;                                                  \
    pr[44] += PM_TICKS() - (t0);                                                                                   \
    pr[47] += (groups);                                                                                            \
  })

// ---- a swept row (stream_drain, stream_bitmap_sweep): this batch's gathers waited for (the next batch's eight loads may stay
// in flight) in front of its evaluation, both booked behind it; the passes over the bitmap and the drains, ticks and counts
// DRAIN_PROF_WAIT declares t0_, t1_ for DRAIN_PROF_BOOK behind it; SWEEP_PROF_MARK, SWEEP_PROF_BOOK read: SWEEP_PROF_DECL's bp_*;
// SWEEP_PROF_BOOK also lane
#define DRAIN_PROF_WAIT(more)                                                                                      \
  PM_PROF(const uint64_t t0_ = PM_TICKS();                                                                         \
          if (more) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");                                               \
          else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                    \
          const uint64_t t1_ = PM_TICKS())
#define DRAIN_PROF_BOOK(q) PM_PROF((q).p_wait_t += t1_ - t0_; (q).p_eval_t += PM_TICKS() - t1_)
#define SWEEP_PROF_DECL PM_PROF(uint64_t bp_t = PM_TICKS(), bp_pass = 0, bp_drain = 0; uint32_t bp_np = 0, bp_nd = 0)
#define SWEEP_PROF_MARK(ticks, count, n) PM_PROF({ const uint64_t t_ = PM_TICKS(); ticks += t_ - bp_t; bp_t = t_; count += (n); })
#define SWEEP_PROF_BOOK(q)                                                                                         \
  PM_PROF(if (lane == 0u) {                                                                                        \
    unsigned long long* pr = (unsigned long long*)p.status->prof;                                                  \
    atomicAdd(&pr[38], (unsigned long long)bp_pass);                                                               \
    atomicAdd(&pr[39], (unsigned long long)bp_drain);                                                              \
    atomicAdd(&pr[40], (unsigned long long)bp_np);                                                                 \
    atomicAdd(&pr[41], (unsigned long long)bp_nd);                                                                 \
  }                                                                                                                \
  (q).p_seg[4] = bp_pass; /* (for the row's own trace events) */                                                   \
  (q).p_seg[5] = bp_drain;)

// ---- a row maker's row (stream_proposer).  What a row costs its wave, by the way it was made (ticks, rows): list 10/12, walk
// 13/14, sweep 15/29; bt0: ticket seen, bt_geo: the seed's columns there, bt1: candidates swept
// reads: lane; wave_sum; everything else is a parameter (q: the NearRow, with its p_* fields)
#define PROP_PROF_ROW(t, mode, q, n_mine, bt0, bt_geo, bt1)                                                        \
  PM_PROF({                                                                                                        \
    const uint32_t swept_p = wave_sum(n_mine);                                                                     \
    if (lane == 0u) {                                                                                              \
      unsigned long long* pr = (unsigned long long*)p.status->prof;                                                \
      const uint64_t dt = PM_TICKS() - bt0;                                                                        \
      const uint32_t a = mode == SROW_BITMAP ? 10u : mode == SROW_WALK ? 13u : 15u, b = mode == SROW_BITMAP ? 12u : mode == SROW_WALK ? 14u : 29u; \
      atomicAdd(&pr[a], (unsigned long long)dt);                                                                   \
      atomicAdd(&pr[b], 1ull);                                                                                     \
      atomicMax(&pr[30], (unsigned long long)dt);                                                                  \
      atomicAdd(&pr[35], (unsigned long long)(bt1 - bt0));           /* ticket seen -> candidates swept */          \
      atomicAdd(&pr[36], (unsigned long long)(PM_TICKS() - bt1));    /* row finished and written */                 \
      atomicAdd(&pr[37], (unsigned long long)swept_p);                                                             \
      atomicAdd(&pr[48], (unsigned long long)q.p_ins_t);                                                           \
      atomicAdd(&pr[49], (unsigned long long)q.p_ins_n);                                                           \
      atomicAdd(&pr[50], (unsigned long long)q.p_trk_t);                                                           \
      atomicAdd(&pr[51], (unsigned long long)q.p_trk_n);                                                           \
      atomicAdd(&pr[52], (unsigned long long)q.p_hav_t);                                                           \
      atomicAdd(&pr[53], (unsigned long long)q.p_hav_n);                                                           \
      atomicAdd(&pr[54], (unsigned long long)q.p_ev_n);                                                            \
      atomicAdd(&pr[55], (unsigned long long)q.p_strides);                                                         \
      atomicAdd(&pr[56], (unsigned long long)q.p_wait_t);                                                          \
      atomicAdd(&pr[57], (unsigned long long)q.p_eval_t);                                                          \
      atomicAdd(&pr[58], (unsigned long long)q.p_key_t);                                                           \
      atomicAdd(&pr[59], (unsigned long long)q.p_off_t);                                                           \
      for (uint32_t i = 0; i < 4u; ++i) atomicAdd(&pr[60u + i], (unsigned long long)(i < 3u ? q.p_seg[i == 0u ? 0u : i == 1u ? 2u : 3u] : q.p_seg[5])); \
      STREAM_TRACE(8, t, (uint32_t)dt);                                                                            \
      if (mode == SROW_BITMAP) { /* where a swept row's time went: ticket seen -> sweep begins; the passes; the batches: waiting, evaluating, the rest; finish + write */ \
        STREAM_TRACE(20, t, (uint32_t)(bt_geo - bt0));                                                             \
        STREAM_TRACE(21, t, (uint32_t)q.p_seg[4]);                                                                 \
        STREAM_TRACE(22, t, (uint32_t)q.p_wait_t);                                                                 \
        STREAM_TRACE(23, t, (uint32_t)q.p_eval_t);                                                                 \
        STREAM_TRACE(24, t, (uint32_t)(q.p_seg[5] - q.p_wait_t - q.p_eval_t));                                     \
        STREAM_TRACE(25, t, (uint32_t)(PM_TICKS() - bt1));                                                         \
      }                                                                                                            \
    }                                                                                                              \
  })
// ... and its record (PM_ROW_REC), eight words by ticket, a lane each: ticket seen, first pass packed, first keys, swept,
// finished, stored, how it was made | candidates, the CU it ran on
// reads: lane; everything else is a parameter (bulk: the BulkCtx, with its rec_pass / rec_keys)
#define PROP_REC_ROW(t, mode, n_mine, rec_seen, bulk, rec_swept, rec_fin)                                          \
  PM_REC(if (t < PM_STREAM_TRACE_CAP / 8u) {                                                                       \
    const uint64_t rec_end = STREAM_CLOCK();                                                                       \
    const uint32_t hw = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)); /* HW_ID */                   \
    const uint32_t swept_r = wave_sum(n_mine);                                                                     \
    const uint64_t w = lane == 0u ? rec_seen : lane == 1u ? bulk.rec_pass : lane == 2u ? bulk.rec_keys : lane == 3u ? rec_swept \
                       : lane == 4u ? rec_fin : lane == 5u ? rec_end : lane == 6u ? ((uint64_t)mode << 32 | swept_r) : (uint64_t)hw; \
    if (lane < 8u) p.stream_trace[(size_t)t * 8u + lane] = w;                                                      \
  })

// ---- the batch pipeline's preparation (PM_BATCH_LOG; experiment builds, tools/prune_probe.py)
// carve_prep_place_kernel — this block, start to ticket: sum, max, count (reads: tid)
#define BLOG_BLOCK_TICKET(pl_t0)                                                                                   \
  PM_BLOG(if (tid == 0) {                                                                                          \
    const uint64_t dt = PM_TICKS() - (pl_t0);                                                                      \
    atomicAdd((unsigned long long*)&p.status->prof[8], (unsigned long long)dt);                                    \
    atomicMax((unsigned long long*)&p.status->prof[9], (unsigned long long)dt);                                    \
    atomicAdd((unsigned long long*)&p.status->prof[10], 1ull);                                                     \
  })
// ... a line of the batch log (thread 0): what the preparation produced — nothing,
#define BLOG_LINE_NONE()                                                                                           \
  PM_BLOG({                                                                                                        \
    const uint32_t k = p.status->blog_n++;                                                                         \
    if (k < 512u) p.status->blog[3u * k] = p.status->blog[3u * k + 1u] = p.status->blog[3u * k + 2u] = 0u;         \
  })
// ... or a list
#define BLOG_LINE(n_list, n_seeds, cell_g)                                                                         \
  PM_BLOG({                                                                                                        \
    const uint32_t k = p.status->blog_n++;                                                                         \
    if (k < 512u) {                                                                                                \
      p.status->blog[3u * k] = (n_list);                                                                           \
      p.status->blog[3u * k + 1u] = (n_seeds);                                                                     \
      p.status->blog[3u * k + 2u] = (cell_g);                                                                      \
    }                                                                                                              \
  })
// ... the placement's span (thread 0 of the last block; prof[5]: the earliest block start) and its tail from pl_t1 on
#define BLOG_PLACED(pl_t1)                                                                                         \
  PM_BLOG({                                                                                                        \
    const uint64_t pl_t2 = PM_TICKS();                                                                             \
    p.status->prof[11] += (pl_t1) - p.status->prof[5]; /* first block start -> last block through */               \
    p.status->prof[12] += pl_t2 - (pl_t1);             /* the tail */                                              \
    p.status->prof[13] += 1ull;                                                                                    \
  })
// carve_propose_kernel — where a seed's walk over the spatial index stopped, what it cost (reads: lane)
#define BLOG_WALK(wt0, n_mine, stop_r)                                                                             \
  PM_BLOG(if (lane == 0) {                                                                                         \
    const uint64_t dt = PM_TICKS() - (wt0);                                                                        \
    unsigned long long* pr = (unsigned long long*)p.status->prof;                                                  \
    atomicAdd(&pr[0], (unsigned long long)dt);                                                                     \
    atomicMax(&pr[1], (unsigned long long)dt);                                                                     \
    atomicAdd(&pr[2], 1ull);                                                                                       \
    atomicAdd(&pr[3], (unsigned long long)(n_mine));                                                               \
    atomicAdd(&pr[16u + ((stop_r) < 15u ? (stop_r) : 15u)], 1ull);                                                 \
  })
