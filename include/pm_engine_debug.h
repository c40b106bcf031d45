/* pm_engine_debug.h — test hooks and instrumentation of libpm_engine.so.
 *
 * NOT part of the drop-in boundary (include/pm_engine.h is; the Rust shim binds nothing from here).  These entry
 * points exist for tests/, tools/ and bench.py: they force code paths a test could not otherwise reach, or read
 * counters back.  They are exported by every build of the library so that the tests run against the shipped binary;
 * tests/test_host_helpers.py checks that each one declared here is exported.
 */
#ifndef PM_ENGINE_DEBUG_H
#define PM_ENGINE_DEBUG_H

#include "pm_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Counters of the last carve.  out[0..32) and out[56..88): s_memtime phase counters (all zero unless the library was
 * built with -DPM_CARVE_PROF: tools/stream_prof.py, tools/carve_prof.py); out[32..56): how the carve went — reasons
 * its launches ended, index geometry, streaming-carve tickets / timeouts / switches (protocol_amd/engine.py
 * debug_carve_counters names them).  out[72..88): the row makers' anatomy, tools/stream_prof.py.  out[88..97): the
 * incremental state a long-running engine keeps, not the last carve's (engine.py debug_task_space;
 * tests/test_gpu_soak.py bounds it) — t_lo, t_cap (the task index space: the swept range is [t_lo, t_cap)), T (live
 * tasks), t_dead (tombstones inside the range), regrowths and compactions of the index space since creation, entries
 * of the host group list, its tombstones (dissolved, not yet compacted), retired snapshot buffers.  out[97]: the last
 * carve's again — times the streaming carve dropped a configuration's outstanding tickets and issued them afresh
 * (debug_carve_counters: stream_refreshes).  out[98], out[99]: the address book's pm_addresses_rank calls that ended on the
 * one-word sort (no two rows share their first ten characters) and on the all-words sort, since creation (engine.py
 * debug_address_sorts; off or on again does not reset them).  Copies min(cap, 100) words. */
int32_t pm_debug_carve_prof(pm_engine* e, unsigned long long* out, uint32_t cap);

/* Timeline of the last streaming carve launch (PM_CARVE_PROF builds; otherwise *n = 0): up to cap events of two words
 * {s_memtime, type | a << 8 | b << 32} (STREAM_TRACE, csrc/pm_measure.inc, lists the types); tools/stream_trace.py decodes them. */
int32_t pm_debug_stream_trace(pm_engine* e, unsigned long long* out, uint32_t cap, uint32_t* n);

/* Test hook: candidate lists longer than n slots take the all-in-HBM carve path (carve_step_mem), which otherwise
 * needs more than 262,144 candidates of one configuration; 0 = off. */
int32_t pm_debug_mem_lists_above(pm_engine* e, uint32_t n);

/* Test hook: the streaming carve (carve_variant 0) gives its launch up — CARVE_STATE_ABORTED, what a lost hand-shake
 * inside the validator workgroup ends in — as soon as n steps of the carve are committed (and the chain's budget runs
 * out there); the engine then continues the carve on the batch pipeline from the configuration it stopped in
 * (pm_stats / debug_carve_counters: stream_aborts).  0 = off. */
int32_t pm_debug_stream_abort_after(pm_engine* e, uint32_t n);

/* Counter: merge configurations (try_merge_groups_for_config, mod.rs:676-709) whose selections went through the streaming
 * carve (lists of PM_MERGE_STREAM_MIN = 512 compatible solo groups or more; the environment variable lowers it for tests)
 * since the engine was created. */
int32_t pm_debug_merge_streamed(pm_engine* e, uint32_t* n);

/* Counter: how often the device's copy of the group state was brought up to date by a DELTA — the workers of the groups
 * dissolved since and the rows appended since, a scatter and a fill — instead of compacting and uploading the whole list
 * (pm_engine.cpp push_groups: the path of a tick that follows status changes and new workers), since the engine was created.
 * pm_get_groups, pm_dissolve_group and the merge pass compact the list: the tick after them uploads it whole. */
int32_t pm_debug_delta_pushes(pm_engine* e, uint32_t* n);

/* Read-only: the way the last per-task call (pm_match_per_task, pm_match_per_task_device) took.  From 200,000 swept rows on
 * (t_cap - t_lo: tombstones count), below 64 configurations and with sweep_variant 0, the call counts the distinct masks of
 * the live tasks — restricted to the installed configurations, the empty mask left out — and sweeps once per distinct mask
 * while there are at most 65,536 of them; otherwise one row per task.  *distinct_masks = that count (0 when the call did
 * not count), *interned = 1 when it swept per distinct mask.  tests/test_gpu_task_table_edges.py holds both edges to it. */
int32_t pm_debug_per_task_path(pm_engine* e, uint32_t* distinct_masks, uint32_t* interned);

/* Test hook / experiment: when the proposers walk the spatial index instead of sweeping the whole candidate list —
 * 0 never, 1 when it pays (default), 2 whenever the carve has an index, 3 = 2 with every seed forced through the
 * whole-list fallback.  (PM_PRUNE_MODE in the environment sets the default of new engines.) */
int32_t pm_debug_prune_mode(pm_engine* e, uint32_t mode);

/* Stream triad (a = b + 3c, f64) over 3 x n_doubles on the engine's stream, best of reps: the measured HBM rate
 * bench.py cites beside the roofline's 8 TB/s. */
int32_t pm_debug_hbm_triad(pm_engine* e, uint64_t n_doubles, uint32_t reps, double* gb_per_s);

/* A measuring build's (-DPM_ROW_REC) record of the last streaming launch's rows: eight words per ticket — the real-time
 * counter (100 MHz, one clock for all CUs; the validator's events of such a build carry the same) when the ticket was seen, when the first pass of the sweep was packed, when the first batch's keys were there, when the candidates
 * were through, when the row was finished, when it was stored; candidates evaluated | mode << 32; hardware id.  n_rows = 0 from
 * a product build.  (These three records are written by PROP_REC_ROW, CHAIN_REC_* and PARK_REC_* of csrc/pm_measure.inc.) */
int32_t pm_debug_row_records(pm_engine* e, unsigned long long* out, uint32_t cap_rows, uint32_t* n_rows);
/* ... and the batches of steps its chain took up: four words each — the clock at the top of the chain's loop; first entry |
 * entries << 24 | live ones << 32 | commits so far << 40; the clock when the entries had been looked at; the clock behind the steps.
 * n = 0 from a product build. */
int32_t pm_debug_chain_batches(pm_engine* e, unsigned long long* out, uint32_t cap, uint32_t* n);
/* ... and the blocks of sixteen tickets its parkers took up, eight words each, indexed by first ticket / 16: first ticket | tickets
 * whose rows were asked for << 32 | tickets in the block << 48 | 1 << 63; clock at that moment; when the rows were all there; when the
 * block had its turn; when it had room in the ring; when it was parked; first entry | tickets parked << 32 | block of the run << 48. */
int32_t pm_debug_park_records(pm_engine* e, unsigned long long* out, uint32_t cap_blocks, uint32_t* n_blocks);

/* Neighbour rows two ways from the same keys (keys[n_waves * n_per_wave], ~0 = no candidate; the low slot_bits of a key index
 * sites[1 << slot_bits]; n_waves a multiple of four): the serial insertion, and four strides at a time through the sorting networks for the first `upto`
 * keys of a row (what the streaming carve's rows do).  Compared on the device: mismatches[0] = 1 a register differs | 2 a
 * threshold | 4 what a tracker answers, mismatches[1] = rows that differ; rows_out[n_waves * 64] = the networks' rows. */
int32_t pm_debug_row_networks(pm_engine* e, const uint64_t* keys, const uint32_t* sites, uint32_t n_waves, uint32_t n_per_wave,
                              uint32_t slot_bits, uint64_t ulps, uint32_t upto, uint64_t* rows_out, uint32_t* mismatches);

/* The same rows three ways — (0) the serial insertion, (1) the networks' out-of-line copy, (2) their inline copy, which the
 * streaming carve's sweep runs — and what near_row_finish makes of each (tests/test_gpu_row_certificates.py holds all of it to a
 * brute-force reference).  n_waves: a multiple of four, at most 4096; slot_bits: 13 or 18, the widths rows run at.  Per wave w and row r, at [w][r]: rows_out[64] the keys;
 * track_out[5] = tau, tau_hi, m1, m2, s1; and for K = 1 .. 63, at [K - 1], flags_out = the flags word of
 * near_row_finish(K, slot_bits, tie_band) and mine_out[64] = the lanes' entries.  mismatches: as above, rows 0 and 1. */
int32_t pm_debug_row_certificates(pm_engine* e, const uint64_t* keys, const uint32_t* sites, uint32_t n_waves, uint32_t n_per_wave,
                                  uint32_t slot_bits, uint64_t ulps, uint32_t upto, double tie_band, uint64_t* rows_out,
                                  uint64_t* track_out, uint32_t* flags_out, uint64_t* mine_out, uint32_t* mismatches);

/* The carve's distance key through the device functions the carve runs (tests/test_gpu_distance_key.py).  mode 0: in[5n] =
 * lat[2n] (the n first points, then the n second points), lon[2n], slot[n] (integers as f64); geo_kernel gives each point its
 * cos(lat) and unit vector, and per pair out[20n] holds, twenty f64 a pair: sin_band(dlat / 2), sin_band(dlon / 2), cos(lat)
 * and ux, uy, uz of the first point, the same of the second, hav_a, prox_a, 1 if prox_a took the chord form (else 0),
 * candidate_key's unpacked key (its f64 bits), then pack_key(prox_a, slot) at the 13, 18 and 21 slot bits of the library, and
 * pack_key(hav_a, slot) at the same three widths (f64 bits; the slot taken modulo the width).  mode 1: out[n] = sin_band(in[n]).
 * mode 2 (in, n unused): out[8] = PM_A_CHORD_MIN, PM_A_MAX_SAFE, the three certificate bands, the three slot widths.
 * mode 3: mode 0's input and kernel, but out[n] = candidate_key's unpacked key alone (word 13 of each record: the host copies
 * that column out of the device's records, a twentieth of the transfer — tests/test_gpu_first_batch.py asks for millions of
 * pairs). */
int32_t pm_debug_distance_keys(pm_engine* e, const double* in, uint32_t n, uint32_t mode, double* out);

/* The first batch of a formation on the batch pipeline (carve_variant 3), as the device holds it: pm_debug_first_batch_arm arms
 * a snapshot for the engine's NEXT formation (pm_form_groups, pm_tick); behind that formation's first propose launch — the list
 * preparation, the spatial index and the neighbour rows are all still in HBM, the validation launch not yet queued — the host
 * copies the parts below out in stream order into memory the engine owns, and the carve runs on as always (no kernel reads or
 * writes anything for this; unarmed the cost is one host-side branch).  An engine of another carve_variant refuses with
 * PM_ESTATE: the streaming carve keeps its rows in a ring for microseconds and has no such moment.
 * pm_debug_first_batch_get copies part `part` to out (cap_bytes) and returns its size in *n_bytes; out = NULL asks for the size
 * alone; PM_ESTATE when no snapshot was taken since the last arm (the formation had nothing to carve, or took another path:
 * the arm ends with that formation either way and is not carried to a later one).  A snapshot stands until the next arm.
 * Lengths: n = n_eligible, n_list, n_seeds, g = the carve's cell_g (the index parts are empty when it is 0), n_indexed. */
enum {
  PM_FB_HEAD = 0,    /* u32[PM_FB_HEAD_WORDS]: BatchDesc {planned, ci0, total_available, valid, none, ci, n_list, prop_k, prop_limit,
                        n_seeds, cell_g}; CarveStatus {n_eligible, cell_g, n_indexed, prune_fallbacks, pruned_batches, n_props,
                        prop_keys lo, hi}; the index scan's ticket word; CarveArgs::prune_mode; 0, 0, 0 */
  PM_FB_ORDER,       /* u32[n]   per position of the eligible list: the worker row */
  PM_FB_C_SITE,      /* u32[n] */
  PM_FB_C_UX,        /* f64[n] */
  PM_FB_C_UY,
  PM_FB_C_UZ,
  PM_FB_C_LAT,
  PM_FB_C_LON,
  PM_FB_C_COS,
  PM_FB_C_COMPAT,    /* u64[n] */
  PM_FB_LOC_G,       /* u64[ceil(n / 64)]  positions with a location */
  PM_FB_ALIVE_SNAP,  /* u64[ceil(n / 64)]  positions no group held when the list was prepared */
  PM_FB_SLOT_WID,    /* u32[n_list]  per slot of the prepared list: the worker row */
  PM_FB_SLOT_POS,    /* u32[n_list]  its position | has a location << 31 */
  PM_FB_CC_SITE,     /* u32[n_list] */
  PM_FB_SLOT_ALIVE,  /* u64[ceil(n_list / 64)] */
  PM_FB_SLOT_LOC,    /* u64[ceil(n_list / 64)] */
  PM_FB_SEED_MAP,    /* u64[ceil(prop_limit / 64)] */
  PM_FB_SEED_PREFIX, /* u32[ceil(prop_limit / 64)] */
  PM_FB_SEED_SLOTS,  /* u32[n_seeds] */
  PM_FB_PROP,        /* u64[n_seeds][PM_PROP_ROW = 96]: the flags word, 63 keys; from word 64 on 64 x u32: the flags, 63 slots */
  PM_FB_CELL_START,  /* u32[g^3 + 1] */
  PM_FB_CELL_CNT,    /* u32[g^3] */
  PM_FB_POS_CELL,    /* u32[n] */
  PM_FB_CS_OF_POS,   /* u32[n] */
  PM_FB_CS_SLOT,     /* u32[n_indexed] */
  PM_FB_CS_SITE,     /* u32[n_indexed] */
  PM_FB_CS_UX,       /* f64[n_indexed] */
  PM_FB_CS_UY,
  PM_FB_CS_UZ,
  PM_FB_PARTS
};
#define PM_FB_HEAD_WORDS 24
int32_t pm_debug_first_batch_arm(pm_engine* e);
int32_t pm_debug_first_batch_get(pm_engine* e, uint32_t part, void* out, uint64_t cap_bytes, uint64_t* n_bytes);

/* What every engine of this process holds from the HIP runtime right now: out[0] = device bytes, out[1] = pinned host bytes,
 * out[2] = events and streams.  Counted where an allocation is made or given back, not per call: an engine that is destroyed
 * returns all three to what they were before it was created (tests/test_gpu_lifetime.py). */
void pm_debug_live_allocations(uint64_t out[3]);

/* Test hook of the admission ledger's nonce set (pm_admission_enable): the standing array and each batch are sorted by the first
 * k bits of a nonce's digest instead of the first 64, so that a handful of nonces makes long runs of equal keys — equality is
 * still decided on all 256 bits over the run.  Not a call of its own: pm_admission_enable(e, PM_AD_DEBUG_PREFIX_BITS(k)) turns
 * admission on with 1 <= k <= 64 (bits 8 .. 15 of `on`; 0 there, as in a plain on = 1, is 64).  PM_EINVAL above 64. */
#define PM_AD_DEBUG_PREFIX_BITS(k) (1u | ((uint32_t)(k) << 8))

#ifdef __cplusplus
}
#endif
#endif
