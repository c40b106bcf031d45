// pm_device.h — argument blocks shared by the kernels (pm_kernels.hip) and the engine (pm_engine.cpp).
#ifndef PM_DEVICE_H
#define PM_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pm_engine.h"

namespace pm {

static constexpr double PM_RAD = 3.14159265358979323846 / 180.0;  // f64::to_radians factor
static constexpr uint64_t PM_KEY_NOLOC = 0x7FEFFFFFFFFFFFFFull;   // bits of f64::MAX (mod.rs:244,249)
static constexpr double PM_A_MAX_SAFE = 1.0 - 1.0 / 1048576.0;    // near-antipodal => settle on host
// below this Haversine term (about 14.5 km) the chord-length form of the key is not accurate enough for the
// certificate band and the proposer evaluates the sine form instead (see prox_a in pm_validate.inc): the chord form's
// error against the reference's a is up to 2e-15 / sqrt(a), and at 1.3e-6 that is 1.75e-12, within an eighth of the
// narrowest band (tests/test_distance_key_model.py)
static constexpr double PM_A_CHORD_MIN = 1.3e-6;
// carve kernel geometry
static constexpr uint32_t PM_CARVE_SLOTS = 8192;       // candidate slots with positions/bitmaps in LDS, keys in VGPRs
static constexpr uint32_t PM_CARVE_PART = 64;          // per-wave partial selection capacity (max_group_size - 1)
static constexpr uint32_t PM_CARVE_SEL_CAP = 256;      // selected slots staged in LDS before the member stores
static constexpr uint32_t PM_CARVE_SLOT_BITS = 13;     // log2(PM_CARVE_SLOTS): low key bits that hold the slot
static constexpr uint32_t PM_CARVE_BIG_SLOTS = 262144; // lists up to here keep their bitmaps + staged rows in LDS
static constexpr uint32_t PM_CARVE_SLOT_BITS_BIG = 18; // log2(PM_CARVE_BIG_SLOTS)
static constexpr uint32_t PM_CARVE_SLOT_BITS_MEM = 21; // same for lists kept in HBM (up to 2M candidates)
// certificate bands: 8x the truncation step of the packed key (2^-(52-bits)) — see carve_kernel
static constexpr double PM_TIE_BAND = 1.0 / 68719476736.0;      // 2^-36
static constexpr double PM_TIE_BAND_BIG = 1.0 / 2147483648.0;   // 2^-31
static constexpr double PM_TIE_BAND_MEM = 1.0 / 268435456.0;    // 2^-28
static constexpr uint32_t PM_PROP_ROW = 96;            // proposal row stride (u64 words): word 0 = flags, words 1..63 = keys,
static constexpr uint32_t PM_PROP_SLOTS = 64;          // then from this word on 64 x u32: flags, the slots of entries 0..62
static constexpr uint32_t PM_PROP_KMAX = 63;           // neighbours a row can list (word 0 carries the flags)
// flags word of a proposal row (low 32 bits of word 0): bits 0..7 entries, bits 8..15 first entry that lies within
// the certificate band of the LAST entry (a selection that ends in front of it never touches the row's tail)
static constexpr uint32_t PM_ROW_SAFE = 1u << 27;        // no listed Haversine term beyond PM_A_MAX_SAFE
static constexpr uint32_t PM_ROW_TAIL_CLEAR = 1u << 28;  // the first unlisted candidate is beyond the band of the last entry
static constexpr uint32_t PM_ROW_CLEAN = 1u << 29;       // no two entries within the band of each other at different sites
static constexpr uint32_t PM_ROW_TAIL_OK = 1u << 30;     // everything unlisted within the band of the last entry sits at its site
static constexpr uint32_t PM_ROW_COMPLETE = 1u << 31;    // the row lists every candidate that can be alive at its seed's turn: every live
                                                         // one but (FORM) the located ones in front of the seed, which are in a group by
                                                         // then — read at the seed's turn only (carve_fast_steps, carve_chain's second
                                                         // look, the parkers' digest for it), never for another seed or another moment
static constexpr uint32_t PM_PROP_RESERVE = 64;        // entries beyond max_group_size - 1: the proposer's register holds 64 sorted
                                                       // keys whatever K is, so every row is as long as a row can be (K = 63)
static constexpr uint32_t PM_PROP_MAX_SEEDS = 16384;   // located slots that get a proposal per configuration
// spatial index of a carve's located positions (cell_*_kernel): a G x G x G grid over the unit-vector cube [-1, 1]^3,
// x fastest, so a run of cells along x is one contiguous range of the cell-sorted entries
static constexpr uint32_t PM_CELL_G_MAX = 64;
static constexpr uint32_t PM_CELL_TABLE = PM_CELL_G_MAX * PM_CELL_G_MAX * PM_CELL_G_MAX + 2;  // starts of every cell + the end
static constexpr uint32_t PM_CELL_MIN_N = 6000;        // eligible positions below which the grid is 32^3 whatever is asked for (forced modes)
// eligible positions from which a carve builds the index of its own accord (prune_mode 1).  Measured with the streaming
// carve (profiles/r05_index_crossover.txt, tools/index_crossover.py): with and without the index a cold match costs
// the same within +-3 % from 6,000 to 30,000 workers (10,000: 1.074 against 1.047 ms — the four cell_* launches are
// not paid back), and the index wins from 50,000 on (3.88 against 3.99 ms; 100,000: 6.9 against 9.1)
static constexpr uint32_t PM_CELL_AUTO_N = 40000;
static constexpr uint32_t PM_CELL_BIG_N = 40000;       // ... from which the grid is 64^3 instead of 32^3
static constexpr uint32_t PM_CELL_RMAX = 14;           // rings of cells a seed walks before it falls back to the whole list
// part | alive, loc bitmaps | wid | site | key | sel_out | BlockRed + s_n
static constexpr size_t PM_CARVE_LDS_BYTES = size_t(16) * PM_CARVE_PART * 8 + size_t(PM_CARVE_SLOTS / 64) * 16 +
                                             size_t(PM_CARVE_SLOTS) * 16 + size_t(PM_CARVE_SEL_CAP) * 4 + 1024;
// ---- streaming carve (carve_stream_kernel): one launch per try_form_new_groups pass; workgroup 0 validates, the
// others compute neighbour rows for the seeds a bounded look-ahead in front of the chain
static constexpr uint32_t PM_STREAM_SQ = 8192;      // seed-ticket ring (8-byte granules): > waves that can hold a claim
static constexpr uint32_t PM_STREAM_RQ = 8192;      // row ring: rows of tickets t, t + RQ share a slot
static constexpr uint32_t PM_STREAM_TP = 4096;      // tickets whose seed position the validator remembers (LDS)
static constexpr uint32_t PM_STREAM_LA_MAX = 3072;  // look-ahead: tickets issued and not yet handed to the chain
static constexpr uint32_t PM_STREAM_CTL_WORDS = 64; // control block (u32): see the SC_* indices
#ifndef PM_STREAM_PROP_WAVES_N  // (settable in a variant build: with few row-making workgroups per pool — K pools on one
#define PM_STREAM_PROP_WAVES_N 4  // GPU — eight waves a workgroup trade a row's latency for rows per second)
#endif
static constexpr uint32_t PM_STREAM_PROP_WAVES = PM_STREAM_PROP_WAVES_N; // waves of a proposer workgroup that build rows (one per SIMD)
static constexpr uint32_t PM_STREAM_SLW_TREQ = PM_STREAM_TP;      // words of the validator's ticket state that
static constexpr uint32_t PM_STREAM_SLW_PAY = PM_STREAM_TP + 1;   // carve_fast_steps<STREAM> reads (pm_stream.inc: SLW_*)
static constexpr size_t PM_STREAM_LDS_BYTES = PM_CARVE_LDS_BYTES + size_t(PM_STREAM_TP) * 4 + 128;
// control words in global memory (each hot word on its own 64-byte line)
enum { SC_CLAIM = 0,    // next ticket a proposer wave takes (atomicAdd)
       SC_QUIT = 16,    // the validator is through: proposers leave
       SC_DROP = 32,    // configuration << 26 | ticket: that configuration's tickets below this one are not wanted any more (its
                        // tickets were issued afresh, or it is over) — a row maker that holds one lets it be
       SC_ROWS = 48,    // rows the proposers delivered (statistics)
       SC_LET_BE = 53,  // rows given up half-made because their ticket was dropped (statistics)
       SC_GAVE_UP = 49, // proposer waves that left because nothing was asked of them for too long
       SC_FINISH = 50,  // the carve launch ran (carve_finish_kernel has records to finish)
       SC_FINISH_TICKET = 52,  // carve_finish_kernel: blocks through (the last one mirrors the status to the host)
       SC_TRACE = 51,   // PM_CARVE_PROF builds: events written to the trace buffer
       SC_BATCHES = 54  // PM_ROW_REC builds: batches of steps the chain has recorded
};
static constexpr uint32_t PM_STREAM_TRACE_CAP = 1u << 17;  // events (two u64 each) of a PM_CARVE_PROF build's timeline
// how the rows of a ticket are made (bits 24..25 of the ticket's payload)
enum { SROW_NONE = 0, SROW_BITMAP = 1, SROW_WALK = 2, SROW_SWEEP = 3 };

struct CompatArgs {
  uint32_t W, n_cfgs, model_words;
  const uint32_t *flags, *gpu_count, *gpu_mem, *gpu_cls, *cpu_cores, *ram, *storage;
  const pm_config_row* cfgs;
  const pm_gpu_alt_row* alts;
  const uint32_t* model_bits;
  uint64_t* compat;
};

// counters of one configuration in ReportArgs::out / the LDS copy (REP_STRIDE words a configuration)
enum : uint32_t {
  REP_WHY = 0,  // [0, PM_WHY_N): eligible workers by code
  REP_IDLE = PM_WHY_N,
  REP_GROUPS,
  REP_MEMBERS,
  REP_NO_TASK,
  REP_TASKS,
  REP_STRIDE = 16
};

struct ReportArgs {
  CompatArgs c;                 // worker columns (flags: the current host column), configurations, alternatives, model rule
  const int32_t* group_of;      // current (host truth): -1 = in no group
  // the group list: slots [0, G); live_bits (one bit a slot) marks the live ones, nullptr = all of them
  const uint32_t *g_cfg, *g_n, *g_task, *live_bits;
  uint32_t G;
  // the task index space [t_lo, t_cap): topology masks, live bitmap, per-word live prefix (positions)
  const uint64_t *tmask, *tlive;
  const uint32_t* tprefix;
  uint32_t t_lo, t_cap;
  uint32_t* out;                // pm_config_report: [n_cfgs][REP_STRIDE]; pm_task_report: [PM_MAX_CONFIGS] groups per config
  uint32_t *running, *workers, *allowed;  // pm_task_report, T entries each (running / workers zeroed beforehand)
};

// pm_group_spread / pm_config_spread (pm_spread.inc).  Output row k is the k-th live group; it reads slot slot_of_row[k]
// of the group arrays (the device mirror in place, or a dense scratch copy).  `small` / `big` list the rows of groups of
// at most 64 / more than 64 members.
struct SpreadArgs {
  const uint32_t *g_n, *g_off, *members, *slot_of_row, *small, *big;
  uint32_t n_small, n_big, W;
  const uint32_t *flags, *addr_rank;  // flags: the current host column
  const double *lat, *lon, *coslat;
  pm_group_spread_row* out;
};
// one configuration's accumulators of config_spread_kernel
enum : uint32_t { SPC_GROUPS = 0, SPC_MEASURED = 1, SPC_HIST = 2, SPC_N = 2 + PM_SPREAD_BUCKETS, SPC_STRIDE = 8 };
enum : uint32_t { SPV_MAX_DIAMETER = 0, SPV_MAX_HOP = 1, SPV_SUM_DIAMETER = 2, SPV_SUM_RING = 3 };
struct SpreadCfgAcc {
  uint32_t cnt[SPC_STRIDE];
  unsigned long long v[4];
};

// pm_nearest_workers (pm_near.inc): one workgroup per query.  Output of query q: rows[q], workers[q * k + j], km[q * k + j].
static constexpr uint32_t PM_NEAR_CAP = 2u * PM_NEAR_MAX_K;  // a wave's selection buffer: max(2 k, k + 64) entries
struct NearArgs {
  CompatArgs c;                 // worker columns (flags: the current host column), configurations, alternatives, model rule
  const int32_t* group_of;      // current (host truth): -1 = in no group
  const double *lat, *lon, *coslat;
  const pm_near_query* q;
  uint32_t n_q, pool, k;
  pm_near_row* rows;
  uint32_t* workers;
  double* km;
};

// pm_probe_configs / pm_config_overlap (pm_probe.inc).  Counters of one probe in ProbeArgs::out / the LDS copy (PRB_STRIDE
// words a probe), then the P x C matrix of idle workers that meet probe p and installed configuration c.
enum : uint32_t {
  PRB_WHY = 0,  // [0, PM_WHY_N): eligible workers by code
  PRB_IDLE = PM_WHY_N,
  PRB_LOCATED,
  PRB_EXCL,
  PRB_STRIDE = 16
};
struct ProbeArgs {
  CompatArgs c;             // worker columns (flags: the current host column) and the INSTALLED tables
  CompatArgs p;             // the same columns with the probes' rows, alternatives and model bits (n_cfgs = probes)
  const int32_t* group_of;  // current (host truth): -1 = in no group
  uint64_t enabled;         // pm_set_enabled_mask bits (idle_exclusive)
  uint32_t* out;            // [P][PRB_STRIDE] then [P][C], zeroed beforehand
  uint64_t* mask_out;       // [W] or nullptr
};

// the change feed (pm_changes.inc): what a publish remembers of a worker's row.  All zeroes = in no group (next_worker and the
// task handle are stored complemented: PM_NONE reads 0), so rows a grown buffer has just gained need no initialising pass.
struct alignas(16) ChangeIdent {
  uint32_t group_id_lo, group_id_hi, group_index, group_size;
  uint32_t not_next_worker, not_task_handle, unused[2];
};
static constexpr uint32_t PM_CHG_SCAN_WORDS = 4;  // bitmap words a thread of change_scan_kernel takes per pass (x 256 threads)
struct ChangeDiffArgs {
  uint32_t W, G, resync;        // rows; group slots g_task holds; != 0: every row < W changed, all bits
  const pm_assignment* table;   // the committed table (d_table)
  const uint32_t* g_task;       // the committed task words: handles
  ChangeIdent* ident;           // [W] remembered identities
  uint8_t* what;                // [W] pending PM_CHG_* bits
  uint64_t* bitmap;             // [ceil(W / 64)] pending rows
};

// liveness (pm_liveness.inc): one process_nodes pass over the ledger
struct LiveSweepArgs {
  uint32_t W, m;             // rows; missing_heartbeat_threshold
  uint64_t now_ms;
  const uint64_t* beat;      // [W] last beat, ms; 0 = never
  const uint64_t* pool;      // [ceil(W / 64)] is_node_in_pool bits, or nullptr = all in pool
  uint8_t* status;           // [W] PM_NS_*
  uint32_t* counter;         // [W]
  uint8_t* old_status;       // [W] written for listed rows only
  uint64_t* bitmap;          // [ceil(W / 64)] listed rows: every word is stored
  uint32_t* census;          // [PM_NS_N], zero at launch
};

// discovery sync (pm_discovery.inc): one DiscoveryMonitor pass, the ledger's status column joined with the discovery list
struct DiscArgs {
  uint32_t W, D, E, max_same;  // table rows; discovery rows; endpoint ids; max_healthy_nodes_with_same_endpoint
  uint64_t now_ms;
  const pm_disc_row* rows;     // [D]
  const uint32_t* row_endpoint;  // [W] endpoint id or PM_EP_NONE
  uint8_t* status;             // [W] the ledger's status bytes
  uint32_t* pos_of_row;        // [W] position in the list, preset to PM_DISC_NEW (= unlisted)
  uint32_t* base;              // [E] S: unlisted Healthy rows per endpoint, zero at launch
  uint32_t* ev_cnt;            // [E] events per endpoint, zero at launch
  uint32_t* ev_off;            // [E] first event of the endpoint's segment (written where ev_cnt != 0)
  uint32_t* ev_fill;           // [E] scatter cursor inside the segment, zero at launch
  uint32_t* cursor;            // [1] segments handed out so far, zero at launch
  uint64_t* events;            // [sum of ev_cnt <= 2 D] position << 1 | kind (0 = before, 1 = after)
  pm_disc_result* out;         // [D]
};

// metrics ledger (pm_metrics.inc).  Internal row 0 is the manual row, internal row w + 1 is worker w; R = rows of the table.
static constexpr uint32_t PM_MX_TOUCHED = 0x80000000u;  // a row's new length word: the fold wrote it (the copy skips the row)
static constexpr uint32_t PM_MX_CHUNK = 1024;           // entries of one radix chunk: fixed, so the regroup does not depend on the grid
struct MxFoldArgs {
  uint32_t n_touched;
  const uint32_t* t_row;     // [n_touched] internal row, no two equal
  const uint32_t* t_first;   // [n_touched] first of the row's beats in `beats`
  const uint32_t* t_nb;      // [n_touched] its beats (contiguous, in batch order)
  const pm_mx_beat* beats;   // the batch's beats, stably sorted by row
  const pm_mx_entry* entries;
  const uint32_t* off_old;   // [R + 1]
  const uint32_t* ser_old;
  const double* val_old;
  uint32_t* new_n;           // [R] count pass: length | PM_MX_TOUCHED of every touched row
  uint32_t* over;            // [1] count pass: != 0 = a row would pass PM_MX_ROW_MAX
  const uint32_t* off_new;   // [R + 1] write pass
  uint32_t* ser_new;
  double* val_new;
};
struct MxRowsArgs {
  uint32_t n, total;           // listed rows; entries to write
  const uint32_t* rows;        // [n] internal rows, or nullptr: row k is internal row k
  const uint32_t* out_off;     // [n + 1] first output entry of listed row k
  const uint32_t* off;         // [R + 1] the ledger
  const uint32_t* ser;
  const double* val;
  const int32_t* group_of;     // [W] host truth, -1 = in no group
  const uint64_t* g_id;        // per group slot
  const uint32_t* g_cfg;
  pm_mx_row* out;
};

// rollout ledger (pm_rollout.inc).  A group slot is an index into the host's list as it stands (tombstones included); what the
// reads report is RoGroup::slot, the slot pm_get_groups would number it.
static constexpr uint32_t PM_AB_WORDS = 4;                 // address book: 64-bit words of a row's text key, 10 characters of 5 bits each
static constexpr uint32_t PM_AB_PASSES = 7;                // ... radix passes of 8 bits over a word's 50
static constexpr uint32_t PM_AB_TEXT = 43;                 // ... bytes of a rendered text: "0x", 40 characters, NUL
static constexpr uint32_t PM_RO_CHUNK = 1024;             // keys of one radix chunk: fixed, so the sort does not depend on the grid
static constexpr uint32_t PM_RO_GCNT = PM_TS_N + 2;       // a group's counters: same[PM_TS_N], other, silent
static constexpr uint32_t PM_RO_CLAIM = 0x80000000u;      // a sorted key's side word: a group's claim (| list slot), else a reporter's state
static constexpr uint32_t PM_RO_CENSUS = PM_RO_N + PM_TS_N + 2;  // by_class, by_state (+ no report), groups_converged
struct RoGroup {  // 32 bytes, one per entry of the host's list
  uint64_t id, uid;   // the group's id; the claimed task's id
  uint32_t cfg, task;  // configuration; the claimed task's position in the current list, PM_NONE: it holds none
  uint32_t size;
  uint32_t slot;      // its slot in pm_get_groups order, PM_NONE: dissolved
};
struct RoPrepArgs {
  uint32_t W, G;
  const int32_t* group_of;  // [W] host truth, -1 = in no group
  const RoGroup* g;         // [G]
  const uint64_t* uid;      // [W] the ledger
  const uint8_t* state;     // [W]
  uint8_t* cls;             // [W] out: PM_RO_*
  uint32_t* g_cnt;          // [G * PM_RO_GCNT] zeroed; out
  uint32_t* census;         // [PM_RO_CENSUS] zeroed; out
  uint32_t* flag;           // [W + G] out: row w reports / list entry g is listed
  const uint32_t* off;      // [W + G + 1] the flags' exclusive scan (the emit pass)
  uint64_t* key;            // [N] out: the ids of the reporters, behind them those of the claims
  uint32_t* val;            // [N] out: the state, or PM_RO_CLAIM | list slot
};

// node directory (pm_directory.inc): the ordered, paged listing over the liveness ledger, the groups and the rollout ledger
static constexpr uint32_t PM_DIR_NO_CLASS = 0xFFu;        // DirArgs::cls of a row the query does not list
struct DirGroup {  // 24 bytes, one per entry of the host's list (tombstones included)
  uint64_t id;
  uint32_t cfg, task;  // configuration; the claimed task's position in the current list, PM_NONE: it holds none
  uint32_t size;
  uint32_t slot;       // its slot in pm_get_groups order, PM_NONE: dissolved
};
struct DirArgs {
  uint32_t W, G;
  uint32_t status_mask, membership;  // the query's filter (pm_dir_query)
  uint32_t offset, n_rows;           // the window [offset, offset + n_rows) of the ordered list
  const uint8_t* status;     // [W] the liveness ledger
  const uint32_t* counter;   // [W]
  const int32_t* group_of;   // [W] host truth, -1 = in no group
  const DirGroup* g;         // [G]
  const uint32_t* addr_rank; // [W]
  const uint64_t* uid;       // [W] the rollout ledger, or nullptr: it is off
  const uint8_t* state;      // [W]
  uint8_t* cls;              // [W] out: PM_DC_*, PM_DIR_NO_CLASS: not listed
  uint32_t* flag;            // [PM_DC_N * W] out, class-major: row w is listed in class c
  uint32_t* census;          // [PM_NS_N] zeroed; out: listed rows per status
  const uint32_t* off;       // [PM_DC_N * W + 1] the flags' exclusive scan: a listed row's place in (class, row) order
  uint32_t* win;             // [n_rows] out (BY_ROW): the window's rows
  uint64_t* key;             // [total] out (BY_ADDRESS): class << 32 | rank, in (class, row) order
  uint32_t* val;             // [total] out: the row
};

// group directory (pm_groupdir.inc): the groups' ordered, filtered, paged listing joined with both ledgers.  A list entry's
// record is the rollout ledger's RoGroup (the id, the claimed task's id and position, the size, the reported slot).
static constexpr uint32_t PM_GD_CNT = PM_NS_N + 4;            // a group's counters: by_status[PM_NS_N], converged, behind, other, silent
static constexpr uint32_t PM_GD_CENSUS = PM_MAX_CONFIGS + PM_GH_N + PM_GR_N + 1;  // by_config, by_health, by_rollout, members_total
static constexpr uint32_t PM_GD_TEXT_CLASSES = 16;            // BY_ID_TEXT: the hex digits of a u64 id, 1..16
static constexpr uint32_t PM_GD_NO_CLASS = 0xFFu;             // GdirArgs::cls of an entry the query does not list
struct GdirArgs {
  uint32_t W, G;
  uint64_t config_mask;              // the query's filter (pm_gdir_query)
  uint32_t holds, size_min, size_max, health_mask, rollout_mask, order;
  uint32_t n_cls;                    // classes of the ordered compaction: PM_GD_TEXT_CLASSES (BY_ID_TEXT) or 1
  uint32_t offset, n_rows;           // the window [offset, offset + n_rows) of the ordered list
  const int32_t* group_of;   // [W] host truth, -1 = in no group
  const RoGroup* g;          // [G]
  const uint8_t* status;     // [W] the liveness ledger, or nullptr: it is off
  const uint64_t* uid;       // [W] the rollout ledger, or nullptr: it is off
  const uint8_t* state;      // [W]
  uint32_t* g_cnt;           // [G * PM_GD_CNT] zeroed; out (member pass), in (group pass, emit)
  uint32_t* census;          // [PM_GD_CENSUS] zeroed; out
  uint8_t* cls;              // [G] out: the entry's class of the compaction, PM_GD_NO_CLASS: not listed
  uint8_t* hr;               // [2 G] out: the entry's health and rollout class
  uint32_t* flag;            // [n_cls * G] out, class-major: entry k is listed in class c
  const uint32_t* off;       // [n_cls * G + 1] the flags' exclusive scan: a listed entry's place in (class, slot) order
  uint32_t* win;             // [n_rows] out (BY_SLOT): the window's entries
  uint64_t* key;             // [total] out (sorted orders): the sort key, in (class, slot) order
  uint32_t* val;             // [total] out: the entry
};

// task directory (pm_taskdir.inc): the tasks' ordered, filtered, paged listing joined with the groups' claims and the rollout
// ledger.  A SLOT is a handle of the task index space counted from t_lo: slot r is handle t_lo + r, r < R = t_cap - t_lo.
enum : uint32_t {  // a slot's counters
  TD_RUNNING = 0,       // live groups that hold the row
  TD_WORKERS,           // their members
  TD_HOLD_CONV,         // those of them that are converged
  TD_ALLOWED,           // live groups of the configurations its mask allows
  TD_G_CONV,            // the reported columns, by id: pm_ro_task_row.groups_converged,
  TD_CONV,              // ... .converged,
  TD_REP,               // ... .reporters[PM_TS_N]
  PM_TD_CNT = TD_REP + PM_TS_N
};
enum : uint32_t {  // the census, behind the per-configuration counts
  TD_C_SERVE = PM_MAX_CONFIGS,
  TD_C_ROLLOUT = TD_C_SERVE + PM_TKS_N,
  TD_C_UNRESTRICTED = TD_C_ROLLOUT + PM_TKR_N,
  TD_C_WORKERS,
  TD_C_REPORTERS,
  TD_C_ORPHAN_UIDS,
  TD_C_ORPHAN_REPORTERS,
  PM_TD_CENSUS
};
struct TdirGroup {  // 16 bytes, one per entry of the host's list (tombstones included)
  uint32_t cfg, size;
  uint32_t handle;    // the claimed task's handle, PM_NONE: it holds none
  uint32_t live;      // 0: dissolved
};
struct TdirArgs {
  uint32_t G, n_cfgs, t_lo, t_cap;
  uint64_t config_mask;              // the query's filter (pm_tdir_query)
  uint32_t serve_mask, rollout_mask, workers_min, workers_max, order;
  uint32_t rollout_on;
  uint32_t offset, n_rows, total;    // the window [offset, offset + n_rows) of the ordered list of `total` entries
  const TdirGroup* g;        // [G]
  const uint32_t* ro_gcnt;   // [G * PM_RO_GCNT] the rollout ledger's counters of the groups, or nullptr: it is off
  const uint64_t *tmask, *tlive;  // the task index space: masks, live bitmap,
  const uint32_t* tprefix;        // per-word live prefix (positions),
  const int64_t* created;         // created_at
  uint32_t* g_per_cfg;       // [PM_MAX_CONFIGS] zeroed; out (group pass): live groups per configuration
  uint32_t* cnt;             // [R * PM_TD_CNT] zeroed; out (group pass, join, task pass), in (emit)
  uint32_t* census;          // [PM_TD_CENSUS] zeroed; out
  uint8_t* cls;              // [2 R] out: the slot's serving and rollout class
  uint32_t* flag;            // [R] out: the slot is listed
  const uint32_t* off;       // [R + 1] the flags' exclusive scan: a listed slot's place in list order
  uint32_t* win;             // [n_rows] out (BY_LIST, BY_OLDEST): the window's slots
  uint64_t* key;             // [total] out (the _DESC orders): the complemented key, in list order
  uint32_t* val;             // [total] out: the slot
};

struct ClaimArgs {
  uint32_t R;            // rows: all workers, or the workers `rows` lists (multi-GPU: the ones this rank owns)
  const uint32_t* rows;  // nullptr = row r is worker r
  const int32_t* group_of;
  const uint32_t *g_n, *g_off, *g_task;
  const uint64_t* g_id;
  uint32_t* g_task_next;
  const uint32_t* chosen;         // per row
  const uint32_t* rank_in_group;  // per worker
  const uint32_t* by_rank;        // per member slot: worker of that rank
  const uint64_t* t_live;     // task table: live bitmap and live-prefix per word (handle -> published position)
  const uint32_t* t_prefix;
  pm_assignment* table;  // per worker; with `rows`: per row (this rank's segment of the exchange buffer)
  uint32_t* task_col;    // compact per-worker task column (device-side consumers; not written with `rows`)
  // The snapshot buffer the look-ups will read (pinned host memory, the one that is not current) and the groups' task words
  // beside it: written by the claim itself — a row is 32 bytes of a coalesced store over PCIe — instead of by two copies
  // queued behind it (each a launch of the runtime's copy kernel with a 12 us gap in front).  nullptr: the caller copies.
  pm_assignment* h_table;
  uint32_t* h_gtask;     // [groups]: written by the group's member of rank 0
};

// Behind the carve, in front of the pair sweep (one engine, every worker a row): what is per worker or per group and needs
// no pair — the worker's selector, the sweep's outputs at their neutral values, GROUP_INDEX and the members by rank, the
// groups' task words carried over — in ONE launch where there were three kernels and a copy (each 4 - 5 us with 5 - 6 us of an
// idle GPU in front: profiles/r06_timeline.txt).
struct MatchPrepArgs {
  uint32_t W, G;
  const int32_t* group_of;
  const uint32_t *g_cfg, *g_n, *g_off, *members, *addr_rank, *g_task;
  uint64_t* sel;                      // [W]
  uint32_t *first, *count;            // [W]: PM_NONE / 0
  uint32_t *rank_in_group, *by_rank;  // group_rank_kernel's outputs
  uint32_t* g_task_next;              // [G] <- g_task
};

// pm_update_workers / pm_append_workers: n packed rows (one H2D copy) scattered into the worker columns
struct RowUpdateArgs {
  uint32_t n;
  const double *lat_in, *lon_in;  // [n] each
  const uint32_t* u32_in;         // 10 columns of n: idx, flags, gpu_count, gpu_mem, gpu_cls, cpu_cores, ram, storage, addr_rank, site
  uint32_t *flags, *gpu_count, *gpu_mem, *gpu_cls, *cpu_cores, *ram, *storage, *addr_rank, *site;
  double *lat, *lon, *coslat;
  double *ux, *uy, *uz;  // unit vector of the location (cos lat cos lon, cos lat sin lon, sin lat)
};

enum { CARVE_MODE_FORM = 0, CARVE_MODE_MERGE = 1 };
enum { CARVE_STATE_RUNNING = 0, CARVE_STATE_DONE = 1, CARVE_STATE_UNCERTAIN = 2, CARVE_STATE_OVERFLOW = 3,
       CARVE_STATE_ABORTED = 4 };  // ABORTED: a bounded wait inside the launch gave up (what was committed stands)
// launch flags of carve_kernel
enum {
  CARVE_F_INIT = 1u << 0,   // build the eligible list + position columns (first launch of a carve)
  CARVE_F_RUN = 1u << 1,    // process the prepared configuration
  CARVE_F_ALL = 1u << 2,    // keep going through every configuration in this launch (no proposals)
  CARVE_F_PROPS = 1u << 3,  // neighbour-list proposals of carve_propose_kernel are available
  CARVE_F_EXTPREP = 1u << 4 // the candidate lists are prepared by carve_prep_*_kernel between the launches
};
// Device-resident state of one carve (try_form_new_groups / one merge configuration); it persists across
// the launches of the propose / validate sequence.
struct CarveStatus {
  uint32_t state;
  uint32_t stop_ci;      // configuration (position in the carve order) to resume at after UNCERTAIN
  uint32_t n_groups;     // records written so far (in/out)
  uint32_t n_members;    // member slots used so far (in/out)
  uint32_t steps_total;  // committed steps over all launches of this tick
  uint32_t n_eligible;   // length of the eligible list
  uint32_t cur_ci;       // prepared configuration (position in the carve order); n_avail = none left
  uint32_t n_list;       // slots of the prepared candidate list
  unsigned long long cand_sum;  // sum over committed steps of the candidates scanned
  uint32_t prop_k;       // entries per proposal for the prepared configuration (0 = no proposals)
  uint32_t prop_limit;   // proposals exist for located slots below this slot number
  uint32_t n_seeds;      // seeds of the batch
  uint32_t total_available;
  uint32_t fast_steps;   // steps committed from proposals
  uint32_t slow_steps;   // steps that needed the full key sweep
  uint32_t n_solo;       // single-node groups carved (the merge pass only runs when there are two or more)
  uint32_t n_props;      // neighbour lists computed by this rank's proposer
  uint32_t g_lo, g_hi;   // groups appended by the last validation launch (their group_of is written by the prep kernels)
  uint32_t n_batches;    // validation launches that had a prepared list to run (the host sizes its next queue by it)
  uint32_t n_void;       // validation launches whose batch had been prepared for another configuration, or for nothing
  // how validation launches ended: 0 chain: list thinned out, 1 seeds of the batch used up, 2 exact step: thinned out,
  // 3 configuration exhausted, 4 batch prepared for another configuration, 5 batch too stale, 6 configuration not entered
  uint32_t why[8];
  uint32_t stream_timeouts; // streaming carve: rows the validator stopped waiting for (the step took the exact sweep)
  uint32_t stream_tickets;  // streaming carve: seeds handed to the proposers
  uint32_t stream_switches; // streaming carve: configurations that went from walking the index to sweeping the bitmap
  uint32_t stream_listed;   // streaming carve: configurations entered sweeping the bitmap
  uint32_t stream_pre_used; // streaming carve: configurations that started on tickets issued ahead
  uint32_t stream_pre_lost; // streaming carve: tickets issued ahead for a configuration that was not the next one
  uint32_t stream_refreshes; // streaming carve: times a configuration's outstanding tickets were dropped and issued afresh
  uint32_t _pad_sr;
  uint32_t cell_g;          // grid size of the spatial index built for this carve's positions (0 = none)
  uint32_t n_indexed;       // located positions in the index
  uint32_t pruned_batches;  // batches whose proposals walked the index instead of the whole list
  uint32_t prune_fallbacks; // seeds of such batches that gave up on the index (rings exhausted) and swept the list
#ifdef PM_BATCH_LOG  // (experiment builds, tools/prune_probe.py: what every preparation of the carve produced)
  uint32_t blog_n;
  uint32_t blog[3 * 512];   // per preparation: list length (0 = none), seeds, grid of the walk (0 = whole-list sweep)
#endif
  unsigned long long prop_keys;  // keys (Haversine terms) those sweeps evaluated
  unsigned long long prof[64];  // PM_CARVE_PROF builds: accumulated s_memtime ticks per phase
};

// The proposal batch as its preparation describes it: carve_prep_count_kernel plans it from the carve's own state
// (plan_batch) and carve_prep_place_kernel fills it in; the proposer and the validator read it.  There is one batch
// at a time, prepared behind the validation launch in front of it on the same stream.  The host queues these
// launches without looking, so the validator takes a batch only if it started from the configuration the carve is
// at (ci0); a launch that finds another is void (CarveStatus::n_void).
struct alignas(16) BatchDesc {  // (48 bytes, not 44: the host clears it with ONE fill, a size off 8 bytes takes two)
  uint32_t planned;          // the plan ran (the carve was RUNNING)
  uint32_t ci0;              // configuration (position in the carve order) the preparation started from
  uint32_t total_available;  // as of the plan (an upper bound of what the validator will find)
  uint32_t valid;            // a candidate list was prepared: configuration `ci`, the first from ci0 on that can be entered
  uint32_t none;             // no configuration from ci0 on can be entered any more
  uint32_t ci, n_list, prop_k, prop_limit, n_seeds;
  uint32_t cell_g;           // the proposals of this batch walk the spatial index (grid size; 0 = sweep the whole list)
};

struct CarveArgs {
  uint32_t mode;   // CARVE_MODE_*
  uint32_t W;
  uint32_t proximity;
  uint32_t debug_uncertain_every;
  // worker columns
  const uint32_t* wflags;
  const double *lat, *lon, *coslat;
  const double *ux, *uy, *uz;  // unit vectors: the proposer's chord-length key (see prox_key)
  const uint32_t* site;  // equal (lat, lon) bit patterns <=> equal site id (host-interned)
  const uint64_t* compat;
  int32_t* group_of;  // FORM: read (eligibility) and written (commit)
  // ordered eligible list: FORM -> written by the kernel (eligible rows in input order);
  // MERGE -> supplied by the engine (nodes of the compatible solo groups in group-id order)
  uint32_t* order;
  uint32_t n_order;
  uint32_t _pad2;
  // scratch (capacity W each): columns indexed by position in the eligible list ...
  double *c_lat, *c_lon, *c_cos;
  double *c_ux, *c_uy, *c_uz;
  uint32_t* c_site;
  uint64_t* c_compat;
  uint64_t *alive_g, *loc_g;  // bitmaps over positions (bits_stride words each)
  // ... and by candidate slot of the prepared configuration
  double *cc_lat, *cc_lon, *cc_cos;
  double *cc_ux, *cc_uy, *cc_uz;
  uint32_t* cc_site;
  uint32_t* slot_pos;      // slot -> position (for the alive_g write-back)
  uint32_t* slot_wid;      // slot -> worker id
  uint64_t* bits_scratch;  // slot bitmaps: alive, loc (bits_stride words each)
  uint64_t* keys;          // packed keys when the candidate list does not fit in LDS
  uint32_t bits_stride;
  uint32_t _pad0;
  // proposals (carve_propose_kernel): one row of PM_PROP_ROW u64 per seed of the batch — the flags word (PM_ROW_*)
  // in word 0, then the packed keys sorted ascending.  Seed i of a batch (rank among the live located slots
  // below prop_limit) has row i.  Every engine makes all rows of its own carve: a multi-GPU engine carves the
  // whole pool like a single one, and the carve knows no rank.
  uint64_t* prop;
  uint64_t* seed_map;      // per bitmap word below prop_limit: the batch's seeds (live & located at preparation)
  uint32_t* seed_prefix;   // per bitmap word: seeds in front of the word
  uint32_t* seed_slots;    // seed number -> slot (PM_PROP_MAX_SEEDS + 64 entries)
  uint32_t count_keys, _pad_ck;  // proposer: count the keys it sweeps (bench bookkeeping)
  uint32_t* prep_block_counts;   // [blocks][PM_MAX_CONFIGS] live compatible positions per block and configuration
  uint32_t* prep_counts;         // [PM_MAX_CONFIGS] totals, [PM_MAX_CONFIGS] = finished-blocks ticket
  BatchDesc* desc;               // this argument block's batch (the per-batch scratch above belongs to it)
  uint64_t* alive_snap;          // the position bitmap as the preparation saw it (bits_stride words)
  uint32_t _pad_sp;
  uint32_t debug_mem_above;      // test hook: candidate lists longer than this take the all-in-HBM path (0 = off)
  // spatial index over the located positions (built once per carve behind the eligible list, see cell_count_kernel)
  uint32_t* cell_cnt;            // [PM_CELL_TABLE] members per cell while the index is built; zero between builds
  uint32_t* cell_start;          // [PM_CELL_TABLE] first entry of every cell (+ the end)
  uint32_t *pos_cell, *pos_rank; // per position: its cell, its rank among the cell's members
  uint32_t* cs_of_pos;           // per position: its entry in cell order (located positions only)
  uint32_t* cs_slot;             // per entry: the candidate slot it has in the prepared list, ~0 = none (per batch)
  double *cs_ux, *cs_uy, *cs_uz; // per entry: unit vector
  uint32_t* cs_site;             // per entry: site id
  uint32_t prune_mode;           // 0 never, 1 when it pays (list length vs live fraction), 2 whenever there is an index,
                                 // 3 = 2 with every seed forced through the whole-list fallback (test hooks)
  uint32_t prune_factor;         // mode 1: walk when n_list^2 >= prune_factor x (indexed positions)
  uint32_t walk_cap_div, _pad_w; // seeds of a batch that walks the index: n_list / walk_cap_div
  // ---- streaming carve (carve_stream_kernel).  Slot == position: cc_* alias c_*, slot_wid aliases order,
  // bits_scratch = {the published `free` bitmap (positions no group holds yet — the proposers' view, a few commits
  // behind), loc_g}, alive_g = the validator's own master copy of it (brought up to date between configurations).
  uint32_t stream, stream_tag0;  // stream: 1 = this argument block drives carve_stream_kernel; tag0: first ticket tag
  // gather copies of the columns a row maker reads per candidate, 32 bytes a record = ONE memory line per candidate
  // instead of five (unit vector x 3, site, located bit): {ux, uy, uz, site | located << 32} — a row is a chain of
  // gathers, and its latency is what the chain waits for at every cold start
  double* c_pack;                // [n][4] by position (carve_elig_place_kernel)
  double* cs_pack;               // [n_indexed][4] by entry of the spatial index (cell_place_kernel)
  uint64_t* cfgbits;             // [n_avail][bits_stride] per configuration (carve order): compatible positions
  unsigned long long* stream_sq;      // [PM_STREAM_SQ] seed tickets: {tag, position | ci << 18 | mode << 24}
  unsigned long long* stream_row_lo;  // [PM_STREAM_RQ][64] rows: {tag, flags word | low half of the packed key of entry g - 1}
  unsigned long long* stream_row_hi;  // [PM_STREAM_RQ][64]       {tag, high half}
  uint32_t* stream_ctl;               // [PM_STREAM_CTL_WORDS] SC_*
  uint32_t stream_la, stream_row_spins;  // look-ahead cap (0 = default); polls before the validator gives a row up
  uint32_t stream_la_div;                // look-ahead = candidates / (la_div x (max_group_size - 1)) (0 = default)
  uint32_t debug_abort_after;            // test hook (pm_debug_stream_abort_after): the chain gives the launch up — CARVE_STATE_ABORTED —
                                         // once this many steps of the carve are committed (0 = off)
  // behind the streaming carve, carve_finish_kernel completes the records of the groups the launch appended — worker ids for
  // positions, group_of, and: their ids (generate_group_id's stream: output k + 1 of id_state for group id_g0 + k), an
  // empty task word, and a copy of the records and of the status in pinned HOST memory (stage_*, h_status: written by the
  // kernel over PCIe) — so that nothing has to be copied, and no launch queued, between the carve and the pair sweep
  unsigned long long id_state;
  uint32_t id_g0, stage_m0;              // first group / member slot of this carve (the staging arrays start there)
  uint32_t stage_cap_g, stage_cap_m;     // entries the staging arrays hold
  uint32_t *stage_cfg, *stage_n, *stage_off, *stage_mem;  // pinned host memory (null: no host copy)
  unsigned long long* g_id_out;          // [cap_groups] ids (null: none written)
  uint32_t* g_task_out;                  // [cap_groups] task words
  CarveStatus* h_status;                 // pinned host memory (null: no mirror)
  unsigned long long* stream_trace;      // PM_CARVE_PROF builds: [PM_STREAM_TRACE_CAP][2] {s_memtime, type | a << 8 | b << 32}
  // configurations in carve order (get_available_configurations, mod.rs:399-418)
  uint32_t n_avail, start_ci;
  uint32_t avail_cfg[PM_MAX_CONFIGS];
  uint32_t min_size[PM_MAX_CONFIGS];
  uint32_t max_size[PM_MAX_CONFIGS];
  // output group records (slots n_groups.. are appended)
  uint32_t *g_cfg, *g_n, *g_off, *members;
  uint32_t cap_groups, cap_members;
  CarveStatus* status;
};

void launch_compat(const CompatArgs& a, hipStream_t s);
// diagnostics (pm_report.inc)
void launch_explain(const CompatArgs& p, const uint32_t* rows, uint32_t n, uint32_t stride, uint32_t* why_out, hipStream_t s);
void launch_config_report(const ReportArgs& a, uint32_t max_blocks, hipStream_t s);
void launch_task_report(const ReportArgs& a, uint32_t max_blocks, hipStream_t s);
// group geography (pm_spread.inc)
void launch_group_spread(const SpreadArgs& a, hipStream_t s);
void launch_config_spread(const pm_group_spread_row* rows, const uint32_t* row_cfg, uint32_t n_rows, uint32_t n_cfgs,
                          SpreadCfgAcc* out, uint32_t max_blocks, hipStream_t s);
// nearest candidates (pm_near.inc)
void launch_nearest(const NearArgs& a, hipStream_t s);
// probes and configuration overlap (pm_probe.inc)
void launch_probe(const ProbeArgs& a, uint32_t max_blocks, hipStream_t s);
// assignment change feed (pm_changes.inc)
void launch_assign_diff(const ChangeDiffArgs& a, hipStream_t s);
void launch_change_list(const uint64_t* bitmap, uint32_t n_words, const uint8_t* what, uint32_t* prefix, uint32_t* total_host,
                        pm_change_row* out, hipStream_t s);
// liveness (pm_liveness.inc)
void launch_liveness_init(const uint32_t* flags, uint32_t first, uint32_t W, uint8_t* status, uint32_t* counter, hipStream_t s);
void launch_liveness_sweep(const LiveSweepArgs& a, hipStream_t s);
void launch_liveness_list(const uint64_t* bitmap, uint32_t n_words, const uint8_t* old_status, const uint8_t* status,
                          const uint32_t* counter, uint32_t* prefix, uint32_t* total_host, pm_live_row* out, hipStream_t s);
void launch_liveness_set(const uint32_t* stage, uint32_t n, uint8_t* status, uint32_t* counter, hipStream_t s);
void launch_liveness_get(const uint32_t* idx, uint32_t n, const uint8_t* status, const uint32_t* counter, uint32_t* out,
                         hipStream_t s);
// discovery sync (pm_discovery.inc): mark, base, segments + scatter, query and decide, in this order on s
void launch_discovery_sync(const DiscArgs& a, hipStream_t s);
// metrics ledger (pm_metrics.inc)
void launch_mx_fill(uint32_t* p, uint32_t first, uint32_t end, uint32_t v, hipStream_t s);
void launch_mx_lengths(const uint32_t* off, uint32_t R, uint32_t* new_n, hipStream_t s);
void launch_mx_fold(const MxFoldArgs& a, bool write, hipStream_t s);
// out[i] = sum of (in[j] & ~PM_MX_TOUCHED) over j < i, out[n] = the total (also to *total_host where given: pinned)
void launch_mx_scan(const uint32_t* in, uint32_t n, uint32_t* out, uint32_t* total_host, hipStream_t s);
void launch_mx_copy(const uint32_t* off_old, const uint32_t* new_n, const uint32_t* off_new, uint32_t R, uint32_t N_old,
                    const uint32_t* ser_old, const double* val_old, uint32_t* ser_new, double* val_new, hipStream_t s);
void launch_mx_mark_dead(const pm_live_row* list, uint32_t n, uint32_t R, const uint32_t* off, uint32_t* new_n, uint32_t* hit_host,
                         hipStream_t s);
void launch_mx_row_lengths(const uint32_t* rows, uint32_t n, const uint32_t* off, uint32_t* len, hipStream_t s);
void launch_mx_rows(const MxRowsArgs& a, hipStream_t s);
// one radix pass over digit (series >> shift) & 255: hist [256][chunks] (digit-major), scanned in place into `hist_scan`
void launch_mx_radix_pass(const uint32_t* ser_in, const double* val_in, uint32_t N, uint32_t shift, uint32_t* hist,
                          uint32_t* hist_scan, uint32_t* ser_out, double* val_out, hipStream_t s);
void launch_mx_sums(const uint32_t* ser_sorted, const double* val_sorted, uint32_t N, uint32_t n_series, double* sum,
                    uint32_t* count, hipStream_t s);
// rollout ledger (pm_rollout.inc)
void launch_ro_fill(uint64_t* uid, uint8_t* state, uint32_t* last, uint32_t first, uint32_t end, hipStream_t s);
// the n reports in array order, last entry of a worker wins; `last` [W] is zero before and after
void launch_ro_ingest(const pm_ro_report* r, uint32_t n, uint32_t* last, uint64_t* uid, uint8_t* state, hipStream_t s);
void launch_ro_get(const uint32_t* idx, uint32_t n, const uint64_t* uid, const uint8_t* state, uint64_t* out_uid, uint8_t* out_state,
                   hipStream_t s);
void launch_ro_classify(const RoPrepArgs& a, hipStream_t s);
void launch_ro_emit(const RoPrepArgs& a, hipStream_t s);
// one radix pass over digit (key >> shift) & 255: hist [256][chunks] (digit-major), scanned into `hist_scan`
void launch_ro_radix_pass(const uint64_t* key_in, const uint32_t* val_in, uint32_t N, uint32_t shift, uint32_t* hist,
                          uint32_t* hist_scan, uint64_t* key_out, uint32_t* val_out, hipStream_t s);
// what a key sort works in: keys and side words, ping-pong, and a pass's histogram and its scan (KeySort of
// pm_engine_types.inc owns and sizes them)
struct RoSortBufs {
  uint64_t* key[2];
  uint32_t* val[2];
  uint32_t *hist, *hist_scan;
};
// `passes` stable passes from the low byte over the N keys of buffer `cur`; returns the buffer that holds the result
uint32_t launch_ro_radix_sort(const RoSortBufs& b, uint32_t N, uint32_t passes, uint32_t cur, hipStream_t s);
void launch_ro_heads(const uint64_t* key, uint32_t N, uint32_t* head, hipStream_t s);
void launch_ro_starts(const uint32_t* head, const uint32_t* head_off, uint32_t N, uint32_t* start, hipStream_t s);
// one row per run of equal keys: start [D] the runs' first entries
void launch_ro_reduce(const uint64_t* key, const uint32_t* val, uint32_t N, const uint32_t* start, uint32_t D, const RoGroup* g,
                      const uint32_t* g_cnt, pm_ro_task_row* rows, hipStream_t s);
void launch_ro_group_rows(const RoGroup* g, uint32_t G, const uint32_t* listed, const uint32_t* off, const uint32_t* g_cnt,
                          pm_ro_group_row* rows, hipStream_t s);
void launch_ro_worker_flags(const uint8_t* cls, uint32_t W, uint32_t class_mask, uint32_t* flag, hipStream_t s);
void launch_ro_worker_rows(const RoPrepArgs& a, const uint32_t* flag, const uint32_t* off, pm_ro_worker_row* rows, hipStream_t s);
// node directory (pm_directory.inc)
void launch_dir_classify(const DirArgs& a, hipStream_t s);
// the three directories' window (Args: DirArgs, GdirArgs, TdirArgs): of the n_index entries of the index space, those whose
// place falls in [a.offset, a.offset + a.n_rows) write themselves to a.win[place - a.offset]
template <class Args>
void launch_list_window(const Args& a, uint32_t n_index, hipStream_t s);
void launch_dir_keys(const DirArgs& a, hipStream_t s);
// rows[k] = the joined record of worker list[k], k < n
void launch_dir_emit(const DirArgs& a, const uint32_t* list, uint32_t n, pm_dir_row* rows, hipStream_t s);
// group directory (pm_groupdir.inc)
void launch_gdir_members(const GdirArgs& a, hipStream_t s);
void launch_gdir_groups(const GdirArgs& a, hipStream_t s);
void launch_gdir_keys(const GdirArgs& a, hipStream_t s);
// rows[k] = the joined record of list entry list[k], k < n (member_begin is the host's: it lays the members out)
void launch_gdir_emit(const GdirArgs& a, const uint32_t* list, uint32_t n, pm_gdir_row* rows, hipStream_t s);
// task directory (pm_taskdir.inc)
void launch_tdir_groups(const TdirArgs& a, hipStream_t s);
// run d of the rollout ledger's per-task table -> the slot of the first live row that carries its id (key / val [n_pairs]: the
// live (id, slot) pairs sorted by id, ties in slot order), or an orphan
void launch_tdir_join(const TdirArgs& a, const pm_ro_task_row* runs, uint32_t D, const uint64_t* key, const uint32_t* val,
                      uint32_t n_pairs, hipStream_t s);
void launch_tdir_tasks(const TdirArgs& a, hipStream_t s);
void launch_tdir_keys(const TdirArgs& a, hipStream_t s);
// rows[k] = the joined record of slot list[k], handles[k] its handle, k < n (uid is the host's: the ids never went up whole)
void launch_tdir_emit(const TdirArgs& a, const uint32_t* list, uint32_t n, pm_tdir_row* rows, uint32_t* handles, hipStream_t s);
// keccak-256 (pm_keccak.inc): message i is bytes[off[i], off[i + 1]), its digest the little-endian bytes of out[4 i, 4 i + 4)
void launch_keccak_many(const uint8_t* bytes, const uint32_t* off, uint32_t n, uint64_t* out, hipStream_t s);
// address book (pm_addresses.inc).  in: n addresses of five words; the rows first.. take bytes, case mask, text key and flag
void launch_ab_set(const uint32_t* in, uint32_t first, uint32_t n, uint32_t* bytes, uint64_t* mask, uint64_t* key, uint8_t* set,
                   hipStream_t s);
// out[43 k ..) = the EIP-55 text of row rows[k] (null: row k)
void launch_ab_text(const uint32_t* rows, uint32_t n, const uint32_t* bytes, const uint64_t* mask, uint8_t* out, hipStream_t s);
void launch_ab_clear(uint8_t* set, uint32_t first, uint32_t end, hipStream_t s);
// (word 0, row) of every row sorted into key / val [returned buffer]; *ties += neighbours that share word 0
uint32_t launch_ab_sort_shallow(const uint64_t* keys, uint32_t W, const RoSortBufs& b, uint32_t* ties, hipStream_t s);
// the rows sorted by all PM_AB_WORDS words into val [returned buffer]
uint32_t launch_ab_sort_deep(const uint64_t* keys, uint32_t W, const RoSortBufs& b, hipStream_t s);
// rank[val[i]] = i
void launch_ab_rank(const uint32_t* val, uint32_t W, uint32_t* rank, hipStream_t s);
// digest / signing [4 k, 4 k + 4): the invite digest of row rows[k] and its EIP-191 signing hash; nonce [4 n], expiration [n]
void launch_invite_digests(const uint32_t* rows, uint32_t n, const uint32_t* bytes, uint32_t domain_id, uint32_t pool_id,
                           const uint64_t* nonce, const uint64_t* expiration, uint64_t* digest, uint64_t* signing, hipStream_t s);
// request gate (pm_secp256k1.inc).  hash: 32 big-endian bytes an entry (aligned words), sig: 65 bytes an entry -> ok [n], addr
// [5 n] the address's bytes as words, pub [8 n] (null: not wanted) Qx | Qy as the words that hold their big-endian bytes
void launch_ecrecover(const uint64_t* hash, const uint8_t* sig, uint32_t n, uint32_t* addr, uint64_t* pub, uint8_t* ok, hipStream_t s);
// out[4 i, 4 i + 4) = the EIP-191 hash of message bytes[off[i], off[i + 1]), as launch_keccak_many lays a digest out
void launch_eip191_many(const uint8_t* bytes, const uint32_t* off, uint32_t n, uint64_t* out, hipStream_t s);
// the book's rows sorted by their 20 bytes, equal ones by row, rows without an address last, into val [returned buffer]
uint32_t launch_gate_index(const uint32_t* bytes, const uint8_t* set, uint32_t W, const RoSortBufs& b, hipStream_t s);
// out [8 n]: pm_rq_verdict as words; counts [PM_RQ_N_CODES] += the census; status null: liveness is off
void launch_gate_verdict(const uint32_t* addr, const uint8_t* ok, const uint8_t* sig, const uint32_t* claimed, const uint8_t* flags,
                         uint32_t n, const uint32_t* idx, uint32_t n_idx, const uint32_t* book, const uint8_t* status, uint32_t* out,
                         uint32_t* counts, hipStream_t s);
// request gate: admission (pm_admission.inc; the argument blocks are declared there).  launch_ad_rate: the requests sorted by
// row into b (returns the buffer), stage [n] by request; launch_ad_rate_commit: the heads of that order write the windows;
// launch_ad_nonces: the batch's nonces sorted by key into b (returns the buffer), replay [n], keep_new [n], keep_old [N];
// launch_ad_merge: the next standing array; launch_ad_final: the codes, the beats, counts [PM_AD_N_CODES] += the census
struct AdRateArgs {
  const uint64_t* key;    // [n] sorted: rows, W behind them
  const uint32_t* val;    // [n] the requests
  uint32_t n, W;
  uint64_t now_ms;
  const uint64_t* win;    // [W]
  const uint32_t* cnt;    // [W]
  const uint8_t* flags;   // [n] or null
  const uint64_t* ts;     // [n] or null (every request carries NO_TIMESTAMP)
  const uint8_t* nonce;   // the nonces' bytes
  const uint32_t* noff;   // [n + 1] or null (every request carries NO_NONCE)
  uint32_t* stage;        // [n] by request
};
struct AdNonceArgs {
  const uint64_t* key;      // [n] the batch's keys, sorted
  const uint32_t* val;      // [n] the requests
  uint32_t n, N, kbits;
  uint64_t now_ms;
  const uint32_t* stage;    // [n] by request
  const uint64_t* dig;      // [4 n] by request
  const uint64_t* old_dig;  // [4 N] the standing set
  const uint64_t* old_ms;   // [N]
  uint32_t* replay;         // [n] by request
  uint32_t* keep_new;       // [n] by sorted position
};
struct AdMergeArgs {
  const uint64_t* key;       // [n] the batch's keys, sorted
  const uint32_t* val;       // [n]
  uint32_t n, N, kbits, cap; // cap: entries the next array has room for
  uint64_t now_ms;
  const uint64_t* dig;       // [4 n] by request
  const uint32_t* keep_new;  // [n]
  const uint32_t* rank_new;  // [n + 1] its exclusive scan
  const uint64_t* old_dig;   // [4 N]
  const uint64_t* old_ms;    // [N]
  const uint32_t* keep_old;  // [N]
  const uint32_t* rank_old;  // [N + 1]
  uint64_t* out_dig;         // [4 cap]
  uint64_t* out_ms;          // [cap]
};
uint32_t launch_ad_rate(AdRateArgs a, const uint32_t* verdict, const RoSortBufs& b, hipStream_t s);
uint32_t launch_ad_nonces(AdNonceArgs a, const RoSortBufs& b, uint32_t* keep_old, hipStream_t s);
void launch_ad_merge(const AdMergeArgs& a, hipStream_t s);
void launch_ad_rate_commit(const uint64_t* key, uint32_t n, uint32_t W, uint64_t now_ms, uint64_t* win, uint32_t* cnt, hipStream_t s);
void launch_ad_old_live(const uint64_t* old_ms, uint32_t N, uint64_t now_ms, uint32_t* keep_old, hipStream_t s);
void launch_ad_final(uint32_t* verdict, uint32_t n, uint32_t W, const uint32_t* stage, const uint32_t* replay, const uint8_t* flags,
                     uint64_t now_ms, uint64_t* beat, uint32_t* counts, hipStream_t s);
void launch_ad_gather(const uint32_t* idx, uint32_t n, const uint64_t* a64, const uint32_t* a32, uint64_t* out64, uint32_t* out32,
                      hipStream_t s);
void launch_ad_scatter(const uint32_t* idx, uint32_t n, uint32_t W, const uint64_t* in64, const uint32_t* in32, uint64_t* a64,
                       uint32_t* a32, hipStream_t s);
void launch_ad_beat_max(const uint64_t* col, uint32_t W, uint64_t* out, hipStream_t s);
void launch_geo(const double* lat, const double* lon, double* coslat, double* ux, double* uy, double* uz, uint32_t W,
                hipStream_t s);
void launch_triad(const double* b, const double* c, double* a, size_t n, hipStream_t s);
#ifdef PM_ROW_BENCH
hipError_t launch_row_bench(const CarveArgs* d_args, uint32_t seed, uint32_t ci, uint32_t reps, uint32_t mode, unsigned long long* d_out, hipStream_t s);
#endif
void launch_row_network_test(const uint64_t* keys, const uint32_t* sites, uint32_t n_waves, uint32_t n_per_wave, uint32_t slot_bits,
                             uint64_t ulps, uint32_t upto, uint64_t* rows_out, uint32_t* mismatches, hipStream_t s, double tie_band = 0.0,
                             uint64_t* cert_rows = nullptr, uint64_t* cert_track = nullptr, uint32_t* cert_flags = nullptr,
                             uint64_t* cert_mine = nullptr);  // (the cert_* of pm_debug_row_certificates: all four or none)
// debug (pm_debug_distance_keys): the distance key of n pairs through the carve's device functions; PM_DK_WORDS f64 per pair
static constexpr uint32_t PM_DK_WORDS = 20;
void launch_distance_key_test(const double* in, const double* geo, uint32_t n, uint32_t mode, double* out, hipStream_t s);
void launch_update_rows(const RowUpdateArgs& a, hipStream_t s);
void launch_worker_selector(const int32_t* group_of, const uint32_t* g_cfg, uint32_t R, const uint32_t* rows,
                            uint64_t* sel, hipStream_t s);
void launch_eligible_selector(const uint32_t* wflags, const int32_t* group_of, const uint64_t* compat,
                              uint64_t enabled, uint32_t W, const uint8_t* shard, uint32_t my_rank, uint64_t* sel,
                              hipStream_t s);
void launch_chooser_rank(const int32_t* group_of, const uint64_t* g_id, const uint32_t* count, uint32_t R,
                         const uint32_t* rows, uint64_t seed, uint32_t* rank, hipStream_t s);
void launch_table_scatter(const pm_assignment* x, const uint32_t* xrow, uint32_t W, pm_assignment* table,
                          uint32_t* task_col, uint32_t* g_task_next, const uint64_t* t_live, const uint32_t* t_prefix,
                          hipStream_t s);
void launch_group_rank(const int32_t* group_of, const uint32_t* g_n, const uint32_t* g_off, const uint32_t* members,
                       const uint32_t* addr_rank, uint32_t W, uint32_t* rank_in_group, uint32_t* by_rank,
                       hipStream_t s);
void launch_claim_publish(const ClaimArgs& a, hipStream_t s);
void launch_match_prep(const MatchPrepArgs& a, hipStream_t s);
void launch_build_planes(const uint64_t* col_mask, uint32_t n_cols, uint32_t c_begin, uint32_t c_end, uint32_t stride,
                         uint32_t n_planes, uint64_t* planes, hipStream_t s);
void launch_pair_sweep(int variant, const uint64_t* row_sel, uint32_t R, const uint64_t* col_mask,
                       const uint64_t* planes, uint32_t c_begin, uint32_t c_end, uint32_t stride, uint32_t n_planes,
                       uint32_t* first, uint32_t* count, hipStream_t s, bool inited = false);
void launch_pair_select(int variant, const uint64_t* row_sel, uint32_t R, const uint64_t* col_mask,
                        const uint64_t* planes, uint32_t c_begin, uint32_t c_end, uint32_t stride, uint32_t n_planes,
                        const uint32_t* rank, uint32_t* out, hipStream_t s);
void launch_task_prefix(const uint64_t* live, uint32_t w_begin, uint32_t w_end, uint32_t* prefix, hipStream_t s);
void launch_task_delete(const uint32_t* slots, uint32_t n, uint64_t* tmask, uint64_t* live, uint64_t* planes,
                        uint32_t stride, uint32_t n_planes, hipStream_t s);
void launch_task_intern(const uint64_t* tmask, const uint64_t* live, uint32_t u_begin, uint32_t u_end, uint64_t valid,
                        uint64_t* keys, uint32_t n_slots, uint32_t* vals, uint32_t* counter_and_overflow, uint64_t* umask,
                        uint32_t cap_u, hipStream_t s);
void launch_task_compact_class(const uint32_t* first_c, const uint32_t* count_c, const uint64_t* tmask, uint64_t valid,
                               const uint64_t* keys, const uint32_t* vals, uint32_t n_slots, uint32_t u_begin,
                               uint32_t u_end, const uint64_t* live, const uint32_t* prefix, uint32_t* first_out,
                               uint32_t* count_out, hipStream_t s);
void launch_task_compact(const uint32_t* first_u, const uint32_t* count_u, uint32_t u_begin, uint32_t u_end,
                         const uint64_t* live, const uint32_t* prefix, uint32_t* first_out, uint32_t* count_out,
                         hipStream_t s);
void launch_newest(const int64_t* created_at, const uint64_t* live, uint32_t t_begin, uint32_t t_end,
                   uint32_t* idx_by_block, long long* val_by_block, uint32_t n_blocks, hipStream_t s);
void launch_group_ids(uint64_t* g_id, uint32_t* g_task, uint32_t n, uint64_t rng_state, hipStream_t s);
hipError_t carve_kernels_init();  // per device: the carve kernels' dynamic LDS sizes (pm_engine_create)
hipError_t launch_carve(const CarveArgs* d_args, uint32_t flags, uint32_t start_ci, size_t lds_bytes, hipStream_t s);
uint32_t launch_carve_prep(const CarveArgs* d_args, uint32_t W, hipStream_t s);  // count + place
// eligible list [+ spatial index]; returns the launches.  fresh: the status block is initialised by the first kernel
// (state RUNNING, n_groups0 groups, n_members0 member slots, everything else zero) instead of by a copy in front of it
hipError_t launch_carve_args_put(const CarveArgs& a, CarveArgs* d_args, hipStream_t s);
uint32_t launch_carve_elig(CarveArgs* d_args, const CarveArgs* put, uint32_t W, uint32_t n_bound, uint32_t index_min, uint32_t start_ci,
                           bool fresh, uint32_t n_groups0, uint32_t n_members0, hipStream_t s);
void launch_carve_apply(const CarveArgs* d_args, uint32_t W, hipStream_t s);
void launch_carve_propose(const CarveArgs* d_args, uint32_t W, hipStream_t s);
hipError_t launch_carve_stream(const CarveArgs* d_args, uint32_t start_ci, uint32_t n_prop_wgs, hipStream_t s);
void launch_scatter_const(uint32_t* dst, const uint32_t* idx, uint32_t n, uint32_t v, hipStream_t s);
void launch_scatter_pairs(uint32_t* dst, const uint32_t* pairs, uint32_t n, hipStream_t s);
void launch_merge_place(const CarveArgs* d_args, uint32_t n_order, uint32_t n_groups0, uint32_t n_members0, uint32_t steps0,
                        hipStream_t s);

}  // namespace pm
#endif
