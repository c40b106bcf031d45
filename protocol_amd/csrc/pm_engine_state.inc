// pm_engine_state.inc — part of pm_engine.cpp (one translation unit; included in place): struct pm_engine: every table, mirror and scratch buffer of one engine.
//
// Every buffer, event and stream below is held by an owning type of pm_owned.h: `delete e` gives them all back, and a new
// member costs its declaration and nothing else.

// ---- assignment change feed (pm_engine_changes.inc): remembered identities, pending bits and rows of the workers [0, W);
// everything behind W reads zero.  The drain's scratch: per-word prefix, the list, its count in pinned memory.
struct ChangeFeed {
  bool on = false;
  bool resync = false;       // the remembered identities are meaningless: the next publish lists every row
  bool resync_flag = false;  // ... and did: the next successful drain returns PM_CHANGES_RESYNC
  bool list_valid = false;   // rows / n are the pending marks as they are now
  uint32_t W = 0, n = 0;
  DevBuf<ChangeIdent> ident;
  DevBuf<uint8_t> what;
  DevBuf<uint64_t> bitmap;
  DevBuf<uint32_t> prefix;
  DevBuf<pm_change_row> rows;
  PinBuf<uint32_t> h_count;
};

// ---- liveness (pm_engine_liveness.inc): the ledger (status byte, unhealthy counter) of the workers [0, W); rows behind W hold
// nothing yet (the init step writes them from the host's flags when the next liveness call sees them).  The last sweep's list:
// bitmap, old-status side bytes, per-word prefix, the rows; its count and the census in pinned memory.
struct Liveness {
  bool on = false;
  bool reinit = false;     // the row identities are gone (an upload that dropped the groups): initialise every row again
  bool rows_host = false;  // h_rows holds the last sweep's list (an apply sweep brought it over)
  uint32_t m = 0;          // missing_heartbeat_threshold
  uint32_t W = 0, n = 0;
  DevBuf<uint8_t> status, old;
  DevBuf<uint32_t> counter;
  DevBuf<uint64_t> bitmap;
  DevBuf<uint32_t> prefix;
  DevBuf<pm_live_row> rows;
  DevBuf<uint32_t> census;  // PM_NS_N words
  DevBuf<uint64_t> beat;    // the sweep's inputs: the beat column, behind it the pool bits
  DevBuf<uint32_t> stage;   // set / get / init: indices, counters, packed status bytes
  std::vector<pm_live_row> h_rows;
  std::vector<uint32_t> h_stage;
  PinBuf<uint32_t> h_count;  // [0] listed rows, [1, 1 + PM_NS_N) census
};

// ---- discovery sync (pm_engine_discovery.inc): scratch of one pm_discovery_sync, released with the liveness ledger
struct Discovery {
  DevBuf<uint64_t> in;      // the staged inputs: the rows (32 bytes each), behind them the endpoint column
  DevBuf<uint32_t> work;    // pos_of_row [W] | base, ev_cnt, ev_fill [E each], cursor [1] | ev_off [E]
  DevBuf<uint64_t> events;  // [2 n_rows]
  DevBuf<pm_disc_result> out;
  std::vector<uint64_t> h_in;
  std::vector<pm_disc_result> h_out;
  std::vector<uint32_t> h_seen;  // [W] the call (epoch) that last listed the row: a row listed twice
  uint32_t epoch = 0;
};

// ---- metrics ledger (pm_engine_metrics.inc): a CSR over the internal rows [0, R) — 0 the manual row, w + 1 worker w — in two
// buffers (cur is the table, the other one the next ingest's target); N its entries.  Rows behind R hold nothing yet: the next
// metrics call extends the offsets.
struct Metrics {
  bool on = false;
  bool reinit = false;        // an upload dropped the row identities: every worker row is emptied by the next metrics call
  bool totals_valid = false;  // h_sum / h_cnt are the totals of the table as it stands
  uint32_t cur = 0, R = 0, N = 0, n_series = 0;
  DevBuf<uint32_t> off[2], ser[2];
  DevBuf<double> val[2];
  DevBuf<uint32_t> new_n;     // [R] a rebuild's row lengths (| PM_MX_TOUCHED)
  DevBuf<uint32_t> stage;     // an ingest's touched rows (3 columns); a listing's rows, lengths and offsets
  DevBuf<pm_mx_beat> beats;
  DevBuf<pm_mx_entry> entries;
  DevBuf<uint32_t> flag;      // [1] the count pass's "a row would pass the bound"
  DevBuf<uint32_t> sort_ser[2], hist, hist_scan, cnt, gcfg;
  DevBuf<double> sort_val[2], sum;
  DevBuf<int32_t> gof;        // the join's inputs: the host's group_of, the groups' ids and configurations by slot
  DevBuf<uint64_t> gid;
  DevBuf<pm_mx_row> out;
  PinBuf<uint32_t> h_pin;     // [0] a scan's total, [1] the bound flag, [2] the liveness hook's "a row was emptied"
  std::vector<double> h_sum;
  std::vector<uint32_t> h_cnt, h_stage;
  std::vector<pm_mx_beat> h_beats;
  std::vector<uint64_t> h_gid;
  std::vector<uint32_t> h_gcfg;
};

// ---- rollout ledger (pm_engine_rollout.inc): the reported task id and state of the workers [0, W); rows behind W hold nothing
// yet (the next rollout call fills them empty).  Everything else is scratch of one call: nothing is cached between reads.
struct Rollout {
  bool on = false;
  bool reinit = false;        // an upload dropped the row identities: every row is emptied by the next rollout call
  uint32_t W = 0;
  DevBuf<uint64_t> uid;       // [W] the ledger
  DevBuf<uint8_t> state;
  DevBuf<uint32_t> last;      // [W] the ingest's highest report index per worker: zero between calls
  DevBuf<pm_ro_report> reports;
  DevBuf<uint32_t> idx;       // pm_rollout_get: the indices, ...
  DevBuf<uint64_t> get_uid;   // ... the gathered ids and states
  DevBuf<uint8_t> get_state;
  DevBuf<int32_t> gof;        // the join's other side: the host's group_of, its group list
  DevBuf<RoGroup> g;
  DevBuf<uint8_t> cls;        // [W]
  DevBuf<uint32_t> cnt;       // [G * PM_RO_GCNT] the groups' counters, behind them [PM_RO_CENSUS] the census
  DevBuf<uint32_t> flag, off;  // [W + G] (+ 1): reports / is listed, and the scan; the lists' flags and offsets
  KeySort sort;               // the id sort: the keys (buffer 0 is made by every read) and their side words
  DevBuf<uint32_t> head, head_off, start;
  DevBuf<pm_ro_task_row> task_rows;
  DevBuf<pm_ro_group_row> group_rows;
  DevBuf<pm_ro_worker_row> worker_rows;
  PinBuf<uint32_t> h_pin;     // [0] a scan's total, [1, 1 + PM_RO_CENSUS) the census
  std::vector<RoGroup> h_g;
  std::vector<uint8_t> h_state;
};

// ---- node directory (pm_engine_directory.inc): scratch of one pm_directory call and nothing else — there is no ledger of its
// own, no enable call and no hook in the upload path; nothing is cached between calls.
struct Directory {
  DevBuf<int32_t> gof;        // the join's other side: the host's group_of, its group list
  DevBuf<DirGroup> g;
  DevBuf<uint8_t> cls;        // [W]
  ListPage pg;                // [PM_DC_N * W] class flags; BY_ROW is scan order, BY_ADDRESS sorted; PM_NS_N census words
  DevBuf<uint32_t> census;    // [PM_NS_N]
  DevBuf<pm_dir_row> rows;
  std::vector<DirGroup> h_g;
};

// ---- group directory (pm_engine_groupdir.inc): scratch of one pm_group_directory call and nothing else, like Directory
struct GroupDir {
  DevBuf<int32_t> gof;        // the join's other side: the host's group_of, its group list
  DevBuf<RoGroup> g;
  DevBuf<uint32_t> cnt;       // [G * PM_GD_CNT] the groups' counters, behind them [PM_GD_CENSUS] the census
  DevBuf<uint8_t> cls, hr;    // [G], [2 G]
  ListPage pg;                // [n_cls * G] class flags; BY_SLOT is scan order, the others sorted; PM_GD_CENSUS census words
  DevBuf<pm_gdir_row> rows;
  std::vector<RoGroup> h_g;
  std::vector<uint32_t> h_of_slot;  // reported slot -> list entry
  std::vector<pm_gdir_row> h_rows;  // the window, before the caller's buffers are known to hold it
};

// ---- task directory (pm_engine_taskdir.inc): scratch of one pm_task_directory call and nothing else, like Directory
struct TaskDir {
  DevBuf<TdirGroup> g;        // the join's other side: the host's group list
  DevBuf<uint32_t> cnt;       // [R * PM_TD_CNT] the slots' counters, behind them [PM_MAX_CONFIGS] the live groups per configuration, [PM_TD_CENSUS] the census
  DevBuf<uint8_t> cls;        // [2 R]
  ListPage pg;                // [R] listing flags; BY_LIST and BY_OLDEST are scan order, the _DESC orders sorted; PM_TD_CENSUS
                              // census words.  pg.sort holds the id join's sorted (id, slot) pairs first
  DevBuf<pm_tdir_row> rows;
  DevBuf<uint32_t> handles;   // the window's handles (the host writes the ids by them)
  std::vector<TdirGroup> h_g;
  std::vector<uint64_t> h_key;      // the live rows' ids, in list order, ...
  std::vector<uint32_t> h_val;      // ... and their slots
  std::vector<pm_tdir_row> h_rows;  // the window, before the caller's buffer is known to hold it
  std::vector<uint32_t> h_handles;
};

// ---- address book (pm_engine_addresses.inc): the 20 bytes, the EIP-55 case mask, the text key and a "set" flag of the workers
// [0, W); rows behind W hold nothing yet (the next book call clears their flags).  Everything else is scratch of one call.
struct AddressBook {
  bool on = false;
  bool reinit = false;        // an upload dropped the row identities: every flag is cleared by the next book call
  uint32_t W = 0, n_set = 0;  // rows covered; rows of them that hold an address
  uint64_t epoch = 0;         // grows whenever a row's address, or the rows themselves, may have changed: what the request gate's index is built against
  uint64_t shallow = 0, deep = 0;  // ranks that ended on the one-word / the all-words sort, since creation (pm_debug_carve_prof 98, 99)
  DevBuf<uint32_t> bytes;     // [5 W]
  DevBuf<uint64_t> mask;      // [W]
  DevBuf<uint64_t> keys;      // [PM_AB_WORDS W]
  DevBuf<uint8_t> set;        // [W]
  std::vector<uint8_t> h_set; // (the flags' host mirror: what n_set counts)
  DevBuf<uint32_t> stage;     // a call's inputs: addresses, rows, offsets
  KeySort sort;               // the rank's sort: keys and rows
  DevBuf<uint32_t> ties;
  DevBuf<uint8_t> text;       // rendered texts; pm_keccak256_many's messages
  DevBuf<uint64_t> in64, out64;  // nonces and expirations; digests
  PinBuf<uint32_t> h_pin;     // [0] the ties
};

// ---- request gate (pm_engine_gate.inc): the index of the address book's rows by their 20 bytes — built by the first
// pm_verify_requests that needs it and again whenever the book's epoch has moved — and the scratch of one call
struct Gate {
  bool valid = false;         // sort.val[cur][0, n_idx) is the index of the book at `epoch` with W rows
  uint32_t cur = 0, n_idx = 0, W = 0;
  uint64_t epoch = 0;
  uint64_t builds = 0;        // indexes built since creation
  KeySort sort;               // the index: three-word keys, rows
  DevBuf<uint8_t> text;       // the requests' messages
  DevBuf<uint32_t> off;       // their offsets
  DevBuf<uint64_t> hash;      // [4 n] the hashes: pm_ecrecover_many's input, the EIP-191 kernel's output
  DevBuf<uint8_t> sig;        // [65 n]
  DevBuf<uint32_t> addr;      // [5 n] recovered
  DevBuf<uint64_t> pub;       // [8 n]
  DevBuf<uint8_t> ok, flags;  // [n]
  DevBuf<uint32_t> claimed;   // [5 n]
  DevBuf<uint32_t> out;       // [8 n] the verdicts, behind them [PM_RQ_N_CODES] the census
};

// ---- request gate: admission (pm_engine_admission.inc): the rate window and the last beat of every worker row, the standing
// nonce set — a sorted array, two buffers that take turns: a call merges the batch into the other one — and a call's scratch
struct Admission {
  bool on = false;
  bool reinit = false;        // an upload dropped the row identities: the next admission call empties the rate ledger and the beats
  uint32_t W = 0;             // rows covered
  uint32_t kbits = 64;        // bits of a digest that make its sort key (the debug header's hook narrows it)
  DevBuf<uint64_t> win;       // [W] window_start_ms
  DevBuf<uint32_t> cnt;       // [W] count
  DevBuf<uint64_t> beat;      // [W] last_beat_ms
  DevBuf<uint64_t> dig[2];    // [4 N] the standing digests, sorted by key
  DevBuf<uint64_t> ms[2];     // [N] stored_ms
  uint32_t cur = 0, N = 0;    // the buffer that holds the set; entries held
  KeySort sort;               // a call's two sorts: by row, then by key
  DevBuf<uint8_t> text;       // the batch's nonces
  DevBuf<uint32_t> off;       // [n + 1]
  DevBuf<uint64_t> ndig;      // [4 n] their digests
  DevBuf<uint64_t> ts;        // [n]
  DevBuf<uint32_t> stage, replay, keep_new, rank_new;  // [n] (+ 1)
  DevBuf<uint32_t> keep_old, rank_old;                 // [N] (+ 1)
  DevBuf<uint32_t> counts;    // [PM_AD_N_CODES]
  DevBuf<uint32_t> idx, io32; // the hand-over calls' rows and counts
  DevBuf<uint64_t> io64;
  PinBuf<uint32_t> h_pin;     // [0] kept new entries, [1] kept standing entries
};

struct pm_engine {
  Stream stream_owned;  // created with the engine.  Declared first, so destroyed last: everything below may be freed on a live stream
  pm_engine_config cfg{};
  hipStream_t stream = nullptr;  // the stream every kernel and copy of this engine goes to: stream_owned unless pm_set_stream handed one in
  bool own_stream = true;
  Event ev[6];
  Event kev[6];  // kernel-only brackets: compat, carve, sweep
  hipEvent_t k_carve_begin = nullptr;  // the event in front of the carve's kernels: kev[2], or an event the caller has behind the compat sweep anyway (one barrier packet less)
  hipEvent_t k_compat_end = nullptr;  // the event behind this tick's compat kernel: kev[1], or the phase event handed to ensure_compat
  bool one_event_behind_carve = false;  // this tick's ev[2] stands for kev[3] and ev[3] too (pm_tick's queued-ahead path)
  float k_ms_compat = 0, k_ms_carve = 0, k_ms_sweep = 0;
  bool k_sweep_recorded = false, k_compat_recorded = false;
  std::chrono::steady_clock::time_point tick_t0{};  // when this tick began on the host (tick_reset)
  bool end_event_queued = false;  // this tick's ev[5] stands behind the claim already (the claim publishes: there is no copy phase behind it, and no ev[4])
  uint64_t tick_cand_sum = 0;
  unsigned long long carve_prof[64]{};
  unsigned long long carve_why[25]{};  // CarveStatus::why of the last carve, its batches and void launches, the spatial
                                       // index, the streaming carve's counters
  uint32_t debug_mem_above = 0;  // pm_debug_mem_lists_above
  uint32_t debug_abort_after = 0;  // pm_debug_stream_abort_after
  uint32_t delta_pushes = 0;       // push_groups calls that went up as a delta (since creation)
  uint32_t pt_distinct = 0;        // pm_debug_per_task_path: distinct valid masks the last per-task call counted (0: it did not count)
  bool pt_interned = false;        // ... and whether it swept once per distinct mask
  uint32_t merge_streamed = 0;     // merge configurations whose selections went through the streaming carve (since creation)
  uint32_t merge_stream_min = 512; // PM_MERGE_STREAM_MIN: compatible solo groups from which a merge configuration does (tests: 8)
  uint32_t prune_mode = 1;       // pm_debug_prune_mode / PM_PRUNE_MODE: CarveArgs::prune_mode
  uint32_t prune_factor = 512;   // PM_PRUNE_FACTOR: CarveArgs::prune_factor (measured crossover, see DESIGN 4.2)
  uint32_t walk_cap_div = 0;     // PM_WALK_CAP_DIV: CarveArgs::walk_cap_div (0 = the kernels' default)
#ifdef PM_BATCH_LOG
  std::vector<uint32_t> blog;    // the preparations of the last carve (tools/prune_probe.py)
#endif
  std::mutex mu;

  // ---- configuration tables
  std::vector<pm_config_row> cfgs;
  std::vector<pm_gpu_alt_row> alts;
  std::vector<uint32_t> model_bits;
  uint32_t model_rows = 0, model_classes = 0;
  bool cls_check_dirty = true;  // gpu_model_class of some row, or the model table, changed since ensure_compat last checked the column
  uint64_t enabled = ~0ull;
  DevBuf<pm_config_row> d_cfgs;
  DevBuf<pm_gpu_alt_row> d_alts;
  DevBuf<uint32_t> d_model_bits;
  bool have_cfgs = false;

  // ---- worker table (host mirror + HBM columns)
  uint32_t W = 0;
  bool have_workers = false;
  std::vector<uint32_t> h_flags, h_gpu_count, h_gpu_mem, h_gpu_cls, h_cpu_cores, h_ram, h_storage, h_price,
      h_addr_rank;
  std::vector<double> h_lat, h_lon;
  std::vector<uint32_t> h_site;  // equal (lat, lon) bit patterns <=> equal site id
  DevBuf<uint32_t> d_site, d_c_site, d_cc_site, d_seed_prefix, d_seed_slots, d_prep_block_counts, d_prep_counts;
  DevBuf<uint64_t> d_prop, d_seed_map;
  uint32_t tick_fast_steps = 0;
  DevBuf<uint32_t> d_flags, d_gpu_count, d_gpu_mem, d_gpu_cls, d_cpu_cores, d_ram, d_storage, d_addr_rank;
  DevBuf<double> d_lat, d_lon, d_coslat, d_ux, d_uy, d_uz;
  DevBuf<uint64_t> d_compat;
  bool compat_dirty = true;
  std::vector<uint64_t> h_compat;
  bool h_compat_valid = false;
  bool any_price = false, price_dirty = true;
  std::vector<uint32_t> price_perm;  // workers sorted by (price, index); rebuilt lazily (ensure_price_order)
  // coordinates -> site id (identical bit patterns <=> identical id); located population per site; bit 31 of a
  // worker's site word marks a site shared by >= 2 located workers (a hint for the carve: only those can have
  // same-site neighbours).  The bits are refreshed for the whole column when a site crosses the 1 <-> 2 line.
  SiteMap site_map;
  std::vector<uint32_t> site_pop;
  bool site_bits_dirty = false;
  DevBuf<unsigned char> d_row_stage;  // packed rows of pm_update_workers / pm_append_workers
  PinBuf<unsigned char> h_row_pin;    // ... and their pinned host staging (the copy is asynchronous: nothing waits for it)
  Event ev_row_stage;  // behind the last scatter that read the staging: asked (hipEventQuery) before the next one writes it

  // ---- task table
  // The table lives in a fixed-capacity index space [0, t_cap) and is filled from the TOP: the used part is
  // [t_lo, t_cap), ascending index u = get_all_tasks order (created_at desc).  New tasks are the newest, so they
  // go in FRONT — at lower indices — without moving anything (pm_tasks_insert_front); a deleted task leaves a
  // tombstone (mask 0, not live).  A task's index u is therefore a stable HANDLE (what groups store as their
  // claim); its position in the caller's current list — what the ABI reports — is the number of live tasks in
  // front of it (live bitmap + per-word prefix, on the device and lazily on the host).
  uint32_t T = 0;  // live tasks
  // Tombstones are reclaimed: the index space is rebuilt from the live rows alone when it regrows, and when more than
  // T + PM_TASK_DEAD_SLACK of them lie inside [t_lo, t_cap) (tasks_rebuild): the swept range stays within 2T + slack.
  uint32_t t_cap = 0, t_lo = 0, t_dead = 0;
  uint32_t t_regrowths = 0, t_compactions = 0;  // rebuilds of the index space since creation (pm_debug_carve_prof words 88..96)
  bool have_tasks = false;
  std::vector<uint64_t> h_tmask, h_tuid, h_tlive;  // indexed by u (h_tlive: bitmap words)
  std::vector<int64_t> h_created;
  std::vector<uint32_t> h_tprefix;
  bool h_tprefix_valid = false;
  bool tasks_have_uid = false;
  std::unordered_map<uint64_t, uint32_t> uid_to_u;  // built on the first pm_tasks_delete
  bool uid_map_valid = false;
  bool uid_dup = false;  // some id is carried by two live rows (seen when the map was built, or by an insertion since)
  uint32_t cfg_app_count[PM_MAX_CONFIGS]{};         // live tasks applicable per configuration (merge path)
  bool cfg_app_valid = false;
  DevBuf<uint64_t> d_tmask, d_tplanes, d_tlive;
  DevBuf<int64_t> d_created;
  DevBuf<uint32_t> d_tprefix, d_first_c, d_count_c, d_tdel;
  bool tplanes_dirty = true, tprefix_dirty = true;

  // ---- groups: the host vector is the source of truth between calls; device arrays mirror it
  std::vector<Group> groups;
  size_t n_dead_groups = 0;  // dissolved entries still in `groups` (slots shift only when they are removed)
  bool flags_dirty = false;  // h_flags changed since the last upload of the column
  std::vector<int32_t> h_group_of;
  uint64_t id_rng = 0;
  bool groups_dirty = true;
  // Delta sync of the device's group state (the churn path: a tick's status changes and new rows touch a few thousand
  // entries of tables that hold a hundred thousand).  While groups_delta_ok the device arrays are the host list as of the
  // last full push_groups / carve, except for what these record: workers whose group was dissolved since (group_of -> -1;
  // the dissolved group stays in both lists as a tombstone — no slot moves), rows appended since (group_of -> -1 for the
  // tail).  Anything else that changes the list clears the flag, and the next push_groups compacts and uploads it whole.
  bool groups_delta_ok = false;
  std::vector<uint32_t> delta_free;
  uint32_t delta_tail_from = PM_NONE;
  // ... and of the flags column: rows whose flags changed since the last upload, while flags_delta_ok
  bool flags_delta_ok = false;
  std::vector<uint32_t> delta_flags;
  PinBuf<uint32_t> h_delta_pin[2];  // pinned staging: [0] freed workers (indices), [1] flags ({index, value} pairs)
  DevBuf<uint32_t> d_delta[2];
  DevBuf<int32_t> d_group_of;
  DevBuf<uint32_t> d_g_cfg, d_g_n, d_g_off, d_g_task, d_g_task_next, d_members, d_by_rank, d_rank_in_group;
  DevBuf<uint64_t> d_g_id;
  uint32_t d_n_groups = 0, d_n_members = 0;

  // ---- carve scratch
  DevBuf<uint32_t> d_order;
  uint32_t form_rounds_hint = 0;  // validation rounds the last proposal-driven carve needed (0 = unknown)
  bool tick_needs_merge = false;  // the last pm_tick found two or more single-node groups (the merge pass ran): the next one does
                                  // not queue its pair sweep before it has seen the carve's result
  // group life-cycle feed (pm_enable_group_events / pm_drain_group_events)
  bool events_on = false;
  std::vector<pm_group_event> ev_log;
  std::vector<uint32_t> ev_members;
  DevBuf<double> d_c_lat, d_c_lon, d_c_cos, d_cc_lat, d_cc_lon, d_cc_cos, d_c_u[3], d_cc_u[3];
  DevBuf<uint64_t> d_c_compat, d_keys, d_bits;
  DevBuf<uint32_t> d_slot_pos, d_slot_wid;
  DevBuf<CarveStatus> d_status;
  DevBuf<CarveArgs> d_carve_args;   // the carve's argument block
  DevBuf<BatchDesc> d_desc;         // the proposal batch in preparation or under validation
  DevBuf<uint64_t> d_snap;          // [stride] the position bitmap as the preparation saw it
  // spatial index of a carve's located positions (cell_*_kernel)
  DevBuf<uint32_t> d_cell_cnt, d_cell_start, d_pos_cell, d_pos_rank, d_cs_of_pos, d_cs_slot, d_cs_site;
  DevBuf<double> d_cs_u[3];
  // pm_debug_first_batch_arm / _get: the host's copies of what the batch pipeline's first preparation and propose launch left in
  // HBM (form_queue_pairs takes them when armed; PM_FB_* of include/pm_engine_debug.h number the parts)
  bool fb_armed = false, fb_taken = false;
  std::vector<std::vector<unsigned char>> fb_part;
  DevBuf<double> d_c_pack, d_cs_pack;  // streaming carve: 32-byte gather records by position / by index entry
  // streaming carve (carve_stream_kernel): per-configuration bitmaps, ticket and row rings, control block, candidate list
  DevBuf<uint64_t> d_cfgbits, d_stream_sq, d_stream_row_lo, d_stream_row_hi, d_stream_trace;
  DevBuf<uint32_t> d_stream_ctl;
  uint32_t stream_seq = 0;       // launches so far: the tags of a launch's tickets start at stream_seq << 25
  uint32_t stream_wgs_env = 0;   // PM_STREAM_WGS: proposer workgroups (0 = by the size of the eligible list)
  uint32_t stream_la_env = 0;    // PM_STREAM_LA: look-ahead cap (0 = the kernel's default)
  uint32_t stream_la_div_env = 0;  // PM_STREAM_LA_DIV: look-ahead divisor (0 = the kernel's default)
  uint32_t stream_row_spins_env = 0;  // PM_STREAM_ROW_SPINS: polls before the validator gives a row up (0 = default)
  uint32_t n_cus = 256;
  uint32_t tick_stream_timeouts = 0, tick_stream_tickets = 0, tick_stream_aborts = 0;
  DevBuf<uint64_t> d_ikeys, d_umask;  // per-task orientation: table of the distinct topology masks, the masks densely
  DevBuf<uint32_t> d_ivals;
  DevBuf<uint32_t> d_m_cfg, d_m_n, d_m_off, d_m_members;  // MERGE batches

  // ---- sweep scratch
  DevBuf<uint64_t> d_sel, d_wplanes, d_sel_perm;
  DevBuf<uint32_t> d_first, d_count, d_rank, d_chosen, d_perm;
  DevBuf<pm_assignment> d_table;
  DevBuf<uint32_t> d_task_col;
  const pm_assignment* h_table = nullptr;  // the snapshot published last (host side of the lock-free look-up)
  uint64_t groups_epoch = 0, pub_groups_epoch = ~0ull;  // slot numbering of e->groups / the one the published rows use
  std::unordered_map<uint64_t, uint32_t> slot_of_id;    // pub_patch: group id -> slot under numbering slot_of_id_epoch
  uint64_t slot_of_id_epoch = ~0ull;
  // pinned staging for the group records a carve appended (absorbed into the host list by absorb_groups)
  PinBuf<uint32_t> h_gstage;
  const uint32_t *ab_cfg_p = nullptr, *ab_n_p = nullptr, *ab_off_p = nullptr, *ab_mem_p = nullptr;  // the staged records absorb_groups reads
  PinBuf<CarveStatus> h_status;  // pinned: carve_finish_kernel mirrors the status block here (streaming carve)
  Event ev_groups;
  bool absorb_pending = false;
  uint32_t ab_g0 = 0, ab_g1 = 0, ab_m0 = 0, ab_m1 = 0, ab_solo = 0;
  PinBuf<uint32_t> h_gtask_pinned;
  // set by publish_open for the run_match behind it: the claim writes the snapshot buffer and the task words itself
  pm_assignment* claim_h_table = nullptr;
  uint32_t* claim_h_gtask = nullptr;
  DevBuf<uint32_t> d_nb_idx;
  DevBuf<long long> d_nb_val;

  PubTable pub[2];
  std::atomic<int> pub_cur{-1};
  std::vector<PinBuf<uint64_t>> pub_retired;  // replaced snapshot buffers: a reader may still hold one, so they live as long as the engine
  pm_stats last_stats{};

  // ---- diagnostics scratch (pm_engine_report.inc): the reports read the engine's tables and write only these
  DevBuf<uint32_t> d_rep_rows, d_rep_why, d_rep_flags, d_rep_live, d_rep_g, d_rep_tprefix, d_rep_cnt, d_rep_task;
  DevBuf<int32_t> d_rep_gof;
  // ... of the group geography reports (pm_engine_spread.inc)
  DevBuf<uint32_t> d_spr_idx;
  DevBuf<pm_group_spread_row> d_spr_rows;
  DevBuf<SpreadCfgAcc> d_spr_acc;
  // ... of pm_nearest_workers (pm_engine_near.inc): the queries; km, rows and workers of every query, packed
  DevBuf<pm_near_query> d_near_q;
  DevBuf<double> d_near_out;
  std::vector<double> h_near_out;
  // ... of pm_probe_configs / pm_config_overlap (pm_engine_probe.inc): the probes' rows, alternatives and model bits, packed;
  // the masks (u64 a worker, when asked for) and the counters behind them, packed
  DevBuf<uint32_t> d_probe_in;
  DevBuf<uint64_t> d_probe_out;
  std::vector<uint32_t> h_probe_in;
  std::vector<uint64_t> h_probe_out;

  // ---- multi-GPU (pm_dist_*): this engine is rank `dist_rank` of `dist_world`, every rank holds the whole swarm
  uint32_t dist_rank = 0, dist_world = 1;
  std::vector<uint8_t> h_shard;        // owner rank of every worker
  std::vector<uint32_t> h_own_rows;    // workers owned by this rank, ascending
  uint32_t dist_cap_t = 0;             // table rows per rank in the exchange buffer (largest shard)
  DevBuf<uint8_t> d_shard;
  DevBuf<uint32_t> d_own_rows, d_xrow; // d_xrow[w] = shard * cap_t + index within the shard
  DevBuf<uint64_t> d_sel_own;
  DevBuf<pm_assignment> d_table_x;     // [world][cap_t] exchange buffer of published rows
  std::unique_ptr<pm::FormRun> form;   // carve in progress (stepwise tick)
  int dist_phase = 0;                  // 0 idle, 1 carving, 2 carve done, 3 match queued
  uint32_t dist_n_formed = 0, dist_n_merged = 0;
  uint32_t tick_host_resolved = 0, tick_carve_launches = 0, tick_carve_steps = 0;
  uint32_t tick_props = 0;
  uint64_t tick_prop_keys = 0;
  float k_ms_propose = 0;
  std::vector<Event> prop_ev;  // (start, stop) pairs of the proposer launches of the current poll interval
  size_t prop_ev_used = 0;

  // ---- the optional ledgers (the structs above): switched off by assigning a fresh one
  ChangeFeed chg;
  Liveness live;
  Discovery disc;
  Metrics mx;
  Rollout ro;
  Directory dir;  // (scratch only: never switched)
  GroupDir gdir;  // (the same)
  TaskDir tdir;   // (the same)
  AddressBook ab;
  Gate gate;      // (the book's index and scratch: never switched)
  Admission ad;
};
