// pm_carve_kernel.inc — carve_kernel (included by pm_kernels.hip inside namespace pm): the one-workgroup validator of
// the batch pipeline (carve_variant 3; also the merge pass and everything the streaming carve hands back).
__global__ __launch_bounds__(CARVE_THREADS) void carve_kernel(const CarveArgs* __restrict__ pa, uint32_t flags_in,
                                                              uint32_t start_ci) {
  const CarveArgs& p = *pa;  // argument block in device memory (a by-value struct this large would be
                             // copied to scratch as soon as a callee takes its address)
  // All LDS lives in the dynamic region, every carve offset a multiple of 16 B (a static __shared__ in
  // front of it would shift the base and put every 64-bit DS access on the 64-cycle misaligned path).
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  uint64_t* part = reinterpret_cast<uint64_t*>(s_raw);                       // [16 * PART]
  uint64_t* lds_alive = part + CARVE_WAVES * PM_CARVE_PART;                  // [SLOTS / 64]
  uint64_t* lds_loc = lds_alive + PM_CARVE_SLOTS / 64;                       // [SLOTS / 64]
  uint32_t* lds_wid = reinterpret_cast<uint32_t*>(lds_loc + PM_CARVE_SLOTS / 64);  // [SLOTS] big lists: the alive bitmap (small lists: unused)
  uint32_t* lds_site = lds_wid + PM_CARVE_SLOTS;                             // [SLOTS]
  uint64_t* lds_key = reinterpret_cast<uint64_t*>(lds_site + PM_CARVE_SLOTS);  // [SLOTS]
  uint32_t* sel_out = reinterpret_cast<uint32_t*>(lds_key + PM_CARVE_SLOTS);  // [SEL_CAP]
  BlockRed& red = *reinterpret_cast<BlockRed*>(sel_out + PM_CARVE_SEL_CAP);
  uint32_t& s_n = *reinterpret_cast<uint32_t*>(reinterpret_cast<unsigned char*>(&red) + sizeof(BlockRed));

  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const auto st = G(p.status);
  uint32_t flags = flags_in;
  if (!(flags & CARVE_F_INIT) && st->state != CARVE_STATE_RUNNING) return;  // queued behind a finished carve
  // (one batch at a time: the totals + ticket of the preparation behind this launch)
  if ((flags & CARVE_F_EXTPREP) && threadIdx.x <= PM_MAX_CONFIGS) p.prep_counts[threadIdx.x] = 0u;
  PROF_DECL;

  uint32_t n;
  StepCtx c;
  c.mode = p.mode;
  c.proximity = p.proximity;
  c.use_props = (flags_in & CARVE_F_PROPS) != 0u;
  c.steps = 0;
  c.fast_steps = 0;
  c.cand_sum = 0;
  uint32_t ci;          // configuration being prepared / run
  bool prepared;
  if (flags & CARVE_F_INIT) {
    // ---- ordered eligible list.  FORM: compact the eligible rows (Healthy & p2p & unassigned,
    // mod.rs:492-497) in input order.  MERGE: supplied by the engine.
    if (p.mode == CARVE_MODE_FORM) {
      if (tid == 0) s_n = 0;
      __syncthreads();
      for (uint32_t base = 0; base < p.W; base += CARVE_THREADS) {
        const uint32_t w = base + tid;
        bool e = false;
        if (w < p.W) {
          const uint32_t f = G(p.wflags)[w];
          e = (f & PM_W_HEALTHY) && (f & PM_W_HAS_P2P) && G(p.group_of)[w] < 0;
        }
        const uint64_t bal = __ballot(e);
        if (lane == 0) red.a[wave] = __popcll(bal);
        __syncthreads();
        uint32_t off = s_n;
        for (uint32_t k = 0; k < wave; ++k) off += red.a[k];
        if (e) G(p.order)[off + __popcll(bal & ((1ull << lane) - 1ull))] = w;
        __syncthreads();
        if (tid == 0) {
          uint32_t tot = 0;
          for (uint32_t k = 0; k < CARVE_WAVES; ++k) tot += red.a[k];
          s_n += tot;
        }
        __syncthreads();
      }
      n = s_n;
    } else {
      n = p.n_order;
    }
    const uint32_t n_words = (n + 63u) >> 6;
    // position-indexed columns + alive / loc bitmaps (L2 resident)
    for (uint32_t base = 0; base < n_words * 64u; base += CARVE_THREADS) {
      const uint32_t i = base + tid;
      bool has_loc = false;
      if (i < n) {
        const uint32_t w = G(p.order)[i];
        has_loc = (G(p.wflags)[w] & PM_W_HAS_LOC) != 0;
        G(p.c_lat)[i] = G(p.lat)[w];
        G(p.c_lon)[i] = G(p.lon)[w];
        G(p.c_cos)[i] = G(p.coslat)[w];
        G(p.c_ux)[i] = G(p.ux)[w];
        G(p.c_uy)[i] = G(p.uy)[w];
        G(p.c_uz)[i] = G(p.uz)[w];
        G(p.c_site)[i] = G(p.site)[w];
        G(p.c_compat)[i] = G(p.compat)[w];
      }
      const uint64_t bl = __ballot(has_loc);
      const uint64_t ba = __ballot(i < n);
      if (lane == 0 && (i >> 6) < n_words) {
        G(p.loc_g)[i >> 6] = bl;
        G(p.alive_g)[i >> 6] = ba;
      }
    }
    __syncthreads();
    c.total_available = n;  // mod.rs:503
    ci = start_ci;
    prepared = false;
    if (flags & CARVE_F_EXTPREP) {  // the lists are prepared by carve_prep_*_kernel on the whole chip
      if (tid <= PM_MAX_CONFIGS) p.prep_counts[tid] = 0u;
      if (tid == 0) {
        st->n_eligible = n;
        st->total_available = n;
        st->cur_ci = start_ci;
        st->g_lo = st->g_hi = st->n_groups;
      }
      return;
    }
  } else {
    n = st->n_eligible;
    c.total_available = st->total_available;
    ci = st->cur_ci;
    prepared = true;
    if (flags & CARVE_F_EXTPREP) {
      // the batch the preparation kernels describe: acceptable if it started from the configuration the carve is at
      const BatchDesc d = *p.desc;
      if (!d.planned || d.ci0 != ci || !(d.valid || d.none)) {
        if (tid == 0) {  // (prepared beside the batch in front, for the configuration it did not end at)
          st->n_void += 1u;
          st->why[4] += 1u;
        }
        return;
      }
      if (d.none) {  // no configuration left that can be entered
        if (tid == 0) {
          st->state = CARVE_STATE_DONE;
          st->cur_ci = p.n_avail;
        }
        return;
      }
      ci = d.ci;  // (the ones in between cannot be entered)
    }
    if (ci >= p.n_avail) return;
  }
  c.n_groups = st->n_groups;
  c.mem_off = st->n_members;
  const uint32_t groups_at_entry = c.n_groups;
  const uint32_t steps_before = st->steps_total;
  uint32_t exit_state = CARVE_STATE_RUNNING, stop_ci = p.n_avail;
  uint32_t slow_before_cfg = 0;

  PROF_MARK(15);  // init / status load
  for (;;) {
    // ---- prepare: candidate list of the next configuration whose loop would be entered
    // (mod.rs:505-519; the list is mod.rs:511-515 evaluated once, removals are applied to bitmaps)
    if (!prepared) {
      c.n_list = 0;
      c.prop_k = 0;
      c.prop_limit = 0;
      c.n_seeds = 0;
      for (; ci < p.n_avail; ++ci) {
        c.min_s = p.min_size[ci];
        c.max_s = p.max_size[ci];
        if (p.mode == CARVE_MODE_FORM && c.total_available < c.min_s) continue;  // `while` never entered (:507)
        const uint64_t cbit = 1ull << p.avail_cfg[ci];
        PROF_MARK(29);  // loop overhead
        c.n_list = carve_compact_count(p, red, n, cbit, p.alive_g);
        PROF_MARK(26);
        PM_PROF(if (tid == 0) G(p.status)->prof[30] += 1;)
        if (c.n_list < c.min_s || c.n_list == 0) continue;  // mod.rs:517-519
        carve_compact_place(p, red, n, cbit, c.n_list, p.alive_g);
        PROF_MARK(27);
        break;
      }
      if (ci >= p.n_avail) {
        exit_state = CARVE_STATE_DONE;
        break;
      }
      // proposals: one neighbour list per located slot, K = (max - 1) + reserve entries
      if ((flags & CARVE_F_PROPS) && p.proximity && c.n_list <= PM_CARVE_BIG_SLOTS && c.max_s - 1u < PM_PROP_KMAX) {
        const uint32_t k = c.max_s - 1u + PM_PROP_RESERVE;
        c.prop_k = k < PM_PROP_KMAX ? k : PM_PROP_KMAX;  // the last entry of a row carries its flags word
        // one proposal per located slot, at most PM_PROP_MAX_SEEDS per round: prop_limit = the slot after the
        // PM_PROP_MAX_SEEDS-th located one (a later round covers the rest)
        uint32_t n_seeds = 0;
        c.prop_limit = carve_prop_limit(p, red, c.n_list, &n_seeds);
        c.n_seeds = n_seeds;
      }
      prepared = true;
      PROF_MARK(28);
      if (!(flags & CARVE_F_RUN)) break;  // prepare-only launch
    } else if (flags & CARVE_F_EXTPREP) {
      const BatchDesc d = *p.desc;
      c.n_list = d.n_list;
      c.prop_k = d.prop_k;
      c.prop_limit = d.prop_limit;
      c.n_seeds = d.n_seeds;
      c.min_s = p.min_size[ci];
      c.max_s = p.max_size[ci];
    } else {
      c.n_list = st->n_list;
      c.prop_k = st->prop_k;
      c.prop_limit = st->prop_limit;
      c.n_seeds = st->n_seeds;
      c.min_s = p.min_size[ci];
      c.max_s = p.max_size[ci];
    }
    c.cfg = p.avail_cfg[ci];
    c.n_cand = c.n_list;
    c.n_start = c.n_list;

    // ---- run the prepared configuration.  Three storage modes:
    //   small (<= PM_CARVE_SLOTS slots):  every per-slot array in LDS
    //   big   (<= PM_CARVE_BIG_SLOTS):    bitmaps + staged proposal rows in LDS, per-slot arrays in HBM/L2
    //   mem   (larger):                   everything in HBM/L2, exact sweep only
    ctx_set_geometry(c);
    const bool force_mem = p.debug_mem_above && c.n_list > p.debug_mem_above;  // (test hook)
    const bool in_lds = c.n_list <= PM_CARVE_SLOTS && !force_mem;
    const bool big = !in_lds && c.n_list <= PM_CARVE_BIG_SLOTS && !force_mem;
    const uint32_t lw = (c.n_list + 63u) >> 6;
    uint64_t* g_alive = p.bits_scratch;
    uint64_t* g_loc = p.bits_scratch + p.bits_stride;
    // big mode: the worker-id / site-id regions (32 KiB each) hold the bitmaps instead
    uint64_t* r_alive = in_lds ? lds_alive : (big ? reinterpret_cast<uint64_t*>(lds_wid) : g_alive);
    uint64_t* r_loc = in_lds ? lds_loc : (big ? reinterpret_cast<uint64_t*>(lds_site) : g_loc);
    if (in_lds || big) {
      for (uint32_t j = tid; j < lw; j += CARVE_THREADS) {
        r_alive[j] = g_alive[j];
        r_loc[j] = g_loc[j];
      }
    }
    if (in_lds)
      for (uint32_t sl = tid; sl < c.n_list; sl += CARVE_THREADS) lds_site[sl] = G(p.cc_site)[sl];
    __syncthreads();
    PROF_MARK(10);
    const uint32_t slow0 = c.steps - c.fast_steps;
    const uint32_t mem_before_run = c.mem_off;
    int rc;
    if (in_lds) {
      rc = carve_run_lds<false>(p, red, c, p.slot_wid, lds_site, lds_key, r_alive, r_loc, part, sel_out,
                                reinterpret_cast<uint32_t*>(lds_key), steps_before);
    } else if (big) {
      rc = carve_run_lds<true>(p, red, c, p.slot_wid, p.cc_site, p.keys, r_alive, r_loc, part, sel_out,
                               reinterpret_cast<uint32_t*>(lds_key), steps_before);
    } else {
      do {
        rc = carve_step_mem(p, red, c, part, p.keys, p.slot_wid, g_alive, g_loc, steps_before);
      } while (rc == STEP_CONTINUE && !(c.n_cand * 2u < c.n_list));
    }
    (void)slow0;
    (void)slow_before_cfg;
    __syncthreads();
    PROF_MARK(13);
    if (in_lds || big) {
      // Everything this run took is a member it appended (recorded as a SLOT): clear its position in the eligible
      // bitmap, so the next compaction / configuration sees the removal, and replace the slot by the worker id.
      // (Proportional to the groups formed, not to the length of the list.)
      for (uint32_t k = mem_before_run + tid; k < c.mem_off; k += CARVE_THREADS) {
        const uint32_t sl = G(p.members)[k];
        const uint32_t i = G(p.slot_pos)[sl] & 0x7FFFFFFFu;  // bit 31: the slot has a location
        atomicAnd((unsigned long long*)&G(p.alive_g)[i >> 6], ~(1ull << (i & 63u)));
        G(p.members)[k] = G(p.slot_wid)[sl];
      }
    } else {  // lists in HBM: carve_step_mem records worker ids; dead slots -> position bitmap
      const uint64_t* alive = r_alive;
      for (uint32_t sl = tid; sl < c.n_list; sl += CARVE_THREADS)
        if (!bit_at(alive, sl)) {
          const uint32_t i = G(p.slot_pos)[sl] & 0x7FFFFFFFu;
          atomicAnd((unsigned long long*)&G(p.alive_g)[i >> 6], ~(1ull << (i & 63u)));
        }
    }
    __syncthreads();
    PROF_MARK(12);
    if (rc == STEP_UNCERTAIN || rc == STEP_OVERFLOW || rc == STEP_ABORT) {
      exit_state = rc == STEP_UNCERTAIN ? CARVE_STATE_UNCERTAIN : rc == STEP_ABORT ? CARVE_STATE_ABORTED : CARVE_STATE_OVERFLOW;
      stop_ci = ci;
      break;
    }
    prepared = false;
    if (rc == STEP_BREAK) {  // configuration exhausted; STEP_CONTINUE => re-prepare the same configuration
      ++ci;
      if (tid == 0) st->why[3] += 1u;
    }
    if (flags & CARVE_F_EXTPREP) break;  // the next list is prepared on the whole chip (carve_prep_*_kernel)
    if (!(flags & CARVE_F_ALL)) flags &= ~CARVE_F_RUN;  // per-configuration launch: prepare the next list, leave
  }

  // group_of for everything carved by this launch (FORM), one parallel pass at the end — or, with the external
  // preparation, left to carve_prep_count_kernel (every CU); single-node groups are counted here either way
  const bool ext = (flags_in & CARVE_F_EXTPREP) != 0u;
  // (a launch with the external preparation runs ONE configuration, c.min_s is its minimum: groups of one node can
  // only come from a configuration that allows them — otherwise there is nothing to do here, and a loop with a
  // dependent load per group is a tenth of the launch at 100 k workers)
  const bool need_pass = !ext || c.min_s <= 1u;
  if (p.mode == CARVE_MODE_FORM && need_pass) {
    __syncthreads();
    for (uint32_t g = groups_at_entry + wave; g < c.n_groups; g += CARVE_WAVES) {
      const uint32_t off = G(p.g_off)[g], gn = G(p.g_n)[g];
      if (!ext)  // (the preparation behind this launch does it on every CU)
        for (uint32_t k = lane; k < gn; k += 64u) G(p.group_of)[G(p.members)[off + k]] = (int32_t)g;
      if (gn == 1u && lane == 0) atomicAdd(&p.status->n_solo, 1u);  // rare
    }
  }
  __syncthreads();
  PROF_MARK(14);
  if (tid == 0) {
    st->state = exit_state;
    st->n_groups = c.n_groups;
    st->n_members = c.mem_off;
    st->steps_total = steps_before + c.steps;
    st->stop_ci = stop_ci;
    st->n_eligible = n;
    st->cand_sum += c.cand_sum;
    st->cur_ci = exit_state == CARVE_STATE_DONE ? p.n_avail : ci;
    st->n_list = c.n_list;
    st->prop_k = c.prop_k;
    st->prop_limit = c.prop_limit;
    st->n_seeds = c.n_seeds;
    st->total_available = c.total_available;
    if (ext) {
      st->g_lo = groups_at_entry;
      st->g_hi = c.n_groups;
    }
    st->fast_steps += c.fast_steps;
    st->slow_steps += c.steps - c.fast_steps;
    if (!(flags_in & CARVE_F_INIT)) st->n_batches += 1;
  }
}

