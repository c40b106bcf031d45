// pm_launch.inc — the launchers pm_engine.cpp calls (included by pm_kernels.hip inside namespace pm).
// ------------------------------------------------------------------------------------------------
// launchers (called from pm_engine.cpp)

void launch_compat(const CompatArgs& a, hipStream_t s) {
  if (a.W == 0) return;
  if (a.W < 65536u)  // (few workers: a workgroup's four waves share the configurations — see compat_body)
    hipLaunchKernelGGL(compat_sliced_kernel, dim3((a.W + 63u) / 64u), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(compat_kernel, dim3((a.W + 255u) / 256u), dim3(256), 0, s, a);
}
void launch_triad(const double* b, const double* c, double* a, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(triad_kernel, dim3(256 * 32), dim3(256), 0, s, b, c, a, n);
}
void launch_row_network_test(const uint64_t* keys, const uint32_t* sites, uint32_t n_waves, uint32_t n_per_wave, uint32_t slot_bits,
                             uint64_t ulps, uint32_t upto, uint64_t* rows_out, uint32_t* mismatches, hipStream_t s, double tie_band,
                             uint64_t* cert_rows, uint64_t* cert_track, uint32_t* cert_flags, uint64_t* cert_mine) {
  hipLaunchKernelGGL(row_network_test_kernel, dim3(n_waves / 4u), dim3(256), 0, s, keys, sites, n_per_wave, slot_bits, ulps, upto, rows_out,
                     mismatches, tie_band, RowCertOut{cert_rows, cert_track, cert_flags, cert_mine});
}
void launch_distance_key_test(const double* in, const double* geo, uint32_t n, uint32_t mode, double* out, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(distance_key_test_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, in, geo, n, mode, out);
}
void launch_geo(const double* lat, const double* lon, double* coslat, double* ux, double* uy, double* uz, uint32_t W,
                hipStream_t s) {
  if (W == 0) return;
  hipLaunchKernelGGL(geo_kernel, dim3((W + 255u) / 256u), dim3(256), 0, s, lat, lon, coslat, ux, uy, uz, W);
}
void launch_update_rows(const RowUpdateArgs& a, hipStream_t s) {
  if (a.n == 0) return;
  hipLaunchKernelGGL(update_rows_kernel, dim3((a.n + 255u) / 256u), dim3(256), 0, s, a);
}
void launch_worker_selector(const int32_t* group_of, const uint32_t* g_cfg, uint32_t R, const uint32_t* rows,
                            uint64_t* sel, hipStream_t s) {
  if (R == 0) return;
  hipLaunchKernelGGL(worker_selector_kernel, dim3((R + 255u) / 256u), dim3(256), 0, s, group_of, g_cfg, R, rows, sel);
}
void launch_chooser_rank(const int32_t* group_of, const uint64_t* g_id, const uint32_t* count, uint32_t R,
                         const uint32_t* rows, uint64_t seed, uint32_t* rank, hipStream_t s) {
  if (R == 0) return;
  hipLaunchKernelGGL(chooser_rank_kernel, dim3((R + 255u) / 256u), dim3(256), 0, s, group_of, g_id, count, R, rows,
                     seed, rank);
}
void launch_eligible_selector(const uint32_t* wflags, const int32_t* group_of, const uint64_t* compat,
                              uint64_t enabled, uint32_t W, const uint8_t* shard, uint32_t my_rank, uint64_t* sel,
                              hipStream_t s) {
  if (W == 0) return;
  hipLaunchKernelGGL(eligible_selector_kernel, dim3((W + 255u) / 256u), dim3(256), 0, s, wflags, group_of, compat,
                     enabled, W, shard, my_rank, sel);
}
void launch_table_scatter(const pm_assignment* x, const uint32_t* xrow, uint32_t W, pm_assignment* table,
                          uint32_t* task_col, uint32_t* g_task_next, const uint64_t* t_live, const uint32_t* t_prefix,
                          hipStream_t s) {
  if (W == 0) return;
  hipLaunchKernelGGL(table_scatter_kernel, dim3((W + 255u) / 256u), dim3(256), 0, s, x, xrow, W, table, task_col,
                     g_task_next, t_live, t_prefix);
}
void launch_group_rank(const int32_t* group_of, const uint32_t* g_n, const uint32_t* g_off, const uint32_t* members,
                       const uint32_t* addr_rank, uint32_t W, uint32_t* rank_in_group, uint32_t* by_rank,
                       hipStream_t s) {
  if (W == 0) return;
  hipLaunchKernelGGL(group_rank_kernel, dim3((W + 255u) / 256u), dim3(256), 0, s, group_of, g_n, g_off, members,
                     addr_rank, W, rank_in_group, by_rank);
}
void launch_match_prep(const MatchPrepArgs& a, hipStream_t s) {
  const uint32_t n = a.W > a.G ? a.W : a.G;
  if (n == 0) return;
  hipLaunchKernelGGL(match_prep_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, a);
}
void launch_claim_publish(const ClaimArgs& a, hipStream_t s) {
  if (a.R == 0) return;
  hipLaunchKernelGGL(claim_publish_kernel, dim3((a.R + 255u) / 256u), dim3(256), 0, s, a);
}

// A swept axis is the column range [c_begin, c_end) of an index space of n_cols columns whose bit planes have a
// stride of `stride` words (c_begin need not be word-aligned: the bits below it are zero in every plane).
void launch_build_planes(const uint64_t* col_mask, uint32_t n_cols, uint32_t c_begin, uint32_t c_end, uint32_t stride,
                         uint32_t n_planes, uint64_t* planes, hipStream_t s) {
  const uint32_t w0 = c_begin / 64u, w1 = (c_end + 63u) / 64u;
  if (w1 <= w0) return;
  hipLaunchKernelGGL(build_planes_kernel, dim3(((w1 - w0) * 64u + 255u) / 256u), dim3(256), 0, s, col_mask, n_cols, w0,
                     w1, stride, n_planes, planes);
}

// Pair sweep: rows x cols -> first hit (absolute column index) + hit count per row.
void launch_pair_sweep(int variant, const uint64_t* row_sel, uint32_t R, const uint64_t* col_mask,
                       const uint64_t* planes, uint32_t c_begin, uint32_t c_end, uint32_t stride, uint32_t n_planes,
                       uint32_t* first, uint32_t* count, hipStream_t s, bool inited) {
  if (R == 0) return;
  const uint32_t rb = (R + 255u) / 256u;
  // (inited: first / count hold PM_NONE / 0 already — match_prep_kernel)
  // enough workgroups to cover 256 CUs — several times over when the rows are many (a split's results are merged by
  // atomics: first = min, count = add, 8 bytes of write traffic per row and split); with up to 16,384 rows (the
  // reference orientation at configs[1]: one row per worker) twice over is enough, and the atomics of 52 splits were
  // 4.2 MB of the sweep's 5.7 MB against 1.8 MB of compulsory traffic (profiles/r04_pmc_traffic.json)
#ifndef PM_SWEEP_RPT4_MIN_RB
#define PM_SWEEP_RPT4_MIN_RB 256u  // row blocks from which a thread takes four rows (pair_sweep_planes_kernel<4>): configs[2]'s 100k workers: sweep kernel 0.62 -> 0.41 ms
#endif
  const bool rpt4 = rb >= PM_SWEEP_RPT4_MIN_RB;
#ifndef PM_SWEEP_RPT_N
#define PM_SWEEP_RPT_N 4u
#endif
  const uint32_t rbe = (rpt4 && rb < 1024u) ? (rb + PM_SWEEP_RPT_N - 1u) / PM_SWEEP_RPT_N : rb;  // (workgroups along the rows, for the splits' count)
  // (where a thread takes four rows, 1,400 workgroups: 15 splits of configs[2]'s 98 row blocks where 2,048 made 21 — every
  // (row, split) is two atomics counted at line granularity: a third less of them, and 5 % off the kernel;
  // profiles/r06_pipeline_experiments.txt)
  const uint32_t want_split = ((R <= 16384u ? 512u : (rpt4 && rb < 1024u) ? 1400u : 2048u) + rbe - 1u) / rbe;
  const uint32_t n_cols = c_end > c_begin ? c_end - c_begin : 0u;
  if (n_cols == 0) {
    if (!inited) hipLaunchKernelGGL(pair_init_kernel, dim3(rb), dim3(256), 0, s, first, count, R);
    return;
  }
  if (variant == 1) {
    uint32_t n_split = want_split < n_cols ? want_split : n_cols;
    const uint32_t chunk = (n_cols + n_split - 1u) / n_split;
    n_split = (n_cols + chunk - 1u) / chunk;
    if (n_split > 1u && !inited) hipLaunchKernelGGL(pair_init_kernel, dim3(rb), dim3(256), 0, s, first, count, R);
    hipLaunchKernelGGL(pair_sweep_scalar_kernel, dim3(rb, n_split), dim3(256), 0, s, row_sel, R, col_mask, c_begin,
                       c_end, chunk, first, count, n_split > 1u ? 1u : 0u);
    return;
  }
  const uint32_t w0 = c_begin / 64u, w1 = (c_end + 63u) / 64u, n_words = w1 - w0;
  uint32_t n_split = want_split < n_words ? want_split : n_words;
  const uint32_t wps = (n_words + n_split - 1u) / n_split;
  n_split = (n_words + wps - 1u) / wps;
  const uint32_t lds_cap_words = ((48u * 1024u / 8u) / (n_planes + 1u)) - 1u;  // n_planes + 1 planes, padded stride
  const uint32_t wpp = wps < lds_cap_words ? wps : lds_cap_words;
  const size_t lds = (size_t)(n_planes + 1u) * (wpp | 1u) * sizeof(uint64_t);
  if (n_split > 1u && !inited) hipLaunchKernelGGL(pair_init_kernel, dim3(rb), dim3(256), 0, s, first, count, R);
  if (rpt4)  // very many rows (a million tasks): four per thread, a quarter of the plane staging
    hipLaunchKernelGGL(pair_sweep_planes_kernel<PM_SWEEP_RPT_N>, dim3((rb + PM_SWEEP_RPT_N - 1u) / PM_SWEEP_RPT_N, n_split), dim3(256), lds, s,
                       row_sel, R, planes, stride, w0, w1, n_planes, wps, wpp, first, count, n_split > 1u ? 1u : 0u);
  else
    hipLaunchKernelGGL(pair_sweep_planes_kernel<1u>, dim3(rb, n_split), dim3(256), lds, s, row_sel, R, planes, stride, w0,
                       w1, n_planes, wps, wpp, first, count, n_split > 1u ? 1u : 0u);
}

void launch_pair_select(int variant, const uint64_t* row_sel, uint32_t R, const uint64_t* col_mask,
                        const uint64_t* planes, uint32_t c_begin, uint32_t c_end, uint32_t stride, uint32_t n_planes,
                        const uint32_t* rank, uint32_t* out, hipStream_t s) {
  if (R == 0) return;
  const uint32_t rb = (R + 255u) / 256u;
  if (variant == 1) {
    hipLaunchKernelGGL(pair_select_scalar_kernel, dim3(rb), dim3(256), 0, s, row_sel, R, col_mask, c_begin, c_end,
                       rank, out);
  } else {
    hipLaunchKernelGGL(pair_select_planes_kernel, dim3(rb), dim3(256), 0, s, row_sel, R, planes, stride,
                       c_begin / 64u, (c_end + 63u) / 64u, n_planes, rank, out);
  }
}

void launch_task_prefix(const uint64_t* live, uint32_t w_begin, uint32_t w_end, uint32_t* prefix, hipStream_t s) {
  if (w_end <= w_begin) return;
  hipLaunchKernelGGL(task_prefix_kernel, dim3(1), dim3(64), 0, s, live, w_begin, w_end, prefix);
}
void launch_task_delete(const uint32_t* slots, uint32_t n, uint64_t* tmask, uint64_t* live, uint64_t* planes,
                        uint32_t stride, uint32_t n_planes, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(task_delete_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, slots, n, tmask, live, planes,
                     stride, n_planes);
}
void launch_task_intern(const uint64_t* tmask, const uint64_t* live, uint32_t u_begin, uint32_t u_end, uint64_t valid,
                        uint64_t* keys, uint32_t n_slots, uint32_t* vals, uint32_t* counter_and_overflow, uint64_t* umask,
                        uint32_t cap_u, hipStream_t s) {
  (void)hipMemsetAsync(keys, 0xFF, size_t(n_slots) * 8, s);
  (void)hipMemsetAsync(counter_and_overflow, 0, 8, s);
  if (u_end > u_begin)
    hipLaunchKernelGGL(task_intern_insert_kernel, dim3((u_end - u_begin + 255u) / 256u), dim3(256), 0, s, tmask, live, u_begin,
                       u_end, valid, (unsigned long long*)keys, n_slots - 1u, counter_and_overflow + 1);
  hipLaunchKernelGGL(task_intern_number_kernel, dim3((n_slots + 255u) / 256u), dim3(256), 0, s,
                     (const unsigned long long*)keys, n_slots, vals, counter_and_overflow, umask, cap_u);
}
void launch_task_compact_class(const uint32_t* first_c, const uint32_t* count_c, const uint64_t* tmask, uint64_t valid,
                               const uint64_t* keys, const uint32_t* vals, uint32_t n_slots, uint32_t u_begin,
                               uint32_t u_end, const uint64_t* live, const uint32_t* prefix, uint32_t* first_out,
                               uint32_t* count_out, hipStream_t s) {
  if (u_end <= u_begin) return;
  hipLaunchKernelGGL(task_compact_class_kernel, dim3((u_end - u_begin + 255u) / 256u), dim3(256), 0, s, first_c, count_c,
                     tmask, valid, (const unsigned long long*)keys, vals, n_slots - 1u, u_begin, u_end, live, prefix,
                     first_out, count_out);
}
void launch_task_compact(const uint32_t* first_u, const uint32_t* count_u, uint32_t u_begin, uint32_t u_end,
                         const uint64_t* live, const uint32_t* prefix, uint32_t* first_out, uint32_t* count_out,
                         hipStream_t s) {
  if (u_end <= u_begin) return;
  hipLaunchKernelGGL(task_compact_kernel, dim3((u_end - u_begin + 255u) / 256u), dim3(256), 0, s, first_u, count_u,
                     u_begin, u_end, live, prefix, first_out, count_out);
}

void launch_newest(const int64_t* created_at, const uint64_t* live, uint32_t t_begin, uint32_t t_end,
                   uint32_t* idx_by_block, long long* val_by_block, uint32_t n_blocks, hipStream_t s) {
  hipLaunchKernelGGL(newest_kernel, dim3(n_blocks), dim3(256), 0, s, created_at, live, t_begin, t_end,
                     (unsigned long long*)nullptr, idx_by_block, val_by_block);
}

void launch_carve_propose(const CarveArgs* d_args, uint32_t W, hipStream_t s) {
  // one wave per located slot, grid-stride; 2048 workgroups x 4 waves keep all 256 CUs busy
  uint32_t blocks = (W + 3u) / 4u;
  if (blocks > 2048u) blocks = 2048u;
  if (blocks == 0) blocks = 1;
  hipLaunchKernelGGL(carve_propose_kernel, dim3(blocks), dim3(256), 0, s, d_args);
}

// ids of freshly carved groups: outputs k+1 .. of the splitmix64 stream whose state is `state`
// (generate_group_id, injected — SURVEY section 8c), and an empty task word for each
__global__ __launch_bounds__(256) void group_ids_kernel(uint64_t* __restrict__ g_id, uint32_t* __restrict__ g_task,
                                                        uint32_t n, uint64_t state) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  uint64_t z = state + (uint64_t)(k + 1u) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  g_id[k] = z ^ (z >> 31);
  g_task[k] = PM_NONE;
}
void launch_group_ids(uint64_t* g_id, uint32_t* g_task, uint32_t n, uint64_t rng_state, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(group_ids_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, g_id, g_task, n, rng_state);
}

// the two full-chip kernels that prepare the next candidate list: one 64-position word per wave
uint32_t launch_carve_prep(const CarveArgs* d_args, uint32_t W, hipStream_t s) {  // returns the launches it made
  uint32_t blocks = ((W + 63u) / 64u + PREP_WAVES - 1u) / PREP_WAVES;
  if (blocks == 0) blocks = 1;
  hipLaunchKernelGGL(carve_prep_count_kernel, dim3(blocks), dim3(256), 0, s, d_args);
  hipLaunchKernelGGL(carve_prep_place_kernel, dim3(blocks), dim3(256), 0, s, d_args);
  return 2u;
}
// n_bound: rows outside any group (an upper bound of the eligible list); index_min: build the spatial index when
// n_bound reaches it (0 = never; the kernels decide the grid from the real length and may still decline)
// put: the argument block is not on the device yet — it travels as the first kernel's own argument, which stores it
uint32_t launch_carve_elig(CarveArgs* d_args, const CarveArgs* put, uint32_t W, uint32_t n_bound, uint32_t index_min, uint32_t start_ci,
                           bool fresh, uint32_t n_groups0, uint32_t n_members0, hipStream_t s) {
  uint32_t blocks = ((W + 63u) / 64u + PREP_WAVES - 1u) / PREP_WAVES;
  if (blocks == 0) blocks = 1;
  if (put) {
    CarveArgWords w{};
    __builtin_memcpy(w.w, put, sizeof(CarveArgs));
    hipLaunchKernelGGL(carve_elig_count_put_kernel, dim3(blocks), dim3(256), 0, s, w, reinterpret_cast<uint32_t*>(d_args),
                       fresh ? 1u : 0u, n_groups0, n_members0);
  } else {
    hipLaunchKernelGGL(carve_elig_count_kernel, dim3(blocks), dim3(256), 0, s, d_args, fresh ? 1u : 0u, n_groups0, n_members0);
  }
  hipLaunchKernelGGL(carve_elig_place_kernel, dim3(blocks), dim3(256), 0, s, d_args, start_ci);
  if (!index_min || n_bound < index_min) return 2u;  // (the status of a fresh carve says cell_g = 0)
  const uint32_t pb = (n_bound + 255u) / 256u;
  hipLaunchKernelGGL(cell_count_kernel, dim3(pb), dim3(256), 0, s, d_args);
  const uint32_t sb = (PM_CELL_TABLE + CELL_SCAN_PER_BLOCK - 1u) / CELL_SCAN_PER_BLOCK;  // (blocks beyond the grid in use return)
  hipLaunchKernelGGL(cell_scan_sums_kernel, dim3(sb), dim3(256), 0, s, d_args);
  hipLaunchKernelGGL(cell_scan_apply_kernel, dim3(sb), dim3(256), 0, s, d_args);
  hipLaunchKernelGGL(cell_place_kernel, dim3(pb), dim3(256), 0, s, d_args);
  return 6u;
}
// The argument block of a carve goes up as the ARGUMENT of a one-workgroup kernel — the words travel in the launch packet's
// kernarg segment and the kernel stores them — instead of as a host-to-device copy: between two kernels of a stream a copy is
// a launch of the runtime's copy kernel with 17 us of an idle GPU in front of it and 7 behind (profiles/r06_timeline.txt),
// a kernel is 5.
__global__ __launch_bounds__(256) void carve_args_put_kernel(CarveArgWords a, uint32_t* __restrict__ dst) {
  for (uint32_t i = threadIdx.x; i < sizeof(CarveArgWords) / 4u; i += 256u) dst[i] = a.w[i];
}
hipError_t launch_carve_args_put(const CarveArgs& a, CarveArgs* d_args, hipStream_t s) {
  CarveArgWords w{};
  __builtin_memcpy(w.w, &a, sizeof(CarveArgs));
  hipLaunchKernelGGL(carve_args_put_kernel, dim3(1), dim3(256), 0, s, w, reinterpret_cast<uint32_t*>(d_args));
  return hipGetLastError();
}
// group_of for the groups of the last validation launch (the count kernel's first half), e.g. after the carve ended
void launch_carve_apply(const CarveArgs* d_args, uint32_t W, hipStream_t s) {
  uint32_t blocks = ((W + 63u) / 64u + PREP_WAVES - 1u) / PREP_WAVES;
  if (blocks == 0) blocks = 1;
  hipLaunchKernelGGL(carve_prep_count_kernel, dim3(blocks), dim3(256), 0, s, d_args);
}

// The carve kernels' dynamic LDS sizes, for the CURRENT device: called by pm_engine_create behind hipSetDevice (the
// attribute is per device and function; a process-wide "already set" flag raced between engines' host threads and
// left a second device without it).
hipError_t carve_kernels_init() {
  hipError_t e = hipFuncSetAttribute((const void*)carve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PM_CARVE_LDS_BYTES);
  if (e != hipSuccess) return e;
  return hipFuncSetAttribute((const void*)carve_stream_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PM_STREAM_LDS_BYTES);
}

#ifdef PM_ROW_BENCH
hipError_t launch_row_bench(const CarveArgs* d_args, uint32_t seed, uint32_t ci, uint32_t reps, uint32_t mode, unsigned long long* d_out, hipStream_t s) {
  hipError_t e = hipMemcpyToSymbolAsync(HIP_SYMBOL(g_rowb_mode), &mode, 4, 0, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return e;
  e = hipFuncSetAttribute((const void*)carve_row_bench_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PM_STREAM_LDS_BYTES);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(carve_row_bench_kernel, dim3(1), dim3(CARVE_THREADS), PM_STREAM_LDS_BYTES, s, d_args, seed, ci, reps, d_out);
  static const uint32_t zero = 0u;
  (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_rowb_mode), &zero, 4, 0, hipMemcpyHostToDevice, s);
  return hipGetLastError();
}
#endif
hipError_t launch_carve(const CarveArgs* d_args, uint32_t flags, uint32_t start_ci, size_t lds_bytes, hipStream_t s) {
  hipLaunchKernelGGL(carve_kernel, dim3(1), dim3(CARVE_THREADS), lds_bytes, s, d_args, flags, start_ci);
  return hipGetLastError();
}


// the merge pass through the streaming carve: columns + bitmaps + status of a supplied list, one launch
void launch_merge_place(const CarveArgs* d_args, uint32_t n_order, uint32_t n_groups0, uint32_t n_members0, uint32_t steps0,
                        hipStream_t s) {
  const uint32_t blocks = ((n_order ? n_order : 1u) + 255u) / 256u;
  hipLaunchKernelGGL(merge_place_kernel, dim3(blocks), dim3(256), 0, s, d_args, n_groups0, n_members0, steps0);
}

// delta sync of per-worker columns (pm_engine.cpp push_groups / sync_flags): a few thousand entries of a column of a
// hundred thousand, instead of the column
__global__ __launch_bounds__(256) void scatter_const_kernel(uint32_t* __restrict__ dst, const uint32_t* __restrict__ idx, uint32_t n,
                                                            uint32_t v) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k < n) dst[idx[k]] = v;
}
__global__ __launch_bounds__(256) void scatter_pairs_kernel(uint32_t* __restrict__ dst, const uint32_t* __restrict__ pairs, uint32_t n) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k < n) dst[pairs[2u * k]] = pairs[2u * k + 1u];
}
void launch_scatter_const(uint32_t* dst, const uint32_t* idx, uint32_t n, uint32_t v, hipStream_t s) {
  if (n) hipLaunchKernelGGL(scatter_const_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, dst, idx, n, v);
}
void launch_scatter_pairs(uint32_t* dst, const uint32_t* pairs, uint32_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL(scatter_pairs_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, dst, pairs, n);
}
