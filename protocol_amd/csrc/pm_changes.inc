// pm_changes.inc — the assignment change feed's kernels (included by pm_kernels.hip inside namespace pm):
// pm_enable_assignment_changes / pm_drain_assignment_changes of include/pm_engine.h, with their launchers.  They read the
// table a publish committed and the groups' committed task words, and write the feed's own three buffers and the drain's list.
//
// A worker's remembered identity is a ChangeIdent (pm_device.h): group id, GROUP_INDEX, GROUP_SIZE (mod.rs:424-434), and the
// COMPLEMENTS of next_worker and of the task handle — so a row of zeroes is "in no group" (0, 0, 0, PM_NONE, PM_NONE), which
// is what a buffer that has just grown holds for its new rows.
//
// assign_diff_kernel, once per publish: one thread per row, 256 a workgroup; a wave (64 lanes on gfx950) covers the rows
// [64 j, 64 j + 64) — exactly word j of the pending bitmap, and no other wave touches that word: the ballot of "changed" is
// OR-ed in by one lane with a plain read-modify-write.  The `what` byte and the identity of a row belong to the row's thread.
//
// The drain's list, two launches behind one another: change_scan_kernel (ONE workgroup of 256 threads, PM_CHG_SCAN_WORDS = 4
// words a thread, so 1024 words a pass) turns the bitmap's popcounts into an exclusive prefix per word and the total (to
// pinned host memory); change_expand_kernel (a wave per word, a lane per bit) writes pm_change_row{w, what[w]}
// at prefix[word] + the number of set bits below the lane's — ascending worker order by construction.

// rows [0, W): the three PM_CHG_* bits of this publish against the remembered identities (all three where `resync`)
__global__ __launch_bounds__(256) void assign_diff_kernel(ChangeDiffArgs a) {
  static_assert(sizeof(pm_assignment) == 32 && sizeof(ChangeIdent) == 32, "a row and an identity are two 16-byte pieces each");
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;
  const bool in = w < a.W;
  uint32_t bits = 0u;
  if (in) {
    const uint4* const row = reinterpret_cast<const uint4*>(a.table + w);
    const uint4 r0 = row[0];  // task position, group_slot, group_index, group_size
    const uint4 r1 = row[1];  // next_worker, (padding), group_id
    uint4* const mem = reinterpret_cast<uint4*>(a.ident + w);
    const uint4 m0 = mem[0], m1 = mem[1];
    // the task itself, not its position: the handle in the task word the claim completed (slots the device has no group for
    // read as "no task": never an index past the array)
    const uint32_t task = r0.y < a.G ? a.g_task[r0.y] : PM_NONE;
    const uint4 n0 = make_uint4(r1.z, r1.w, r0.z, r0.w);
    const uint4 n1 = make_uint4(~r1.x, ~task, 0u, 0u);
    if (n0.x != m0.x || n0.y != m0.y) bits |= PM_CHG_GROUP;
    if (n0.z != m0.z || n0.w != m0.w || n1.x != m1.x) bits |= PM_CHG_RING;
    if (n1.y != m1.y) bits |= PM_CHG_TASK;
    if (a.resync) bits = PM_CHG_GROUP | PM_CHG_RING | PM_CHG_TASK;
    if (bits) {
      a.what[w] = (uint8_t)(a.what[w] | bits);
      mem[0] = n0, mem[1] = n1;
    }
  }
  const uint64_t changed = __ballot(bits != 0u);  // (every lane of the wave gets here; lanes at or above W vote 0)
  if ((threadIdx.x & 63u) == 0u && changed) a.bitmap[w >> 6] |= changed;  // (lane 0: w < W wherever a bit is set)
}

// prefix[j] = set bits in words [0, j) of the bitmap, j < n_words; *total_host (pinned host memory) = all of them
__global__ __launch_bounds__(256) void change_scan_kernel(const uint64_t* __restrict__ bitmap, uint32_t n_words,
                                                          uint32_t* __restrict__ prefix, uint32_t* __restrict__ total_host) {
  __shared__ uint32_t s_wave[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t acc = 0u;
  for (uint32_t base = 0u; base < n_words; base += 256u * PM_CHG_SCAN_WORDS) {  // (uniform: n_words <= 2^18 + 1)
    const uint32_t j0 = base + tid * PM_CHG_SCAN_WORDS;
    uint32_t c[PM_CHG_SCAN_WORDS], sum = 0u;
#pragma unroll
    for (uint32_t k = 0; k < PM_CHG_SCAN_WORDS; ++k) {
      c[k] = j0 + k < n_words ? (uint32_t)__popcll(bitmap[j0 + k]) : 0u;
      sum += c[k];
    }
    const uint32_t incl = wave_incl_scan_u32(sum);
    if (lane == 63u) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0u, tile = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      const uint32_t v = s_wave[k];
      before += k < wave ? v : 0u;
      tile += v;
    }
    uint32_t at = acc + before + incl - sum;
#pragma unroll
    for (uint32_t k = 0; k < PM_CHG_SCAN_WORDS; ++k) {
      if (j0 + k < n_words) prefix[j0 + k] = at;
      at += c[k];
    }
    acc += tile;
    __syncthreads();  // (s_wave is rewritten by the next pass)
  }
  if (tid == 0u) *total_host = acc;
}

// out[prefix[j] + rank of bit b in word j] = {64 j + b, what[64 j + b]} for every set bit
__global__ __launch_bounds__(256) void change_expand_kernel(const uint64_t* __restrict__ bitmap, uint32_t n_words,
                                                            const uint32_t* __restrict__ prefix,
                                                            const uint8_t* __restrict__ what, pm_change_row* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t j = blockIdx.x * 4u + (threadIdx.x >> 6);  // (wave-uniform)
  if (j >= n_words) return;
  const uint64_t word = bitmap[j];
  if (!((word >> lane) & 1ull)) return;
  const uint32_t w = j * 64u + lane;  // (< W: the diff sets no bit at or above W)
  const uint32_t at = prefix[j] + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));
  out[at] = pm_change_row{w, what[w]};
}

void launch_assign_diff(const ChangeDiffArgs& a, hipStream_t s) {
  if (!a.W) return;
  hipLaunchKernelGGL(assign_diff_kernel, dim3((a.W + 255u) / 256u), dim3(256), 0, s, a);
}

// the pending rows of the bitmap's first n_words words -> out (room for every set bit), ascending; their number ->
// *total_host (pinned); prefix: n_words words of scratch
void launch_change_list(const uint64_t* bitmap, uint32_t n_words, const uint8_t* what, uint32_t* prefix, uint32_t* total_host,
                        pm_change_row* out, hipStream_t s) {
  hipLaunchKernelGGL(change_scan_kernel, dim3(1), dim3(256), 0, s, bitmap, n_words, prefix, total_host);
  if (n_words) hipLaunchKernelGGL(change_expand_kernel, dim3((n_words + 3u) / 4u), dim3(256), 0, s, bitmap, n_words, prefix, what, out);
}
