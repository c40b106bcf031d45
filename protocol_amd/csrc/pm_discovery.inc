// pm_discovery.inc — the discovery sync's kernels (included by pm_kernels.hip inside namespace pm): pm_discovery_sync of
// include/pm_engine.h, with their launcher.  DiscoveryMonitor::get_nodes -> sync_single_node_with_discovery
// (orchestrator/src/discovery/monitor.rs:218-435) for a whole discovery list at once.  They read and write the liveness ledger's
// status byte; nothing of the tick reads it.
//
// The reference is sequential: row j counts the Healthy nodes on its endpoint in the store as the rows before it left it.  What
// makes it parallel: a node's status is written only in its own step, no step makes a node Healthy, and a Healthy snapshot never
// takes step 1 — so what a Healthy node does is a function of its own row alone (disc_rule with any count).  Row j's count for
// endpoint k is then
//     S[k]                                                         unlisted Healthy table rows on k
//   + #{BEFORE events (p, k): p > j}                               listed Healthy rows whose step is still to come
//   + #{AFTER events (p, k): p < j}                                listed rows still Healthy, on k, after their own step
// and the strict inequalities leave the node itself out (monitor.rs:228).  Events live in one array, a disjoint segment per
// endpoint; a segment's order is whatever the scatter's atomics made it, and nothing reads more of it than the two counts.
//
// Five launches on one stream, 256 threads a workgroup: mark (a thread per discovery row), count (per table row), segments (per
// endpoint: one atomicAdd on a cursor per non-empty endpoint), scatter (per table row, the same events again), decide (per
// discovery row).  A decide thread walks a segment of up to DISC_WALK_ALONE events by itself; a longer one the row's wave walks
// together, 64 events a step, one such row after the other.

#define DISC_WALK_ALONE 64u

// one row's pass through monitor.rs:252-396; upd_old / upd_new are packed a byte per update, unused bytes PM_NS_N
struct DiscStep {
  uint32_t status, n_upd, ops, upd_old, upd_new;
};

__device__ __forceinline__ void disc_update(DiscStep& d, uint32_t to) {  // :65-88
  const uint32_t sh = 8u * d.n_upd;
  d.upd_old = (d.upd_old & ~(0xFFu << sh)) | (d.status << sh);
  d.upd_new = (d.upd_new & ~(0xFFu << sh)) | (to << sh);
  d.status = to;
  d.ops |= PM_DO_STAMP_NOW;
  ++d.n_upd;
}

// add_node(existing_node.clone() with one field changed): the snapshot's status and stamp are back (node_store.rs:27-60)
__device__ __forceinline__ void disc_put_back(DiscStep& d, uint32_t s, uint32_t op) {
  d.status = s;
  d.ops = (d.ops & ~uint32_t(PM_DO_STAMP_NOW)) | op;
}

// THE row rule: s = the snapshot's status, cnt = the Healthy others on the discovery row's endpoint, ip_differs = :336
__device__ __forceinline__ DiscStep disc_rule(uint32_t s, uint32_t cnt, const pm_disc_row& r, bool ip_differs, uint64_t now_ms) {
  const uint32_t none = (uint32_t)PM_NS_N * 0x010101u;
  DiscStep d{s, 0u, 0u, none, none};
  const bool validated = r.flags & PM_DF_VALIDATED, white = r.flags & PM_DF_WHITELISTED, active = r.flags & PM_DF_ACTIVE;
  if (cnt > 0u && s != PM_NS_HEALTHY) {  // :254-268
    disc_update(d, PM_NS_DEAD);
    return d;
  }
  if (validated && !white) disc_update(d, PM_NS_EJECTED);                      // :270-280
  if (validated && white && s == PM_NS_EJECTED) disc_update(d, PM_NS_DEAD);    // :284-297
  if (!active && s == PM_NS_HEALTHY) {                                          // :298-334
    // now.signed_duration_since(stamp) > 5 min: a stamp at or after now never marks
    const bool mark = r.last_change_ms == 0ull || (now_ms > r.last_change_ms && now_ms - r.last_change_ms > (uint64_t)PM_DISC_GRACE_MS);
    if (mark) disc_update(d, white ? PM_NS_DEAD : PM_NS_EJECTED);
  }
  if (ip_differs) disc_put_back(d, s, PM_DO_IP_REWRITE);                        // :336-344
  if (r.flags & PM_DF_LOCATION_NEW) d.ops |= PM_DO_LOCATION;                    // :345-357
  if (s == PM_NS_DEAD && r.last_change_ms != 0ull && r.last_updated_ms != 0ull && r.last_change_ms < r.last_updated_ms) {  // :359-383
    if (r.flags & PM_DF_SPECS_DIFFER) disc_put_back(d, s, PM_DO_SPECS_REWRITE);
    disc_update(d, PM_NS_DISCOVERED);
  }
  if (r.flags & PM_DF_BALANCE_ZERO) disc_update(d, PM_NS_LOWBALANCE);           // :385-395
  return d;
}

// the endpoint a listed row holds after its step
__device__ __forceinline__ uint32_t disc_endpoint_after(const DiscStep& d, const pm_disc_row& r, uint32_t table_ep) {
  return (d.ops & PM_DO_IP_REWRITE) && !(d.ops & PM_DO_SPECS_REWRITE) ? r.endpoint_after : table_ep;
}

// what the Healthy table row w adds to the counts: true = it is listed, and then ep_before / ep_after are the endpoints of its
// two events (PM_EP_NONE = no such event) and pos its position; false = it is unlisted (one more in base[its endpoint])
__device__ __forceinline__ bool disc_events_of(const DiscArgs& a, uint32_t w, uint32_t& pos, uint32_t& ep_before, uint32_t& ep_after) {
  ep_before = a.row_endpoint[w];
  ep_after = PM_EP_NONE;
  pos = a.pos_of_row[w];
  if (pos == PM_DISC_NEW) return false;
  const pm_disc_row r = a.rows[pos];
  const DiscStep d = disc_rule(PM_NS_HEALTHY, 0u, r, r.endpoint_after != ep_before, a.now_ms);  // (the pure case: cnt is not read)
  if (d.status == PM_NS_HEALTHY) ep_after = disc_endpoint_after(d, r, ep_before);
  return true;
}

// 1. pos_of_row[row] = j (the host has checked: every row below W or PM_DISC_NEW, no table row twice)
__global__ __launch_bounds__(256) void discovery_mark_kernel(DiscArgs a) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= a.D) return;
  const uint32_t row = a.rows[j].row;
  if (row != PM_DISC_NEW) a.pos_of_row[row] = j;
}

// 2. the Healthy table rows: the unlisted ones into base, the listed ones' events counted per endpoint
__global__ __launch_bounds__(256) void discovery_count_kernel(DiscArgs a) {
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;
  if (w >= a.W || a.status[w] != PM_NS_HEALTHY) return;
  uint32_t pos, eb, ea;
  if (!disc_events_of(a, w, pos, eb, ea)) {
    if (eb != PM_EP_NONE) atomicAdd(&a.base[eb], 1u);
    return;
  }
  if (eb != PM_EP_NONE) atomicAdd(&a.ev_cnt[eb], 1u);
  if (ea != PM_EP_NONE) atomicAdd(&a.ev_cnt[ea], 1u);
}

// 3a. every endpoint with events gets ev_cnt[k] consecutive slots (which ones depends on the arrival order: no result does)
__global__ __launch_bounds__(256) void discovery_segment_kernel(DiscArgs a) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= a.E) return;
  const uint32_t n = a.ev_cnt[k];
  if (n) a.ev_off[k] = atomicAdd(a.cursor, n);
}

// 3b. the same events again, now into their segments
__global__ __launch_bounds__(256) void discovery_scatter_kernel(DiscArgs a) {
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;
  if (w >= a.W || a.status[w] != PM_NS_HEALTHY) return;
  uint32_t pos, eb, ea;
  if (!disc_events_of(a, w, pos, eb, ea)) return;
  // (a slot: below ev_off[k] + ev_cnt[k], because the count kernel counted exactly these events)
  if (eb != PM_EP_NONE) a.events[a.ev_off[eb] + atomicAdd(&a.ev_fill[eb], 1u)] = (uint64_t)pos << 1;
  if (ea != PM_EP_NONE) a.events[a.ev_off[ea] + atomicAdd(&a.ev_fill[ea], 1u)] = ((uint64_t)pos << 1) | 1ull;
}

// a BEFORE event counts for the queries in front of it, an AFTER event for the ones behind it
__device__ __forceinline__ uint32_t disc_event_counts(uint64_t ev, uint32_t j) {
  const uint64_t p = ev >> 1;
  return (ev & 1ull) ? (p < (uint64_t)j ? 1u : 0u) : (p > (uint64_t)j ? 1u : 0u);
}

// 4. cnt, then the row rule or the admission test; the result row and the ledger byte
__global__ __launch_bounds__(256) void discovery_decide_kernel(DiscArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  const bool in = j < a.D;
  pm_disc_row r{};
  uint32_t cnt = 0u, n = 0u, off = 0u;
  if (in) {
    r = a.rows[j];
    cnt = a.base[r.endpoint];
    n = a.ev_cnt[r.endpoint];
    if (n) off = a.ev_off[r.endpoint];
    if (n <= DISC_WALK_ALONE)
      for (uint32_t i = 0; i < n; ++i) cnt += disc_event_counts(a.events[off + i], j);
  }
  // the long segments, one row of the wave after the other, every lane walking (every lane of every wave gets here)
  uint64_t todo = __ballot(in && n > DISC_WALK_ALONE);
  while (todo) {
    const int l = __ffsll((unsigned long long)todo) - 1;
    todo &= todo - 1ull;
    const uint32_t n_l = __shfl(n, l), off_l = __shfl(off, l), j_l = __shfl(j, l);
    uint32_t part = 0u;
    for (uint32_t i = lane; i < n_l; i += 64u) part += disc_event_counts(a.events[off_l + i], j_l);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) part += __shfl_xor(part, d);
    if ((int)lane == l) cnt += part;
  }
  if (!in) return;
  uint32_t w1, w2, w3;
  if (r.row == PM_DISC_NEW) {  // :397-413
    const uint32_t admit = cnt >= a.max_same ? 0u : 1u;
    const uint32_t none = (uint32_t)PM_NS_N;
    w1 = none | ((admit ? (uint32_t)PM_NS_DISCOVERED : none) << 8) | ((admit ? (uint32_t)PM_DO_ADMIT : (uint32_t)PM_DO_SKIP) << 24);
    w2 = none * 0x01010101u;
    w3 = none * 0x0101u;
  } else {
    const uint32_t s = a.status[r.row];
    const DiscStep d = disc_rule(s, cnt, r, r.endpoint_after != a.row_endpoint[r.row], a.now_ms);
    if (d.status != s) a.status[r.row] = (uint8_t)d.status;
    w1 = s | (d.status << 8) | (d.n_upd << 16) | (d.ops << 24);
    w2 = d.upd_old | (d.upd_new << 24);
    w3 = d.upd_new >> 8;
  }
  reinterpret_cast<uint4*>(a.out)[j] = make_uint4(cnt, w1, w2, w3);
}

void launch_discovery_sync(const DiscArgs& a, hipStream_t s) {
  if (!a.D) return;
  hipLaunchKernelGGL(discovery_mark_kernel, dim3((a.D + 255u) / 256u), dim3(256), 0, s, a);
  if (a.W) hipLaunchKernelGGL(discovery_count_kernel, dim3((a.W + 255u) / 256u), dim3(256), 0, s, a);
  if (a.E) hipLaunchKernelGGL(discovery_segment_kernel, dim3((a.E + 255u) / 256u), dim3(256), 0, s, a);
  if (a.W) hipLaunchKernelGGL(discovery_scatter_kernel, dim3((a.W + 255u) / 256u), dim3(256), 0, s, a);
  hipLaunchKernelGGL(discovery_decide_kernel, dim3((a.D + 255u) / 256u), dim3(256), 0, s, a);
}
