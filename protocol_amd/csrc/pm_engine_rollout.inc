// pm_engine_rollout.inc — part of pm_engine.cpp (one translation unit; included in place): the rollout ledger: its columns, their
// growth, the preparation the four reads share (namespace pm) — and, behind them (extern "C"), C ABI: pm_rollout_enable /
// _ingest / _get / _summary / _tasks / _groups / _workers (kernels in pm_rollout.inc).  Included at file scope.
//
// The ledger is two columns over the workers [0, ro.W): the reported task id and the reported state (PM_TS_NONE: no report).
// pm_upload_workers(keep_groups = 0) sets ro.reinit, the one hook in the upload path; everything else happens when the next
// rollout call runs rollout_prepare.  Everything is queued on the engine's stream.  Like the reports, a rollout call leaves
// the tick's state alone: no pending delta is consumed, nothing is compacted, no cache flag is cleared.
namespace pm {

// a fresh ledger: every buffer goes back; whether it is on stays
static void rollout_release(pm_engine* e) {
  Rollout fresh;
  fresh.on = e->ro.on;
  e->ro = std::move(fresh);
}

// the columns cover the workers [0, W): creates them, fills appended rows empty, empties every row behind an upload that
// dropped the row identities (queued, not waited for)
static int32_t rollout_prepare(pm_engine* e) {
  const uint32_t W = e->W;
  if (!e->ro.h_pin.p) HIPCHK(e->ro.h_pin.ensure(1 + PM_RO_CENSUS, 1 + PM_RO_CENSUS));
  uint32_t keep = e->ro.W;
  if (e->ro.reinit || W < keep) keep = 0;  // (a shorter table is a new table)
  if (W > keep || e->ro.reinit) {
    HIPCHK(e->ro.uid.grow_keep(W ? W : 1, keep, e->stream));
    HIPCHK(e->ro.state.grow_keep(W ? W : 1, keep, e->stream));
    HIPCHK(e->ro.last.grow_keep(W ? W : 1, keep, e->stream));
    launch_ro_fill(e->ro.uid.p, e->ro.state.p, e->ro.last.p, keep, W, e->stream);
    HIPCHK(hipGetLastError());
  }
  e->ro.W = W;
  e->ro.reinit = false;
  return PM_OK;
}

// what every rollout call but pm_rollout_enable asks first
static int32_t rollout_guard(pm_engine* e) {
  if (!e->ro.on) return set_error(PM_ESTATE, "the rollout ledger is off");
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  if (e->dist_world > 1) return set_error(PM_ESTATE, "the rollout ledger does not cover multi-GPU engines");
  if (!e->have_workers) return set_error(PM_ESTATE, "workers must be uploaded first");
  return PM_OK;
}

// One record per entry of the host's list, tombstones included, for the reads that join the groups on the device (the rollout
// reads, pm_directory, pm_group_directory): id, configuration, size, the slot pm_get_groups would number it (tombstones are
// skipped; PM_NONE: dissolved) and the claimed task's position in the current list.  RoGroup also takes the claimed task's id.
// of_slot (optional): reported slot -> list entry.  Returns the live entries that hold a task.
static inline void group_record_uid(RoGroup& o, uint64_t uid) { o.uid = uid; }
static inline void group_record_uid(DirGroup&, uint64_t) {}
template <class Rec>
static uint32_t group_records(pm_engine* e, std::vector<Rec>& out, std::vector<uint32_t>* of_slot = nullptr) {
  const uint32_t G = uint32_t(e->groups.size());
  out.resize(G);
  if (of_slot) of_slot->clear();
  uint32_t live = 0, held = 0;
  for (uint32_t k = 0; k < G; ++k) {
    const Group& gr = e->groups[k];
    Rec& o = out[k];
    o.id = gr.id;
    o.cfg = gr.cfg;
    o.size = uint32_t(gr.members.size());
    o.slot = gr.dead ? PM_NONE : live++;  // (tombstones are skipped, as pm_get_groups numbers the list)
    o.task = gr.dead ? PM_NONE : task_position(e, gr.task);
    group_record_uid(o, o.task == PM_NONE || !e->tasks_have_uid ? 0ull : e->h_tuid[gr.task]);
    held += o.task != PM_NONE;
    if (of_slot && !gr.dead) of_slot->push_back(k);
  }
  return held;
}

// What the four reads share: the host's groups go up (the join's other side, as pm_metrics_rows takes it), the workers are
// classified, the groups' counters and the census are made; with `tasks`, the ids are sorted and ro.task_rows holds the
// per-task table, *n_tasks its rows.  On return the stream is idle, h_pin[1..] holds the census, `a` names the buffers.
static int32_t rollout_read(pm_engine* e, bool tasks, RoPrepArgs* a, uint32_t* n_listed, uint32_t* n_tasks) {
  int32_t rc = rollout_guard(e);
  if (rc) return rc;
  if (e->have_tasks && !e->tasks_have_uid && e->T)
    return set_error(PM_ESTATE, "the task table carries no ids (pm_task_soa.uid)");
  HIPCHK(hipSetDevice(e->cfg.device));
  ABSORB_PENDING(e);  // (the groups of a tick that has not been taken in yet: pm_get_groups would report them)
  if ((rc = rollout_prepare(e))) return rc;
  Rollout& ro = e->ro;
  const uint32_t W = e->W, G = uint32_t(e->groups.size());
  const uint32_t listed = group_records(e, ro.h_g);
  if ((rc = upload(ro.gof, e->h_group_of.data(), size_t(W), e->stream))) return rc;
  if ((rc = upload(ro.g, ro.h_g.data(), size_t(G), e->stream))) return rc;
  const size_t n_cnt = size_t(G) * PM_RO_GCNT + PM_RO_CENSUS, n_flag = size_t(W) + G;
  HIPCHK(ro.cls.ensure(W ? W : 1));
  HIPCHK(ro.cnt.ensure(n_cnt));
  HIPCHK(ro.flag.ensure(n_flag ? n_flag : 1));
  HIPCHK(ro.off.ensure(n_flag + 1));
  HIPCHK(hipMemsetAsync(ro.cnt.p, 0, n_cnt * sizeof(uint32_t), e->stream));
  *a = RoPrepArgs{};
  a->W = W, a->G = G;
  a->group_of = ro.gof.p;
  a->g = ro.g.p;
  a->uid = ro.uid.p;
  a->state = ro.state.p;
  a->cls = ro.cls.p;
  a->g_cnt = ro.cnt.p;
  a->census = ro.cnt.p + size_t(G) * PM_RO_GCNT;
  a->flag = ro.flag.p;
  launch_ro_classify(*a, e->stream);
  launch_mx_scan(ro.flag.p, uint32_t(n_flag), ro.off.p, ro.h_pin.p, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));
  const uint32_t N = ro.h_pin.p[0];  // reporting rows + listed groups
  if (N > n_flag) return set_error(PM_ESTATE, "rollout: more keys than rows and groups");
  HIPCHK(ro.sort.ensure_first(N));
  a->off = ro.off.p;
  a->key = ro.sort.key[0].p;
  a->val = ro.sort.val[0].p;
  launch_ro_emit(*a, e->stream);  // (also without `tasks`: it counts the converged groups)
  uint32_t D = 0;
  if (tasks && N) {
    HIPCHK(ro.sort.ensure(N));
    HIPCHK(ro.head.ensure(N));
    HIPCHK(ro.head_off.ensure(size_t(N) + 1));
    const uint32_t cur = ro.sort.sort(N, 8u, 0u, e->stream);  // every byte of the id
    launch_ro_heads(ro.sort.key[cur].p, N, ro.head.p, e->stream);
    launch_mx_scan(ro.head.p, N, ro.head_off.p, ro.h_pin.p, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    D = ro.h_pin.p[0];
    if (D > N) return set_error(PM_ESTATE, "rollout: more runs than keys");
    HIPCHK(ro.start.ensure(D ? D : 1));
    HIPCHK(ro.task_rows.ensure(D ? D : 1));
    launch_ro_starts(ro.head.p, ro.head_off.p, N, ro.start.p, e->stream);
    launch_ro_reduce(ro.sort.key[cur].p, ro.sort.val[cur].p, N, ro.start.p, D, ro.g.p, ro.cnt.p, ro.task_rows.p, e->stream);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(ro.h_pin.p + 1, a->census, PM_RO_CENSUS * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  *n_listed = listed;
  if (n_tasks) *n_tasks = D;
  return PM_OK;
}

}  // namespace pm

extern "C" {

int32_t pm_rollout_enable(pm_engine* e, uint32_t on) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  if (on && e->dist_world > 1) return set_error(PM_ESTATE, "the rollout ledger does not cover multi-GPU engines");
  HIPCHK(hipSetDevice(e->cfg.device));
  HIPCHK(hipStreamSynchronize(e->stream));
  rollout_release(e);
  e->ro.on = on != 0;
  if (!e->ro.on) return PM_OK;
  int32_t rc = rollout_prepare(e);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(e->stream));
  return PM_OK;
}

int32_t pm_rollout_ingest(pm_engine* e, const pm_ro_report* reports, uint32_t n) {
  if (!e || (n && !reports)) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = rollout_guard(e);
  if (rc) return rc;
  if (n > 0x7FFFFFFFu) return set_error(PM_ERANGE, "too many reports in one call");
  for (uint32_t i = 0; i < n; ++i) {
    if (reports[i].state >= PM_TS_N && reports[i].state != PM_TS_NONE) return set_error(PM_EINVAL, "not a task state");
    if (reports[i].worker >= e->W) return set_error(PM_ERANGE, "worker index out of range");
  }
  HIPCHK(hipSetDevice(e->cfg.device));
  if ((rc = rollout_prepare(e))) return rc;
  if (!n) return PM_OK;
  HIPCHK(e->ro.reports.ensure(n));
  HIPCHK(hipMemcpyAsync(e->ro.reports.p, reports, size_t(n) * sizeof(pm_ro_report), hipMemcpyHostToDevice, e->stream));
  launch_ro_ingest(e->ro.reports.p, n, e->ro.last.p, e->ro.uid.p, e->ro.state.p, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));  // pageable source
  return PM_OK;
}

int32_t pm_rollout_get(pm_engine* e, const uint32_t* idx, uint32_t n, uint64_t* uid, uint8_t* state) {
  if (!e || (n && !idx)) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = rollout_guard(e);
  if (rc) return rc;
  for (uint32_t k = 0; k < n; ++k)
    if (idx[k] >= e->W) return set_error(PM_ERANGE, "worker index out of range");
  HIPCHK(hipSetDevice(e->cfg.device));
  if ((rc = rollout_prepare(e))) return rc;
  if (!n) return PM_OK;
  HIPCHK(e->ro.idx.ensure(n));
  HIPCHK(e->ro.get_uid.ensure(n));
  HIPCHK(e->ro.get_state.ensure(n));
  HIPCHK(hipMemcpyAsync(e->ro.idx.p, idx, size_t(n) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  launch_ro_get(e->ro.idx.p, n, e->ro.uid.p, e->ro.state.p, e->ro.get_uid.p, e->ro.get_state.p, e->stream);
  HIPCHK(hipGetLastError());
  if (uid) HIPCHK(hipMemcpyAsync(uid, e->ro.get_uid.p, size_t(n) * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
  if (state) HIPCHK(hipMemcpyAsync(state, e->ro.get_state.p, size_t(n), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return PM_OK;
}

int32_t pm_rollout_summary(pm_engine* e, pm_ro_summary* out) {
  if (!e || !out) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  RoPrepArgs a;
  uint32_t listed = 0, D = 0;
  int32_t rc = rollout_read(e, true, &a, &listed, &D);
  if (rc) return rc;
  const uint32_t* c = e->ro.h_pin.p + 1;
  std::copy(c, c + PM_RO_N, out->by_class);
  std::copy(c + PM_RO_N, c + PM_RO_N + PM_TS_N + 1, out->by_state);
  out->groups_with_task = listed;
  out->groups_converged = c[PM_RO_CENSUS - 1];
  out->distinct_uids = D;
  return PM_OK;
}

int32_t pm_rollout_tasks(pm_engine* e, pm_ro_task_row* rows, uint32_t cap, uint32_t* n) {
  if (!e || !n) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  RoPrepArgs a;
  uint32_t listed = 0, D = 0;
  int32_t rc = rollout_read(e, true, &a, &listed, &D);
  if (rc) return rc;
  *n = D;
  if (D && (!rows || cap < D)) return set_error(PM_ERANGE, "rollout task buffer too small");
  if (!D) return PM_OK;
  HIPCHK(hipMemcpyAsync(rows, e->ro.task_rows.p, size_t(D) * sizeof(pm_ro_task_row), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  // the id's position in the current list: the D listed rows through the id map, never the W inputs
  if (e->have_tasks && e->tasks_have_uid && e->T) {
    ensure_uid_map(e);
    for (uint32_t d = 0; d < D; ++d) {
      if (rows[d].uid == ~0ull) continue;  // (an id of all ones names no task)
      const auto it = e->uid_to_u.find(rows[d].uid);
      if (it != e->uid_to_u.end()) rows[d].task = task_position(e, it->second);
    }
  }
  return PM_OK;
}

int32_t pm_rollout_groups(pm_engine* e, pm_ro_group_row* rows, uint32_t cap, uint32_t* n) {
  if (!e || !n) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  RoPrepArgs a;
  uint32_t listed = 0;
  int32_t rc = rollout_read(e, false, &a, &listed, nullptr);
  if (rc) return rc;
  *n = listed;
  if (listed && (!rows || cap < listed)) return set_error(PM_ERANGE, "rollout group buffer too small");
  if (!listed) return PM_OK;
  // the listed entries keep their order: the flags behind the workers' were scanned with them, their offsets start at the
  // number of reporting rows — scanned again on their own
  Rollout& ro = e->ro;
  HIPCHK(ro.group_rows.ensure(listed));
  HIPCHK(ro.head_off.ensure(size_t(a.G) + 1));
  launch_mx_scan(ro.flag.p + a.W, a.G, ro.head_off.p, nullptr, e->stream);
  launch_ro_group_rows(ro.g.p, a.G, ro.flag.p + a.W, ro.head_off.p, ro.cnt.p, ro.group_rows.p, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(rows, ro.group_rows.p, size_t(listed) * sizeof(pm_ro_group_row), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return PM_OK;
}

int32_t pm_rollout_workers(pm_engine* e, uint32_t class_mask, pm_ro_worker_row* rows, uint32_t cap, uint32_t* n) {
  if (!e || !n) return set_error(PM_EINVAL, "null argument");
  if (!class_mask || (class_mask >> PM_RO_N)) return set_error(PM_EINVAL, "not a set of rollout classes");
  std::lock_guard<std::mutex> lk(e->mu);
  RoPrepArgs a;
  uint32_t listed = 0;
  int32_t rc = rollout_read(e, false, &a, &listed, nullptr);
  if (rc) return rc;
  Rollout& ro = e->ro;
  *n = 0;
  if (!a.W) return PM_OK;
  launch_ro_worker_flags(ro.cls.p, a.W, class_mask, ro.flag.p, e->stream);  // (the preparation's flags have done their work)
  launch_mx_scan(ro.flag.p, a.W, ro.off.p, ro.h_pin.p, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));
  const uint32_t total = ro.h_pin.p[0];
  *n = total;
  if (total > a.W) return set_error(PM_ESTATE, "rollout: more listed workers than workers");
  if (total && (!rows || cap < total)) return set_error(PM_ERANGE, "rollout worker buffer too small");
  if (!total) return PM_OK;
  HIPCHK(ro.worker_rows.ensure(total));
  launch_ro_worker_rows(a, ro.flag.p, ro.off.p, ro.worker_rows.p, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(rows, ro.worker_rows.p, size_t(total) * sizeof(pm_ro_worker_row), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return PM_OK;
}

}  // extern "C"
