// pm_engine.cpp — host side of libpm_engine.so: owns the HBM-resident SoA tables, drives the kernels of
// pm_kernels.hip on one HIP stream and implements the C ABI of include/pm_engine.h.
//
// Reference behaviour mirrored here (paths relative to /root/reference/crates/orchestrator/src):
//   plugins/node_groups/mod.rs:113-175   constructor checks + config sort      -> pm_set_configs
//   plugins/node_groups/mod.rs:478-628   try_form_new_groups                   -> pm_form_groups
//   plugins/node_groups/mod.rs:631-971   try_merge_solo_groups                 -> pm_merge_solo_groups
//   plugins/node_groups/mod.rs:1423-1487 dissolve_group                        -> pm_dissolve_group
//   plugins/node_groups/scheduler_impl.rs:11-110  filter_tasks (all workers)   -> pm_match
//   plugins/node_groups/status_update_impl.rs:8-39 handle_status_change        -> pm_on_worker_status
//   plugins/newest_task/mod.rs:8-19                                            -> pm_newest_task
//   scheduler/mod.rs:26-36               get_task_for_node                     -> pm_lookup_task_for_worker
// There is no CPU fallback: without a gfx950 device pm_engine_create fails with PM_ENODEV.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "pm_device.h"
#include "pm_engine.h"
#include "pm_internal.h"
#include "pm_members.h"
#include "pm_owned.h"

namespace pm {

static thread_local std::string g_last_error;

int32_t set_error(int32_t code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

#define HIPCHK(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess)                                                                              \
      return set_error(PM_ENODEV, std::string(#expr) + ": " + hipGetErrorString(e_));                  \
  } while (0)

#include "pm_engine_types.inc"
}  // namespace pm

using namespace pm;

namespace pm {
struct FormRun;
}

#include "pm_engine_state.inc"

namespace pm {
static int32_t changes_publish(pm_engine* e);  // pm_engine_changes.inc; publish_end (pm_engine_match.inc) calls it

#include "pm_engine_groups.inc"
#include "pm_engine_carve.inc"
#include "pm_engine_match.inc"
#include "pm_engine_merge.inc"
}  // namespace pm

// ================================================================================================
// C ABI

extern "C" {

const char* pm_last_error(void) { return pm::g_last_error.c_str(); }

void pm_engine_config_default(pm_engine_config* c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->abi_version = PM_ABI_VERSION;
  c->device = 0;
  c->proximity_enabled = 1;
  c->switching_enabled = 1;
  c->prefer_larger_groups = 1;
  c->chooser = PM_CHOOSE_FIRST;
  c->group_id_seed = 1;
}

int32_t pm_engine_create(const pm_engine_config* cfg, pm_engine** out) {
  if (!cfg || !out) return set_error(PM_EINVAL, "null argument");
  if (cfg->abi_version != PM_ABI_VERSION) return set_error(PM_EINVAL, "ABI version mismatch");
  if (cfg->carve_variant != 0 && cfg->carve_variant != 1 && cfg->carve_variant != 3)
    return set_error(PM_EINVAL, "carve_variant: 0 (streaming carve), 1 (exact sweep only) or 3 (batch pipeline); 2 and 4 were removed");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
    return set_error(PM_ENODEV, "no HIP device visible: the matching engine needs an MI355X (gfx950); there is no CPU fallback");
  if (cfg->device < 0 || cfg->device >= n_dev) return set_error(PM_EINVAL, "device ordinal out of range");
  HIPCHK(hipSetDevice(cfg->device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, cfg->device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return set_error(PM_ENODEV, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
  HIPCHK(carve_kernels_init());  // (per device; idempotent)
  std::unique_ptr<pm_engine> e(new (std::nothrow) pm_engine());
  if (!e) return set_error(PM_ENOMEM, "out of host memory");
  e->cfg = *cfg;
  e->id_rng = cfg->group_id_seed;
  if (const char* v = getenv("PM_PRUNE_MODE")) {  // (experiments: see pm_debug_prune_mode)
    if (v[0] >= '0' && v[0] <= '3' && !v[1]) e->prune_mode = uint32_t(v[0] - '0');
  }
  if (const char* v = getenv("PM_WALK_CAP_DIV")) {
    const long f = atol(v);
    if (f > 0 && f < 1000) e->walk_cap_div = uint32_t(f);
  }
  if (const char* v = getenv("PM_PRUNE_FACTOR")) {
    const long f = atol(v);
    if (f > 0 && f < (1l << 30)) e->prune_factor = uint32_t(f);
  }
  if (const char* v = getenv("PM_STREAM_WGS")) {
    const long f = atol(v);
    if (f > 0 && f < 4096) e->stream_wgs_env = uint32_t(f);
  }
  if (const char* v = getenv("PM_STREAM_ROW_SPINS")) {  // (tests: a validator that hardly waits for its rows)
    const long f = atol(v);
    if (f > 0 && f < (1l << 24)) e->stream_row_spins_env = uint32_t(f);
  }
  if (const char* v = getenv("PM_STREAM_LA_DIV")) {
    const long f = atol(v);
    if (f > 0 && f < 4096) e->stream_la_div_env = uint32_t(f);
  }
  if (const char* v = getenv("PM_MERGE_STREAM_MIN")) {
    const long f = atol(v);
    if (f >= 2 && f <= (1l << 30)) e->merge_stream_min = uint32_t(f);
  }
  if (const char* v = getenv("PM_STREAM_LA")) {
    const long f = atol(v);
    if (f > 0 && f <= long(PM_STREAM_LA_MAX)) e->stream_la_env = uint32_t(f);
  }
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && cus > 0)
      e->n_cus = uint32_t(cus);
  }
  // (an engine owns ONE stream: K engines in a process take K of the HIP runtime's hardware queues)
  if (e->stream_owned.create(hipStreamNonBlocking) != hipSuccess) return set_error(PM_ENODEV, "hipStreamCreate failed");
  e->stream = e->stream_owned;
  for (auto& ev : e->ev)
    if (ev.create() != hipSuccess) return set_error(PM_ENODEV, "hipEventCreate failed");
  for (auto& ev : e->kev)
    if (ev.create() != hipSuccess) return set_error(PM_ENODEV, "hipEventCreate failed");
  if (e->ev_groups.create(hipEventDisableTiming) != hipSuccess) return set_error(PM_ENODEV, "hipEventCreate failed");
  *out = e.release();
  return PM_OK;
}

void pm_engine_destroy(pm_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->cfg.device);
  (void)hipStreamSynchronize(e->stream);
  delete e;  // (every member gives back what it holds: pm_engine_state.inc)
}

int32_t pm_set_configs(pm_engine* e, const pm_config_row* cfgs, uint32_t n_cfgs, const pm_gpu_alt_row* alts,
                       uint32_t n_alts) {
  if (!e || (n_cfgs && !cfgs) || (n_alts && !alts)) return set_error(PM_EINVAL, "null argument");
  if (n_cfgs > PM_MAX_CONFIGS) return set_error(PM_EINVAL, "more than PM_MAX_CONFIGS configurations");
  for (uint32_t i = 0; i < n_cfgs; ++i) {
    if (cfgs[i].max_group_size < cfgs[i].min_group_size)
      return set_error(PM_EINVAL, "Plugin configuration is invalid (max_group_size < min_group_size)");  // mod.rs:145
    if (cfgs[i].min_group_size == 0)
      return set_error(PM_EINVAL, "min_group_size == 0 is rejected (the reference would form empty groups forever)");
    if (uint64_t(cfgs[i].alt_begin) + cfgs[i].alt_count > n_alts)
      return set_error(PM_ERANGE, "alternative range outside the alt table");
  }
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  HIPCHK(hipSetDevice(e->cfg.device));
  e->cfgs.assign(cfgs, cfgs + n_cfgs);
  e->alts.assign(alts, alts + n_alts);
  int32_t rc = upload(e->d_cfgs, e->cfgs.data(), e->cfgs.size(), e->stream);
  if (rc) return rc;
  rc = upload(e->d_alts, e->alts.data(), e->alts.size(), e->stream);
  if (rc) return rc;
  HIPCHK(e->d_model_bits.ensure(1));
  HIPCHK(hipStreamSynchronize(e->stream));
  e->have_cfgs = true;
  e->compat_dirty = true;
  e->tplanes_dirty = true;
  return PM_OK;
}

int32_t pm_set_model_table(pm_engine* e, const uint32_t* bits, uint32_t n_rows, uint32_t n_classes) {
  if (!e || (n_rows && n_classes && !bits)) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(hipSetDevice(e->cfg.device));
  const size_t words = size_t(n_rows) * ((n_classes + 31u) / 32u);
  e->model_bits.assign(bits, bits + words);
  e->model_rows = n_rows;
  e->model_classes = n_classes;
  e->cls_check_dirty = true;
  int32_t rc = upload(e->d_model_bits, e->model_bits.data(), words, e->stream);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(e->stream));
  e->compat_dirty = true;
  return PM_OK;
}

int32_t pm_set_enabled_mask(pm_engine* e, uint64_t enabled) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  e->enabled = enabled;
  return PM_OK;
}

#include "pm_engine_workers.inc"
#include "pm_engine_tasks.inc"
#include "pm_engine_api.inc"
#include "pm_engine_adopt.inc"
#include "pm_engine_report.inc"
#include "pm_engine_spread.inc"
#include "pm_engine_near.inc"
#include "pm_engine_probe.inc"
}  // extern "C"

// the optional ledgers: each file holds its helpers (namespace pm) and, behind them, its entry points (extern "C").  Liveness
// calls the metrics hook, and discovery asks liveness's guard: hence the order.
#include "pm_engine_changes.inc"
#include "pm_engine_metrics.inc"
#include "pm_engine_liveness.inc"
#include "pm_engine_discovery.inc"
#include "pm_engine_rollout.inc"
#include "pm_engine_directory.inc"
#include "pm_engine_groupdir.inc"
#include "pm_engine_taskdir.inc"
#include "pm_engine_addresses.inc"
#include "pm_engine_gate.inc"
#include "pm_engine_admission.inc"

extern "C" {
#include "pm_engine_tick.inc"
#include "pm_engine_dist.inc"
#include "pm_engine_debug.inc"
}  // extern "C"
