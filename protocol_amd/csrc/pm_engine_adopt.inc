// pm_engine_adopt.inc — part of pm_engine.cpp (one translation unit; included in place): C ABI: adopting the groups a store
// already holds (pm_adopt_groups) and the state of the group id stream (pm_group_id_state) (inside extern "C").
//
// An orchestrator that restarts, or a pool that moves from NodeGroupsPlugin to the engine, finds its groups and their claimed
// tasks in the store (node_group:<id>, group_task:<id>; node_groups/mod.rs:25-28).  Adoption installs them as they stand: the
// host list, h_group_of and the id stream; the device mirror follows with the next full push_groups.  No kernel of its own:
// the carve continues the id stream at the first free slot (a.id_g0 = d_n_groups, a.id_state = id_rng), the merge orders by
// the ids' hex text and the seeded chooser hashes the id — none of them assumes the ids came from the stream.

// handle of the task at position `pos` of the caller's get_all_tasks list (pos < T): the inverse of task_position
static uint32_t task_handle(pm_engine* e, uint32_t pos) {
  (void)task_position(e, e->t_lo);  // (builds h_tprefix if it is stale)
  const uint32_t w0 = e->t_lo / 64u, stride = e->t_cap / 64u;
  // the last word whose prefix is <= pos holds it (words without a live row share their prefix with the next one)
  const uint32_t j = uint32_t(std::upper_bound(e->h_tprefix.begin() + w0, e->h_tprefix.begin() + stride, pos) - e->h_tprefix.begin()) - 1u;
  uint64_t w = e->h_tlive[j];
  for (uint32_t k = pos - e->h_tprefix[j]; k; --k) w &= w - 1ull;  // drop the live rows in front of it
  return j * 64u + uint32_t(__builtin_ctzll(w));
}

int32_t pm_adopt_groups(pm_engine* e, const pm_group* groups, uint32_t n_groups, const uint32_t* members, uint32_t n_members,
                        uint64_t id_state) {
  if (!e || (n_groups && !groups) || (n_members && !members)) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  if (!e->have_cfgs || !e->have_workers) return set_error(PM_ESTATE, "configs and workers must be uploaded first");
  if (e->absorb_pending) return set_error(PM_ESTATE, "the records of a carve wait to be absorbed");
  if (e->groups.size() != e->n_dead_groups) return set_error(PM_ESTATE, "the engine holds groups: adoption needs an empty list");
  const uint32_t C = uint32_t(e->cfgs.size()), W = e->W;
  // ---- validation, all of it before anything changes
  auto bad = [](uint32_t g, const std::string& rule) {
    return set_error(PM_EINVAL, "pm_adopt_groups: group " + std::to_string(g) + ": " + rule);
  };
  bool any_task = false;
  for (uint32_t g = 0; g < n_groups; ++g) any_task |= groups[g].task != PM_NONE;
  if (any_task && !e->have_tasks) return set_error(PM_ESTATE, "a group names a task: tasks must be uploaded first");
  std::vector<uint32_t> owner(W, PM_NONE);
  for (uint32_t g = 0; g < n_groups; ++g) {
    const pm_group& gr = groups[g];
    if (gr.config >= C) return bad(g, "config >= n_cfgs");
    if (gr.n_members < 1 || gr.n_members > e->cfgs[gr.config].max_group_size)
      return bad(g, "n_members outside 1..max_group_size of its configuration");
    if (uint64_t(gr.member_begin) + gr.n_members > n_members) return bad(g, "member_begin + n_members > n_members");
    if (gr.task != PM_NONE && gr.task >= e->T) return bad(g, "task >= T");
    for (uint32_t k = 0; k < gr.n_members; ++k) {
      const uint32_t w = members[gr.member_begin + k];
      if (w >= W) return bad(g, "member >= W");
      if (owner[w] != PM_NONE) return bad(g, "worker " + std::to_string(w) + " appears twice (also in group " + std::to_string(owner[w]) + ")");
      owner[w] = g;
    }
  }
  if (n_groups > 1) {
    std::vector<std::pair<uint64_t, uint32_t>> ids(n_groups);
    for (uint32_t g = 0; g < n_groups; ++g) ids[g] = {groups[g].id, g};
    std::sort(ids.begin(), ids.end());
    for (uint32_t k = 1; k < n_groups; ++k)
      if (ids[k].first == ids[k - 1].first) return bad(std::max(ids[k].second, ids[k - 1].second), "its id is another group's");
  }
  // ---- install: slots 0..n-1 in the given order (their creation order)
  e->groups.clear();
  e->groups.reserve(n_groups);
  e->n_dead_groups = 0;
  size_t solo = 0;
  for (uint32_t g = 0; g < n_groups; ++g) {
    const pm_group& src = groups[g];
    Group gr;
    gr.id = src.id;
    gr.cfg = src.config;
    gr.task = src.task == PM_NONE ? PM_NONE : task_handle(e, src.task);
    gr.task_uid = gr.task == PM_NONE ? 0 : (e->tasks_have_uid ? e->h_tuid[gr.task] : uint64_t(src.task));
    gr.members.assign(members + src.member_begin, members + src.member_begin + src.n_members);
    solo += src.n_members == 1;
    e->groups.push_back(std::move(gr));
  }
  e->h_group_of.assign(W, -1);
  for (uint32_t w = 0; w < W; ++w)
    if (owner[w] != PM_NONE) e->h_group_of[w] = int32_t(owner[w]);
  e->id_rng = id_state;
  e->tick_needs_merge = solo >= 2;
  // the device mirror goes up whole with the next push_groups (no delta: it holds another list, or none)
  e->groups_dirty = true, e->groups_delta_ok = false;
  e->delta_free.clear();
  e->delta_tail_from = PM_NONE;
  // The published rows know nothing of these groups: "no group" until the next pm_match / pm_tick publishes (as after
  // pm_reset_groups), and pub_patch resolves nothing against the new numbering.
  e->groups_epoch++;
  pub_clear(e);
  return PM_OK;
}

int32_t pm_group_id_state(pm_engine* e, uint64_t* state) {
  if (!e || !state) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  ABSORB_PENDING(e);  // (a deferred absorb draws the ids of its groups)
  *state = e->id_rng;
  return PM_OK;
}
