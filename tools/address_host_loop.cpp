// address_host_loop.cpp — the baseline of tools/address_probe.py: what the plugin does today when nodes join (sync_nodes,
// gpu_match_plugin.cpp) — each new address's text goes into a vector of rows kept sorted by text (one binary search, one insert),
// the ranks of all W rows are rebuilt from it, and the whole column goes up with pm_set_addr_ranks — on one host thread.  To be
// fair to a host that wants the reference's order, the text of each new address is its EIP-55 text, computed here
// (pm_host_eip55: one keccak-256 a new address).
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "pm_engine.h"

namespace {
std::vector<std::string> g_text;   // by row
std::vector<uint32_t> g_by_text;   // rows in text order
std::vector<uint32_t> g_rank;
}  // namespace

extern "C" {

void addr_host_reset(void) {
  g_text.clear();
  g_by_text.clear();
}

// rows [W0, W0 + n) join with the addresses addr20[20 n]; the engine already holds W0 + n rows.  Returns the engine's error.
int32_t addr_host_append(pm_engine* e, const uint8_t* addr20, uint32_t n) {
  for (uint32_t k = 0; k < n; ++k) {
    char t[43];
    pm_host_eip55(addr20 + 20 * size_t(k), t);
    const uint32_t row = uint32_t(g_text.size());
    g_text.emplace_back(t);
    const std::string& key = g_text.back();
    const auto at = std::partition_point(g_by_text.begin(), g_by_text.end(), [&](uint32_t j) { return g_text[j] < key; });
    g_by_text.insert(at, row);
  }
  g_rank.resize(g_text.size());
  uint32_t r = 0;
  for (uint32_t row : g_by_text) g_rank[row] = r++;
  return pm_set_addr_ranks(e, g_rank.data(), uint32_t(g_rank.size()));
}

// the first load of a host that starts with W addresses: texts, one sort, the ranks
int32_t addr_host_load(pm_engine* e, const uint8_t* addr20, uint32_t n) {
  addr_host_reset();
  g_text.resize(n);
  g_by_text.resize(n);
  for (uint32_t k = 0; k < n; ++k) {
    char t[43];
    pm_host_eip55(addr20 + 20 * size_t(k), t);
    g_text[k] = t;
    g_by_text[k] = k;
  }
  std::stable_sort(g_by_text.begin(), g_by_text.end(), [&](uint32_t a, uint32_t b) { return g_text[a] < g_text[b]; });
  g_rank.resize(n);
  uint32_t r = 0;
  for (uint32_t row : g_by_text) g_rank[row] = r++;
  return n ? pm_set_addr_ranks(e, g_rank.data(), n) : PM_OK;
}

const uint32_t* addr_host_ranks(void) { return g_rank.data(); }

}  // extern "C"
