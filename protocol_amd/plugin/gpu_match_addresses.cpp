// gpu_match_addresses.cpp — GpuMatchPlugin::enable_address_book / invite_digests and sync_nodes' engine calls with the book on
// (see gpu_match_plugin.hpp): the engine's address book (pm_addresses_* / pm_invite_digests).  The twin of the same methods of
// rust/gpu_match_plugin.rs — whose Address is the 20 bytes, so that it parses nothing, knows no second spelling and needs no
// second index key: everything else is its transcription (INTEGRATION.md "Address book").  (A file of its own: the plugin's
// other methods are also linked against a mock engine that has not these exports.)
#include <algorithm>
#include <shared_mutex>
#include <stdexcept>

#include "gpu_match_plugin.hpp"

namespace orchestrator {

// (the exclusive node lock is held.)  The bytes of the rows [first, end) — or of every row — go up, the engine ranks its texts,
// and the rows that render no device text yet get theirs: 43 bytes a new row come back, once
void GpuMatchPlugin::book_sync(GpuMatchPlugin& self, uint32_t first, bool all) {
  NodeTable& t = self.nodes_;
  AddressBookState& b = self.book_;
  const uint32_t W = uint32_t(t.rows.size());
  if (b.bytes.size() != 20 * size_t(W)) throw EngineError(PM_ESTATE, "the address book and the plugin's row map disagree");
  const uint32_t from = all ? 0u : first;
  if (from < W) self.check(pm_addresses_set(self.engine_, from, b.bytes.data() + 20 * size_t(from), W - from));
  if (!W) return;
  b.ranks.resize(W);
  self.check(pm_addresses_rank(self.engine_, b.ranks.data()));  // (kept: a rewritten row is sent with the rank it has)
  if (b.texts < W) {
    const uint32_t n = W - uint32_t(b.texts);
    std::vector<uint32_t> rows(n);
    for (uint32_t k = 0; k < n; ++k) rows[k] = uint32_t(b.texts) + k;
    std::vector<char> text(43 * size_t(n));
    self.check(pm_addresses_text(self.engine_, rows.data(), n, text.data()));
    for (uint32_t k = 0; k < n; ++k) {
      t.address_strings[rows[k]].assign(text.data() + 43 * size_t(k), 42);
      // the text the plugin shows is a key too (beside the spelling the store gave): what was read here can be handed back
      // (the Rust twin's Address is the 20 bytes, so its index needs no second entry)
      t.index.emplace(Address(t.address_strings[rows[k]]), rows[k]);
    }
    b.texts = W;
  }
}

void GpuMatchPlugin::enable_address_book() {
  std::unique_lock<std::shared_mutex> lk(nodes_mu_);
  if (book_.on) return;
  NodeTable& t = nodes_;
  AddressBookState fresh;
  for (size_t i = 0; i < t.rows.size(); ++i) {  // the rows the plugin has already: all of them must parse, before anything changes
    const std::string& text = t.addresses[i].to_string();
    std::array<uint8_t, 20> a{};
    if (!parse_address_text(text, a.data())) throw EngineError(PM_EINVAL, "not an address: '" + text + "'");
    fresh.bytes.insert(fresh.bytes.end(), a.begin(), a.end());
    if (!fresh.by_bytes.emplace(std::string(reinterpret_cast<const char*>(a.data()), a.size()), uint32_t(i)).second)
      throw EngineError(PM_EINVAL, "an address that has a row under another spelling: '" + text + "'");
  }
  check(pm_addresses_enable(engine_, 1u));
  fresh.on = true;
  book_ = std::move(fresh);
  book_sync_ = &GpuMatchPlugin::book_sync;
  t.by_address.clear();  // (not kept any more: row_of_address_text goes by the bytes)
  if (!t.rows.empty() && nodes_synced_.load() && !engine_rows_stale_) book_sync(*this, 0u, true);
}

std::vector<GpuMatchPlugin::InviteDigest> GpuMatchPlugin::invite_digests(uint32_t domain_id, uint32_t pool_id,
                                                                         const std::function<std::array<uint8_t, 32>()>& nonce,
                                                                         uint64_t expiration_s) const {
  std::shared_lock<std::shared_mutex> nodes(nodes_mu_);
  if (!book_.on) throw EngineError(PM_ESTATE, "the address book is off (enable_address_book)");
  const pm_dir_query q{1u << PM_NS_DISCOVERED, PM_DIR_ANY, PM_DIR_BY_ROW, 0u, 0xFFFFFFFFu};  // uninvited_nodes' query
  uint32_t total = 0;
  const std::vector<pm_dir_row> listed = directory_locked(q, &total, nullptr);
  const uint32_t n = uint32_t(listed.size());
  std::vector<InviteDigest> out(n);
  if (!n) return out;
  std::vector<uint32_t> rows(n);
  std::vector<uint8_t> nonces(32 * size_t(n)), digest(32 * size_t(n)), signing(32 * size_t(n));
  const std::vector<uint64_t> expiration(n, expiration_s);
  for (uint32_t k = 0; k < n; ++k) {
    rows[k] = listed[k].worker;
    out[k].address = nodes_.address_strings[rows[k]];
    out[k].nonce = nonce();
    std::copy(out[k].nonce.begin(), out[k].nonce.end(), nonces.begin() + 32 * size_t(k));
  }
  check(pm_invite_digests(engine_, domain_id, pool_id, rows.data(), n, nonces.data(), expiration.data(), digest.data(), signing.data()));
  for (uint32_t k = 0; k < n; ++k) {
    std::copy(digest.begin() + 32 * size_t(k), digest.begin() + 32 * size_t(k + 1), out[k].digest.begin());
    std::copy(signing.begin() + 32 * size_t(k), signing.begin() + 32 * size_t(k + 1), out[k].signing_hash.begin());
  }
  return out;
}

}  // namespace orchestrator
