// pm_engine_addresses.inc — part of pm_engine.cpp (one translation unit; included in place): the address book: its columns and
// their growth (namespace pm) — and, behind them (extern "C"), C ABI: pm_addresses_enable / _set / _rank / _text,
// pm_keccak256_many, pm_invite_digests (kernels in pm_keccak.inc and pm_addresses.inc).  Included at file scope.
//
// The book is four columns over the workers [0, ab.W): the 20 bytes, the EIP-55 case mask, the text key, a "set" flag (mirrored
// on the host: ab.h_set, ab.n_set).  pm_upload_workers(keep_groups = 0) sets ab.reinit, the one hook in the upload path;
// everything else happens when the next book call runs addresses_prepare.  Everything is queued on the engine's stream.  A
// book call leaves the tick's state alone but for pm_addresses_rank, which writes what pm_set_addr_ranks writes.
namespace pm {

// a fresh book: every buffer goes back; whether it is on and the path counters stay
static void addresses_release(pm_engine* e) {
  AddressBook fresh;
  fresh.on = e->ab.on;
  fresh.shallow = e->ab.shallow, fresh.deep = e->ab.deep;
  fresh.epoch = e->ab.epoch + 1;
  e->ab = std::move(fresh);
}

// the columns cover the workers [0, W): creates them, clears the flags of appended rows, and every flag behind an upload that
// dropped the row identities (queued, not waited for)
static int32_t addresses_prepare(pm_engine* e) {
  AddressBook& ab = e->ab;
  const uint32_t W = e->W;
  if (!ab.h_pin.p) HIPCHK(ab.h_pin.ensure(1, 1));
  uint32_t keep = ab.W;
  if (ab.reinit || W < keep) keep = 0;  // (a shorter table is a new table)
  if (W > keep || ab.reinit) {
    HIPCHK(ab.bytes.grow_keep(5 * size_t(W ? W : 1), 5 * size_t(keep), e->stream));
    HIPCHK(ab.mask.grow_keep(W ? W : 1, keep, e->stream));
    HIPCHK(ab.keys.grow_keep(PM_AB_WORDS * size_t(W ? W : 1), PM_AB_WORDS * size_t(keep), e->stream));
    HIPCHK(ab.set.grow_keep(W ? W : 1, keep, e->stream));
    launch_ab_clear(ab.set.p, keep, W, e->stream);
    HIPCHK(hipGetLastError());
    if (!keep) ab.h_set.clear(), ab.n_set = 0;
    ab.h_set.resize(W, 0);
    ab.epoch++;
  }
  ab.W = W;
  ab.reinit = false;
  return PM_OK;
}

// what every book call but pm_addresses_enable asks first
static int32_t addresses_guard(pm_engine* e) {
  if (!e->ab.on) return set_error(PM_ESTATE, "the address book is off");
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  if (!e->have_workers) return set_error(PM_ESTATE, "workers must be uploaded first");
  return PM_OK;
}

// rows[0, n) (null: 0 .. n - 1) name rows of the table that hold an address
static int32_t addresses_rows_ok(pm_engine* e, const uint32_t* rows, uint32_t n) {
  if (!rows && n > e->W) return set_error(PM_ERANGE, "more rows than the table has");
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t w = rows ? rows[k] : k;
    if (w >= e->W) return set_error(PM_ERANGE, "worker index out of range");
    if (!e->ab.h_set[w]) return set_error(PM_ESTATE, "the row holds no address (pm_addresses_set)");
  }
  return PM_OK;
}

}  // namespace pm

extern "C" {

int32_t pm_addresses_enable(pm_engine* e, uint32_t on) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");
  HIPCHK(hipSetDevice(e->cfg.device));
  HIPCHK(hipStreamSynchronize(e->stream));
  addresses_release(e);
  e->ab.on = on != 0;
  if (!e->ab.on || !e->have_workers) return PM_OK;
  int32_t rc = addresses_prepare(e);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(e->stream));
  return PM_OK;
}

int32_t pm_addresses_set(pm_engine* e, uint32_t first_row, const uint8_t* addr20, uint32_t n) {
  if (!e || (n && !addr20)) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = addresses_guard(e);
  if (rc) return rc;
  if (uint64_t(first_row) + n > e->W) return set_error(PM_ERANGE, "rows behind the worker table");
  HIPCHK(hipSetDevice(e->cfg.device));
  if ((rc = addresses_prepare(e))) return rc;
  if (!n) return PM_OK;
  AddressBook& ab = e->ab;
  HIPCHK(ab.stage.ensure(5 * size_t(n)));
  HIPCHK(hipMemcpyAsync(ab.stage.p, addr20, 20 * size_t(n), hipMemcpyHostToDevice, e->stream));
  launch_ab_set(ab.stage.p, first_row, n, ab.bytes.p, ab.mask.p, ab.keys.p, ab.set.p, e->stream);
  HIPCHK(hipGetLastError());
  ab.epoch++;
  for (uint32_t k = 0; k < n; ++k) {
    ab.n_set += ab.h_set[first_row + k] ? 0u : 1u;
    ab.h_set[first_row + k] = 1;
  }
  HIPCHK(hipStreamSynchronize(e->stream));  // pageable source
  return PM_OK;
}

int32_t pm_addresses_rank(pm_engine* e, uint32_t* rank_out) {
  if (!e) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = addresses_guard(e);
  if (rc) return rc;
  HIPCHK(hipSetDevice(e->cfg.device));
  if ((rc = addresses_prepare(e))) return rc;
  AddressBook& ab = e->ab;
  const uint32_t W = e->W;
  if (ab.n_set != W) return set_error(PM_ESTATE, "rows without an address (pm_addresses_set)");
  if (!W) return PM_OK;
  HIPCHK(ab.sort.ensure(W));
  HIPCHK(ab.ties.ensure(1));
  HIPCHK(e->d_addr_rank.ensure(W));  // (the worker upload sized it)
  const RoSortBufs bufs = ab.sort.bufs();
  HIPCHK(hipMemsetAsync(ab.ties.p, 0, sizeof(uint32_t), e->stream));
  uint32_t cur = launch_ab_sort_shallow(ab.keys.p, W, bufs, ab.ties.p, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(ab.h_pin.p, ab.ties.p, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (ab.h_pin.p[0]) {  // two rows share their first ten characters: every word decides
    cur = launch_ab_sort_deep(ab.keys.p, W, bufs, e->stream);
    ab.deep++;
  } else {
    ab.shallow++;
  }
  launch_ab_rank(bufs.val[cur], W, e->d_addr_rank.p, e->stream);
  HIPCHK(hipGetLastError());
  e->h_addr_rank.resize(W);
  HIPCHK(hipMemcpyAsync(e->h_addr_rank.data(), e->d_addr_rank.p, size_t(W) * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (rank_out) std::memcpy(rank_out, e->h_addr_rank.data(), size_t(W) * sizeof(uint32_t));
  return PM_OK;
}

int32_t pm_addresses_text(pm_engine* e, const uint32_t* rows, uint32_t n, char* out) {
  if (!e || (n && !out)) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = addresses_guard(e);
  if (rc) return rc;
  HIPCHK(hipSetDevice(e->cfg.device));
  if ((rc = addresses_prepare(e))) return rc;
  if ((rc = addresses_rows_ok(e, rows, n))) return rc;
  if (!n) return PM_OK;
  if (uint64_t(n) * PM_AB_TEXT > 0x7FFFFFFFull) return set_error(PM_ERANGE, "too many rows in one call");
  AddressBook& ab = e->ab;
  HIPCHK(ab.text.ensure(size_t(n) * PM_AB_TEXT));
  if (rows) {
    HIPCHK(ab.stage.ensure(n));
    HIPCHK(hipMemcpyAsync(ab.stage.p, rows, size_t(n) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  }
  launch_ab_text(rows ? ab.stage.p : nullptr, n, ab.bytes.p, ab.mask.p, ab.text.p, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, ab.text.p, size_t(n) * PM_AB_TEXT, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return PM_OK;
}

int32_t pm_keccak256_many(pm_engine* e, const uint8_t* bytes, const uint32_t* offsets, uint32_t n, uint8_t* out) {
  if (!e || (n && (!offsets || !out))) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");  // (it queues on the engine's stream)
  if (!n) return PM_OK;
  if (n > 0x07FFFFFFu) return set_error(PM_ERANGE, "too many messages in one call");
  for (uint32_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) return set_error(PM_EINVAL, "the offsets must not descend");
  const uint32_t total = offsets[n];  // (the buffer goes up from its first byte, whatever offsets[0] is)
  if (total && !bytes) return set_error(PM_EINVAL, "null argument");
  HIPCHK(hipSetDevice(e->cfg.device));
  AddressBook& ab = e->ab;
  HIPCHK(ab.text.ensure(size_t(total) + 8));  // (the kernel reads whole aligned words: the last may end behind the last byte)
  HIPCHK(ab.stage.ensure(size_t(n) + 1));
  HIPCHK(ab.out64.ensure(4 * size_t(n)));
  if (total) HIPCHK(hipMemcpyAsync(ab.text.p, bytes, total, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(ab.stage.p, offsets, (size_t(n) + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  launch_keccak_many(ab.text.p, ab.stage.p, n, ab.out64.p, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, ab.out64.p, 32 * size_t(n), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return PM_OK;
}

int32_t pm_invite_digests(pm_engine* e, uint32_t domain_id, uint32_t pool_id, const uint32_t* rows, uint32_t n, const uint8_t* nonce,
                          const uint64_t* expiration_s, uint8_t* digest, uint8_t* signing_hash) {
  if (!e || (n && (!rows || !nonce || !expiration_s || !digest || !signing_hash))) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = addresses_guard(e);
  if (rc) return rc;
  HIPCHK(hipSetDevice(e->cfg.device));
  if ((rc = addresses_prepare(e))) return rc;
  if (!n) return PM_OK;
  if (n > 0x03FFFFFFu) return set_error(PM_ERANGE, "too many rows in one call");
  if ((rc = addresses_rows_ok(e, rows, n))) return rc;
  AddressBook& ab = e->ab;
  HIPCHK(ab.stage.ensure(n));
  HIPCHK(ab.in64.ensure(5 * size_t(n)));   // [4 n] the nonces, [n] the expirations
  HIPCHK(ab.out64.ensure(8 * size_t(n)));  // [4 n] the digests, [4 n] the signing hashes
  HIPCHK(hipMemcpyAsync(ab.stage.p, rows, size_t(n) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(ab.in64.p, nonce, 32 * size_t(n), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(ab.in64.p + 4 * size_t(n), expiration_s, 8 * size_t(n), hipMemcpyHostToDevice, e->stream));
  launch_invite_digests(ab.stage.p, n, ab.bytes.p, domain_id, pool_id, ab.in64.p, ab.in64.p + 4 * size_t(n), ab.out64.p,
                        ab.out64.p + 4 * size_t(n), e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(digest, ab.out64.p, 32 * size_t(n), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(signing_hash, ab.out64.p + 4 * size_t(n), 32 * size_t(n), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return PM_OK;
}

}  // extern "C"
