// pm_engine_gate.inc — part of pm_engine.cpp (one translation unit; included in place, behind pm_engine_addresses.inc and
// pm_engine_liveness.inc, whose prepare steps it calls): the request gate: the index of the address book's rows by their 20
// bytes (namespace pm) — and, behind it (extern "C"), C ABI: pm_ecrecover_many, pm_verify_requests (kernels in
// pm_secp256k1.inc).  Included at file scope.
//
// Both calls read the engine's tables and write only the gate's own scratch and index; everything is queued on the engine's
// stream and a call synchronises once before it returns.
namespace pm {

// the index stands for the book as it is now: built when the book's epoch or the row count has moved (queued, not waited for)
static int32_t gate_index(pm_engine* e) {
  Gate& g = e->gate;
  const AddressBook& ab = e->ab;
  if (g.valid && g.epoch == ab.epoch && g.W == e->W) return PM_OK;
  const uint32_t W = e->W;
  HIPCHK(g.sort.ensure(W ? W : 1));
  g.cur = launch_gate_index(ab.bytes.p, ab.set.p, W, g.sort.bufs(), e->stream);
  HIPCHK(hipGetLastError());
  g.n_idx = ab.n_set;
  g.W = W, g.epoch = ab.epoch, g.valid = true;
  g.builds++;
  return PM_OK;
}

// sig65 [65 n] to the device, and room for what the recovery writes
static int32_t gate_stage_recovery(pm_engine* e, const uint8_t* sig65, uint32_t n, bool want_pub) {
  Gate& g = e->gate;
  HIPCHK(g.sig.ensure(65 * size_t(n)));
  HIPCHK(g.addr.ensure(5 * size_t(n)));
  HIPCHK(g.ok.ensure(n));
  if (want_pub) HIPCHK(g.pub.ensure(8 * size_t(n)));
  HIPCHK(hipMemcpyAsync(g.sig.p, sig65, 65 * size_t(n), hipMemcpyHostToDevice, e->stream));
  return PM_OK;
}

// what a batch of requests must be before anything is queued for it (n > 0)
static int32_t gate_check(const uint8_t* bytes, const uint32_t* offsets, uint32_t n) {
  if (n > 0x01FFFFFFu) return set_error(PM_ERANGE, "too many requests in one call");
  for (uint32_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) return set_error(PM_EINVAL, "the offsets must not descend");
  const uint32_t total = offsets[n];  // (the buffer goes up from its first byte, whatever offsets[0] is)
  if (total && !bytes) return set_error(PM_EINVAL, "null argument");
  if (total > 0xFFFFFF00u) return set_error(PM_ERANGE, "too many message bytes in one call");
  return PM_OK;
}

// the gate's stages for a checked batch, queued: the index, the staging, the EIP-191 hashes, the recoveries and the verdicts —
// g.out [8 n], behind them the census.  What pm_verify_requests copies out and pm_admit_requests goes on from.
static int32_t gate_queue(pm_engine* e, const uint8_t* bytes, const uint32_t* offsets, const uint8_t* sig65, const uint8_t* claimed20,
                          const uint8_t* flags, uint32_t n) {
  int32_t rc;
  const uint32_t total = offsets[n];
  HIPCHK(hipSetDevice(e->cfg.device));
  if ((rc = addresses_prepare(e))) return rc;
  const bool live = e->live.on && e->dist_world <= 1;
  if (live && (rc = liveness_prepare(e))) return rc;
  if ((rc = gate_index(e))) return rc;
  Gate& g = e->gate;
  HIPCHK(g.text.ensure(size_t(total) + 8));  // (the kernel reads whole aligned words: the last may end behind the last byte)
  HIPCHK(g.off.ensure(size_t(n) + 1));
  HIPCHK(g.hash.ensure(4 * size_t(n)));
  HIPCHK(g.claimed.ensure(5 * size_t(n)));
  HIPCHK(g.out.ensure(8 * size_t(n) + PM_RQ_N_CODES));
  if (flags) HIPCHK(g.flags.ensure(n));
  if ((rc = gate_stage_recovery(e, sig65, n, false))) return rc;
  if (total) HIPCHK(hipMemcpyAsync(g.text.p, bytes, total, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(g.off.p, offsets, (size_t(n) + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(g.claimed.p, claimed20, 20 * size_t(n), hipMemcpyHostToDevice, e->stream));
  if (flags) HIPCHK(hipMemcpyAsync(g.flags.p, flags, n, hipMemcpyHostToDevice, e->stream));
  uint32_t* d_counts = g.out.p + 8 * size_t(n);
  HIPCHK(hipMemsetAsync(d_counts, 0, PM_RQ_N_CODES * sizeof(uint32_t), e->stream));
  launch_eip191_many(g.text.p, g.off.p, n, g.hash.p, e->stream);
  launch_ecrecover(g.hash.p, g.sig.p, n, g.addr.p, nullptr, g.ok.p, e->stream);
  launch_gate_verdict(g.addr.p, g.ok.p, g.sig.p, g.claimed.p, flags ? g.flags.p : nullptr, n, g.sort.val[g.cur].p, g.n_idx, e->ab.bytes.p,
                      live ? e->live.status.p : nullptr, g.out.p, d_counts, e->stream);
  HIPCHK(hipGetLastError());
  return PM_OK;
}

}  // namespace pm

extern "C" {

int32_t pm_ecrecover_many(pm_engine* e, const uint8_t* hash32, const uint8_t* sig65, uint32_t n, uint8_t* addr20_out, uint8_t* pub64_out,
                          uint8_t* ok_out) {
  if (!e || (n && (!hash32 || !sig65 || !addr20_out || !ok_out))) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->dist_phase != 0) return set_error(PM_ESTATE, "a stepwise tick is in progress");  // (it queues on the engine's stream)
  if (!n) return PM_OK;
  if (n > 0x01FFFFFFu) return set_error(PM_ERANGE, "too many signatures in one call");
  HIPCHK(hipSetDevice(e->cfg.device));
  Gate& g = e->gate;
  HIPCHK(g.hash.ensure(4 * size_t(n)));
  int32_t rc = gate_stage_recovery(e, sig65, n, pub64_out != nullptr);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(g.hash.p, hash32, 32 * size_t(n), hipMemcpyHostToDevice, e->stream));
  launch_ecrecover(g.hash.p, g.sig.p, n, g.addr.p, pub64_out ? g.pub.p : nullptr, g.ok.p, e->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(addr20_out, g.addr.p, 20 * size_t(n), hipMemcpyDeviceToHost, e->stream));
  if (pub64_out) HIPCHK(hipMemcpyAsync(pub64_out, g.pub.p, 64 * size_t(n), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(ok_out, g.ok.p, n, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return PM_OK;
}

int32_t pm_verify_requests(pm_engine* e, const uint8_t* bytes, const uint32_t* offsets, const uint8_t* sig65, const uint8_t* claimed20,
                           const uint8_t* flags, uint32_t n, pm_rq_verdict* out, uint32_t* counts) {
  static_assert(sizeof(pm_rq_verdict) == 32 && offsetof(pm_rq_verdict, row) == 4 && offsetof(pm_rq_verdict, status) == 8 &&
                    offsetof(pm_rq_verdict, address) == 12,
                "the verdict kernel writes a verdict as eight words");
  if (!e || (n && (!offsets || !sig65 || !claimed20 || !out || !counts))) return set_error(PM_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  int32_t rc = addresses_guard(e);
  if (rc) return rc;
  if (!n) return PM_OK;
  if ((rc = gate_check(bytes, offsets, n))) return rc;
  if ((rc = gate_queue(e, bytes, offsets, sig65, claimed20, flags, n))) return rc;
  Gate& g = e->gate;
  uint32_t* d_counts = g.out.p + 8 * size_t(n);
  HIPCHK(hipMemcpyAsync(out, g.out.p, sizeof(pm_rq_verdict) * size_t(n), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(counts, d_counts, PM_RQ_N_CODES * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return PM_OK;
}

}  // extern "C"
