// CPU unit test of the owning types of protocol_amd/csrc/pm_owned.h (DevBuf, PinBuf, Event, Stream, the live-allocation
// counter) over stubs of the HIP runtime calls they make: malloc and counters, with a switch that makes the next allocation
// fail.  Links against no HIP library.  Built and run by tests/test_host_helpers.py (g++, with the address sanitizer when it
// links: a buffer freed twice or never is its finding as well as the counters').
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "pm_owned.h"

// ---- the stubs
static long g_dev_live = 0, g_pin_live = 0, g_handles_live = 0;  // allocations the stubs have handed out and not got back
static long g_dev_allocs = 0, g_dev_frees = 0, g_pin_allocs = 0, g_pin_frees = 0, g_ev_destroyed = 0, g_syncs = 0;
static bool g_fail_next = false;  // the next allocation answers hipErrorOutOfMemory
static void* g_last_freed = nullptr;

static bool fail_now() {
  const bool f = g_fail_next;
  g_fail_next = false;
  return f;
}
extern "C" {
hipError_t hipMalloc(void** p, size_t n) {
  if (fail_now()) return hipErrorOutOfMemory;
  *p = std::malloc(n ? n : 1);
  ++g_dev_live, ++g_dev_allocs;
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  std::free(p);
  g_last_freed = p;
  --g_dev_live, ++g_dev_frees;
  return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) {
  if (fail_now()) return hipErrorOutOfMemory;
  *p = std::malloc(n ? n : 1);
  ++g_pin_live, ++g_pin_allocs;
  return hipSuccess;
}
hipError_t hipHostFree(void* p) {
  std::free(p);
  --g_pin_live, ++g_pin_frees;
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* ev, unsigned) {
  if (fail_now()) return hipErrorOutOfMemory;
  *ev = reinterpret_cast<hipEvent_t>(std::malloc(1));
  ++g_handles_live;
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* ev) { return hipEventCreateWithFlags(ev, 0); }
hipError_t hipEventDestroy(hipEvent_t ev) {
  std::free(ev);
  --g_handles_live, ++g_ev_destroyed;
  return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {
  if (fail_now()) return hipErrorOutOfMemory;
  *s = reinterpret_cast<hipStream_t>(std::malloc(1));
  ++g_handles_live;
  return hipSuccess;
}
hipError_t hipStreamCreate(hipStream_t* s) { return hipStreamCreateWithFlags(s, 0); }
hipError_t hipStreamDestroy(hipStream_t s) {
  std::free(s);
  --g_handles_live;
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) {
  ++g_syncs;
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind, hipStream_t) {
  std::memcpy(dst, src, n);
  return hipSuccess;
}
}  // extern "C"

#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                 \
    }                                                           \
  } while (0)

static uint64_t held(int k) { return pm::g_live_allocs[k].load(); }
// nothing is held: by the stubs' count and by the header's own
static bool all_zero() {
  return !g_dev_live && !g_pin_live && !g_handles_live && !held(0) && !held(1) && !held(2);
}

using pm::DevBuf;
using pm::Event;
using pm::PinBuf;
using pm::Stream;
static_assert(!std::is_copy_constructible<DevBuf<int>>::value && !std::is_copy_assignable<DevBuf<int>>::value, "move-only");
static_assert(!std::is_copy_constructible<PinBuf<int>>::value && !std::is_copy_constructible<Event>::value &&
                  !std::is_copy_constructible<Stream>::value, "move-only");
static_assert(std::is_nothrow_move_constructible<Event>::value && std::is_nothrow_move_constructible<PinBuf<uint64_t>>::value,
              "std::vector<Event> and the retired snapshot buffers must move, not copy, when the vector grows");

static int test_ensure() {
  {
    DevBuf<uint32_t> b;
    CHECK(b.ensure(0) == hipSuccess && !b.p && !b.cap && g_dev_allocs == 0);  // nothing asked for, nothing made
    CHECK(b.ensure(1000) == hipSuccess && b.p && b.cap == 1000 + 1000 / 8 + 64);
    CHECK(held(0) == b.cap * sizeof(uint32_t) && g_dev_live == 1);
    uint32_t* const p0 = b.p;
    const long allocs = g_dev_allocs;
    const uint64_t held0 = held(0);
    for (size_t n : {size_t(0), size_t(1), size_t(1000), b.cap}) {  // at or below the capacity: a no-op, the counter untouched
      CHECK(b.ensure(n) == hipSuccess && b.p == p0 && b.cap == 1189 && g_dev_allocs == allocs && held(0) == held0);
    }
    CHECK(b.ensure(1190) == hipSuccess && b.cap == 1190 + 1190 / 8 + 64 && g_dev_live == 1 && g_last_freed == p0);
    CHECK(held(0) == b.cap * sizeof(uint32_t));
    g_fail_next = true;  // a failed growth leaves an empty buffer, as it always did: ensure gives the old one up first
    CHECK(b.ensure(100000) != hipSuccess && !b.cap && g_dev_live == 0 && held(0) == 0);
  }
  CHECK(all_zero());
  return 0;
}

static int test_grow_keep() {
  {
    DevBuf<uint64_t> b;
    const long s0 = g_syncs;
    CHECK(b.grow_keep(10, 0, nullptr) == hipSuccess && b.cap == 10 + 10 / 4 + 64 && g_syncs == s0);
    for (size_t i = 0; i < b.cap; ++i) b.p[i] = 7000 + i;
    uint64_t* const p0 = b.p;
    const size_t cap0 = b.cap;
    CHECK(b.grow_keep(cap0, 5, nullptr) == hipSuccess && b.p == p0 && b.cap == cap0);  // room: a no-op
    g_fail_next = true;  // the new allocation fails: the old buffer is intact
    CHECK(b.grow_keep(1000, 50, nullptr) != hipSuccess && b.p == p0 && b.cap == cap0 && g_dev_live == 1);
    for (size_t i = 0; i < cap0; ++i) CHECK(b.p[i] == 7000 + i);
    CHECK(held(0) == cap0 * sizeof(uint64_t));
    CHECK(b.grow_keep(1000, 50, nullptr) == hipSuccess && b.cap == 1000 + 1000 / 4 + 64 && b.p != nullptr);
    CHECK(g_syncs == s0 + 1 && g_dev_live == 1 && g_last_freed == p0);  // synchronised before the old buffer went
    for (size_t i = 0; i < 50; ++i) CHECK(b.p[i] == 7000 + i);
    CHECK(held(0) == b.cap * sizeof(uint64_t));
    b.release();
    CHECK(!b.p && !b.cap && all_zero());
    b.release();  // (twice is once)
    CHECK(g_dev_allocs == g_dev_frees);
  }
  CHECK(all_zero());
  return 0;
}

static int test_moves() {
  {
    DevBuf<int> a, b;
    CHECK(a.ensure(10) == hipSuccess && b.ensure(20) == hipSuccess);
    int *const pa = a.p, *const pb = b.p;
    const size_t ca = a.cap, cb = b.cap;
    DevBuf<int> c(std::move(a));  // construction: the source is empty, nothing is freed
    CHECK(!a.p && !a.cap && c.p == pa && c.cap == ca && g_dev_live == 2);
    const long frees = g_dev_frees;
    c = std::move(b);  // assignment: the target's old buffer is freed exactly once, the source is empty
    CHECK(!b.p && !b.cap && c.p == pb && c.cap == cb && g_dev_frees == frees + 1 && g_last_freed == pa && g_dev_live == 1);
    CHECK(held(0) == cb * sizeof(int));
    DevBuf<int>& self = c;
    c = std::move(self);  // onto itself: nothing happens
    CHECK(c.p == pb && c.cap == cb && g_dev_frees == frees + 1);
    // std::swap (publish_end exchanges the task words and the next ones) goes through the moves
    DevBuf<int> d;
    CHECK(d.ensure(300) == hipSuccess);
    int* const pd = d.p;
    const size_t cd = d.cap;
    std::swap(c, d);
    CHECK(c.p == pd && c.cap == cd && d.p == pb && d.cap == cb && g_dev_live == 2 && g_dev_frees == frees + 1);
    // release is assignment: a struct of buffers replaced by a fresh one gives them all back
    struct Ledger {
      bool on = false;
      DevBuf<int> x[2];
      PinBuf<uint32_t> pin;
    } l;
    l.on = true;
    CHECK(l.x[0].ensure(5) == hipSuccess && l.x[1].ensure(6) == hipSuccess && l.pin.ensure(4, 4) == hipSuccess);
    CHECK(g_dev_live == 4 && g_pin_live == 1);
    l = Ledger();
    CHECK(!l.on && !l.x[0].p && !l.x[1].p && !l.pin.p && g_dev_live == 2 && g_pin_live == 0 && held(1) == 0);
  }
  CHECK(all_zero() && g_dev_allocs == g_dev_frees);
  return 0;
}

static int test_pin() {
  {
    PinBuf<uint32_t> h;
    const long a0 = g_pin_allocs, f0 = g_pin_frees;
    CHECK(h.ensure(0, 16) == hipSuccess && !h.p && g_pin_allocs == a0);  // cap < n is what allocates
    CHECK(h.ensure(1, 1) == hipSuccess && h.p && h.cap == 1);        // a fixed-size pin on first use
    uint32_t* const p1 = h.p;
    CHECK(h.ensure(1, 1) == hipSuccess && h.p == p1 && g_pin_allocs == a0 + 1);
    CHECK(h.ensure(100, 100 + 50 + 4096) == hipSuccess && h.cap == 4246 && g_pin_live == 1 && g_pin_frees == f0 + 1);  // the caller's rule
    CHECK(held(1) == 4246 * sizeof(uint32_t));
    uint32_t* const p2 = h.p;
    h.p[4245] = 9u;
    const uint64_t held1 = held(1);
    for (size_t n : {size_t(0), size_t(100), size_t(4246)}) {  // cap >= n: the pointer stays, whatever `want` says
      CHECK(h.ensure(n, 2 * n + 100000) == hipSuccess && h.p == p2 && h.cap == 4246 && g_pin_allocs == a0 + 2 && held(1) == held1);
    }
    CHECK(h.p[4245] == 9u);
    g_fail_next = true;
    CHECK(h.ensure(5000, 5000) != hipSuccess && !h.p && !h.cap && g_pin_live == 0 && held(1) == 0);
    // a vector of owners (the retired snapshot buffers): growth moves them, the end frees each once
    std::vector<PinBuf<uint64_t>> retired;
    for (int k = 0; k < 9; ++k) {
      PinBuf<uint64_t> b;
      CHECK(b.ensure(8, 8) == hipSuccess);
      retired.push_back(std::move(b));
      CHECK(g_pin_live == k + 1);
    }
    CHECK(held(1) == 9 * 8 * sizeof(uint64_t));
  }
  CHECK(all_zero() && g_pin_allocs == g_pin_frees);
  return 0;
}

static int test_handles() {
  {
    const long d0 = g_ev_destroyed;
    std::vector<Event> evs;
    for (int k = 0; k < 40; ++k) {  // grows (reallocating as it goes) ...
      Event x;
      CHECK(!x && x.create() == hipSuccess && x);
      hipEvent_t raw = x;
      evs.push_back(std::move(x));
      CHECK(!x && hipEvent_t(evs.back()) == raw);
    }
    CHECK(g_handles_live == 40 && held(2) == 40 && g_ev_destroyed == d0);
    evs.resize(10);  // ... and shrinks: each event that leaves is destroyed once
    CHECK(g_handles_live == 10 && held(2) == 10 && g_ev_destroyed == d0 + 30);
    evs.shrink_to_fit();
    CHECK(g_handles_live == 10 && g_ev_destroyed == d0 + 30);
    Event arr[3];
    g_fail_next = true;
    CHECK(arr[0].create() != hipSuccess && !arr[0] && held(2) == 10);
    CHECK(arr[1].create(hipEventDisableTiming) == hipSuccess && held(2) == 11);
    arr[2] = std::move(arr[1]);
    CHECK(!arr[1] && arr[2] && held(2) == 11);
    Stream s;
    CHECK(s.create(hipStreamNonBlocking) == hipSuccess && hipStream_t(s) != nullptr && held(2) == 12 && g_handles_live == 12);
    Stream t(std::move(s));
    CHECK(!s && t && held(2) == 12);
  }
  CHECK(all_zero() && g_ev_destroyed == 41);
  return 0;
}

int main() {
  if (test_ensure() || test_grow_keep() || test_moves() || test_pin() || test_handles()) return 1;
  CHECK(all_zero());
  std::printf("owned_test ok\n");
  return 0;
}
