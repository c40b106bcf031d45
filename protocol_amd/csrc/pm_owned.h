// pm_owned.h — what the engine holds from the HIP runtime, as types that give it back: device buffers, pinned host buffers,
// events, the engine's own stream.  Host code over the runtime's C API only (a plain C++17 compiler reads it: tests/cpp/owned_test.cpp
// does, over stubs), so that the lifetime of everything in struct pm_engine is the struct's own.
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace pm {

// What these types hold right now, process-wide (pm_debug_live_allocations): [0] device bytes, [1] pinned host bytes, [2] events
// and streams.  Touched only where the runtime is asked to allocate or free — never on an ensure that has room — so no tick sees it.
inline std::atomic<uint64_t> g_live_allocs[3];
inline void live_add(int k, uint64_t n) { g_live_allocs[k].fetch_add(n, std::memory_order_relaxed); }
inline void live_sub(int k, uint64_t n) { g_live_allocs[k].fetch_sub(n, std::memory_order_relaxed); }

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = std::exchange(o.p, nullptr), cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~DevBuf() { release(); }
  hipError_t ensure(size_t n) {
    if (n <= cap) return hipSuccess;
    release();
    return alloc(&p, &cap, n + n / 8 + 64);
  }
  // capacity for n elements, keeping the first `keep` (device-to-device copy on `s` when the buffer moves)
  hipError_t grow_keep(size_t n, size_t keep, hipStream_t s) {
    if (n <= cap) return hipSuccess;
    DevBuf q;
    hipError_t e = alloc(&q.p, &q.cap, n + n / 4 + 64);
    if (e != hipSuccess) return e;
    if (p && keep) {
      e = hipMemcpyAsync(q.p, p, keep * sizeof(T), hipMemcpyDeviceToDevice, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);  // the old buffer is freed right below
      if (e != hipSuccess) return e;
    }
    *this = std::move(q);
    return hipSuccess;
  }
  void release() {
    if (p) (void)hipFree(p), live_sub(0, cap * sizeof(T));
    p = nullptr;
    cap = 0;
  }

 private:
  static hipError_t alloc(T** q, size_t* q_cap, size_t want) {
    const hipError_t e = hipMalloc((void**)q, want * sizeof(T));
    if (e == hipSuccess) *q_cap = want, live_add(0, want * sizeof(T));
    return e;
  }
};

// Pinned host staging whose capacity only grows.  ensure(n, want): room for n elements; when there is not, the contents go and
// `want` (>= n: the caller's growth rule) elements are allocated.
template <typename T>
struct PinBuf {
  T* p = nullptr;
  size_t cap = 0;
  PinBuf() = default;
  PinBuf(PinBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  PinBuf& operator=(PinBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = std::exchange(o.p, nullptr), cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~PinBuf() { release(); }
  hipError_t ensure(size_t n, size_t want) {
    if (n <= cap) return hipSuccess;
    release();
    const hipError_t e = hipHostMalloc((void**)&p, want * sizeof(T), hipHostMallocDefault);
    if (e == hipSuccess) cap = want, live_add(1, want * sizeof(T));
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p), live_sub(1, cap * sizeof(T));
    p = nullptr;
    cap = 0;
  }
};

// One runtime handle (an event, a stream), destroyed with its holder; reads as the handle where one is asked for.
template <typename H, hipError_t (*Destroy)(H)>
struct Handle {
  H h = nullptr;
  Handle() = default;
  Handle(Handle&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
  Handle& operator=(Handle&& o) noexcept {
    if (this != &o) {
      reset();
      h = std::exchange(o.h, nullptr);
    }
    return *this;
  }
  ~Handle() { reset(); }
  operator H() const { return h; }
  void reset() {
    if (h) (void)Destroy(h), live_sub(2, 1);
    h = nullptr;
  }
};

struct Event : Handle<hipEvent_t, hipEventDestroy> {
  hipError_t create(unsigned flags = hipEventDefault) {
    reset();
    const hipError_t e = hipEventCreateWithFlags(&h, flags);
    if (e == hipSuccess) live_add(2, 1);
    return e;
  }
};

struct Stream : Handle<hipStream_t, hipStreamDestroy> {
  hipError_t create(unsigned flags) {
    reset();
    const hipError_t e = hipStreamCreateWithFlags(&h, flags);
    if (e == hipSuccess) live_add(2, 1);
    return e;
  }
};

}  // namespace pm
