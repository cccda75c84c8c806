// devbuf.hpp -- the owner types of the host side of the library: device memory (DevBuf) and a pair of events (EventPair).
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>

namespace dmt {

// Owner of one device array of T: hipFree on destruction, movable, not copyable.  Every device allocation of the
// host side goes through this type.
template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) reset(), p_ = o.p_, n_ = o.n_, o.p_ = nullptr, o.n_ = 0;
    return *this;
  }
  DevBuf(DevBuf const&) = delete;
  DevBuf& operator=(DevBuf const&) = delete;
  ~DevBuf() { reset(); }
  T* get() const { return p_; }
  size_t size() const { return n_; }  // elements allocated
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr, n_ = 0;
  }
  // room for at least n elements, contents not kept.  The old array is freed before the new one is allocated, so a
  // large scratch buffer never exists twice; on failure the buffer is empty.
  hipError_t reserve(size_t n) {
    if (n_ >= n) return hipSuccess;
    reset();
    hipError_t const e = hipMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T));
    if (e != hipSuccess) p_ = nullptr;
    else n_ = n;
    return e;
  }
  // max(n, 1) elements holding the n elements of T at `host`
  hipError_t assign(void const* host, size_t n) {
    hipError_t e = reserve(n ? n : 1);
    if (e == hipSuccess && n) e = hipMemcpy(p_, host, n * sizeof(T), hipMemcpyHostToDevice);
    return e;
  }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

// Two HIP events around a span of a stream, destroyed on every exit path.  The user creates them (hipEventCreate(&p.a)).
struct EventPair {
  hipEvent_t a = nullptr, b = nullptr;
  EventPair() = default;
  EventPair(EventPair const&) = delete;
  EventPair& operator=(EventPair const&) = delete;
  ~EventPair() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

}  // namespace dmt
