// probe_stage.hpp -- host-side staging of one device probe call (probes.hpp): inputs uploaded, outputs reserved and copied
// back.  The number of cases is stated once per call and an array's elements per case once per array; every byte count
// follows from them and sizeof(T).
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>

#include <vector>

#include "devbuf.hpp"

namespace dmt {

// One probe call over n cases on `device`: the launch geometry, the first HIP error of its staging with the call that gave
// it, and the copies its outputs still owe.
class Probe {
 public:
  Probe(int device, size_t n) : n_(n) { ok(hipSetDevice(device), "hipSetDevice"); }
  hipError_t err = hipSuccess;
  char const* call = "";  // the failing call, for the error message
  size_t cases() const { return n_; }
  // blocks of `block` threads, one thread per case, and the threads they hold
  unsigned blocks(unsigned block) const { return unsigned((n_ + block - 1) / block); }
  size_t threads(unsigned block) const { return size_t(blocks(block)) * block; }
  // keeps the first error; false once there is one
  bool ok(hipError_t e, char const* what) {
    if (err == hipSuccess && e != hipSuccess) err = e, call = what;
    return err == hipSuccess;
  }
  void owe(void* host, void const* dev, size_t bytes) { owed_.push_back({host, dev, bytes}); }
  // after the kernel has finished: every output to its host array, in the order the outputs were declared
  hipError_t fetch() {
    for (Copy const& c : owed_)
      if (!ok(hipMemcpy(c.host, c.dev, c.bytes, hipMemcpyDeviceToHost), "hipMemcpy (probe output to host)")) break;
    return err;
  }

 private:
  struct Copy { void* host; void const* dev; size_t bytes; };
  size_t n_;
  std::vector<Copy> owed_;
};

// Input array, `width` elements of T per case at `host`, uploaded; a null `host` (an optional input) leaves it empty.
template <class T>
class ProbeIn {
 public:
  ProbeIn(Probe& p, void const* host, size_t width) {
    if (host && p.err == hipSuccess) p.ok(d_.assign(host, width * p.cases()), "hipMalloc + hipMemcpy (probe input to device)");
  }
  T const* get() const { return d_.get(); }

 private:
  DevBuf<T> d_;
};

// Output array, `width` elements of T per case: reserved for the kernel to write, and owed to `host` unless `host` is null
// or the array is empty -- an optional output the caller did not ask for is written on the device and dropped.
template <class T>
class ProbeOut {
 public:
  ProbeOut(Probe& p, void* host, size_t width) {
    size_t const n = width * p.cases();
    if (p.err == hipSuccess && p.ok(d_.reserve(n), "hipMalloc (probe output)") && host && n) p.owe(host, d_.get(), n * sizeof(T));
  }
  T* get() const { return d_.get(); }

 private:
  DevBuf<T> d_;
};

}  // namespace dmt
