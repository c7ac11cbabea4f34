// hip_mem.h -- the owner of one piece of device memory (hipMalloc) or page-locked host memory (hipHostMalloc).
// Every buffer of the engine is held by one, so it is freed exactly once, on every path out, and has no capacity
// apart from size(): after ANY failed call the owner is empty (null, size 0), and the next "is it large enough"
// check goes through the allocation again.  The owner never synchronises: whether queued work still uses the
// memory is what the call site knows, and its stream synchronisation stands in front of alloc() / grow() / reset().
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <utility>

#include "../../include/ratsdf.h"

namespace ratsdf {

template <bool kPinned>
class HipMem {
 public:
  HipMem() = default;
  HipMem(HipMem&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  HipMem& operator=(HipMem&& o) noexcept {  // (frees what THIS held; what moves in is not touched)
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      bytes_ = std::exchange(o.bytes_, 0);
    }
    return *this;
  }
  HipMem(const HipMem&) = delete;
  HipMem& operator=(const HipMem&) = delete;
  ~HipMem() { reset(); }

  void reset() {
    if (p_) (void)(kPinned ? hipHostFree(p_) : hipFree(p_));
    p_ = nullptr;
    bytes_ = 0;
  }
  // frees what it held, then allocates: RATSDF_OK, or RATSDF_ERR_DEVICE with the owner left empty
  int alloc(size_t bytes) {
    reset();
    void* p = nullptr;
    const hipError_t err = kPinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
    if (err != hipSuccess) {
      fprintf(stderr, "[ratsdf] HIP error %s at %s:%d: %s(%zu bytes)\n", hipGetErrorName(err), __FILE__, __LINE__,
              kPinned ? "hipHostMalloc" : "hipMalloc", bytes);
      return RATSDF_ERR_DEVICE;
    }
    p_ = p;
    bytes_ = p ? bytes : 0;  // (0 bytes asked for: success and a null pointer)
    return RATSDF_OK;
  }
  // as alloc(), unless what it holds is large enough already (the contents are NOT carried over)
  int grow(size_t bytes) { return bytes <= bytes_ ? RATSDF_OK : alloc(bytes); }
  size_t size() const { return bytes_; }
  explicit operator bool() const { return p_ != nullptr; }
  template <class T>
  T* as() const { return static_cast<T*>(p_); }

 private:
  void* p_ = nullptr;
  size_t bytes_ = 0;
};
using DevMem = HipMem<false>;
using HostMem = HipMem<true>;

}  // namespace ratsdf
