// buffer.h — the owning buffer type of the runner and the encoder contexts.
#pragma once

#include <hip/hip_runtime.h>

#include <utility>

#include "runtime.h"

namespace uph {

// Device or pinned host memory that grows on demand and frees itself.  The
// contents do not survive a growth: every user fills the buffer afresh.
class Buffer {
 public:
  enum Kind { Device, Pinned };
  explicit Buffer(Kind kind) : kind_(kind) {}
  Buffer(Buffer&& o) noexcept : kind_(o.kind_), p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
  Buffer& operator=(Buffer&& o) noexcept {
    if (this != &o) {
      release();
      kind_ = o.kind_;
      std::swap(p_, o.p_);
      std::swap(cap_, o.cap_);
    }
    return *this;
  }
  ~Buffer() { release(); }
  // Room for `bytes`; a buffer too small is replaced by one of bytes + slack.
  // A failed allocation leaves the buffer empty.
  bool reserve(size_t bytes, size_t slack = 0) {
    if (cap_ >= bytes) return true;
    release();
    const size_t n = bytes + slack;
    if (!(kind_ == Pinned ? UPH_HIP(hipHostMalloc(&p_, n, hipHostMallocDefault)) : UPH_HIP(hipMalloc(&p_, n)))) {
      p_ = nullptr;
      return false;
    }
    cap_ = n;
    return true;
  }
  void release() {
    if (p_) kind_ == Pinned ? (void)hipHostFree(p_) : (void)hipFree(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  template <class T = uint8_t>
  T* as() const {
    return static_cast<T*>(p_);
  }
  size_t capacity() const { return cap_; }

 private:
  Kind kind_;
  void* p_ = nullptr;
  size_t cap_ = 0;
};

}  // namespace uph
