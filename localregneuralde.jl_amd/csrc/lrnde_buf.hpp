// Owners of the library's GPU resources: DevBuf<T> (hipMalloc), PinBuf<T> (hipHostMalloc) and HipEvent.  A handle's
// buffers are members of these types, so deleting the handle frees them and no destroy function lists memory
// (DESIGN.md 4.7).  Sizes are in elements of T.  Every call that allocates returns the hipError_t for the caller's
// HIPCHK / CHK; after a failed call the buffer is empty (null, size 0).  A test off the GPU defines
// LRNDE_BUF_HOST_TEST and supplies hipError_t, hipEvent_t and the hip* functions used here itself (tests/test_host_buf.py).
#pragma once
#ifndef LRNDE_BUF_HOST_TEST
#include <hip/hip_runtime.h>
#endif
#include <cstddef>

template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept { take(o); }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { (void)reset(); take(o); }
    return *this;
  }
  ~DevBuf() { (void)reset(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t size() const { return n_; }

  // grow-only: reallocates when n > size(); the contents are not preserved
  hipError_t grow(size_t n) { return n > n_ ? alloc(n) : hipSuccess; }
  // reallocates when n != size()
  hipError_t resize_exact(size_t n) { return n != n_ ? alloc(n) : hipSuccess; }
  // allocates when empty, never again
  hipError_t once(size_t n) { return p_ ? hipSuccess : alloc(n); }
  // grow() for the caller that has a fall-back: false on failure, and HIP's sticky error is cleared
  bool try_grow(size_t n) {
    if (grow(n) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
  }
  // a non-owning alias of o (the companion context's view of the shared weights): its destructor frees nothing
  void borrow(const DevBuf& o) { (void)reset(); p_ = o.p_; n_ = o.n_; owned_ = false; }
  hipError_t reset() {
    T* p = p_;
    const bool owned = owned_;
    p_ = nullptr; n_ = 0; owned_ = true;
    return p && owned ? hipFree(p) : hipSuccess;
  }

 private:
  void take(DevBuf& o) { p_ = o.p_; n_ = o.n_; owned_ = o.owned_; o.p_ = nullptr; o.n_ = 0; o.owned_ = true; }
  hipError_t alloc(size_t n) {
    hipError_t e = reset();
    if (e != hipSuccess) return e;
    e = hipMalloc((void**)&p_, sizeof(T) * n);
    if (e != hipSuccess) { p_ = nullptr; return e; }
    n_ = n;
    return hipSuccess;
  }
  T* p_ = nullptr;
  size_t n_ = 0;
  bool owned_ = true;
};

// The same for pinned host memory.  Allocated with hipHostMallocMapped it also keeps the device's view of the block.
template <class T>
class PinBuf {
 public:
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  PinBuf(PinBuf&& o) noexcept { take(o); }
  PinBuf& operator=(PinBuf&& o) noexcept {
    if (this != &o) { (void)reset(); take(o); }
    return *this;
  }
  ~PinBuf() { (void)reset(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  T* dev() const { return dev_; }   // the device view of a mapped block (null otherwise)
  size_t size() const { return n_; }

  hipError_t grow(size_t n, unsigned flags = 0) { return n > n_ ? alloc(n, flags) : hipSuccess; }
  hipError_t resize_exact(size_t n, unsigned flags = 0) { return n != n_ ? alloc(n, flags) : hipSuccess; }
  hipError_t once(size_t n, unsigned flags = 0) { return p_ ? hipSuccess : alloc(n, flags); }
  hipError_t reset() {
    T* p = p_;
    p_ = dev_ = nullptr; n_ = 0;
    return p ? hipHostFree(p) : hipSuccess;
  }

 private:
  void take(PinBuf& o) { p_ = o.p_; dev_ = o.dev_; n_ = o.n_; o.p_ = o.dev_ = nullptr; o.n_ = 0; }
  hipError_t alloc(size_t n, unsigned flags) {
    hipError_t e = reset();
    if (e != hipSuccess) return e;
    e = hipHostMalloc((void**)&p_, sizeof(T) * n, flags);
    if (e != hipSuccess) { p_ = nullptr; return e; }
    n_ = n;
    if (flags & hipHostMallocMapped) {
      e = hipHostGetDevicePointer((void**)&dev_, p_, 0);
      if (e != hipSuccess) { (void)reset(); return e; }
    }
    return hipSuccess;
  }
  T* p_ = nullptr;
  T* dev_ = nullptr;
  size_t n_ = 0;
};

// One event, destroyed if it was created.
class HipEvent {
 public:
  HipEvent() = default;
  HipEvent(const HipEvent&) = delete;
  HipEvent& operator=(const HipEvent&) = delete;
  ~HipEvent() { if (e_) (void)hipEventDestroy(e_); }
  hipError_t create() { return e_ ? hipSuccess : hipEventCreate(&e_); }
  hipError_t create(unsigned flags) { return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, flags); }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};
