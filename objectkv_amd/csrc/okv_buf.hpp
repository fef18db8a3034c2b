// okv_buf.hpp -- the one owning type of every scratch allocation (device and
// pinned host).  Internal header; it includes no HIP header itself.
//
// Invariant, after every return (error returns included): either
// data() == nullptr and capacity() == 0, or data() is a live allocation of at
// least capacity() elements.  The destructor releases.
//
// Mem says where the memory comes from:
//   using Error;   value-initialised = success, anything else converts to true
//   using Stream;  what must be idle before an allocation in use is released
//   static Error alloc(void** p, size_t bytes);
//   static void release(void* p);
//   static Error idle(Stream s);
//   static Error copy(void* dst, const void* src, size_t bytes, Stream s);
//     (reserve_keep only: enqueue on s)
#pragma once
#include <cstddef>

namespace okv {

template <class T, class Mem>
class Buf {
 public:
  using Error = typename Mem::Error;
  using Stream = typename Mem::Stream;

  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, cap_ = o.cap_;
      o.p_ = nullptr, o.cap_ = 0;
    }
    return *this;
  }
  ~Buf() { reset(); }

  T* data() const { return p_; }
  T* operator->() const { return p_; }
  T& operator*() const { return *p_; }
  size_t capacity() const { return cap_; }              // elements
  size_t bytes() const { return cap_ * sizeof(T); }     // of the whole allocation

  void reset() {
    if (p_) Mem::release(p_);
    p_ = nullptr, cap_ = 0;
  }

  // Room for n elements; the contents are not kept.  Enough room already: a
  // compare, no call.  Otherwise: s idle, the old allocation released, a new
  // one of n elements rounded up to 4 KiB (no geometric growth), then the new
  // capacity; *fresh = true (zero-once buffers are zeroed again then).  A
  // failed allocation leaves the buffer empty.  An empty buffer allocates for
  // n == 0 too, so data() is never null after success.
  Error reserve(Stream s, size_t n, bool* fresh = nullptr) {
    if (n <= cap_ && p_) return Error{};
    return grow(s, n, fresh);
  }

  // reserve() that keeps the first `keep` elements across a growth (copied on
  // s, which is idle on return).  A failure leaves the old allocation.
  Error reserve_keep(Stream s, size_t n, size_t keep) {
    if (n <= cap_ && p_) return Error{};
    if (!p_ || !keep) return grow(s, n, nullptr);
    const size_t bytes = round(n);
    void* q = nullptr;
    if (Error e = Mem::alloc(&q, bytes)) return e;
    Error e = Mem::copy(q, p_, keep * sizeof(T), s);
    if (!e) e = Mem::idle(s);
    if (e) {
      Mem::release(q);
      return e;
    }
    Mem::release(p_);
    p_ = static_cast<T*>(q);
    cap_ = bytes / sizeof(T);
    return Error{};
  }

 private:
  static size_t round(size_t n) { return ((n ? n : 1) * sizeof(T) + 4095) & ~size_t(4095); }

  Error grow(Stream s, size_t n, bool* fresh) {
    if (p_) {
      if (Error e = Mem::idle(s)) return e;  // (still in use: the old allocation stays)
      reset();
    }
    const size_t bytes = round(n);
    void* q = nullptr;
    if (Error e = Mem::alloc(&q, bytes)) return e;
    p_ = static_cast<T*>(q);
    cap_ = bytes / sizeof(T);
    if (fresh) *fresh = true;
    return Error{};
  }

  T* p_ = nullptr;
  size_t cap_ = 0;
};

#ifdef OKV_BUF_HIP  // the includer has included <hip/hip_runtime.h>
struct DeviceMem {
  using Error = hipError_t;
  using Stream = hipStream_t;
  static Error alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void release(void* p) { (void)hipFree(p); }
  static Error idle(Stream s) { return hipStreamSynchronize(s); }
  static Error copy(void* dst, const void* src, size_t bytes, Stream s) {
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s);
  }
};
struct PinnedMem {
  using Error = hipError_t;
  using Stream = hipStream_t;
  static Error alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void release(void* p) { (void)hipHostFree(p); }
  static Error idle(Stream s) { return hipStreamSynchronize(s); }
};
template <class T>
using DevBuf = Buf<T, DeviceMem>;
template <class T>
using PinBuf = Buf<T, PinnedMem>;
#endif

}  // namespace okv
