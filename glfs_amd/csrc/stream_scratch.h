// stream_scratch.h -- what the launch layer (post_kernels.hip) keeps per
// (device, stream) between launches: owning buffers and their registry.
// HIP runtime API only; no kernels.  Not host::DevBuf / PinBuf (host.h): those
// report through fail() and int, free without draining a stream and use other
// hipHostMalloc flags, and the launch layer returns hipError_t.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <utility>
#include <vector>

namespace glfsx {

// The device stream s belongs to (the current device for the null stream),
// current for the scope.  The scratch slots are keyed by (device, stream)
// and allocated on the current device; a caller driving several GPUs may
// reach here with another device current than its stream's (a
// multi-device Writer checked a lane's error word under the wrong device
// and missed it), so the stream, not the thread, names the device.
struct StreamDevice {
  int dev = 0, prev = 0;
  hipError_t e = hipSuccess;
  explicit StreamDevice(hipStream_t s) {
    e = hipGetDevice(&prev);
    if (e != hipSuccess) return;
    dev = prev;
    hipDevice_t d = 0;
    if (s && hipStreamGetDevice(s, &d) == hipSuccess) dev = d;
    if (dev != prev) e = hipSetDevice(dev);
  }
  ~StreamDevice() {
    if (dev != prev) (void)hipSetDevice(prev);
  }
};

// Device memory used by the launches of one stream.  It only grows, by
// discard and reallocate (no caller relies on old contents): launches on one
// stream are ordered, so the old allocation is free once the stream drains.
struct StreamBuf {
  void *p = nullptr;
  size_t cap = 0;  // bytes at p

  StreamBuf() = default;
  StreamBuf(StreamBuf &&o) noexcept
      : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  StreamBuf &operator=(StreamBuf &&o) noexcept {
    if (this != &o) {
      reset();
      p = std::exchange(o.p, nullptr);
      cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~StreamBuf() { reset(); }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T *as() const { return static_cast<T *>(p); }

  // At least `bytes` at p afterwards.  A new allocation has max(bytes +
  // bytes / headroom_div (0: none), floor) bytes, zeroed on s when `zero`.
  // On failure the buffer is empty.
  hipError_t ensure(hipStream_t s, size_t bytes, size_t floor, size_t headroom_div, bool zero) {
    if (cap >= bytes) return hipSuccess;
    if (p) {
      hipError_t e = hipStreamSynchronize(s);
      if (e != hipSuccess) return e;
      reset();
    }
    const size_t want = std::max(bytes + (headroom_div ? bytes / headroom_div : 0), floor);
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    cap = want;
    if (zero && (e = hipMemsetAsync(p, 0, want, s)) != hipSuccess) reset();
    return e;
  }
};

// 64 bytes of pinned coherent host memory, zero when made, and the address
// the kernels reach them at: both set or both null.
struct PinnedBlock {
  void *h = nullptr, *d = nullptr;

  PinnedBlock() = default;
  PinnedBlock(PinnedBlock &&o) noexcept
      : h(std::exchange(o.h, nullptr)), d(std::exchange(o.d, nullptr)) {}
  PinnedBlock &operator=(PinnedBlock &&o) noexcept {
    if (this != &o) {
      reset();
      h = std::exchange(o.h, nullptr);
      d = std::exchange(o.d, nullptr);
    }
    return *this;
  }
  ~PinnedBlock() { reset(); }
  void reset() {
    if (h) (void)hipHostFree(h);
    h = d = nullptr;
  }
  hipError_t ensure() {
    if (h) return hipSuccess;
    void *hp = nullptr, *dp = nullptr;
    hipError_t e = hipHostMalloc(&hp, 64, hipHostMallocCoherent);
    if (e != hipSuccess) return e;
    e = hipHostGetDevicePointer(&dp, hp, 0);
    if (e != hipSuccess) {
      (void)hipHostFree(hp);
      return e;
    }
    memset(hp, 0, 64);
    h = hp;
    d = dp;
    return hipSuccess;
  }
};

// One T per (device, stream).  Every call is made with the caller's lock
// held and the slot's device current (StreamDevice); a T * stays valid until
// its slot is released.
template <class T>
class StreamRegistry {
  struct Entry {
    int dev;
    hipStream_t stream;
    std::unique_ptr<T> slot;
  };
  std::vector<Entry> v_;

 public:
  T *find(int dev, hipStream_t s) const {
    for (const Entry &x : v_)
      if (x.dev == dev && x.stream == s) return x.slot.get();
    return nullptr;
  }
  T *find_or_make(int dev, hipStream_t s) {
    if (T *t = find(dev, s)) return t;
    v_.push_back(Entry{dev, s, std::make_unique<T>()});
    return v_.back().slot.get();
  }
  // Destroys the slot, which frees what it owns.  A slot of the same stream
  // handle on another device is another stream's: left alone.
  void release(int dev, hipStream_t s) {
    for (size_t i = 0; i < v_.size(); ++i)
      if (v_[i].dev == dev && v_[i].stream == s) {
        std::swap(v_[i], v_.back());
        v_.pop_back();
        return;
      }
  }
  size_t size() const { return v_.size(); }
};

}  // namespace glfsx
