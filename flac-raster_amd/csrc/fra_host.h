// fra_host.h -- host-only helpers shared by the plan / execute / host-path code, fra_decode_dev.hip and the units over
// fra_region.h: the error setter, HIPCHK, elem_size, one owner of HIP resources (HipArena) and a call's stream and
// arena (Call).  Compiled by g++ (no HIP) it offers the first and the third only (fra_layout.h); nothing here needs
// more of the library than fra_internal_set_error and, for Call, fra_internal_ctx_stream, which the stand-alone check
// programs under tools/ define themselves.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/flac_raster_amd.h"

// sets the calling thread's fra_last_error() message and returns `code` (fra_api.hip)
extern "C" int fra_internal_set_error(int code, const char* fmt, ...);

inline int elem_size(int dt) {
  switch (dt) {
    case FRA_U8: case FRA_I8: return 1;
    case FRA_U16: case FRA_I16: return 2;
    case FRA_U32: case FRA_I32: case FRA_F32: return 4;
    case FRA_F64: return 8;
  }
  return 0;
}

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#define HIPCHK(x)                                                                                                  \
  do {                                                                                                             \
    hipError_t _e = (x);                                                                                           \
    if (_e != hipSuccess)                                                                                          \
      return fra_internal_set_error(_e == hipErrorOutOfMemory ? FRA_E_NOMEM : FRA_E_HIP, "%s: %s (%s:%d)", #x,     \
                                    hipGetErrorString(_e), __FILE__, __LINE__);                                    \
  } while (0)

// Owner of device memory, page-locked memory, streams and events: whatever was made through it is released when it
// goes out of scope, on every path (the device that made them must be current).  The pointers and handles it hands
// out are plain views.  Move-only.
struct HipArena {
  HipArena() = default;
  HipArena(const HipArena&) = delete;
  HipArena& operator=(const HipArena&) = delete;
  HipArena(HipArena&& o) noexcept { swap(o); }
  HipArena& operator=(HipArena&& o) noexcept { swap(o); return *this; }  // (o releases what this held)
  ~HipArena() {
    for (void* p : dev_) (void)hipFree(p);
    for (void* p : pinned_) (void)hipHostFree(p);
    for (auto s : streams_) (void)hipStreamDestroy(s);
    for (auto e : events_) (void)hipEventDestroy(e);
  }
  // `bytes` of device memory (at least one), ... zero-filled, ... holding a copy of host memory
  template <typename T>
  hipError_t alloc(T** p, size_t bytes) { return keep(dev_, p, hipMalloc((void**)p, bytes ? bytes : 1)); }
  template <typename T>
  hipError_t alloc_zero(T** p, size_t bytes) {
    const hipError_t e = alloc(p, bytes);
    return e == hipSuccess ? hipMemset((void*)*p, 0, bytes ? bytes : 1) : e;
  }
  template <typename T>
  hipError_t upload(T** p, const void* host, size_t bytes) {
    const hipError_t e = alloc(p, bytes);
    return e == hipSuccess && bytes ? hipMemcpy((void*)*p, host, bytes, hipMemcpyHostToDevice) : e;
  }
  template <typename T>
  hipError_t pinned(T** p, size_t bytes, unsigned flags) {
    return keep(pinned_, p, hipHostMalloc((void**)p, bytes, flags));
  }
  // a non-blocking stream, at the default priority or a given one
  hipError_t stream(hipStream_t* s) { return keep(streams_, s, hipStreamCreateWithFlags(s, hipStreamNonBlocking)); }
  hipError_t stream(hipStream_t* s, int priority) {
    return keep(streams_, s, hipStreamCreateWithPriority(s, hipStreamNonBlocking, priority));
  }
  hipError_t event(hipEvent_t* ev, unsigned flags = hipEventDisableTiming) {
    return keep(events_, ev, hipEventCreateWithFlags(ev, flags));
  }

 private:
  template <typename V, typename T>
  static hipError_t keep(V& owned, T* made, hipError_t e) {
    if (e == hipSuccess) owned.push_back((typename V::value_type)*made);
    else *made = nullptr;
    return e;
  }
  void swap(HipArena& o) {
    dev_.swap(o.dev_);
    pinned_.swap(o.pinned_);
    streams_.swap(o.streams_);
    events_.swap(o.events_);
  }
  std::vector<void*> dev_, pinned_;
  std::vector<hipStream_t> streams_;
  std::vector<hipEvent_t> events_;
};

// the context's device and stream (fra_api.hip)
extern "C" void fra_internal_ctx_stream(fra_ctx* ctx, int* device, hipStream_t* stream);

// A call's stream, on its context's device, and the owner of what the call makes: staging buffers, tables, partials,
// reports and events are released on every path.
struct Call {
  hipStream_t s = nullptr;
  HipArena sc;
  explicit Call(fra_ctx* ctx) {
    int device = 0;
    fra_internal_ctx_stream(ctx, &device, &s);
    (void)hipSetDevice(device);
  }
};
#endif  // __HIPCC__
