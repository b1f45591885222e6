// sg_buf.h -- the owners of what the library holds from HIP.  Buf is a device
// (or pinned host) block, pointer and capacity as one unit: every buffer of the
// library is one, grow-only or of one exact size; the capacity asked for is the
// caller's (grow_cap of sg_plan.h with the buffer's floor, or an exact size).
// Event and Stream own a handle each.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

#include "../../include/syzsig.h"

namespace sg {

int hip_fail(hipError_t e, const char* what);  // sg_ctx.hip
#define SG_HIP(call)                                     \
  do {                                                   \
    hipError_t e_ = (call);                              \
    if (e_ != hipSuccess) return ::sg::hip_fail(e_, #call); \
  } while (0)

// After a failed call the object holds a live block with its capacity or
// nothing, never a freed pointer, and no new block is left behind.
template <typename T, bool kPinned = false>
struct Buf {
  T* p = nullptr;
  size_t cap = 0;  // elements

  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { release(); }

  void swap(Buf& o) {
    std::swap(p, o.p);
    std::swap(cap, o.cap);
  }

  int release() {
    T* old = p;
    p = nullptr;
    cap = 0;
    const hipError_t e = !old ? hipSuccess : kPinned ? hipHostFree(old) : hipFree(old);
    return e == hipSuccess ? SG_OK : hip_fail(e, kPinned ? "hipHostFree" : "hipFree");
  }

  // At least `ncap` elements, the contents dropped.  A block that exists may
  // still be read or written by work in flight: `stream`, and `stream2` when
  // there is one (the host pipeline's copy stream, for the staging buffers),
  // are waited for before it is freed.
  int grow_drop(size_t ncap, hipStream_t stream, hipStream_t stream2 = nullptr) {
    if (ncap <= cap) return SG_OK;
    if (p) {
      SG_HIP(hipStreamSynchronize(stream));
      if (stream2) SG_HIP(hipStreamSynchronize(stream2));
      const int rc = release();
      if (rc) return rc;
    }
    return alloc(ncap);
  }

  // At least `ncap` elements, the first `keep` kept: copied on `stream` into
  // the new block, which is adopted only once the copy has been waited for.
  int grow_keep(size_t ncap, size_t keep, hipStream_t stream) {
    static_assert(!kPinned, "only device blocks are grown with their contents");
    if (ncap <= cap) return SG_OK;
    Buf nb;
    const int rc = nb.alloc(ncap);
    if (rc) return rc;
    if (p && keep) SG_HIP(hipMemcpyAsync(nb.p, p, keep * sizeof(T), hipMemcpyDeviceToDevice, stream));
    SG_HIP(hipStreamSynchronize(stream));
    swap(nb);
    return nb.release();
  }

 private:
  // (of an empty object)
  int alloc(size_t n) {
    const hipError_t e = kPinned ? hipHostMalloc((void**)&p, n * sizeof(T), hipHostMallocDefault)
                                 : hipMalloc((void**)&p, n * sizeof(T));
    if (e != hipSuccess) {
      p = nullptr;
      return hip_fail(e, kPinned ? "hipHostMalloc" : "hipMalloc");
    }
    cap = n;
    return SG_OK;
  }
};
template <typename T>
using DevBuf = Buf<T>;
using PinBuf = Buf<char, true>;

// The owner of an event or of a stream: made once by create (nothing when it
// exists), passed as the handle it holds, destroyed with its owner.
template <typename H, hipError_t (*kCreate)(H*, unsigned), hipError_t (*kDestroy)(H)>
struct Handle {
  H h = nullptr;
  Handle() = default;
  Handle(const Handle&) = delete;
  Handle& operator=(const Handle&) = delete;
  ~Handle() {
    if (h) (void)kDestroy(h);
  }
  int create(unsigned flags) {
    const hipError_t e = h ? hipSuccess : kCreate(&h, flags);
    return e == hipSuccess ? SG_OK : hip_fail(e, "creating an event or a stream");
  }
  operator H() const { return h; }
};
using Event = Handle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;

}  // namespace sg
