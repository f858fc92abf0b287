// hostctx.h -- the host scaffolding every context family shares: opening the
// device at create, device buffers that grow, release lists, destroy, sync and
// stream.  HIP only; include after gnsscorr_internal.h.  None of it runs on a
// hot path.
//
// Ownership:
//  - A context owns every device buffer its struct names, fixed ones as raw
//    pointers and growable ones as DevBuf.  They are freed exactly once, by the
//    family's release list inside destroy(), which runs after the context's
//    stream has drained and before the stream is destroyed.  release() nulls
//    what it frees, so a second release of the same member is a no-op.
//  - grow() keeps a buffer that is large enough and otherwise replaces it; the
//    old contents are lost.  A failed growth leaves {nullptr, 0}: the old block
//    is already freed, nothing dangles, and a later grow() starts from scratch.
//    Work queued on the old block must have finished before grow() is called;
//    the host wrappers that use it end in a stream synchronise.
//  - A TempBuf belongs to the scope that declares it and is freed on every
//    path out of that scope.  hipFree waits for the device, so copies and
//    kernels still queued on the buffer at an early return finish first.
//  - create() builds the context and then runs the family's init helper, which
//    returns early on the first failing HIP call (HIP_TRY: the call's own error
//    string, GNSSCORR_EDEVICE) or host allocation (GNSSCORR_ENOMEM).  A failed
//    init goes through the family's destroy, which releases the half-built
//    context.
#ifndef GNSSCORR_HOSTCTX_H
#define GNSSCORR_HOSTCTX_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "gnsscorr_internal.h"

namespace hostctx {

// fn: the exported create function's name, for its error texts.  Leaves the
// device current.
inline int open_device(const char* fn, int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    gnsscorr_set_error("%s: no HIP device", fn);
    return GNSSCORR_ENODEV;
  }
  if (device < 0 || device >= ndev) {
    gnsscorr_set_error("%s: device %d out of range", fn, device);
    return GNSSCORR_EINVAL;
  }
  HIP_TRY(hipSetDevice(device));
  return GNSSCORR_OK;
}

// a device buffer and the number of elements it has room for
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
};

// free and null any mix of raw device pointers and DevBufs
template <class T>
void release_one(T*& p) {
  (void)hipFree((void*)p);
  p = nullptr;
}
template <class T>
void release_one(DevBuf<T>& b) {
  release_one(b.p);
  b.cap = 0;
}
template <class... Bufs>
void release(Bufs&... bufs) { (release_one(bufs), ...); }

// room for n elements (contents lost); a failed growth leaves {nullptr, 0}
template <class T>
int grow(DevBuf<T>& b, size_t n) {
  if (n <= b.cap) return GNSSCORR_OK;
  release(b);
  HIP_TRY(hipMalloc(&b.p, n * sizeof(T)));
  b.cap = n;
  return GNSSCORR_OK;
}

// a device buffer that lives for one host call
template <class T>
struct TempBuf : DevBuf<T> {
  TempBuf() = default;
  TempBuf(const TempBuf&) = delete;
  TempBuf& operator=(const TempBuf&) = delete;
  ~TempBuf() { release(*this); }
};

// Ctx below: any context with cfg.device and stream.

// release_buffers: the family's release list
template <class Ctx, class ReleaseBuffers>
int destroy(Ctx* c, const ReleaseBuffers& release_buffers) {
  if (!c) return GNSSCORR_OK;
  (void)hipSetDevice(c->cfg.device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  release_buffers();
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return GNSSCORR_OK;
}

template <class Ctx>
int sync(Ctx* c) {
  if (!c) return GNSSCORR_EINVAL;
  HIP_TRY(hipSetDevice(c->cfg.device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return GNSSCORR_OK;
}

template <class Ctx>
void* stream(Ctx* c) { return c ? (void*)c->stream : nullptr; }

}  // namespace hostctx
#endif
