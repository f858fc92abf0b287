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
//  - A Staging belongs to one host-array call, the twin of a *_dev call, and
//    owns the device copies of that call's host arrays: up to kMaxBlocks blocks,
//    each from a hipMalloc of its own, freed on every path out of the scope that
//    declares it.  hipFree waits for the device, so copies and kernels still
//    queued on a block at an early return finish first.  in() queues the upload
//    as it allocates; out() and inout() remember the host array, and finish()
//    queues those downloads in the order they were declared and synchronises the
//    stream.  The first failing call makes status() sticky: later in / out /
//    inout calls do nothing and return null, so the twin tests status() once,
//    before it hands the pointers to the *_dev call.  The host arrays stay the
//    caller's; only finish() writes to them.
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

// the device copies of one host-array call's arguments, on the context's stream:
//   Staging st(c->stream);
//   const T* d_x = st.in(h_x, n);  U* d_y = st.out(h_y, m);
//   if (st.status()) return st.status();
//   rc = ..._dev(c, d_x, ..., d_y);
//   return rc ? rc : st.finish();
// n counts elements and may be 0: the block is still a valid device pointer, and
// nothing is copied either way.  A block is the call's own copy, so in() hands
// it out non-const as well.
class Staging {
 public:
  static constexpr int kMaxBlocks = 8;
  explicit Staging(hipStream_t stream) : stream_(stream) {}
  Staging(const Staging&) = delete;
  Staging& operator=(const Staging&) = delete;
  ~Staging() {
    for (int i = 0; i < n_; i++) (void)hipFree(blk_[i].d);
  }

  template <class T>
  T* in(const T* h, size_t n) { return (T*)stage(h, nullptr, n * sizeof(T)); }
  template <class T>
  T* out(T* h, size_t n) { return (T*)stage(nullptr, h, n * sizeof(T)); }
  template <class T>
  T* inout(T* h, size_t n) { return (T*)stage(h, h, n * sizeof(T)); }

  int status() const { return rc_; }

  // the downloads in declaration order, then one synchronise
  int finish() {
    if (rc_) return rc_;
    for (int i = 0; i < n_; i++)
      if (blk_[i].h_out && blk_[i].bytes)
        HIP_TRY(hipMemcpyAsync(blk_[i].h_out, blk_[i].d, blk_[i].bytes, hipMemcpyDeviceToHost,
                               stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    return GNSSCORR_OK;
  }

 private:
  struct Block {
    void* d;
    void* h_out;     // null: nothing to download
    size_t bytes;
  };

  void* stage(const void* h_in, void* h_out, size_t bytes) {
    void* d = nullptr;
    if (!rc_) rc_ = add(h_in, h_out, bytes, &d);
    return rc_ ? nullptr : d;
  }
  int add(const void* h_in, void* h_out, size_t bytes, void** d) {
    if (n_ == kMaxBlocks) {
      gnsscorr_set_error("hostctx::Staging: more than %d blocks in one call", kMaxBlocks);
      return GNSSCORR_EINVAL;
    }
    HIP_TRY(hipMalloc(d, bytes ? bytes : 1));
    blk_[n_++] = Block{*d, h_out, bytes};        // owned from here on
    if (h_in && bytes) HIP_TRY(hipMemcpyAsync(*d, h_in, bytes, hipMemcpyHostToDevice, stream_));
    return GNSSCORR_OK;
  }

  hipStream_t stream_;
  Block blk_[kMaxBlocks];
  int n_ = 0;
  int rc_ = GNSSCORR_OK;
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
