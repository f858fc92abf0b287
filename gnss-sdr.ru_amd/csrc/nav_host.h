// nav_host.h -- what navsym.hip, navbits.hip, navfix.hip, navglo.hip and navb1.hip share on the host: the "nav"
// context, the refusal text and the checks of a series argument.  HIP only;
// include after gnsscorr_internal.h and hostctx.h.
#ifndef GNSSCORR_NAV_HOST_H
#define GNSSCORR_NAV_HOST_H
#include <stdint.h>
#include "gnsscorr_internal.h"
#include "hostctx.h"

struct gnsscorr_nav_ctx {
  struct { int device; } cfg;
  hipStream_t stream = nullptr;
  // work buffers of the *_dev calls.  grow() frees the old block with hipFree,
  // which waits for launches still queued on it.
  // navsym.hip: the decoder's input symbols and the length of each of its streams
  hostctx::DevBuf<uint8_t> d_code;
  hostctx::DevBuf<int32_t> d_len;
  // navbits.hip: the hit bitmap of the GPS search, one bit per epoch
  hostctx::DevBuf<uint64_t> d_hitmap;
  // navfix.hip, navglo.hip, navb1.hip: the receivers' channel offsets of the last *_fix call
  hostctx::DevBuf<int32_t> d_rx_first;
};

namespace navhost {

inline int bad_arguments(const char* fn, const char* what) {
  gnsscorr_set_error("%s: bad arguments (%s)", fn, what);
  return GNSSCORR_EINVAL;
}

// the checks the series entry points share
inline int check_series(const char* fn, const gnsscorr_nav_ctx* c, const void* series,
                        int64_t epoch_stride, int64_t chan_stride, int n_epochs, int n_ch) {
  if (!c || !series) return bad_arguments(fn, "null pointer");
  if (n_epochs < 1 || n_ch < 1) return bad_arguments(fn, "n_epochs >= 1, n_ch >= 1");
  if (epoch_stride < 8 || chan_stride < 8) return bad_arguments(fn, "a stride smaller than 8");
  if (((uintptr_t)series & 7) || (epoch_stride & 7) || (chan_stride & 7))
    return bad_arguments(fn, "fp64 fields: 8-byte aligned pointer and strides");
  return GNSSCORR_OK;
}

// bytes from the first channel's first epoch to the end of the last one's last
inline size_t series_bytes(int64_t epoch_stride, int64_t chan_stride, int n_epochs, int n_ch) {
  return (size_t)(n_ch - 1) * chan_stride + (size_t)(n_epochs - 1) * epoch_stride + 8;
}

}  // namespace navhost
#endif
