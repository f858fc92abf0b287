// track_ctx.h -- the OSG tracking context and the interface between its front
// (track_host.hip: the C ABI, checks, host staging) and its two engines: the IQ
// stream engine (track.hip) and the I-only engine (track_real.hip).  Each engine
// is one plain function that launches one request on the context's stream.
// Internal to libgnsscorr.
#ifndef GNSSCORR_TRACK_CTX_H
#define GNSSCORR_TRACK_CTX_H
#include <hip/hip_runtime.h>
#include "gnsscorr_internal.h"
#include "hostctx.h"

constexpr int kMaxNsamp = 65536;   // samples of one call (track_real.hip: 1024 runs of 64)

struct gnsscorr_track_ctx {
  gnsscorr_track_cfg cfg;
  hipStream_t stream = nullptr;
  uint32_t* d_pk = nullptr;
  uint8_t* d_pk8 = nullptr;   // the same table as 2-bit E/P/L fields (unpack8)
  gnsscorr_chan_state* d_state = nullptr;
  gnsscorr_nco_cmd* d_cmds = nullptr;
  gnsscorr_track_result* d_res = nullptr;
  int32_t* d_dumps = nullptr;
  hostctx::DevBuf<int8_t> d_if;   // gnsscorr_track's staging, in bytes
  int max_dumps = 0;
  int64_t tic = 0, tic_ref = 0;
  int balance = 1;        // GNSSCORR_TRACK_BALANCE=0: no LDS padding for an even spread (A/B)
  int xcall_prefetch = 1;  // GNSSCORR_TRACK_XPF=0: no cross-call piece prefetch (A/B)
  int n_cu = 256;
  size_t lds_max = 0;     // LDS bytes a workgroup may allocate (gnsscorr_device_lds_bytes)
};

inline bool packed(const gnsscorr_track_ctx* c) { return (c->cfg.iq & GNSSCORR_IF_PACKED2) != 0; }
inline int bps_of(const gnsscorr_track_ctx* c) { return (c->cfg.iq & GNSSCORR_IF_IQ) ? 2 : 1; }

// ---- track.hip: osg_stream_kernel, n_calls consecutive calls of every channel in
// one launch (call k reads the IF at + k * nsamp samples of each stream and the
// commands at d_cmds + k * cmd_step; the results go to d_res + k * n_channels).
// tic: the first call's TIC sample (tic_explicit) or the TIC counter to step per
// call.  lcfg/d_loops: the closed loop, every channel's gpsisr step after each
// call.  Checks the call itself (gnsscorr_track_check_steps).  Returns
// GNSSCORR_TRACK_NOT_FUSED when the kernel does not serve the context (I-only
// streams) or the shape (alignment of the later calls of n_calls > 1); a single
// call of an IQ context is always served.
int track_stream_launch(gnsscorr_track_ctx* c, const int8_t* d_if, int64_t stride, int64_t nsamp,
                        int n_calls, gnsscorr_nco_cmd* d_cmds, int cmd_step,
                        gnsscorr_track_result* d_res, int32_t* d_dumps, int64_t tic,
                        int tic_explicit, const gnsscorr_osg_loop_cfg* lcfg,
                        gnsscorr_osg_loop* d_loops, gnsscorr_osg_loop* d_hist);

// ---- track_real.hip: osg_track_kernel, one checked call of an I-only context;
// tic: the call's TIC sample
int track_real_launch(gnsscorr_track_ctx* c, const int8_t* d_if, int64_t stride, int64_t nsamp,
                      const gnsscorr_nco_cmd* d_cmds, gnsscorr_track_result* d_res,
                      int32_t* d_dumps, int64_t tic);
#endif
