// track_host.hip -- the front of the OSG tracking correlator: the context, the
// alignment checks, host staging and the C ABI.  The kernels are behind
// track_ctx.h: the IQ stream engine (track.hip) and the I-only engine
// (track_real.hip).
#include <hip/hip_runtime.h>
#include <vector>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gnsscorr_internal.h"
#include "hostctx.h"
#include "if2.h"
#include "osg_chan.h"
#include "track_ctx.h"

extern "C" int gnsscorr_track_iq(const gnsscorr_track_ctx* ctx) { return ctx && (ctx->cfg.iq & GNSSCORR_IF_IQ); }
// bytes of `samples` consecutive samples of one stream in the context's format
extern "C" int64_t gnsscorr_track_if_bytes(const gnsscorr_track_ctx* c, int64_t samples) {
  return if_bytes(samples * bps_of(c), packed(c));
}

static int set_dev(int dev) {
  HIP_TRY(hipSetDevice(dev));
  return GNSSCORR_OK;
}

// the stream, the device buffers and the code tables on them
static int init_device(gnsscorr_track_ctx* c) {
  const int C = c->cfg.n_channels;
  HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  HIP_TRY(hipMalloc(&c->d_pk, sizeof(uint32_t) * GNSSCORR_OSG_PK_LEN));
  HIP_TRY(hipMalloc(&c->d_pk8, GNSSCORR_OSG_PK_LEN + 64));   // +64: whole-dword row staging
  HIP_TRY(hipMalloc(&c->d_state, sizeof(gnsscorr_chan_state) * C));
  HIP_TRY(hipMalloc(&c->d_cmds, sizeof(gnsscorr_nco_cmd) * C));
  HIP_TRY(hipMalloc(&c->d_res, sizeof(gnsscorr_track_result) * C));
  HIP_TRY(hipMalloc(&c->d_dumps, sizeof(int32_t) * 6 * (size_t)C * c->max_dumps));
  std::vector<uint32_t> pk(GNSSCORR_OSG_PK_LEN);
  gnsscorr_osg_packed_table(pk.data());
  HIP_TRY(hipMemcpy(c->d_pk, pk.data(), sizeof(uint32_t) * GNSSCORR_OSG_PK_LEN,
                    hipMemcpyHostToDevice));
  // pack8: each int8 bit (-1 / 0 / +1) of {late, prompt, early} as a 2-bit field
  std::vector<uint8_t> pk8(GNSSCORR_OSG_PK_LEN);
  for (int i = 0; i < GNSSCORR_OSG_PK_LEN; i++) {
    uint32_t b = 0;
    for (int k = 0; k < 3; k++) b |= ((uint32_t)(int8_t)(pk[i] >> (8 * k)) & 3u) << (2 * k);
    pk8[i] = (uint8_t)b;
  }
  HIP_TRY(hipMemset(c->d_pk8, 0, GNSSCORR_OSG_PK_LEN + 64));
  HIP_TRY(hipMemcpy(c->d_pk8, pk8.data(), GNSSCORR_OSG_PK_LEN, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(c->d_state, 0, sizeof(gnsscorr_chan_state) * C));
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_track_create(gnsscorr_track_ctx** out, const gnsscorr_track_cfg* cfg) {
  if (!out || !cfg || cfg->n_channels < 1 || cfg->max_nsamp < 1 || cfg->max_nsamp > kMaxNsamp ||
      (cfg->iq & ~(GNSSCORR_IF_IQ | GNSSCORR_IF_PACKED2))) {
    gnsscorr_set_error("gnsscorr_track_create: bad config (n_channels>=1, 1<=max_nsamp<=%d, "
                       "iq = GNSSCORR_IF_* flags)", kMaxNsamp);
    return GNSSCORR_EINVAL;
  }
  *out = nullptr;
  int rc = hostctx::open_device(__func__, cfg->device);
  if (rc) return rc;
  auto* c = new gnsscorr_track_ctx();
  c->cfg = *cfg;
  c->lds_max = (size_t)gnsscorr_device_lds_bytes(cfg->device);
  c->max_dumps = osgchan::epoch_cap(cfg->max_nsamp);
  c->tic_ref = (int64_t)(cfg->samp_rate * cfg->tic_period);
  c->tic = c->tic_ref;
  if (const char* e = getenv("GNSSCORR_TRACK_BALANCE")) c->balance = atoi(e) != 0;
  if (const char* e = getenv("GNSSCORR_TRACK_XPF")) c->xcall_prefetch = atoi(e) != 0;
  if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, cfg->device) !=
          hipSuccess || c->n_cu < 1)
    c->n_cu = 256;
  rc = init_device(c);
  if (rc) {
    gnsscorr_track_destroy(c);
    return rc;
  }
  *out = c;
  return GNSSCORR_OK;
}

// Layout hint (round 2: per-channel LDS staging for one stream per channel).
// Neither kernel needs it: osg_stream_kernel gives every channel its own
// wavefront and IF pieces whatever the layout, and osg_track_kernel's threads
// read their runs from global memory.  The hint is validated and has no effect.
extern "C" int gnsscorr_track_set_layout(gnsscorr_track_ctx* c, int one_stream_per_channel) {
  if (!c || one_stream_per_channel < 0 || one_stream_per_channel > 1) {
    gnsscorr_set_error("gnsscorr_track_set_layout: bad arguments");
    return GNSSCORR_EINVAL;
  }
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_track_destroy(gnsscorr_track_ctx* c) {
  return hostctx::destroy(c, [&] {
    hostctx::release(c->d_pk, c->d_pk8, c->d_state, c->d_cmds, c->d_res, c->d_dumps, c->d_if);
  });
}

extern "C" int gnsscorr_track_max_dumps(const gnsscorr_track_ctx* c) { return c ? c->max_dumps : 0; }

extern "C" int64_t gnsscorr_track_next_tic(gnsscorr_track_ctx* c, int64_t nsamp) {
  // correlator.c:155-165
  if (c->tic < nsamp) {
    const int64_t t = c->tic;
    c->tic += c->tic_ref - nsamp;
    return t;
  }
  c->tic -= nsamp;
  return -1;
}

// nsamp and the IF alignment of one call (gnsscorr.h, "IF alignment of the
// device calls"); launches nothing and changes nothing.  step: the call's index
// in a multi-step request, named in the error text (-1: a single call).
//   IQ int8      16-byte base and stream stride (LDS-DMA chunks of 16 bytes)
//   IQ packed    8-byte base and stream stride (packed runs are read in 8-byte words)
//   I-only int8  16-byte base and stream stride (osg_track_kernel's int4 loads)
//   I-only packed any base, whole-byte stream stride (osg_track_kernel<true>
//                reads its runs byte by byte, and a run starts on a multiple of
//                64 elements of its stream)
static int check_call(const gnsscorr_track_ctx* c, const int8_t* d_if, int64_t stride,
                      int64_t nsamp, int step) {
  if (nsamp < 1 || nsamp > c->cfg.max_nsamp) {
    gnsscorr_set_error("nsamp %lld outside [1, max_nsamp=%d]", (long long)nsamp, c->cfg.max_nsamp);
    return GNSSCORR_EINVAL;
  }
  const int bps = bps_of(c);
  const bool pk = packed(c), iq = bps == 2;
  const int base_al = pk ? (iq ? 8 : 1) : 16;
  const int stride_al = base_al;   // bytes
  const int64_t stride_elems = stride * bps;
  // packed: four elements per byte, so the stride and a later step's offset
  // must be whole bytes before their alignment means anything
  const bool whole = !pk || (((stride_elems | (step > 0 ? step * nsamp * bps : 0)) & 3) == 0);
  if (((uintptr_t)d_if & (uintptr_t)(base_al - 1)) || !whole ||
      (if_bytes(stride_elems, pk) & (stride_al - 1))) {
    char at[96] = "";
    if (step >= 0) snprintf(at, sizeof at, "step %d (IF at element offset %lld): ", step,
                            (long long)((int64_t)step * nsamp * bps));
    gnsscorr_set_error("%s%s %s IF needs a %d-byte aligned base and a stream stride of whole "
                       "%d-byte units%s", at, iq ? "IQ" : "I-only", pk ? "packed" : "int8", base_al,
                       stride_al, pk ? " (4 elements per byte)" : "");
    return GNSSCORR_EINVAL;
  }
  return GNSSCORR_OK;
}

// Every step of a multi-step request (step k reads the IF at + k * nsamp
// samples) before any of them runs: a refused request leaves the channel
// state, the TIC counter and the result arrays as they were.
extern "C" int gnsscorr_track_check_steps(const gnsscorr_track_ctx* c, const int8_t* d_if,
                                          int64_t stride, int64_t nsamp, int n_steps) {
  for (int k = 0; k < n_steps; k++)
    if (int rc = check_call(c, d_if + gnsscorr_track_if_bytes(c, (int64_t)k * nsamp), stride, nsamp,
                            n_steps > 1 ? k : -1))
      return rc;
  return GNSSCORR_OK;
}

// one call on the engine of the context's streams
static int launch(gnsscorr_track_ctx* c, const int8_t* d_if, int64_t stride, int64_t nsamp,
                  const gnsscorr_nco_cmd* d_cmds, gnsscorr_track_result* d_res,
                  int32_t* d_dumps, int64_t tic_count) {
  if (int rc = check_call(c, d_if, stride, nsamp, -1)) return rc;
  if (bps_of(c) == 2)   // (one call of an IQ context is never GNSSCORR_TRACK_NOT_FUSED)
    return track_stream_launch(c, d_if, stride, nsamp, 1, const_cast<gnsscorr_nco_cmd*>(d_cmds), 0,
                               d_res, d_dumps, tic_count, 1, nullptr, nullptr, nullptr);
  return track_real_launch(c, d_if, stride, nsamp, d_cmds, d_res, d_dumps, tic_count);
}

extern "C" int gnsscorr_track(gnsscorr_track_ctx* c, const int8_t* h_if, int64_t stride,
                              int n_streams, int64_t nsamp, const gnsscorr_nco_cmd* h_cmds,
                              gnsscorr_track_result* h_res, int32_t* h_all_dumps, int* tic_fired) {
  if (!c || !h_if || !h_cmds || !h_res || n_streams < 1 || nsamp < 1) {
    gnsscorr_set_error("gnsscorr_track: bad arguments");
    return GNSSCORR_EINVAL;
  }
  const int C = c->cfg.n_channels;
  for (int i = 0; i < C; i++) {
    if (h_cmds[i].prn < 0 || h_cmds[i].prn > 32 || h_cmds[i].stream < 0 ||
        h_cmds[i].stream >= n_streams) {
      gnsscorr_set_error("gnsscorr_track: channel %d: prn %d / stream %d invalid", i,
                         h_cmds[i].prn, h_cmds[i].stream);
      return GNSSCORR_EINVAL;
    }
  }
  if (n_streams == 1) stride = 0;
  if (n_streams > 1 && stride < nsamp) {
    gnsscorr_set_error("gnsscorr_track: stream_stride < nsamp");
    return GNSSCORR_EINVAL;
  }
  int rc = set_dev(c->cfg.device);
  if (rc) return rc;
  const int bps = bps_of(c);
  const bool pk = packed(c);
  if (pk && n_streams > 1 && (stride * bps) & 3) {
    gnsscorr_set_error("gnsscorr_track: packed streams need a whole-byte stream stride");
    return GNSSCORR_EINVAL;
  }
  // device copy with an aligned stride (16 int8 bytes / 8 packed bytes = 32 elements)
  const int64_t al = pk ? 32 : 16;
  const int64_t dstride = n_streams > 1 ? ((stride * bps + al - 1) & ~(al - 1)) / bps : 0;
  const size_t need = (size_t)if_bytes((n_streams - 1) * dstride * bps + ((nsamp * bps + al - 1) & ~(al - 1)), pk);
  if ((rc = hostctx::grow(c->d_if, need))) return rc;
  if (n_streams == 1 || dstride == stride) {
    HIP_TRY(hipMemcpyAsync(c->d_if.p, h_if, (size_t)if_bytes(((n_streams - 1) * stride + nsamp) * bps, pk),
                           hipMemcpyHostToDevice, c->stream));
  } else {
    HIP_TRY(hipMemcpy2DAsync(c->d_if.p, if_bytes(dstride * bps, pk), h_if, if_bytes(stride * bps, pk),
                             if_bytes(nsamp * bps, pk), n_streams, hipMemcpyHostToDevice, c->stream));
  }
  HIP_TRY(hipMemcpyAsync(c->d_cmds, h_cmds, sizeof(gnsscorr_nco_cmd) * C, hipMemcpyHostToDevice,
                         c->stream));
  const int64_t tic = gnsscorr_track_next_tic(c, nsamp);
  rc = launch(c, c->d_if.p, dstride, nsamp, c->d_cmds, c->d_res, h_all_dumps ? c->d_dumps : nullptr,
              tic);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(h_res, c->d_res, sizeof(gnsscorr_track_result) * C,
                         hipMemcpyDeviceToHost, c->stream));
  if (h_all_dumps)
    HIP_TRY(hipMemcpyAsync(h_all_dumps, c->d_dumps, sizeof(int32_t) * 6 * (size_t)C * c->max_dumps,
                           hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (tic_fired) *tic_fired = tic >= 0;
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_track_dev(gnsscorr_track_ctx* c, const int8_t* d_if, int64_t stride,
                                  int64_t nsamp, const gnsscorr_nco_cmd* d_cmds,
                                  gnsscorr_track_result* d_res, int32_t* d_all_dumps,
                                  int64_t tic_count) {
  if (!c || !d_if || !d_cmds || !d_res) {
    gnsscorr_set_error("gnsscorr_track_dev: bad arguments");
    return GNSSCORR_EINVAL;
  }
  int rc = set_dev(c->cfg.device);
  if (rc) return rc;
  return launch(c, d_if, stride, nsamp, d_cmds, d_res, d_all_dumps, tic_count);
}

extern "C" int gnsscorr_track_dev_isr(gnsscorr_track_ctx* c, const int8_t* d_if, int64_t stride,
                                      int64_t nsamp, int n_calls, gnsscorr_nco_cmd* d_cmds,
                                      gnsscorr_track_result* d_res, int n_loops,
                                      const gnsscorr_osg_loop_cfg* cfg, gnsscorr_osg_loop* d_loops,
                                      gnsscorr_osg_loop* d_hist) {
  if (!c || !d_if || !d_cmds || !d_res || !cfg || !d_loops || n_calls < 1) {
    gnsscorr_set_error("gnsscorr_track_dev_isr: bad arguments");
    return GNSSCORR_EINVAL;
  }
  if (n_loops != c->cfg.n_channels) return GNSSCORR_TRACK_NOT_FUSED;
  int rc = set_dev(c->cfg.device);
  if (rc) return rc;
  rc = track_stream_launch(c, d_if, stride, nsamp, n_calls, d_cmds, 0, d_res, nullptr, c->tic, 0, cfg,
                           d_loops, d_hist);
  if (rc == GNSSCORR_OK)   // the kernel stepped the TIC counter once per call; so does the host
    for (int k = 0; k < n_calls; k++) (void)gnsscorr_track_next_tic(c, nsamp);
  return rc;
}

extern "C" int gnsscorr_track_replay_dev(gnsscorr_track_ctx* c, const int8_t* d_if, int64_t stride,
                                         int64_t nsamp, int n_steps,
                                         const gnsscorr_nco_cmd* d_cmds,
                                         gnsscorr_track_result* d_res) {
  if (!c || !d_if || !d_cmds || !d_res || n_steps < 1) {
    gnsscorr_set_error("gnsscorr_track_replay_dev: bad arguments");
    return GNSSCORR_EINVAL;
  }
  int rc = set_dev(c->cfg.device);
  if (rc) return rc;
  const int C = c->cfg.n_channels;
  // every call in one launch of the stream engine where it serves the context
  rc = track_stream_launch(c, d_if, stride, nsamp, n_steps, const_cast<gnsscorr_nco_cmd*>(d_cmds), C,
                           d_res, nullptr, c->tic, 0, nullptr, nullptr, nullptr);
  if (rc == GNSSCORR_OK) {
    for (int k = 0; k < n_steps; k++) (void)gnsscorr_track_next_tic(c, nsamp);
    return GNSSCORR_OK;
  }
  if (rc != GNSSCORR_TRACK_NOT_FUSED) return rc;
  // one launch per step (every I-only context; IQ steps that start off the
  // fused kernel's alignment).  All or nothing: every step's IF is checked
  // before the first launch and before the TIC counter moves.
  if ((rc = gnsscorr_track_check_steps(c, d_if, stride, nsamp, n_steps))) return rc;
  for (int k = 0; k < n_steps; k++) {
    const int64_t tic = gnsscorr_track_next_tic(c, nsamp);
    rc = launch(c, d_if + gnsscorr_track_if_bytes(c, (int64_t)k * nsamp), stride, nsamp,
                d_cmds + (int64_t)k * C,
                d_res + (int64_t)k * C, nullptr, tic);
    if (rc) return rc;
  }
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_track_get_state(gnsscorr_track_ctx* c, gnsscorr_chan_state* h) {
  if (!c || !h) return GNSSCORR_EINVAL;
  int rc = set_dev(c->cfg.device);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(h, c->d_state, sizeof(gnsscorr_chan_state) * c->cfg.n_channels,
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_track_set_state(gnsscorr_track_ctx* c, const gnsscorr_chan_state* h) {
  if (!c || !h) return GNSSCORR_EINVAL;
  int rc = set_dev(c->cfg.device);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->d_state, h, sizeof(gnsscorr_chan_state) * c->cfg.n_channels,
                         hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_track_sync(gnsscorr_track_ctx* c) { return hostctx::sync(c); }

extern "C" void* gnsscorr_track_stream(gnsscorr_track_ctx* c) { return hostctx::stream(c); }

extern "C" int gnsscorr_device_lds_bytes(int device) {
  int blk = 0, cu = 0;
  if (hipDeviceGetAttribute(&blk, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess)
    blk = 0;
  // gfx950 lets one workgroup allocate the CU's whole 160 KiB LDS, while the
  // runtime's per-block attribute may report the older 64 KiB; elsewhere the
  // per-block attribute is the limit
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess &&
      strncmp(prop.gcnArchName, "gfx950", 6) == 0 &&
      hipDeviceGetAttribute(&cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, device) ==
          hipSuccess && cu > blk)
    return cu;
  return blk;
}

extern "C" int gnsscorr_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
