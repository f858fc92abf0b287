// ftrack.h -- what the three float trackers (sgt.hip, e1t.hip, l3t.hip) share:
// lane helpers and the carrier rotation, the chunk grid of the chunked paths
// (geometry and the crossing estimate with its margin), the loop-filter steps
// of the epoch end and the host wrappers around a tracking context (on the
// shared host scaffolding of hostctx.h).
// Everything on the device side is __forceinline__ and carries its own fp
// contract(off): the code indices and the NCO carry-over are bit-exact
// restatements of tracking.sci, whose line citations stay next to the call
// sites in each tracker.
// Deliberately not here, although the two kernels spell them alike: the
// per-sample pass loop, the epoch reduction, and the chunk loop's fetch / unpack
// / edge masking, W_n * raw product and opaque table offset.  Each was tried as
// a shared function and each changed the instructions the compiler emits for at
// least one tracking kernel (e1t: up to +6 VGPRs); both kernels sit on their
// register bounds, so those pieces stay in the kernels.
#ifndef GNSSCORR_FTRACK_H
#define GNSSCORR_FTRACK_H
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "gnsscorr_internal.h"
#include "hostctx.h"
#include "if2.h"
#include "if16.h"

namespace ftrack {

// ============================================================================
// lane helpers
// ============================================================================
// indices stay inside their table for every state the loop produces; the clamp
// only keeps a corrupted state inside the LDS table, in one instruction: a
// negative index wraps to a huge unsigned and lands on hi
__device__ __forceinline__ int clampu(int i, int hi) { return (int)min((unsigned)i, (unsigned)hi); }

// a value every lane of the workgroup holds (the channel's state is uniform):
// held in scalar registers instead of a VGPR pair
__device__ __forceinline__ double uni(double v) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = __builtin_amdgcn_readfirstlane((int)b);
  const unsigned hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// wave total, uniform: DPP row_shr 1/2/4/8 (a Hillis-Steele scan in each
// 16-lane row, 0.0 shifted in) leaves each row's sum in its lane 15 and the
// four rows add in scalar registers -- VALU only, where a 64-bit __shfl_xor
// butterfly is two ds_bpermute round trips per step.  Every lane must be active.
template <int CTRL>
__device__ __forceinline__ double dpp_shr(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_f64(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l),
                          __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma clang fp contract(off)
  v += dpp_shr<0x111>(v);
  v += dpp_shr<0x112>(v);
  v += dpp_shr<0x114>(v);
  v += dpp_shr<0x118>(v);
  return (lane_f64(v, 15) + lane_f64(v, 31)) + (lane_f64(v, 47) + lane_f64(v, 63));
}

// (sb, cb) <- (sb, cb) * (sR, cR): the carrier one rotation on (explicit fma:
// the carrier only needs fp64 accuracy)
__device__ __forceinline__ void rotate(double& sb, double& cb, double sR, double cR) {
#pragma clang fp contract(off)
  const double cn = fma(cb, cR, -(sb * sR));
  sb = fma(sb, cR, cb * sR);
  cb = cn;
}

// ============================================================================
// chunked paths: the epoch's samples as chunks of kC on the 16-byte grid of the
// stream.  Chunk q holds samples k0 = q*kC - mis .. k0 + kC - 1, thread tid takes
// q = tid + it*T.  kBps: bytes per sample (2 = IQ records, 1 = real).
// ============================================================================
template <int kBps, int kC>
struct ChunkGrid {
  static constexpr int kW = kC * kBps / 16;   // 16-byte words per chunk
  int mis;           // samples between the grid and the epoch's first
  const uint4* ab;   // the grid word holding the epoch's first sample
  int nC, nIt;       // chunks of the epoch, chunks per thread

  __device__ __forceinline__ ChunkGrid(const int8_t* src, int blk, int T) {
    mis = (int)((uintptr_t)src & 15) / kBps;
    ab = reinterpret_cast<const uint4*>(src - mis * kBps);
    nC = (blk + mis + kC - 1) / kC;
    nIt = (nC + T - 1) / T;
  }
  // Packed records (if2.h): the grid is a function of the sample position alone,
  // the int8 grid of a record whose stream base is 16-byte aligned.  A chunk is
  // then the kW whole dwords from dword first_dword(pos) + q*kW of the stream; ab
  // is not used.
  __device__ __forceinline__ ChunkGrid(int64_t pos, int blk, int T) {
    mis = (int)((kBps * pos) & 15) / kBps;
    ab = nullptr;
    nC = (blk + mis + kC - 1) / kC;
    nIt = (nC + T - 1) / T;
  }
  __device__ __forceinline__ int64_t first_dword(int64_t pos) const {
    return (kBps * (pos - mis)) >> 4;
  }
  // int16 records (if16.h) take the same constructor, kBps still the int8 record's:
  // the grid is defined in samples, chunk q holds the samples it holds on int8, in
  // the 2 * kW 16-byte words from this byte of the stream on
  __device__ __forceinline__ int64_t first_byte16(int64_t pos, int q) const {
    return 2 * (int64_t)kBps * (pos - mis + (int64_t)q * kC);
  }

  // Where an index a + k*step next exceeds j: sample k has index > j iff
  // a + k*step > j, i.e. k > d = (j - a)/step (inv = 1/step), so the first such
  // sample is floor(d) + 1; returned as an offset into the chunk at k0, clamped
  // to [1, kC].  When d lies within 1e-6 samples of an integer the real-valued
  // estimate could round either way: risky is set and the caller recomputes the
  // chunk with the exact fp64 indices, sample by sample.
  static __device__ __forceinline__ int crossing(double j, double a, double inv, int k0,
                                                 bool& risky) {
#pragma clang fp contract(off)
    const double d = (j - a) * inv;
    const double fd = floor(d);
    const double fr = d - fd;
    risky |= !(fr > 1e-6 && fr < 1.0 - 1e-6);
    return min(max((int)fd + 1 - k0, 1), kC);
  }
};

// ============================================================================
// epoch end.  Chan: any channel struct with the common field names
// (gnsscorr_sgt_chan, gnsscorr_e1t_chan).
// ============================================================================
// remCarrPhase after blk samples at A = carrFreq*2*pi rad/s
template <class Chan>
__device__ __forceinline__ void carry_carrier(Chan& c, double A, int blk, double fs) {
#pragma clang fp contract(off)
  const double twopi = 2.0 * M_PI;
  const double last = A * ((double)blk / fs) + c.rem_carr;   // trigarg(blksize+1)
  c.rem_carr = last - trunc(last / twopi) * twopi;
}

// FLL-assisted PLL on the prompt sums: sets carr_freq, returns the PLL discriminator.
// kSignFlip: the previous prompt pair is negated when sign(I_P) changed
// (COMPASS/B1/tracking.sci:295-298; Scilab's sign() is -1, 0 or 1).
template <bool kSignFlip = false, class Chan>
__device__ __forceinline__ double fll_pll_step(Chan& c, double k1, double k2, double k3,
                                               double I_P, double Q_P) {
#pragma clang fp contract(off)
  double I2 = c.i1, Q2 = c.q1;
  c.i1 = I_P; c.q1 = Q_P;
  if (kSignFlip) {
    const int s2 = (I2 > 0.0) - (I2 < 0.0), s1 = (I_P > 0.0) - (I_P < 0.0);
    if (s2 != s1) { I2 = -I2; Q2 = -Q2; }
  }
  const double cross = c.i1 * Q2 - I2 * c.q1;
  const double dot = fabs(c.i1 * I2 + c.q1 * Q2);
  const double freq_err = atan2(cross, dot) / M_PI;
  const double carr_err = atan(Q_P / I_P) / (2.0 * M_PI);
  const double carr_nco = c.old_carr_nco + k1 * carr_err - k2 * c.old_carr_error - k3 * freq_err;
  c.old_carr_nco = carr_nco;
  c.old_carr_error = carr_err;
  c.carr_freq = c.carr_freq_basis + carr_nco;
  return carr_err;
}

// early-minus-late magnitude discriminator and its tau2/tau1 filter (pdi: the
// loop's integration time): updates the NCO command and the kept error,
// returns the discriminator
__device__ __forceinline__ double early_late_step(double I_E, double Q_E, double I_L, double Q_L,
                                                  double tau1, double tau2, double pdi,
                                                  double& old_nco, double& old_error) {
#pragma clang fp contract(off)
  const double mE = sqrt(I_E * I_E + Q_E * Q_E), mL = sqrt(I_L * I_L + Q_L * Q_L);
  const double err = (mE - mL) / (mE + mL);
  const double nco = old_nco + (tau2 / tau1) * (err - old_error) + err * (pdi / tau1);
  old_nco = nco;
  old_error = err;
  return err;
}

// ============================================================================
// host side.  Ctx: a tracking context with cfg.device, p (the kernel's params),
// stream, d_codes and the host wrappers' own growable d_chan / d_ep.  fn: the
// exported function's name, for its error texts.
// ============================================================================
inline int bad_arguments(const char* fn) {
  gnsscorr_set_error("%s: bad arguments", fn);
  return GNSSCORR_EINVAL;
}

// calcLoopCoef.sci:39-43 (k = 1.0)
inline void calc_loop_coef(double lbw, double z, double* tau1, double* tau2) {
  const double wn = lbw * 8 * z / (4 * (z * z) + 1);
  *tau1 = 1.0 / (wn * wn);
  *tau2 = 2.0 * z / wn;
}

// calcFLLPLLLoopCoef.sci:36-38 (T = PDIcarr, 0.001 in every 1 ms loop)
inline void calc_fll_pll_loop_coef(double pll_bw, double fll_bw, double* k1, double* k2,
                                   double* k3, double T = 0.001) {
  const double b = pll_bw / 0.53;
  *k1 = T * (b * b) + 1.414 * b;
  *k2 = 1.414 * b;
  *k3 = T * (fll_bw / 0.25);
}

template <class Ctx>
int destroy(Ctx* c) {
  return hostctx::destroy(c, [&] { hostctx::release(c->d_codes, c->d_chan, c->d_ep); });
}

// the checks *_track_dev share
template <class Ctx>
int check_track_dev(const char* fn, const Ctx* c, const int8_t* d_if, const void* d_chan,
                    const void* d_ep, int n_ch, int n_epochs, int64_t n_samples, int64_t stride) {
  if (!c || !d_if || !d_chan || !d_ep || n_ch < 1 || n_epochs < 1 || n_samples < 0 || stride < 0)
    return bad_arguments(fn);
  return GNSSCORR_OK;
}
template <class Ctx>
int check_iq_aligned(const char* fn, const Ctx* c, const int8_t* d_if) {
  if (c->cfg.file_type == 2 && ((uintptr_t)d_if & 1)) {
    gnsscorr_set_error("%s: IQ record must be 2-byte aligned", fn);
    return GNSSCORR_EINVAL;
  }
  return GNSSCORR_OK;
}

// *_set_packed: the records of later track calls are GNSSCORR_IF_PACKED2 streams
template <class Ctx>
int set_packed(const char* fn, Ctx* c, int packed) {
  if (!c || (packed != 0 && packed != 1)) {
    gnsscorr_set_error("%s: bad arguments (a context, packed 0 or 1)", fn);
    return GNSSCORR_EINVAL;
  }
  c->packed = packed;
  c->i16 = 0;
  return GNSSCORR_OK;
}
// *_set_record_format: 0 = int8, 1 = GNSSCORR_IF_PACKED2 (set_packed(1)), 2 = int16
template <class Ctx>
int set_record_format(const char* fn, Ctx* c, int fmt) {
  if (!c || fmt < 0 || fmt > 2) {
    gnsscorr_set_error("%s: bad arguments (a context, fmt 0 = int8, 1 = 2-bit packed, "
                       "2 = int16)", fn);
    return GNSSCORR_EINVAL;
  }
  c->packed = fmt == 1;
  c->i16 = fmt == 2;
  return GNSSCORR_OK;
}
// packed records: whole 16-byte words from an aligned base, for every stream
template <class Ctx>
int check_packed_aligned(const char* fn, const Ctx* c, const int8_t* d_if, int64_t stride) {
  if (c->packed && (((uintptr_t)d_if & 15) || (stride & 15))) {
    gnsscorr_set_error("%s: packed records need a 16-byte-aligned d_if and a stream_stride "
                       "that is a multiple of 16 bytes", fn);
    return GNSSCORR_EINVAL;
  }
  // int16 records: the chunks are dwordx4 loads from 32-byte steps of the stream
  if (c->i16 && (((uintptr_t)d_if & 15) || (stride & 15))) {
    gnsscorr_set_error("%s: int16 records need a 16-byte-aligned d_if and a stream_stride "
                       "that is a multiple of 16 bytes", fn);
    return GNSSCORR_EINVAL;
  }
  return GNSSCORR_OK;
}

// host channels in, track_dev(d_chan, d_ep) on the context's own buffers, host
// channels and epochs out, synchronised
template <class Ctx, class Chan, class Epoch, class TrackDev>
int track(Ctx* c, int n_ch, Chan* h_chan, int n_epochs, Epoch* h_ep, const TrackDev& track_dev) {
  HIP_TRY(hipSetDevice(c->cfg.device));
  const size_t nc = (size_t)n_ch, ne = nc * (size_t)n_epochs;
  int rc = hostctx::grow(c->d_chan, nc);
  if (!rc) rc = hostctx::grow(c->d_ep, ne);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->d_chan.p, h_chan, nc * sizeof(Chan), hipMemcpyHostToDevice, c->stream));
  rc = track_dev(c->d_chan.p, c->d_ep.p);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(h_chan, c->d_chan.p, nc * sizeof(Chan), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(h_ep, c->d_ep.p, ne * sizeof(Epoch), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return GNSSCORR_OK;
}

// the loop half on given sums: one thread per channel
template <class Ctx, class Kernel, class Chan, class Epoch>
int replay_dev(const char* fn, Ctx* c, Kernel kernel, int n_ch, Chan* d_chan, int n_epochs,
               const double* d_sums, Epoch* d_ep) {
  if (!c || !d_chan || !d_sums || !d_ep || n_ch < 1 || n_epochs < 1) return bad_arguments(fn);
  HIP_TRY(hipSetDevice(c->cfg.device));
  hipLaunchKernelGGL(kernel, dim3((n_ch + 63) / 64), dim3(64), 0, c->stream, c->p, d_chan, n_ch,
                     n_epochs, d_sums, d_ep);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

// host channels and sums [n_ch, n_epochs, N] in, replay_dev(d_chan, d_sums,
// d_ep) on buffers of this call's own, host channels and epochs out
template <int N, class Ctx, class Chan, class Epoch, class ReplayDev>
int replay(const char* fn, Ctx* c, int n_ch, Chan* h_chan, int n_epochs, const double* h_sums,
           Epoch* h_ep, const ReplayDev& replay_dev) {
  if (!c || !h_chan || !h_sums || !h_ep || n_ch < 1 || n_epochs < 1) return bad_arguments(fn);
  HIP_TRY(hipSetDevice(c->cfg.device));
  const size_t nc = (size_t)n_ch, ne = nc * (size_t)n_epochs;
  hostctx::Staging st(c->stream);
  Chan* d_chan = st.inout(h_chan, nc);
  double* d_sums = st.in(h_sums, ne * N);
  Epoch* d_ep = st.out(h_ep, ne);
  if (st.status()) return st.status();
  const int rc = replay_dev(d_chan, d_sums, d_ep);
  return rc ? rc : st.finish();
}

}  // namespace ftrack
#endif
