// l3t.hip -- GLONASS L3OC float tracking loop ("l3t") on gfx950.
//
// GLONASS/L3/tracking.sci:123-423: per 1-ms epoch (one period of the 10230-chip code
// at 10.23 Mcps) one code NCO whose three index sequences (early, prompt, late) read
// two codes, the pilot (generateCAcode(PRN), :172-174) and the data channel
// (generateCAcode(PRN + 32), :177-179): twelve fp64 sums.  The loop is split across
// the two: the FLL discriminator and the DLL run on the data sums, the PLL
// discriminator on the pilot prompt (:353-392).  As in sgt.hip and e1t.hip the record
// lives in HBM and one workgroup (or one wave) runs one channel's loop for many epochs
// without leaving the GPU; the channel state is uniform across the workgroup and
// every thread runs the loop filters itself.
//
//  epoch (uniform fp64 scalars):
//    step = codeFreq / fs, blksize = ceil((10230 - remCode) / step)     :265-267
//  per sample (any rate, any state): k = tid + j*T
//    index    ceil((remCode -/+ spc) + k*step), 0-based into [c(L) c c(1)]  :296-317
//    bits     the three indices read both rows: six bits
//    carrier  one sincos per thread, an fp64 rotation per T samples         :322-336
//    sums     the six bits as sign-bit flips of ib / qb, twelve sums        :339-351
//
// At 24 Msps a chip lasts 2.35 samples (step = 0.426), so neither sgt.hip's +-1.0
// double tables (2 x 82 KB per channel) nor its several-samples-per-chip chunk forms
// apply; there is one path, the per-sample one.
//
// Code table: the padded rows of ids 0..64 as bits (1 = chip -1), 320 words each,
// built once at create (ids 0 and 32 all clear: id 32 is all zero in the reference,
// and no accepted channel reads either).  A workgroup copies its two rows into LDS
// once per launch: 2 x 1280 B, + 768 B of wave partials (2 parities x 4 waves x 12)
// in the 256-thread shape.
//
// Op model: 39 fp64 ops per sample: sgt's 27 (3 index adds, 3 ceils, the k*step
// product and conversion, 4 carrier mix, 4 rotation x 2, 6 sums) + 12 for the second
// code's sums counted as sgt counts its own (an FMA as two).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gnsscorr_internal.h"
#include "ftrack.h"

namespace {
using namespace ftrack;

constexpr int kChips = 10230;
constexpr int kRowLen = kChips + 2;         // [c(L) c c(1)], tracking.sci:174, :179
constexpr int kRowWords = 320;              // 10232 bits, padded to 1280 B
constexpr int kIds = 65;                    // table rows: code ids 0..64
constexpr int kMaxPrn = 31;                 // channels: pilot id PRN, data id PRN + 32
constexpr int kMaxWaves = 4;

struct L3tParams {
  int switch_iq;
  double fs, code_basis, if_freq, nominal, spc, code_len;
  double tau1, tau2, k1, k2, k3;
};

// End of one epoch of blk samples whose twelve sums are S (pilot I_E I_P I_L Q_E Q_P
// Q_L, then the data channel's in the same order): the carry-over (tracking.sci:319,
// :326-327) and, closed loop, the FLL-assisted PLL (:354-373: frequency discriminator
// on the data prompt pair, phase discriminator on the pilot prompt, the FLL term
// added) and the DLL on the data early / late sums (:378-392), then the record
// (:401-422).  One definition for the tracking kernel and the replay kernel.
template <bool CLOSED>
__device__ __forceinline__ gnsscorr_l3t_epoch l3t_epoch_end(const L3tParams& p,
                                                            gnsscorr_l3t_chan& c, int blk,
                                                            double step, const double (&S)[12]) {
#pragma clang fp contract(off)
  const double I_P = S[1], Q_P = S[4];
  const double I_E2 = S[6], I_P2 = S[7], I_L2 = S[8], Q_E2 = S[9], Q_P2 = S[10], Q_L2 = S[11];
  const double A = (c.carr_freq * 2.0) * M_PI;        // (carrFreq * 2.0 * %pi)
  const double tlast = c.rem_code + (double)(blk - 1) * step;   // tcode(blksize), prompt
  c.rem_code = (tlast + step) - p.code_len;                     // :319
  carry_carrier(c, A, blk, p.fs);                               // :322-327
  c.pos += blk;
  double code_err = 0, carr_err = 0;
  if (CLOSED) {
    const double I2 = c.i1, Q2 = c.q1;                          // :354-357
    c.i1 = I_P2; c.q1 = Q_P2;
    const double cross = c.i1 * Q2 - I2 * c.q1;
    const double dot = fabs(c.i1 * I2 + c.q1 * Q2);
    const double freq_err = atan2(cross, dot) / M_PI;           // :362
    carr_err = atan(Q_P / I_P) / (2.0 * M_PI);                  // :365
    const double carr_nco =
        c.old_carr_nco + p.k1 * carr_err - p.k2 * c.old_carr_error + p.k3 * freq_err;   // :368
    c.old_carr_nco = carr_nco;
    c.old_carr_error = carr_err;
    c.carr_freq = c.carr_freq_basis + carr_nco;                 // :373
    code_err = early_late_step(I_E2, Q_E2, I_L2, Q_L2, p.tau1, p.tau2, 0.001, c.old_code_nco,
                               c.old_code_error);               // :378-387
    const double code_nco = c.old_code_nco;
    c.code_freq = p.code_basis - code_nco +
                  ((c.carr_freq - p.if_freq) / (p.nominal / p.code_basis));   // :390-392
  }
  c.n_epochs++;
  gnsscorr_l3t_epoch r;
  r.i_e = S[0]; r.i_p = S[1]; r.i_l = S[2]; r.q_e = S[3]; r.q_p = S[4]; r.q_l = S[5];
  r.i_e2 = I_E2; r.i_p2 = I_P2; r.i_l2 = I_L2; r.q_e2 = Q_E2; r.q_p2 = Q_P2; r.q_l2 = Q_L2;
  r.carr_freq = c.carr_freq;
  r.code_freq = c.code_freq;
  r.absolute_sample = (double)c.pos - c.rem_code * (p.fs / 1000) / p.code_len;   // :401-403
  r.dll_discr = code_err;
  r.dll_discr_filt = c.old_code_nco;
  r.pll_discr = carr_err;
  r.pll_discr_filt = c.old_carr_nco;
  r.blksize = (int32_t)blk;
  r.status = 0;
  return r;
}

__device__ __forceinline__ gnsscorr_l3t_epoch stop_record(int status, double blk_d) {
  gnsscorr_l3t_epoch z = {};
  z.status = status;
  z.blksize = blk_d >= 0.0 && blk_d < 2147483648.0 ? (int32_t)blk_d : -1;
  return z;
}

// v with its sign flipped where s (0 or 0x80000000) says so: exactly +-v
__device__ __forceinline__ double flip(double v, uint32_t s) {
  return __hiloint2double(__double2hiint(v) ^ (int)s, __double2loint(v));
}

// MAXT: the workgroup size: 64 = one wave per channel (many channels), 256 the default
// shape, 128 by override.
// MAXTP: MAXT, + kPacked when the records are GNSSCORR_IF_PACKED2 streams
// (gnsscorr_l3t_set_packed): a sample's pair of 2-bit codes is unpacked to the int8 pair
// the per-sample pass consumes.  Kernels of their own: the int8 ones keep their code and
// their symbols.
// MAXTP + kInt16 (gnsscorr_l3t_set_record_format(ctx, 2)): int16 records (if16.h), a
// sample's pair one dword whose halves convert from their full 16 bits; kernels of their
// own again.
constexpr int kPacked = 4096;
constexpr int kInt16 = 8192;
template <bool CLOSED, int MAXTP>
__global__ __launch_bounds__(MAXTP & (kPacked - 1), (MAXTP & (kPacked - 1)) == 64 ? 2 : 1) void
l3t_track_kernel(
    L3tParams p, const int8_t* __restrict__ ifbuf, int64_t stride, int64_t n_samples,
    const uint32_t* __restrict__ codes, gnsscorr_l3t_chan* __restrict__ chans, int n_epochs,
    gnsscorr_l3t_epoch* __restrict__ out) {
#pragma clang fp contract(off)
  constexpr int MAXT = MAXTP & (kPacked - 1);
  constexpr bool PK = (MAXTP & kPacked) != 0;
  constexpr bool I16 = (MAXTP & kInt16) != 0;
  __shared__ uint32_t s_code[2 * kRowWords];     // pilot row, data row as bits (1 = chip -1)
  __shared__ double s_part[2][kMaxWaves][12];
  const int ch = blockIdx.x;
  constexpr bool WAVE = MAXT == 64;
  // (the workgroup size is the instantiation's: strides and the partials loop are
  // constants, which also keeps the scalar registers of the sample loop unspilled)
  constexpr int T = MAXT, nw = T >> 6;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  gnsscorr_l3t_chan c = chans[ch];
  // (a PRN outside 1..31, reachable through track_dev only, lands on a row of the
  // table, not outside it: negative -> 31, 0 -> the all-clear rows 0 and 32)
  const int prn = clampu(c.code_id, kMaxPrn);
  for (int i = tid; i < kRowWords; i += T) {
    s_code[i] = codes[(size_t)prn * kRowWords + i];
    s_code[kRowWords + i] = codes[(size_t)(prn + 32) * kRowWords + i];
  }
  __syncthreads();

  const int8_t* base = ifbuf + (int64_t)c.stream * stride;
  // I/Q byte order as bit-field offsets (switchIQ, :278-282)
  const int sh_re = p.switch_iq ? 8 : 0, sh_im = 8 - sh_re;
  for (int e = 0; e < n_epochs; e++) {
    gnsscorr_l3t_epoch* rec = out + (int64_t)ch * n_epochs + e;
    if (c.status != 0) {
      if (tid == 0) *rec = stop_record(c.status, 0.0);
      continue;
    }
    const double step = c.code_freq / p.fs;
    const double blk_d = ceil((p.code_len - c.rem_code) / step);
    // :286-292: not enough samples (a NaN, negative or huge blksize from a corrupted
    // state stops too, as does a position before the record)
    if (!(c.pos >= 0 && blk_d >= 1.0 && blk_d <= (double)(n_samples - c.pos) &&
          blk_d < 2147483648.0)) {
      c.status = 1;
      if (tid == 0) *rec = stop_record(1, blk_d);
      continue;
    }
    const int blk = (int)blk_d;
    const double aE = c.rem_code - p.spc, aL = c.rem_code + p.spc, aP = c.rem_code;
    const double A = (c.carr_freq * 2.0) * M_PI;        // (carrFreq * 2.0 * %pi)
    const int8_t* src = base + (PK ? 0 : (I16 ? 4 : 2)) * c.pos;
    double acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    {
      const double th0 = A * ((double)tid / p.fs) + c.rem_carr, thw = A * ((double)T / p.fs);
      double sn, cs, sw, cw;
      sincos(th0, &sn, &cs);
      sincos(thw, &sw, &cw);   // (l3t.o is built with promote-alloca-to-lds off)
      auto load = [&](int k) -> int {
        if constexpr (PK)
          return if2_sample<2>(reinterpret_cast<const uint8_t*>(src), c.pos + k);
        if constexpr (I16) return (int)reinterpret_cast<const uint32_t*>(src)[k];
        return *reinterpret_cast<const uint16_t*>(src + 2 * (int64_t)k);
      };
      auto sample = [&](int k, int w) {
        const double t = (double)k * step;
        // padded-row entries (0-based; the clamp only keeps a state set from outside
        // inside the row: the loop's own indices lie in [0, 10231])
        const int jE = clampu((int)ceil(aE + t), kRowLen - 1);
        const int jP = clampu((int)ceil(aP + t), kRowLen - 1);
        const int jL = clampu((int)ceil(aL + t), kRowLen - 1);
        const uint32_t wE = jE >> 5, wP = jP >> 5, wL = jL >> 5;
        const uint32_t sg[6] = {(s_code[wE] >> (jE & 31)) << 31, (s_code[wP] >> (jP & 31)) << 31,
                                (s_code[wL] >> (jL & 31)) << 31,
                                (s_code[kRowWords + wE] >> (jE & 31)) << 31,
                                (s_code[kRowWords + wP] >> (jP & 31)) << 31,
                                (s_code[kRowWords + wL] >> (jL & 31)) << 31};
        const double re = I16 ? (double)if16_half(w, 2 * sh_re)
                              : (double)(int)__builtin_amdgcn_sbfe(w, sh_re, 8);
        const double im = I16 ? (double)if16_half(w, 2 * sh_im)
                              : (double)(int)__builtin_amdgcn_sbfe(w, sh_im, 8);
        // (explicit fma: the carrier and the sums only need fp64 accuracy; the
        // indices above stay uncontracted and bit-exact)
        const double qb = fma(cs, re, -(sn * im));   // real(carrsig .* rawSignal)
        const double ib = fma(cs, im, sn * re);      // imag(carrsig .* rawSignal)
#pragma unroll
        for (int a = 0; a < 3; a++) {
          acc[a] += flip(ib, sg[a]);
          acc[3 + a] += flip(qb, sg[a]);
          acc[6 + a] += flip(ib, sg[3 + a]);
          acc[9 + a] += flip(qb, sg[3 + a]);
        }
        rotate(sn, cs, sw, cw);
      };
      // kU samples per thread per pass, the next pass's IF words loaded during
      // this one; the last, partial pass is guarded per sample
      constexpr int kU = 4;
      const int n_full = blk / (kU * T);
      int k0 = tid;
      int w[kU];
      if (n_full > 0) {
#pragma unroll
        for (int u = 0; u < kU; u++) w[u] = load(k0 + u * T);
      }
      for (int n = 0; n < n_full; n++, k0 += kU * T) {
        int cur[kU];
#pragma unroll
        for (int u = 0; u < kU; u++) cur[u] = w[u];
        if (n + 1 < n_full) {
#pragma unroll
          for (int u = 0; u < kU; u++) w[u] = load(k0 + kU * T + u * T);
        }
#pragma unroll
        for (int u = 0; u < kU; u++) sample(k0 + u * T, cur[u]);
      }
#pragma unroll
      for (int u = 0; u < kU; u++) {
        const int k = k0 + u * T;
        w[u] = k < blk ? load(k) : 0;
      }
#pragma unroll
      for (int u = 0; u < kU; u++) {
        const int k = k0 + u * T;
        if (k < blk) sample(k, w[u]);
      }
    }
    double S[12];
#pragma unroll
    for (int j = 0; j < 12; j++) S[j] = wave_sum(acc[j]);
    if constexpr (!WAVE) {
      const int par = e & 1;
      if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 12; j++) s_part[par][wave][j] = S[j];
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 12; j++) S[j] = 0.0;
      for (int w = 0; w < nw; w++)
#pragma unroll
        for (int j = 0; j < 12; j++) S[j] += s_part[par][w][j];
    }
    const gnsscorr_l3t_epoch r = l3t_epoch_end<CLOSED>(p, c, blk, step, S);
    if (tid == 0) *rec = r;
  }
  if (tid == 0) chans[ch] = c;
}

// The loop half alone: each thread runs one channel's epochs on given sums
// (sums[(ch*n_epochs + e)*12 + j]).  There is no record, so no out-of-data stop; a
// NaN / negative / >= 2^31 blksize stops the channel with status 1.
__global__ void l3t_replay_kernel(L3tParams p, gnsscorr_l3t_chan* __restrict__ chans, int n_ch,
                                  int n_epochs, const double* __restrict__ sums,
                                  gnsscorr_l3t_epoch* __restrict__ out) {
#pragma clang fp contract(off)
  const int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= n_ch) return;
  gnsscorr_l3t_chan c = chans[ch];
  for (int e = 0; e < n_epochs; e++) {
    gnsscorr_l3t_epoch* rec = out + (int64_t)ch * n_epochs + e;
    if (c.status != 0) {
      *rec = stop_record(c.status, 0.0);
      continue;
    }
    const double step = c.code_freq / p.fs;
    const double blk_d = ceil((p.code_len - c.rem_code) / step);
    if (!(blk_d >= 1.0 && blk_d < 2147483648.0)) {
      c.status = 1;
      *rec = stop_record(1, blk_d);
      continue;
    }
    const double* sp = sums + ((int64_t)ch * n_epochs + e) * 12;
    const double S[12] = {sp[0], sp[1], sp[2], sp[3], sp[4],  sp[5],
                          sp[6], sp[7], sp[8], sp[9], sp[10], sp[11]};
    *rec = l3t_epoch_end<true>(p, c, (int)blk_d, step, S);
  }
  chans[ch] = c;
}

}  // namespace

// ============================================================================
// host side
// ============================================================================
struct gnsscorr_l3t_ctx {
  gnsscorr_l3t_cfg cfg;
  L3tParams p;
  hipStream_t stream = nullptr;
  uint32_t* d_codes = nullptr;                 // kIds padded rows as bits
  hostctx::DevBuf<gnsscorr_l3t_chan> d_chan;   // the host wrappers' own
  hostctx::DevBuf<gnsscorr_l3t_epoch> d_ep;
  int packed = 0;                              // gnsscorr_l3t_set_packed
  int i16 = 0;                                 // gnsscorr_l3t_set_record_format(ctx, 2)
};

extern "C" void gnsscorr_l3t_loop_coefs(const gnsscorr_l3t_cfg* cfg, double* tau1, double* tau2,
                                        double* k1, double* k2, double* k3) {
  calc_loop_coef(cfg->dll_noise_bw, cfg->dll_damping, tau1, tau2);
  calc_fll_pll_loop_coef(cfg->pll_noise_bw, cfg->fll_noise_bw, k1, k2, k3);
}

static int check_cfg(const gnsscorr_l3t_cfg* cfg) {
  if (!cfg || cfg->file_type != 2 || !(cfg->samp_rate > 0) || !(cfg->code_freq_basis > 0) ||
      !(cfg->nominal_freq > 0) || cfg->code_length != kChips ||
      !(cfg->dll_spacing >= 0 && cfg->dll_spacing < 1)) {
    gnsscorr_set_error("l3t: bad config (file_type 2, code_length 10230, 0<=dll_spacing<1, "
                       "positive rates)");
    return GNSSCORR_EINVAL;
  }
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_l3t_init_chan(const gnsscorr_l3t_cfg* cfg, int prn, int stream,
                                      int64_t skip, int64_t code_phase_1b, double acq_freq,
                                      gnsscorr_l3t_chan* o) {
  int rc = check_cfg(cfg);
  if (rc) return rc;
  if (!o || code_phase_1b < 1 || stream < 0 || skip < 0 || prn < 1 || prn > kMaxPrn) {
    gnsscorr_set_error("gnsscorr_l3t_init_chan: bad channel (PRN 1..31, code_phase >= 1)");
    return GNSSCORR_EINVAL;
  }
  memset(o, 0, sizeof *o);
  o->code_id = prn;
  o->stream = stream;
  o->pos = skip + code_phase_1b - 1;   // mseek, tracking.sci:164-169
  o->code_freq = cfg->code_freq_basis; // :184-186, the aiding term times 0
  o->carr_freq = o->carr_freq_basis = acq_freq;
  o->i1 = o->q1 = 0.001;               // :208
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_l3t_destroy(gnsscorr_l3t_ctx* c) { return ftrack::destroy(c); }

extern "C" int gnsscorr_l3t_set_packed(gnsscorr_l3t_ctx* c, int packed) {
  return ftrack::set_packed(__func__, c, packed);
}
extern "C" int gnsscorr_l3t_set_record_format(gnsscorr_l3t_ctx* c, int fmt) {
  return ftrack::set_record_format(__func__, c, fmt);
}

// the stream and the resident code rows of ids 0..64
static int init_device(gnsscorr_l3t_ctx* c) {
  HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  HIP_TRY(hipMalloc(&c->d_codes, sizeof(uint32_t) * (size_t)kIds * kRowWords));
  uint32_t* h = (uint32_t*)calloc((size_t)kIds * kRowWords, sizeof(uint32_t));
  int8_t* code = (int8_t*)malloc(kChips);
  if (!h || !code) {
    free(h);
    free(code);
    gnsscorr_set_error("gnsscorr_l3t_create: out of host memory");
    return GNSSCORR_ENOMEM;
  }
  for (int id = 1; id < kIds; id++) {
    gnsscorr_l3_code(id, code);
    uint32_t* row = h + (size_t)id * kRowWords;
    for (int j = 0; j < kRowLen; j++)
      if (code[(j - 1 + kChips) % kChips] < 0) row[j >> 5] |= 1u << (j & 31);
  }
  const hipError_t e =
      hipMemcpy(c->d_codes, h, sizeof(uint32_t) * (size_t)kIds * kRowWords, hipMemcpyHostToDevice);
  free(h);
  free(code);
  HIP_TRY(e);
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_l3t_create(gnsscorr_l3t_ctx** out, const gnsscorr_l3t_cfg* cfg) {
  if (!out) return GNSSCORR_EINVAL;
  *out = nullptr;
  int rc = check_cfg(cfg);
  if (rc) return rc;
  rc = hostctx::open_device(__func__, cfg->device);
  if (rc) return rc;
  auto* c = new gnsscorr_l3t_ctx();
  c->cfg = *cfg;
  L3tParams& p = c->p;
  p.switch_iq = cfg->switch_iq != 0;
  p.fs = cfg->samp_rate;
  p.code_basis = cfg->code_freq_basis;
  p.if_freq = cfg->if_freq;
  p.nominal = cfg->nominal_freq;
  p.spc = cfg->dll_spacing;
  p.code_len = (double)cfg->code_length;
  gnsscorr_l3t_loop_coefs(cfg, &p.tau1, &p.tau2, &p.k1, &p.k2, &p.k3);
  rc = init_device(c);
  if (rc) {
    gnsscorr_l3t_destroy(c);
    return rc;
  }
  *out = c;
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_l3t_track_dev(gnsscorr_l3t_ctx* c, const int8_t* d_if, int64_t stride,
                                      int64_t n_samples, int n_ch, gnsscorr_l3t_chan* d_chan,
                                      int n_epochs, int closed_loop, gnsscorr_l3t_epoch* d_ep) {
  int rc = check_track_dev(__func__, c, d_if, d_chan, d_ep, n_ch, n_epochs, n_samples, stride);
  if (rc) return rc;
  rc = check_iq_aligned(__func__, c, d_if);
  if (!rc) rc = check_packed_aligned(__func__, c, d_if, stride);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  // two launch shapes: one wave per channel for many channels (throughput),
  // 256-thread workgroups otherwise (epoch latency of a receiver's worth of
  // channels).  GNSSCORR_L3T_THREADS overrides (64 = wave mode, 128, 256).
  int T = n_ch >= 1024 ? 64 : 256;
  if (const char* ov = getenv("GNSSCORR_L3T_THREADS")) {
    const int v = atoi(ov);
    if (v == 64 || v == 128 || v == 256) T = v;
  }
  dim3 grid(n_ch), block(T);
#define L3T_LAUNCH(CL, PK)                                                                    \
  do {                                                                                        \
    if (T == 64)                                                                              \
      hipLaunchKernelGGL((l3t_track_kernel<CL, 64 + PK>), grid, block, 0, c->stream, c->p,    \
                         d_if, stride, n_samples, c->d_codes, d_chan, n_epochs, d_ep);        \
    else if (T == 128)                                                                        \
      hipLaunchKernelGGL((l3t_track_kernel<CL, 128 + PK>), grid, block, 0, c->stream, c->p,   \
                         d_if, stride, n_samples, c->d_codes, d_chan, n_epochs, d_ep);        \
    else                                                                                      \
      hipLaunchKernelGGL((l3t_track_kernel<CL, 256 + PK>), grid, block, 0, c->stream, c->p,   \
                         d_if, stride, n_samples, c->d_codes, d_chan, n_epochs, d_ep);        \
  } while (0)
  if (c->packed) {
    if (closed_loop) L3T_LAUNCH(true, kPacked);
    else L3T_LAUNCH(false, kPacked);
  } else if (c->i16) {
    if (closed_loop) L3T_LAUNCH(true, kInt16);
    else L3T_LAUNCH(false, kInt16);
  } else {
    if (closed_loop) L3T_LAUNCH(true, 0);
    else L3T_LAUNCH(false, 0);
  }
#undef L3T_LAUNCH
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_l3t_track(gnsscorr_l3t_ctx* c, const int8_t* d_if, int64_t stride,
                                  int64_t n_samples, int n_ch, gnsscorr_l3t_chan* h_chan,
                                  int n_epochs, int closed_loop, gnsscorr_l3t_epoch* h_ep) {
  if (!c || !h_chan || !h_ep || n_ch < 1 || n_epochs < 1) return bad_arguments(__func__);
  for (int i = 0; i < n_ch; i++) {
    const int id = h_chan[i].code_id;
    if (id < 1 || id > kMaxPrn) {
      gnsscorr_set_error("gnsscorr_l3t_track: channel %d: PRN %d outside 1..31", i, id);
      return GNSSCORR_EINVAL;
    }
  }
  return ftrack::track(c, n_ch, h_chan, n_epochs, h_ep,
                       [&](gnsscorr_l3t_chan* d_chan, gnsscorr_l3t_epoch* d_ep) {
                         return gnsscorr_l3t_track_dev(c, d_if, stride, n_samples, n_ch, d_chan,
                                                       n_epochs, closed_loop, d_ep);
                       });
}

extern "C" int gnsscorr_l3t_sync(gnsscorr_l3t_ctx* c) { return hostctx::sync(c); }

extern "C" void* gnsscorr_l3t_stream(gnsscorr_l3t_ctx* c) { return hostctx::stream(c); }

extern "C" int gnsscorr_l3t_replay_dev(gnsscorr_l3t_ctx* c, int n_ch, gnsscorr_l3t_chan* d_chan,
                                       int n_epochs, const double* d_sums,
                                       gnsscorr_l3t_epoch* d_ep) {
  return ftrack::replay_dev(__func__, c, l3t_replay_kernel, n_ch, d_chan, n_epochs, d_sums, d_ep);
}

extern "C" int gnsscorr_l3t_replay(gnsscorr_l3t_ctx* c, int n_ch, gnsscorr_l3t_chan* h_chan,
                                   int n_epochs, const double* h_sums, gnsscorr_l3t_epoch* h_ep) {
  return ftrack::replay<12>(__func__, c, n_ch, h_chan, n_epochs, h_sums, h_ep,
                            [&](gnsscorr_l3t_chan* d_chan, double* d_sums, gnsscorr_l3t_epoch* d_ep) {
                              return gnsscorr_l3t_replay_dev(c, n_ch, d_chan, n_epochs, d_sums, d_ep);
                            });
}
