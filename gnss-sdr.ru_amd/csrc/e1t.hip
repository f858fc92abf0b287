// e1t.hip -- Galileo E1B float tracking loop ("e1t") on gfx950.
//
// GALILEO/E1/tracking.sci:95-455: per 1-ms epoch (one quarter of the 4092-chip
// primary code) a code NCO over the quarter's padded 1025-entry row, an
// independent subcarrier ("meandr") NCO over the alternating 2050-entry table,
// five arms (subcarrier x code: E-P, P-E, P-P, P-L, L-P), ten fp64 sums, then the
// FLL-assisted PLL, the DLL (P-E / P-L) and the SLL (E-P / L-P).  As in sgt.hip
// the record lives in HBM and one workgroup (or one wave) runs one channel's
// loop for many epochs without leaving the GPU; the channel state is uniform
// across the workgroup and every thread runs the loop filters itself.
//
//  epoch (uniform fp64 scalars):
//    cstep = codeFreq / fs, mstep = meandrFreq / fs              :263-264
//    blksize = ceil((1023 - remCode) / cstep)                    :266
//  per-sample path (any rate, any state): k = tid + j*T
//    code index   ceil((remCode -/+ dllSpc) + k*cstep)   -> bit of the row
//    subcarrier   ceil((remMeandr -/+ sllSpc) + k*mstep) -> its parity: the
//                 padded table [m($-1) m($) m m(1) m(2)] alternates over all
//                 2050 entries, entry j (1-based) is +1 for odd j, so the value
//                 at ceil(t) + 1 is -1 iff ceil(t) is odd; no table
//    carrier      one sincos per thread, an fp64 rotation per T samples
//    sums         five sign products as sign-bit flips of ib / qb, ten sums
//  chunked path (15*cstep < 1 and 15*mstep < 2: 16 and 16.368 Msps): a lane takes
//    16 consecutive samples.  Per arm the index of the chunk's first sample is
//    the exact formula and the samples at which it next steps come from the
//    crossing (j - a)/step, taken sample by sample with the exact formula when
//    the estimate is within 1e-6 samples of an integer.  A code arm steps at
//    most once in a chunk, a subcarrier arm at most twice.  Each of the six
//    sequences becomes a 16-bit sign mask, the five arms are XORs of two masks,
//    and sample n takes bit n as +-1.0: no fp64 ceil chain per sample.  Carrier:
//    exp(i theta_k0) once per chunk times the LDS table W_n = exp(i*A*n/fs).
//    GNSSCORR_E1T_CHUNK=0 forces the per-sample path.
//
// Code table: all four padded rows of a channel's code in LDS as bits,
// 4 x 36 words = 576 B, loaded once per launch.  LDS per workgroup: 576 B rows +
// 256 B W table = 832 B in the one-wave-per-channel launch, + 640 B partials
// (2 parities x 4 waves x 10) = 1472 B in the 256-thread one.  Occupancy is
// bounded by registers (about 200 VGPRs: 2 waves per SIMD, which the launch
// bound asks for), not by LDS: 8 waves per CU take 6.5 KiB of the 160 KiB.
//
// Op model: 41 fp64 ops per sample (6 index adds, 6 ceils, 2 k*step products, 4
// carrier mix, 4 rotation, 10 sums, conversions).
#include <hip/hip_runtime.h>
#include <type_traits>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gnsscorr_internal.h"
#include "ftrack.h"

namespace {
using namespace ftrack;

constexpr int kChips = 4092;
constexpr int kQuarter = kChips / 4;        // 1023 chips per epoch
constexpr int kRowLen = kQuarter + 2;       // padded row, tracking.sci:157-160
constexpr int kRowWords = 36;               // 1025 bits, padded to 144 B
constexpr int kCodeWords = 4 * kRowWords;   // one code: four rows
constexpr int kMaxWaves = 4;
constexpr int kMeandrTab = 2050;            // [m($-1) m($) m m(1) m(2)], :168
constexpr int kC = 16;                      // samples per chunk (chunked path)

struct E1tParams {
  int file_type, chunked, n_codes;
  double fs, code_basis, meandr_basis, if_freq, dspc, sspc, code_len;
  double tau1c, tau2c, tau1m, tau2m, k1, k2, k3;
};

// End of one epoch of blk samples whose ten sums are S (I_E_P, I_P_E, I_P_P,
// I_P_L, I_L_P, then the same for Q): the carry-over of the three NCOs
// (tracking.sci:310-315, :338, :341-346) and, closed loop, the FLL-assisted PLL
// (:371-389), the DLL (:394-407) and the SLL (:412-425), then the record
// (:433-454).  One definition for the tracking kernel and the replay kernel.
template <bool CLOSED>
__device__ __forceinline__ gnsscorr_e1t_epoch e1t_epoch_end(const E1tParams& p,
                                                            gnsscorr_e1t_chan& c, int blk,
                                                            double cstep, double mstep,
                                                            const double (&S)[10]) {
#pragma clang fp contract(off)
  const double I_E_P = S[0], I_P_E = S[1], I_P_P = S[2], I_P_L = S[3], I_L_P = S[4];
  const double Q_E_P = S[5], Q_P_E = S[6], Q_P_P = S[7], Q_P_L = S[8], Q_L_P = S[9];
  const double A = (c.carr_freq * 2.0) * M_PI;        // (carrFreq * 2.0 * %pi)
  const int seg = c.segment;
  const double tlast = c.rem_code + (double)(blk - 1) * cstep;     // tcode(blksize), prompt
  c.rem_code = (tlast + cstep) - 4092.0 / 4;                       // :310
  c.segment = (c.segment + 1) & 3;                                 // :312-315
  const double mlast = c.rem_meandr + (double)(blk - 1) * mstep;   // tmeandr(blksize), prompt
  c.rem_meandr = (mlast + mstep) - 8184.0 / 4;                     // :338
  carry_carrier(c, A, blk, p.fs);                                  // :341-346
  c.pos += blk;
  double code_err = 0, meandr_err = 0, carr_err = 0;
  if (CLOSED) {
    carr_err = fll_pll_step(c, p.k1, p.k2, p.k3, I_P_P, Q_P_P);   // :371-389
    // DLL on P-E / P-L (:394-407)
    code_err = early_late_step(I_P_E, Q_P_E, I_P_L, Q_P_L, p.tau1c, p.tau2c, 0.001,
                               c.old_code_nco, c.old_code_error);
    const double code_nco = c.old_code_nco;
    c.code_freq = p.code_basis - code_nco + ((c.carr_freq - p.if_freq) / 1540);
    // SLL on E-P / L-P (:412-425)
    meandr_err = early_late_step(I_E_P, Q_E_P, I_L_P, Q_L_P, p.tau1m, p.tau2m, 0.001,
                                 c.old_meandr_nco, c.old_meandr_error);
    const double meandr_nco = c.old_meandr_nco;
    c.meandr_freq = p.meandr_basis - meandr_nco + ((c.carr_freq - p.if_freq) / 770);
  }
  c.n_epochs++;
  gnsscorr_e1t_epoch r;
  r.i_e_p = I_E_P; r.i_p_e = I_P_E; r.i_p_p = I_P_P; r.i_p_l = I_P_L; r.i_l_p = I_L_P;
  r.q_e_p = Q_E_P; r.q_p_e = Q_P_E; r.q_p_p = Q_P_P; r.q_p_l = Q_P_L; r.q_l_p = Q_L_P;
  r.carr_freq = c.carr_freq;
  r.code_freq = c.code_freq;
  r.meandr_freq = c.meandr_freq;
  // :433-435, the whole code length in the divisor as written there
  r.absolute_sample = (double)c.pos - c.rem_code * (p.fs / 1000) / p.code_len;
  r.dll_discr = code_err;
  r.dll_discr_filt = c.old_code_nco;
  r.sll_discr = meandr_err;
  r.sll_discr_filt = c.old_meandr_nco;
  r.pll_discr = carr_err;
  r.pll_discr_filt = c.old_carr_nco;
  r.blksize = (int32_t)blk;
  r.status = 0;
  r.segment = seg;
  r.pad = 0;
  return r;
}

__device__ __forceinline__ gnsscorr_e1t_epoch stop_record(int status, double blk_d, int seg) {
  gnsscorr_e1t_epoch z = {};
  z.status = status;
  z.blksize = blk_d >= 0.0 && blk_d < 2147483648.0 ? (int32_t)blk_d : -1;
  z.segment = seg;
  return z;
}

// v with its sign flipped where s (0 or 0x80000000) says so: exactly +-v
__device__ __forceinline__ double flip(double v, uint32_t s) {
  return __hiloint2double(__double2hiint(v) ^ (int)s, __double2loint(v));
}

// MAXT: 64 = one wave per channel (many channels), 256 the default shape.
template <int FT, bool CLOSED, int MAXT>
__global__ __launch_bounds__(MAXT, MAXT == 64 ? 2 : 1) void e1t_track_kernel(
    E1tParams p, const int8_t* __restrict__ ifbuf, int64_t stride, int64_t n_samples,
    const uint32_t* __restrict__ codes, gnsscorr_e1t_chan* __restrict__ chans, int n_epochs,
    gnsscorr_e1t_epoch* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ uint32_t s_code[kCodeWords];        // four padded rows as bits (1 = chip -1)
  __shared__ double s_part[2][kMaxWaves][10];
  __shared__ double2 s_w[kC];                    // chunked path: exp(i*A*n/fs), n < kC
  const int ch = blockIdx.x;
  constexpr bool WAVE = MAXT == 64;
  const int T = WAVE ? 64 : blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nw = T >> 6;
  gnsscorr_e1t_chan c = chans[ch];
  // a code_id outside the uploaded table (reachable through track_dev only)
  if (c.status == 0 && (c.code_id < 0 || c.code_id >= p.n_codes)) c.status = 3;
  const int row = clampu(c.code_id, p.n_codes - 1);
  for (int i = tid; i < kCodeWords; i += T) s_code[i] = codes[(size_t)row * kCodeWords + i];
  __syncthreads();

  const int8_t* base = ifbuf + (int64_t)c.stream * stride;
  int e = 0;
  for (; e < n_epochs; e++) {
    gnsscorr_e1t_epoch* rec = out + (int64_t)ch * n_epochs + e;
    if (c.status != 0) {
      if (tid == 0) *rec = stop_record(c.status, 0.0, c.segment);
      continue;
    }
    const double cstep = c.code_freq / p.fs;
    const double mstep = c.meandr_freq / p.fs;
    const double blk_d = ceil(((double)kQuarter - c.rem_code) / cstep);
    // :282-286: not enough samples (a NaN, negative or huge blksize from a
    // corrupted state stops too, as does a position before the record)
    if (!(c.pos >= 0 && blk_d >= 1.0 && blk_d <= (double)(n_samples - c.pos) &&
          blk_d < 2147483648.0)) {
      c.status = 1;
      if (tid == 0) *rec = stop_record(1, blk_d, c.segment);
      continue;
    }
    const int blk = (int)blk_d;
    const double aE = c.rem_code - p.dspc, aL = c.rem_code + p.dspc, aP = c.rem_code;
    const double bE = c.rem_meandr - p.sspc, bL = c.rem_meandr + p.sspc, bP = c.rem_meandr;
    // the subcarrier range follows the code NCO's blksize: when its first early
    // or last late index ceil(t) + 1 leaves 1..2050 Scilab aborts on the index
    {
      const double lo = ceil(bE), hi = ceil(bL + (double)(blk - 1) * mstep);
      if (!(mstep > 0.0 && lo >= 0.0 && hi <= (double)(kMeandrTab - 1))) {
        c.status = 2;
        if (tid == 0) *rec = stop_record(2, blk_d, c.segment);
        continue;
      }
    }
    const double A = (c.carr_freq * 2.0) * M_PI;        // (carrFreq * 2.0 * %pi)
    const int8_t* src = base + (FT == 2 ? 2 : 1) * c.pos;
    const uint32_t* srow = s_code + c.segment * kRowWords;
    // bit of padded-row entry j (0-based; the clamp only keeps a state set from
    // outside inside the row: the loop's own indices lie in [0, 1024])
    auto cbit = [&](int j) -> uint32_t {
      const int i = clampu(j, kRowLen - 1);
      return (srow[i >> 5] >> (i & 31)) & 1u;
    };
    double acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // I_E_P I_P_E I_P_P I_P_L I_L_P, Q the same

    // ---- per-sample path
    auto run = [&]() {
      const double th0 = A * ((double)tid / p.fs) + c.rem_carr, thw = A * ((double)T / p.fs);
      double sn, cs, sw, cw;
      sincos(th0, &sn, &cs);
      sincos(thw, &sw, &cw);   // (e1t.o is built with promote-alloca-to-lds off)
      auto load = [&](int k) -> int {
        if (FT == 2) return *reinterpret_cast<const uint16_t*>(src + 2 * (int64_t)k);
        return src[k];
      };
      auto sample = [&](int k, int w) {
        const double kd = (double)k;
        const double tc = kd * cstep, tm = kd * mstep;
        const uint32_t gE = cbit((int)ceil(aE + tc));
        const uint32_t gP = cbit((int)ceil(aP + tc));
        const uint32_t gL = cbit((int)ceil(aL + tc));
        const uint32_t mE = (uint32_t)(int)ceil(bE + tm) & 1u;   // -1 iff ceil(t) is odd
        const uint32_t mP = (uint32_t)(int)ceil(bP + tm) & 1u;
        const uint32_t mL = (uint32_t)(int)ceil(bL + tm) & 1u;
        double re, im;
        if (FT == 2) {
          re = (double)(int)__builtin_amdgcn_sbfe(w, 0, 8);
          im = (double)(int)__builtin_amdgcn_sbfe(w, 8, 8);
        } else {
          re = (double)w;
          im = 0.0;
        }
        // (explicit fma: the carrier and the sums only need fp64 accuracy; the
        // indices above stay uncontracted and bit-exact)
        const double qb = fma(cs, re, -(sn * im));   // real(carrsig .* rawSignal)
        const double ib = fma(cs, im, sn * re);      // imag(carrsig .* rawSignal)
        const uint32_t sg[5] = {(mE ^ gP) << 31, (mP ^ gE) << 31, (mP ^ gP) << 31,
                                (mP ^ gL) << 31, (mL ^ gP) << 31};
#pragma unroll
        for (int a = 0; a < 5; a++) {
          acc[a] += flip(ib, sg[a]);
          acc[5 + a] += flip(qb, sg[a]);
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
    };

    // ---- chunked path: chunk q holds samples k0 = q*kC - mis .. k0 + kC - 1 (the
    // 16-byte grid of the stream), q = tid + it*T
    constexpr int kBps = FT == 2 ? 2 : 1;
    auto run_chunks = [&]() {
      using Grid = ChunkGrid<kBps, kC>;
      const Grid grid(src, blk, T);
      const double cst = uni(cstep), mst = uni(mstep);
      const double inv_c = uni(1.0 / cstep), inv_m = uni(1.0 / mstep);
      const double aX[3] = {uni(aE), uni(aP), uni(aL)};
      const double bX[3] = {uni(bE), uni(bP), uni(bL)};
      double sb, cb, sR, cR;
      sincos(A * ((double)(tid * kC - grid.mis) / p.fs) + c.rem_carr, &sb, &cb);
      if (tid < kC) {
        double swl, cwl;
        sincos(A * ((double)tid / p.fs), &swl, &cwl);
        s_w[tid] = make_double2(cwl, swl);
      }
      sincos(A * ((double)(T * kC) / p.fs), &sR, &cR);   // the carrier T chunks on
      sR = uni(sR);
      cR = uni(cR);
      __syncthreads();
      constexpr int kW = Grid::kW;   // 16-byte words per chunk
      uint4 nx[kW];
      auto fetch = [&](int it, uint4 (&x)[kW]) {
        const int q = it * T + tid;
#pragma unroll
        for (int u = 0; u < kW; u++) {
          // only words holding a sample of the epoch: none past the record's end
          const int ks = q * kC - grid.mis + u * (16 / kBps);
          x[u] = ks < blk ? grid.ab[(int64_t)q * kW + u] : make_uint4(0, 0, 0, 0);
        }
      };
      fetch(0, nx);
      for (int it = 0; it < grid.nIt; it++) {
        uint32_t wd[4 * kW];
#pragma unroll
        for (int u = 0; u < kW; u++) {
          wd[4 * u] = nx[u].x; wd[4 * u + 1] = nx[u].y;
          wd[4 * u + 2] = nx[u].z; wd[4 * u + 3] = nx[u].w;
        }
        if (it + 1 < grid.nIt) fetch(it + 1, nx);
        const int q = it * T + tid;
        const int k0 = q * kC - grid.mis;
        // the epoch's first and last chunks: samples outside [0, blk) count as 0
        if (k0 < 0 || k0 + kC > blk) {
#pragma unroll
          for (int n = 0; n < kC; n++) {
            const bool v = (unsigned)(k0 + n) < (unsigned)blk;
            constexpr int kSpw = 4 / kBps;   // samples per dword
            const uint32_t m = (kBps == 2 ? 0xffffu : 0xffu) << (8 * kBps * (n % kSpw));
            wd[n / kSpw] &= v ? 0xffffffffu : ~m;
          }
        }
        // sign masks of the six sequences over the chunk (bit n: sample k0 + n is -1)
        const double kd0 = (double)k0;
        const double tc0 = kd0 * cst, tm0 = kd0 * mst;
        uint32_t mc[3], ms[3];
        bool risky = false;
        auto low = [](int b) -> uint32_t { return (1u << b) - 1u; };   // b <= kC < 32
#pragma unroll
        for (int x = 0; x < 3; x++) {
          const double jf = ceil(aX[x] + tc0);
          const int j0 = (int)jf;
          const int beta = Grid::crossing(jf, aX[x], inv_c, k0, risky);   // one step at most: 15*cstep < 1
          const uint32_t g0 = 0u - cbit(j0), g1 = 0u - cbit(j0 + 1);
          mc[x] = (g0 & low(beta)) | (g1 & ~low(beta));
          const double hf = ceil(bX[x] + tm0);
          const int b1 = Grid::crossing(hf, bX[x], inv_m, k0, risky);     // two at most: 15*mstep < 2
          const int b2 = max(Grid::crossing(hf + 1.0, bX[x], inv_m, k0, risky), b1);
          const uint32_t flipd = low(b1) ^ low(b2);             // samples [b1, b2): the other sign
          ms[x] = ((int)hf & 1) ? ~flipd : flipd;
        }
        if (risky && q < grid.nC) {
          // a crossing without margin: the chunk's masks from the exact indices
          for (int x = 0; x < 3; x++) mc[x] = ms[x] = 0;
#pragma unroll 1
          for (int n = 0; n < kC; n++) {
            const double kd = (double)(k0 + n);
            const double tc = kd * cst, tm = kd * mst;
#pragma unroll
            for (int x = 0; x < 3; x++) {
              mc[x] |= cbit((int)ceil(aX[x] + tc)) << n;
              ms[x] |= ((uint32_t)(int)ceil(bX[x] + tm) & 1u) << n;
            }
          }
        }
        const uint32_t am[5] = {ms[0] ^ mc[1], ms[1] ^ mc[0], ms[1] ^ mc[1], ms[1] ^ mc[2],
                                ms[2] ^ mc[1]};
        double Ur[5] = {0, 0, 0, 0, 0}, Ui[5] = {0, 0, 0, 0, 0};
        // the W_n reads are loop invariant: an opaque offset per chunk keeps them
        // from being hoisted out of the chunk loop (16 complex in VGPRs)
        int wo = 0;
        asm volatile("" : "+v"(wo));
#pragma unroll
        for (int n = 0; n < kC; n++) {
          double ur, ui;
          const double2 W = s_w[n + wo];   // broadcast read
          if constexpr (FT == 2) {
            const uint32_t w = wd[n >> 1];
            const int sh = (n & 1) * 16;
            const double re = (double)(int)__builtin_amdgcn_sbfe(w, sh, 8);
            const double im = (double)(int)__builtin_amdgcn_sbfe(w, sh + 8, 8);
            ur = fma(W.x, re, -(W.y * im));   // W_n * raw
            ui = fma(W.x, im, W.y * re);
          } else {
            const double re = (double)(int)__builtin_amdgcn_sbfe(wd[n >> 2], (n & 3) * 8, 8);
            ur = W.x * re;
            ui = W.y * re;
          }
#pragma unroll
          for (int a = 0; a < 5; a++) {
            // +-1.0 from bit n of the arm's mask (only the high word differs)
            const uint32_t hi = ((am[a] << (31 - n)) & 0x80000000u) | 0x3ff00000u;
            const double g = __hiloint2double((int)hi, 0);
            Ur[a] = fma(ur, g, Ur[a]);
            Ui[a] = fma(ui, g, Ui[a]);
          }
        }
        // exp(i theta_k0) * U: imaginary part -> I (iBasebandSignal), real -> Q
#pragma unroll
        for (int a = 0; a < 5; a++) {
          acc[a] = fma(sb, Ur[a], fma(cb, Ui[a], acc[a]));
          acc[5 + a] = fma(cb, Ur[a], fma(-sb, Ui[a], acc[5 + a]));
        }
        rotate(sb, cb, sR, cR);
      }
    };
    // chunks need every index inside its table without the clamp mattering
    // (remCode in the loop's own range) and at most one code step and two
    // subcarrier steps in 16 samples
    const bool chunked = p.chunked && c.rem_code >= p.dspc - 1.0 && p.dspc >= 0.0 &&
                         p.dspc < 0.99 && (double)(kC - 1) * cstep < 0.999 &&
                         (double)(kC - 1) * mstep < 1.999 && ((uintptr_t)src & (kBps - 1)) == 0;
    if (chunked) run_chunks();
    else run();
    double S[10];
#pragma unroll
    for (int j = 0; j < 10; j++) S[j] = wave_sum(acc[j]);
    if constexpr (!WAVE) {
      const int par = e & 1;
      if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 10; j++) s_part[par][wave][j] = S[j];
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 10; j++) S[j] = 0.0;
      for (int w = 0; w < nw; w++)
#pragma unroll
        for (int j = 0; j < 10; j++) S[j] += s_part[par][w][j];
    }
    const gnsscorr_e1t_epoch r = e1t_epoch_end<CLOSED>(p, c, blk, cstep, mstep, S);
    if (tid == 0) *rec = r;
  }
  if (tid == 0) chans[ch] = c;
}

// The loop half alone: each thread runs one channel's epochs on given sums
// (sums[(ch*n_epochs + e)*10 + j]).  There is no record, so no status 1 or 2; a
// NaN / negative / >= 2^31 blksize stops the channel with status 1.
__global__ void e1t_replay_kernel(E1tParams p, gnsscorr_e1t_chan* __restrict__ chans, int n_ch,
                                  int n_epochs, const double* __restrict__ sums,
                                  gnsscorr_e1t_epoch* __restrict__ out) {
#pragma clang fp contract(off)
  const int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= n_ch) return;
  gnsscorr_e1t_chan c = chans[ch];
  for (int e = 0; e < n_epochs; e++) {
    gnsscorr_e1t_epoch* rec = out + (int64_t)ch * n_epochs + e;
    if (c.status != 0) {
      *rec = stop_record(c.status, 0.0, c.segment);
      continue;
    }
    const double cstep = c.code_freq / p.fs;
    const double mstep = c.meandr_freq / p.fs;
    const double blk_d = ceil(((double)kQuarter - c.rem_code) / cstep);
    if (!(blk_d >= 1.0 && blk_d < 2147483648.0)) {
      c.status = 1;
      *rec = stop_record(1, blk_d, c.segment);
      continue;
    }
    const double* sp = sums + ((int64_t)ch * n_epochs + e) * 10;
    const double S[10] = {sp[0], sp[1], sp[2], sp[3], sp[4], sp[5], sp[6], sp[7], sp[8], sp[9]};
    *rec = e1t_epoch_end<true>(p, c, (int)blk_d, cstep, mstep, S);
  }
  chans[ch] = c;
}

}  // namespace

// ============================================================================
// host side
// ============================================================================
struct gnsscorr_e1t_ctx {
  gnsscorr_e1t_cfg cfg;
  E1tParams p;
  hipStream_t stream = nullptr;
  uint32_t* d_codes = nullptr;
  int max_codes = 0;
  hostctx::DevBuf<gnsscorr_e1t_chan> d_chan;   // the host wrappers' own
  hostctx::DevBuf<gnsscorr_e1t_epoch> d_ep;
};

extern "C" void gnsscorr_e1t_loop_coefs(const gnsscorr_e1t_cfg* cfg, double* tau1c, double* tau2c,
                                        double* tau1m, double* tau2m, double* k1, double* k2,
                                        double* k3) {
  calc_loop_coef(cfg->dll_noise_bw, cfg->dll_damping, tau1c, tau2c);
  calc_loop_coef(cfg->sll_noise_bw, cfg->sll_damping, tau1m, tau2m);
  calc_fll_pll_loop_coef(cfg->pll_noise_bw, cfg->fll_noise_bw, k1, k2, k3);
}

static int check_cfg(const gnsscorr_e1t_cfg* cfg) {
  if (!cfg || (cfg->file_type != 1 && cfg->file_type != 2) || !(cfg->samp_rate > 0) ||
      !(cfg->code_freq_basis > 0) || !(cfg->meandr_freq_basis > 0) || cfg->code_length != kChips ||
      cfg->meandr_length != 2 * kChips || !(cfg->dll_spacing >= 0 && cfg->dll_spacing < 1) ||
      !(cfg->sll_spacing >= 0 && cfg->sll_spacing < 1) || cfg->max_codes < 0) {
    gnsscorr_set_error("e1t: bad config (file_type 1/2, code_length 4092, meandr_length 8184, "
                       "0<=dll_spacing<1, 0<=sll_spacing<1, positive rates)");
    return GNSSCORR_EINVAL;
  }
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_e1t_init_chan(const gnsscorr_e1t_cfg* cfg, int code_id, int stream,
                                      int64_t skip, int64_t code_phase_1b, double acq_freq,
                                      gnsscorr_e1t_chan* o) {
  int rc = check_cfg(cfg);
  if (rc) return rc;
  if (!o || code_phase_1b < 1 || stream < 0 || skip < 0 || code_id < 0) {
    gnsscorr_set_error("gnsscorr_e1t_init_chan: bad channel (code_id >= 0, code_phase >= 1)");
    return GNSSCORR_EINVAL;
  }
  memset(o, 0, sizeof *o);
  o->code_id = code_id;
  o->stream = stream;
  o->pos = skip + code_phase_1b - 1;   // mseek, tracking.sci:150-151
  o->code_freq = cfg->code_freq_basis;
  o->meandr_freq = cfg->meandr_freq_basis;
  o->carr_freq = o->carr_freq_basis = acq_freq;
  o->i1 = o->q1 = 0.001;               // tracking.sci:205
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_e1t_destroy(gnsscorr_e1t_ctx* c) { return ftrack::destroy(c); }

// the stream and room for the code rows (gnsscorr_e1t_set_codes fills them)
static int init_device(gnsscorr_e1t_ctx* c) {
  HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  HIP_TRY(hipMalloc(&c->d_codes, sizeof(uint32_t) * (size_t)c->max_codes * kCodeWords));
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_e1t_create(gnsscorr_e1t_ctx** out, const gnsscorr_e1t_cfg* cfg) {
  if (!out) return GNSSCORR_EINVAL;
  *out = nullptr;
  int rc = check_cfg(cfg);
  if (rc) return rc;
  rc = hostctx::open_device(__func__, cfg->device);
  if (rc) return rc;
  auto* c = new gnsscorr_e1t_ctx();
  c->cfg = *cfg;
  c->max_codes = cfg->max_codes > 0 ? cfg->max_codes : 50;   // settings.NumberOfE1BCodes
  E1tParams& p = c->p;
  p.file_type = cfg->file_type;
  // GNSSCORR_E1T_CHUNK=0: the per-sample path only (A/B and tests)
  const char* chk = getenv("GNSSCORR_E1T_CHUNK");
  p.chunked = !(chk && chk[0] == '0');
  p.n_codes = 0;
  p.fs = cfg->samp_rate;
  p.code_basis = cfg->code_freq_basis;
  p.meandr_basis = cfg->meandr_freq_basis;
  p.if_freq = cfg->if_freq;
  p.dspc = cfg->dll_spacing;
  p.sspc = cfg->sll_spacing;
  p.code_len = (double)cfg->code_length;
  gnsscorr_e1t_loop_coefs(cfg, &p.tau1c, &p.tau2c, &p.tau1m, &p.tau2m, &p.k1, &p.k2, &p.k3);
  rc = init_device(c);
  if (rc) {
    gnsscorr_e1t_destroy(c);
    return rc;
  }
  *out = c;
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_e1t_set_codes(gnsscorr_e1t_ctx* c, int n_codes, const int8_t* chips) {
  // the chips first: a value other than +-1 is refused before anything else
  if (chips && n_codes >= 1) {
    for (size_t i = 0; i < (size_t)n_codes * kChips; i++) {
      if (chips[i] != 1 && chips[i] != -1) {
        gnsscorr_set_error("gnsscorr_e1t_set_codes: chips must be +-1 (code %d, chip %d is %d)",
                           (int)(i / kChips), (int)(i % kChips), (int)chips[i]);
        return GNSSCORR_EINVAL;
      }
    }
  }
  if (!c || !chips || n_codes < 1 || n_codes > c->max_codes) {
    gnsscorr_set_error("gnsscorr_e1t_set_codes: bad arguments (1 <= n_codes <= max_codes)");
    return GNSSCORR_EINVAL;
  }
  // the four padded rows of tracking.sci:157-160 as bits (1 = chip -1):
  //   row s = [c(1023 s) c(1023 s + 1 : 1023 s + 1023) c(1023 s + 1024)], 1-based
  //   with c(0) = c(4092) and c(4093) = c(1): the pads of rows 1 and 4 wrap
  uint32_t* h = (uint32_t*)calloc((size_t)n_codes * kCodeWords, sizeof(uint32_t));
  if (!h) return GNSSCORR_EINVAL;
  for (int r = 0; r < n_codes; r++) {
    const int8_t* code = chips + (size_t)r * kChips;
    for (int s = 0; s < 4; s++) {
      uint32_t* row = h + (size_t)r * kCodeWords + s * kRowWords;
      for (int j = 0; j < kRowLen; j++) {
        const int chip = (s * kQuarter + j - 1 + kChips) % kChips;
        if (code[chip] < 0) row[j >> 5] |= 1u << (j & 31);
      }
    }
  }
  hipError_t e = hipSetDevice(c->cfg.device);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // no launch still reads the old rows
  if (e == hipSuccess)
    e = hipMemcpy(c->d_codes, h, sizeof(uint32_t) * (size_t)n_codes * kCodeWords,
                  hipMemcpyHostToDevice);
  free(h);
  if (e != hipSuccess) {
    gnsscorr_set_error("gnsscorr_e1t_set_codes: %s", hipGetErrorString(e));
    return GNSSCORR_EDEVICE;
  }
  c->p.n_codes = n_codes;
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_e1t_track_dev(gnsscorr_e1t_ctx* c, const int8_t* d_if, int64_t stride,
                                      int64_t n_samples, int n_ch, gnsscorr_e1t_chan* d_chan,
                                      int n_epochs, int closed_loop, gnsscorr_e1t_epoch* d_ep) {
  int rc = check_track_dev(__func__, c, d_if, d_chan, d_ep, n_ch, n_epochs, n_samples, stride);
  if (rc) return rc;
  if (c->p.n_codes < 1) {
    gnsscorr_set_error("gnsscorr_e1t_track_dev: no codes (call gnsscorr_e1t_set_codes first)");
    return GNSSCORR_EINVAL;
  }
  rc = check_iq_aligned(__func__, c, d_if);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  // two launch shapes: one wave per channel for many channels (throughput),
  // 256-thread workgroups otherwise (epoch latency of a receiver's worth of
  // channels).  GNSSCORR_E1T_THREADS overrides (64 = wave mode, 128, 256).
  int T = n_ch >= 1024 ? 64 : 256;
  if (const char* ov = getenv("GNSSCORR_E1T_THREADS")) {
    const int v = atoi(ov);
    if (v == 64 || v == 128 || v == 256) T = v;
  }
  dim3 grid(n_ch), block(T);
#define E1T_LAUNCH(FT, CL)                                                                    \
  do {                                                                                        \
    if (T == 64)                                                                              \
      hipLaunchKernelGGL((e1t_track_kernel<FT, CL, 64>), grid, block, 0, c->stream, c->p,    \
                         d_if, stride, n_samples, c->d_codes, d_chan, n_epochs, d_ep);        \
    else                                                                                      \
      hipLaunchKernelGGL((e1t_track_kernel<FT, CL, 256>), grid, block, 0, c->stream, c->p,   \
                         d_if, stride, n_samples, c->d_codes, d_chan, n_epochs, d_ep);        \
  } while (0)
  if (c->cfg.file_type == 2) {
    if (closed_loop) E1T_LAUNCH(2, true);
    else E1T_LAUNCH(2, false);
  } else {
    if (closed_loop) E1T_LAUNCH(1, true);
    else E1T_LAUNCH(1, false);
  }
#undef E1T_LAUNCH
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_e1t_track(gnsscorr_e1t_ctx* c, const int8_t* d_if, int64_t stride,
                                  int64_t n_samples, int n_ch, gnsscorr_e1t_chan* h_chan,
                                  int n_epochs, int closed_loop, gnsscorr_e1t_epoch* h_ep) {
  if (!c || !h_chan || !h_ep || n_ch < 1 || n_epochs < 1) return bad_arguments(__func__);
  if (c->p.n_codes < 1) {
    gnsscorr_set_error("gnsscorr_e1t_track: no codes (call gnsscorr_e1t_set_codes first)");
    return GNSSCORR_EINVAL;
  }
  for (int i = 0; i < n_ch; i++) {
    const int id = h_chan[i].code_id;
    if (id < 0 || id >= c->p.n_codes) {
      gnsscorr_set_error("gnsscorr_e1t_track: channel %d: code_id %d outside the %d uploaded codes",
                         i, id, c->p.n_codes);
      return GNSSCORR_EINVAL;
    }
  }
  return ftrack::track(c, n_ch, h_chan, n_epochs, h_ep,
                       [&](gnsscorr_e1t_chan* d_chan, gnsscorr_e1t_epoch* d_ep) {
                         return gnsscorr_e1t_track_dev(c, d_if, stride, n_samples, n_ch, d_chan,
                                                       n_epochs, closed_loop, d_ep);
                       });
}

extern "C" int gnsscorr_e1t_sync(gnsscorr_e1t_ctx* c) { return hostctx::sync(c); }

extern "C" void* gnsscorr_e1t_stream(gnsscorr_e1t_ctx* c) { return hostctx::stream(c); }

extern "C" int gnsscorr_e1t_replay_dev(gnsscorr_e1t_ctx* c, int n_ch, gnsscorr_e1t_chan* d_chan,
                                       int n_epochs, const double* d_sums,
                                       gnsscorr_e1t_epoch* d_ep) {
  return ftrack::replay_dev(__func__, c, e1t_replay_kernel, n_ch, d_chan, n_epochs, d_sums, d_ep);
}

extern "C" int gnsscorr_e1t_replay(gnsscorr_e1t_ctx* c, int n_ch, gnsscorr_e1t_chan* h_chan,
                                   int n_epochs, const double* h_sums, gnsscorr_e1t_epoch* h_ep) {
  return ftrack::replay<10>(__func__, c, n_ch, h_chan, n_epochs, h_sums, h_ep,
                            [&](gnsscorr_e1t_chan* d_chan, double* d_sums, gnsscorr_e1t_epoch* d_ep) {
                              return gnsscorr_e1t_replay_dev(c, n_ch, d_chan, n_epochs, d_sums, d_ep);
                            });
}
