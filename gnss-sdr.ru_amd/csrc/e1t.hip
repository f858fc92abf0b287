// e1t.hip -- Galileo E1B float tracking loops ("e1t") on gfx950.
//
// GALILEO/E1/tracking.sci:95-455 (mode 0): per 1-ms epoch (one quarter of the
// 4092-chip primary code) a code NCO over the quarter's padded 1025-entry row, an
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
// The three loops of GALILEO/E1/BOC_tracking_alternatives/ are modes of the same
// kernels, fixed at compile time (struct Mode; "4ms", "amb_1ms" and "amb_4ms"
// below are tracking_4ms.sci, tracking_ambiguous_1ms.sci and
// tracking_ambiguous_4ms.sci there):
//  mode 1, 4ms: the five arms over the whole code.  One padded 4094-entry row
//    [c($) c c(1)] (4ms:159), no quarters; blksize = ceil((4092 - remCode)/cstep)
//    (:261), carries - 4092.0 and - 8184.0 (:305, :328); every PDI 0.004
//    (:107,115,123).  The subcarrier table [m($) m m(1)] (:163-165) has a
//    one-entry front pad: entry j is +1 for even j, so the value at ceil(t) + 1
//    is -1 iff ceil(t) is even, the opposite sense of mode 0; it still
//    alternates over all 8186 entries, so parity stands in for the table here
//    too, and status 2 is ceil(remMeandr - sllSpc) < 0 or the last late
//    ceil(t) > 8185.
//  modes 2 and 3, amb_1ms / amb_4ms: BOC(1,1) as one sequence ca = kron(c, [1 1])
//    .* [+1 -1 ...] of 8184 entries (amb_1ms:141-145) clocked at 2 * codeFreqBasis
//    (:157), three arms E / P / L, six sums, PLL/FLL and DLL, no subcarrier loop.
//    amb_1ms: four padded rows of 2048 (:148-151), blksize = ceil((8184/4 -
//    remCode)/cstep) (:232), carry - 2046.0 and the row counter (:276-281), PDIs
//    0.001 (:98,107).  amb_4ms: one row [ca($) ca ca(1)] of 8186 (:146), blksize
//    = ceil((8184 - remCode)/cstep) (:224), carry - 8184.0 (:268), PDIcode 0.004
//    and PDIcarr 0.008 as written (:97,106).  Code aiding 2*basis - codeNco +
//    (carrFreq - IF)/770 (amb_1ms:351, amb_4ms:340); absoluteSample divides by
//    2*codeLength (amb_1ms:360-362).  The three-arm body has six accumulators;
//    I_E .. Q_L are recorded as the P-E, P-P, P-L slots of the ten.
//  Chunked path in the new modes.  4ms keeps the predicates of mode 0 (the steps
//    are the same); only the sizes grow: indices reach 8186 and k about 65 600.
//    crossing()'s estimate d = (j - a)*inv carries three roundings, 3.3e-16
//    relative, 2.2e-11 samples at d = 65 600; the exact index ceil(a + k*step) it
//    stands in for carries the roundings of k*step and of the sum, each at most
//    half an ulp of 8186 (9.1e-13 entries), which are 2.8e-11 samples at the
//    smallest step here (0.0625 entries per sample).  Together below 1e-10
//    samples, four orders inside the 1e-6 margin at which a lane falls back to
//    the exact per-sample indices.  The composite arm of the ambiguous modes
//    advances 0.128 entries per sample at 16 Msps, so it steps at most twice in
//    16 samples when 15*cstep < 1.999 (ceil(x + d) - ceil(x) <= ceil(d)): its
//    mask comes from the three row bits j0, j0+1, j0+2 and two crossings, as
//    the subcarrier masks do; its rounding bound is half the one above.
//
// Code table: the rows of a channel's code in LDS as bits, loaded once per
// launch: 4 x 36 words = 576 B (mode 0), 128 words = 512 B (mode 1), 4 x 64 or
// 256 words = 1 KiB (modes 2, 3).  LDS per workgroup in mode 0: 576 B rows +
// 256 B W table = 832 B in the one-wave-per-channel launch, + 640 B partials
// (2 parities x 4 waves x 10) = 1472 B in the 256-thread one.  Occupancy is
// bounded by registers (about 200 VGPRs: 2 waves per SIMD, which the launch
// bound asks for), not by LDS: 8 waves per CU take 6.5 KiB of the 160 KiB.
//
// Op model: 41 fp64 ops per sample in the five-arm modes (6 index adds, 6
// ceils, 2 k*step products, 4 carrier mix, 4 rotation, 10 sums, conversions),
// 22 in the ambiguous ones (3 adds, 3 ceils, 1 product, 4 + 4, 6 sums, 1).
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
constexpr int kQuarter = kChips / 4;        // 1023 chips per 1 ms epoch
constexpr int kMaxWaves = 4;
constexpr int kC = 16;                      // samples per chunk (chunked path)

// What a mode fixes at compile time.  MODE bit 0: the whole-code 4 ms epoch,
// bit 1: the ambiguous three-arm loop over the composite sequence.
//   0  tracking.sci                  1  tracking_4ms.sci
//   2  tracking_ambiguous_1ms.sci    3  tracking_ambiguous_4ms.sci
template <int MODE>
struct Mode {
  static constexpr bool kAmb = (MODE & 2) != 0, k4ms = (MODE & 1) != 0;
  static constexpr int kArms = kAmb ? 3 : 5;
  // entries one epoch runs over: 1023 chips (tracking.sci:266), 4092 chips
  // (4ms:261), 8184/4 composite entries (amb_1ms:232), 8184 (amb_4ms:224);
  // also what remCodePhase gives back at the epoch's end (tracking.sci:310,
  // 4ms:305, amb_1ms:276, amb_4ms:268)
  static constexpr int kEpochLen = (kAmb ? 2 : 1) * (k4ms ? kChips : kQuarter);
  static constexpr int kRowLen = kEpochLen + 2;   // one pad in front, one behind
  static constexpr int kRowWords = (((kRowLen + 31) / 32) + 3) & ~3;   // 16-byte multiple
  static constexpr int kRows = k4ms ? 1 : 4;
  static constexpr int kCodeWords = kRows * kRowWords;   // one code: 144, 128, 256, 256 words
  // five-arm modes: the subcarrier entries of an epoch (tracking.sci:338,
  // 4ms:328), its padded table ([m($-1) m($) m m(1) m(2)], tracking.sci:168;
  // [m($) m m(1)], 4ms:163-165) and the parity of ceil(t) at which the entry
  // ceil(t) + 1 is -1: the one-entry front pad of 4ms flips the sense
  static constexpr int kMeandrLen = k4ms ? 2 * kChips : 2 * kQuarter;
  static constexpr int kMeandrTab = kMeandrLen + (k4ms ? 2 : 4);
  static constexpr int kMeandrPar = k4ms ? 1 : 0;
  // PDIcode = PDImeandr (tracking.sci:107,115; 4ms:107,115; amb_1ms:98; amb_4ms:97)
  static constexpr double kPdi = k4ms ? 0.004 : 0.001;
  // carrier aiding of the code NCO (tracking.sci:407, 4ms:403; amb_1ms:351, amb_4ms:340)
  static constexpr int kAid = kAmb ? 770 : 1540;
};
static_assert(Mode<0>::kCodeWords == 144 && Mode<1>::kCodeWords == 128 &&
              Mode<2>::kCodeWords == 256 && Mode<3>::kCodeWords == 256, "LDS code rows");

// PDIcarr, the T of calcFLLPLLLoopCoef: tracking.sci:123, 4ms:123, amb_1ms:107
// and amb_4ms:106, which says 0.008 for its 4 ms epoch; kept as written
inline double pdi_carr(int mode) { return mode == 1 ? 0.004 : mode == 3 ? 0.008 : 0.001; }

// words per code of a mode's d_codes table
inline int code_words(int mode) { return mode == 0 ? Mode<0>::kCodeWords : mode == 1 ? Mode<1>::kCodeWords : 256; }

// code_basis, code_len: those of the mode (ambiguous: 2 * codeFreqBasis,
// amb_1ms:202, and 2 * codeLength, amb_1ms:91)
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
// The mode gives the row length, the carries, the PDI and the aiding divisor;
// the ambiguous modes (amb_1ms:276-367) read only the P-E, P-P and P-L slots
// of S (their I_E / I_P / I_L), leave the subcarrier state alone and record 0
// in the E-P / L-P slots and the subcarrier fields.
template <int MODE, bool CLOSED>
__device__ __forceinline__ gnsscorr_e1t_epoch e1t_epoch_end(const E1tParams& p,
                                                            gnsscorr_e1t_chan& c, int blk,
                                                            double cstep, double mstep,
                                                            const double (&S)[10]) {
#pragma clang fp contract(off)
  using M = Mode<MODE>;
  const double I_E_P = M::kAmb ? 0.0 : S[0], I_P_E = S[1], I_P_P = S[2], I_P_L = S[3];
  const double I_L_P = M::kAmb ? 0.0 : S[4];
  const double Q_E_P = M::kAmb ? 0.0 : S[5], Q_P_E = S[6], Q_P_P = S[7], Q_P_L = S[8];
  const double Q_L_P = M::kAmb ? 0.0 : S[9];
  const double A = (c.carr_freq * 2.0) * M_PI;        // (carrFreq * 2.0 * %pi)
  const int seg = c.segment;
  const double tlast = c.rem_code + (double)(blk - 1) * cstep;     // tcode(blksize), prompt
  c.rem_code = (tlast + cstep) - (double)M::kEpochLen;             // :310
  if constexpr (!M::k4ms) c.segment = (c.segment + 1) & 3;         // :312-315, amb_1ms:278-281
  if constexpr (!M::kAmb) {
    const double mlast = c.rem_meandr + (double)(blk - 1) * mstep;   // tmeandr(blksize), prompt
    c.rem_meandr = (mlast + mstep) - (double)M::kMeandrLen;          // :338
  }
  carry_carrier(c, A, blk, p.fs);                                  // :341-346
  c.pos += blk;
  double code_err = 0, meandr_err = 0, carr_err = 0;
  if (CLOSED) {
    carr_err = fll_pll_step(c, p.k1, p.k2, p.k3, I_P_P, Q_P_P);   // :371-389
    // DLL on P-E / P-L (:394-407)
    code_err = early_late_step(I_P_E, Q_P_E, I_P_L, Q_P_L, p.tau1c, p.tau2c, M::kPdi,
                               c.old_code_nco, c.old_code_error);
    const double code_nco = c.old_code_nco;
    c.code_freq = p.code_basis - code_nco + ((c.carr_freq - p.if_freq) / M::kAid);
    if constexpr (!M::kAmb) {
      // SLL on E-P / L-P (:412-425)
      meandr_err = early_late_step(I_E_P, Q_E_P, I_L_P, Q_L_P, p.tau1m, p.tau2m, M::kPdi,
                                   c.old_meandr_nco, c.old_meandr_error);
      const double meandr_nco = c.old_meandr_nco;
      c.meandr_freq = p.meandr_basis - meandr_nco + ((c.carr_freq - p.if_freq) / 770);
    }
  }
  c.n_epochs++;
  gnsscorr_e1t_epoch r;
  r.i_e_p = I_E_P; r.i_p_e = I_P_E; r.i_p_p = I_P_P; r.i_p_l = I_P_L; r.i_l_p = I_L_P;
  r.q_e_p = Q_E_P; r.q_p_e = Q_P_E; r.q_p_p = Q_P_P; r.q_p_l = Q_P_L; r.q_l_p = Q_L_P;
  r.carr_freq = c.carr_freq;
  r.code_freq = c.code_freq;
  r.meandr_freq = M::kAmb ? 0.0 : c.meandr_freq;
  // :433-435, the whole code length in the divisor as written there
  r.absolute_sample = (double)c.pos - c.rem_code * (p.fs / 1000) / p.code_len;
  r.dll_discr = code_err;
  r.dll_discr_filt = c.old_code_nco;
  r.sll_discr = meandr_err;
  r.sll_discr_filt = M::kAmb ? 0.0 : c.old_meandr_nco;
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
// FTP: settings.fileType (1, 2), + kPacked when the records are GNSSCORR_IF_PACKED2
// streams (gnsscorr_e1t_set_packed): unpacked in registers to the int8 words both
// paths consume, on the chunk grid of an int8 record with a 16-byte-aligned base, so
// the sums are the int8 path's to the bit.  Kernels of their own: the int8 ones keep
// their code and their symbols.
// FTP + kInt16 (gnsscorr_e1t_set_record_format(ctx, 2)): int16 records (if16.h).  Both
// paths take the int8 path's samples (the same chunk grid, in samples: a 16-sample I,Q
// chunk is 64 bytes) and convert the full 16 bits; kernels of their own again.
constexpr int kPacked = 4;
constexpr int kInt16 = 8;
template <int MODE, int FTP, bool CLOSED, int MAXT>
__global__ __launch_bounds__(MAXT, MAXT == 64 ? 2 : 1) void e1t_track_kernel(
    E1tParams p, const int8_t* __restrict__ ifbuf, int64_t stride, int64_t n_samples,
    const uint32_t* __restrict__ codes, gnsscorr_e1t_chan* __restrict__ chans, int n_epochs,
    gnsscorr_e1t_epoch* __restrict__ out) {
#pragma clang fp contract(off)
  constexpr int FT = FTP & 3;
  constexpr bool PK = (FTP & kPacked) != 0;
  constexpr bool I16 = (FTP & kInt16) != 0;
  using M = Mode<MODE>;
  constexpr int kCodeWords = M::kCodeWords, kRowWords = M::kRowWords, kRowLen = M::kRowLen;
  constexpr int kArms = M::kArms, kSums = 2 * M::kArms;
  __shared__ uint32_t s_code[kCodeWords];        // the padded rows as bits (1 = entry -1)
  __shared__ double s_part[2][kMaxWaves][kSums];
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
  // packed: the stream's bytes and the record's end (no byte at or past it is loaded)
  const uint8_t* pbase = reinterpret_cast<const uint8_t*>(base);
  const int64_t pend = if_bytes((FT == 2 ? 2 : 1) * n_samples, true);
  const int64_t end16 = (int64_t)if16_sample_bytes<FT>() * n_samples;   // int16: likewise
  int e = 0;
  for (; e < n_epochs; e++) {
    gnsscorr_e1t_epoch* rec = out + (int64_t)ch * n_epochs + e;
    if (c.status != 0) {
      if (tid == 0) *rec = stop_record(c.status, 0.0, c.segment);
      continue;
    }
    const double cstep = c.code_freq / p.fs;
    const double mstep = M::kAmb ? 0.0 : c.meandr_freq / p.fs;
    const double blk_d = ceil(((double)M::kEpochLen - c.rem_code) / cstep);
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
    // or last late index ceil(t) + 1 leaves 1..2050 (4 ms: 1..8186) Scilab aborts
    // on the index
    if constexpr (!M::kAmb) {
      const double lo = ceil(bE), hi = ceil(bL + (double)(blk - 1) * mstep);
      if (!(mstep > 0.0 && lo >= 0.0 && hi <= (double)(M::kMeandrTab - 1))) {
        c.status = 2;
        if (tid == 0) *rec = stop_record(2, blk_d, c.segment);
        continue;
      }
    }
    const double A = (c.carr_freq * 2.0) * M_PI;        // (carrFreq * 2.0 * %pi)
    // (packed: sample k is sample c.pos + k of pbase; src only keeps the predicate)
    // (int16: the epoch's first sample, at twice the bytes)
    const int8_t* src = PK ? base : base + (I16 ? 2 : 1) * (FT == 2 ? 2 : 1) * c.pos;
    const uint32_t* srow = s_code + (M::k4ms ? 0 : c.segment * kRowWords);   // 4 ms: one row
    // bit of padded-row entry j (0-based; the clamp only keeps a state set from
    // outside inside the row: the loop's own indices lie in [0, kRowLen - 1])
    auto cbit = [&](int j) -> uint32_t {
      const int i = clampu(j, kRowLen - 1);
      return (srow[i >> 5] >> (i & 31)) & 1u;
    };
    // five arms: I_E_P I_P_E I_P_P I_P_L I_L_P, Q the same; three: I_E I_P I_L, Q the same
    double acc[kSums];
#pragma unroll
    for (int j = 0; j < kSums; j++) acc[j] = 0.0;

    // ---- per-sample path
    auto run = [&]() {
      const double th0 = A * ((double)tid / p.fs) + c.rem_carr, thw = A * ((double)T / p.fs);
      double sn, cs, sw, cw;
      sincos(th0, &sn, &cs);
      sincos(thw, &sw, &cw);   // (e1t.o is built with promote-alloca-to-lds off)
      auto load = [&](int k) -> int {
        if constexpr (PK) return if2_sample<FT>(pbase, c.pos + k);
        if constexpr (I16) return if16_sample<FT>(pbase, c.pos + k);
        if (FT == 2) return *reinterpret_cast<const uint16_t*>(src + 2 * (int64_t)k);
        return src[k];
      };
      auto sample = [&](int k, int w) {
        const double kd = (double)k;
        const double tc = kd * cstep;
        const uint32_t gE = cbit((int)ceil(aE + tc));
        const uint32_t gP = cbit((int)ceil(aP + tc));
        const uint32_t gL = cbit((int)ceil(aL + tc));
        uint32_t sg[kArms];
        if constexpr (M::kAmb) {
          sg[0] = gE << 31; sg[1] = gP << 31; sg[2] = gL << 31;
        } else {
          const double tm = kd * mstep;
          // -1 iff ceil(t) is odd (4 ms: even)
          const uint32_t mE = (uint32_t)((int)ceil(bE + tm) + M::kMeandrPar) & 1u;
          const uint32_t mP = (uint32_t)((int)ceil(bP + tm) + M::kMeandrPar) & 1u;
          const uint32_t mL = (uint32_t)((int)ceil(bL + tm) + M::kMeandrPar) & 1u;
          sg[0] = (mE ^ gP) << 31; sg[1] = (mP ^ gE) << 31; sg[2] = (mP ^ gP) << 31;
          sg[3] = (mP ^ gL) << 31; sg[4] = (mL ^ gP) << 31;
        }
        double re, im;
        if constexpr (I16 && FT == 2) {
          re = (double)if16_half(w, 0);
          im = (double)if16_half(w, 16);
        } else if (FT == 2) {
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
#pragma unroll
        for (int a = 0; a < kArms; a++) {
          acc[a] += flip(ib, sg[a]);
          acc[kArms + a] += flip(qb, sg[a]);
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
      const Grid grid = [&] {
        if constexpr (PK || I16) return Grid(c.pos, blk, T);
        else return Grid(src, blk, T);
      }();
      const double cst = uni(cstep), mst = uni(mstep);
      const double inv_c = uni(1.0 / cstep), inv_m = M::kAmb ? 0.0 : uni(1.0 / mstep);
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
      constexpr int kW = Grid::kW;   // 16-byte words per chunk (packed: dwords)
      constexpr int kXW = I16 ? 2 * kW : kW;   // int16: the same samples in twice the words
      using Word = std::conditional_t<PK, uint32_t, uint4>;
      Word nx[kXW];
      auto fetch = [&](int it, Word (&x)[kXW]) {
        const int q = it * T + tid;
        if constexpr (I16) {
          // only words holding a sample of the epoch, cut at the record's end
          constexpr int kSw = 8 / kBps;   // samples per 16-byte word
          const int k0 = q * kC - grid.mis;
          const int64_t o = grid.first_byte16(c.pos, q);
#pragma unroll
          for (int u = 0; u < kXW; u++) {
            const int ks = k0 + u * kSw;
            x[u] = (ks < blk && ks + kSw > 0) ? if16_load_word(pbase, o + 16 * u, end16)
                                              : make_uint4(0, 0, 0, 0);
          }
        } else if constexpr (PK) {
          // the chunk's kW dwords: one load when the whole chunk lies in the epoch,
          // else only dwords holding a sample of the epoch, cut at the record's end
          const int k0 = q * kC - grid.mis;
          const int64_t d0 = grid.first_dword(c.pos) + (int64_t)q * kW;
          if (k0 + kC <= blk) {
            if2_load_words<kW>(reinterpret_cast<const uint32_t*>(pbase) + d0, x);
          } else {
#pragma unroll
            for (int u = 0; u < kW; u++)
              x[u] = k0 + u * (16 / kBps) < blk ? if2_load_dword(pbase, d0 + u, pend) : 0u;
          }
        } else {
#pragma unroll
        for (int u = 0; u < kW; u++) {
          // only words holding a sample of the epoch: none past the record's end
          const int ks = q * kC - grid.mis + u * (16 / kBps);
          x[u] = ks < blk ? grid.ab[(int64_t)q * kW + u] : make_uint4(0, 0, 0, 0);
        }
        }
      };
      fetch(0, nx);
      for (int it = 0; it < grid.nIt; it++) {
        uint32_t wd[4 * kXW];
#pragma unroll
        for (int u = 0; u < kXW; u++) {
          uint4 v;
          if constexpr (PK) v = if2_expand_word(nx[u]);   // 16 codes -> the four int8 words
          else v = nx[u];
          wd[4 * u] = v.x; wd[4 * u + 1] = v.y;
          wd[4 * u + 2] = v.z; wd[4 * u + 3] = v.w;
        }
        if (it + 1 < grid.nIt) fetch(it + 1, nx);
        const int q = it * T + tid;
        const int k0 = q * kC - grid.mis;
        // the epoch's first and last chunks: samples outside [0, blk) count as 0
        if (k0 < 0 || k0 + kC > blk) {
#pragma unroll
          for (int n = 0; n < kC; n++) {
            const bool v = (unsigned)(k0 + n) < (unsigned)blk;
            if constexpr (I16) {
              if constexpr (FT == 2) wd[n] = v ? wd[n] : 0u;
              else wd[n >> 1] &= v ? 0xffffffffu : ~(0xffffu << (16 * (n & 1)));
              continue;
            }
            constexpr int kSpw = 4 / kBps;   // samples per dword
            const uint32_t m = (kBps == 2 ? 0xffffu : 0xffu) << (8 * kBps * (n % kSpw));
            wd[n / kSpw] &= v ? 0xffffffffu : ~m;
          }
        }
        // sign masks of the sequences over the chunk (bit n: sample k0 + n is -1)
        const double kd0 = (double)k0;
        const double tc0 = kd0 * cst;
        uint32_t am[kArms];
        bool risky = false;
        auto low = [](int b) -> uint32_t { return (1u << b) - 1u; };   // b <= kC < 32
        if constexpr (M::kAmb) {
          // the composite arm steps at most twice: 15*cstep < 2
#pragma unroll
          for (int x = 0; x < 3; x++) {
            const double jf = ceil(aX[x] + tc0);
            const int j0 = (int)jf;
            const int b1 = Grid::crossing(jf, aX[x], inv_c, k0, risky);
            const int b2 = max(Grid::crossing(jf + 1.0, aX[x], inv_c, k0, risky), b1);
            const uint32_t g0 = 0u - cbit(j0), g1 = 0u - cbit(j0 + 1), g2 = 0u - cbit(j0 + 2);
            am[x] = (g0 & low(b1)) | (g1 & (low(b1) ^ low(b2))) | (g2 & ~low(b2));
          }
          if (risky && q < grid.nC) {
            // a crossing without margin: the chunk's masks from the exact indices
            for (int x = 0; x < 3; x++) am[x] = 0;
#pragma unroll 1
            for (int n = 0; n < kC; n++) {
              const double tc = (double)(k0 + n) * cst;
#pragma unroll
              for (int x = 0; x < 3; x++) am[x] |= cbit((int)ceil(aX[x] + tc)) << n;
            }
          }
        } else {
          const double tm0 = kd0 * mst;
          uint32_t mc[3], ms[3];
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
            ms[x] = (((int)hf + M::kMeandrPar) & 1) ? ~flipd : flipd;
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
                ms[x] |= ((uint32_t)((int)ceil(bX[x] + tm) + M::kMeandrPar) & 1u) << n;
              }
            }
          }
          am[0] = ms[0] ^ mc[1]; am[1] = ms[1] ^ mc[0]; am[2] = ms[1] ^ mc[1];
          am[3] = ms[1] ^ mc[2]; am[4] = ms[2] ^ mc[1];
        }
        double Ur[kArms], Ui[kArms];
#pragma unroll
        for (int a = 0; a < kArms; a++) Ur[a] = Ui[a] = 0.0;
        // the W_n reads are loop invariant: an opaque offset per chunk keeps them
        // from being hoisted out of the chunk loop (16 complex in VGPRs)
        int wo = 0;
        asm volatile("" : "+v"(wo));
#pragma unroll
        for (int n = 0; n < kC; n++) {
          double ur, ui;
          const double2 W = s_w[n + wo];   // broadcast read
          if constexpr (I16) {
            // the int8 forms below on the full 16 bits
            const double re = (double)if16_re<FT>(wd, n, 0);
            if constexpr (FT == 2) {
              const double im = (double)if16_im<FT>(wd, n, 0);
              ur = fma(W.x, re, -(W.y * im));
              ui = fma(W.x, im, W.y * re);
            } else {
              ur = W.x * re;
              ui = W.y * re;
            }
          } else if constexpr (FT == 2) {
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
          for (int a = 0; a < kArms; a++) {
            // +-1.0 from bit n of the arm's mask (only the high word differs)
            const uint32_t hi = ((am[a] << (31 - n)) & 0x80000000u) | 0x3ff00000u;
            const double g = __hiloint2double((int)hi, 0);
            Ur[a] = fma(ur, g, Ur[a]);
            Ui[a] = fma(ui, g, Ui[a]);
          }
        }
        // exp(i theta_k0) * U: imaginary part -> I (iBasebandSignal), real -> Q
#pragma unroll
        for (int a = 0; a < kArms; a++) {
          acc[a] = fma(sb, Ur[a], fma(cb, Ui[a], acc[a]));
          acc[kArms + a] = fma(cb, Ur[a], fma(-sb, Ui[a], acc[kArms + a]));
        }
        rotate(sb, cb, sR, cR);
      }
    };
    // chunks need every index inside its table without the clamp mattering
    // (remCode in the loop's own range) and at most one code step and two
    // subcarrier steps in 16 samples (ambiguous: two steps of the composite arm)
    const bool chunked = p.chunked && c.rem_code >= p.dspc - 1.0 && p.dspc >= 0.0 &&
                         p.dspc < 0.99 && (double)(kC - 1) * cstep < (M::kAmb ? 1.999 : 0.999) &&
                         (M::kAmb || (double)(kC - 1) * mstep < 1.999) &&
                         ((uintptr_t)src & (kBps - 1)) == 0;
    if (chunked) run_chunks();
    else run();
    double R[kSums];
#pragma unroll
    for (int j = 0; j < kSums; j++) R[j] = wave_sum(acc[j]);
    if constexpr (!WAVE) {
      const int par = e & 1;
      if (lane == 0) {
#pragma unroll
        for (int j = 0; j < kSums; j++) s_part[par][wave][j] = R[j];
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < kSums; j++) R[j] = 0.0;
      for (int w = 0; w < nw; w++)
#pragma unroll
        for (int j = 0; j < kSums; j++) R[j] += s_part[par][w][j];
    }
    double S[10];
    if constexpr (M::kAmb) {
      // I_E I_P I_L Q_E Q_P Q_L in the P-E, P-P, P-L slots
      S[0] = S[4] = S[5] = S[9] = 0.0;
      S[1] = R[0]; S[2] = R[1]; S[3] = R[2]; S[6] = R[3]; S[7] = R[4]; S[8] = R[5];
    } else {
#pragma unroll
      for (int j = 0; j < 10; j++) S[j] = R[j];
    }
    const gnsscorr_e1t_epoch r = e1t_epoch_end<MODE, CLOSED>(p, c, blk, cstep, mstep, S);
    if (tid == 0) *rec = r;
  }
  if constexpr (MODE == 0) {
    if (tid == 0) chans[ch] = c;
  } else if (tid == 0) {
    // only what this instantiation can change: a field that the whole-struct
    // copy merely carries from the load to the store is parked in scratch
    gnsscorr_e1t_chan& g = chans[ch];
    g.status = c.status;
    g.n_epochs = c.n_epochs;
    g.pos = c.pos;
    g.rem_code = c.rem_code;
    g.rem_carr = c.rem_carr;
    if constexpr (!M::k4ms) g.segment = c.segment;
    if constexpr (!M::kAmb) g.rem_meandr = c.rem_meandr;
    if constexpr (CLOSED) {
      g.code_freq = c.code_freq;
      g.carr_freq = c.carr_freq;
      g.old_code_nco = c.old_code_nco;
      g.old_code_error = c.old_code_error;
      g.old_carr_nco = c.old_carr_nco;
      g.old_carr_error = c.old_carr_error;
      g.i1 = c.i1;
      g.q1 = c.q1;
      if constexpr (!M::kAmb) {
        g.meandr_freq = c.meandr_freq;
        g.old_meandr_nco = c.old_meandr_nco;
        g.old_meandr_error = c.old_meandr_error;
      }
    }
  }
}

// The loop half alone: each thread runs one channel's epochs on given sums
// (sums[(ch*n_epochs + e)*10 + j]).  There is no record, so no status 1 or 2; a
// NaN / negative / >= 2^31 blksize stops the channel with status 1.
template <int MODE>
__global__ void e1t_replay_kernel(E1tParams p, gnsscorr_e1t_chan* __restrict__ chans, int n_ch,
                                  int n_epochs, const double* __restrict__ sums,
                                  gnsscorr_e1t_epoch* __restrict__ out) {
#pragma clang fp contract(off)
  using M = Mode<MODE>;
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
    const double mstep = M::kAmb ? 0.0 : c.meandr_freq / p.fs;
    const double blk_d = ceil(((double)M::kEpochLen - c.rem_code) / cstep);
    if (!(blk_d >= 1.0 && blk_d < 2147483648.0)) {
      c.status = 1;
      *rec = stop_record(1, blk_d, c.segment);
      continue;
    }
    const double* sp = sums + ((int64_t)ch * n_epochs + e) * 10;
    const double S[10] = {sp[0], sp[1], sp[2], sp[3], sp[4], sp[5], sp[6], sp[7], sp[8], sp[9]};
    *rec = e1t_epoch_end<MODE, true>(p, c, (int)blk_d, cstep, mstep, S);
  }
  chans[ch] = c;
}

// cfg -> mode; -1 for values outside the table in include/gnsscorr.h
inline int cfg_mode(const gnsscorr_e1t_cfg* cfg) {
  const int ms = cfg->epoch_ms, amb = cfg->ambiguous;
  if ((ms != 0 && ms != 1 && ms != 4) || (amb != 0 && amb != 1)) return -1;
  return (ms == 4 ? 1 : 0) | (amb ? 2 : 0);
}

}  // namespace

// ============================================================================
// host side
// ============================================================================
struct gnsscorr_e1t_ctx {
  gnsscorr_e1t_cfg cfg;
  E1tParams p;
  int mode = 0;                                // 0..3, struct Mode
  hipStream_t stream = nullptr;
  uint32_t* d_codes = nullptr;                 // code_words(mode) words per code
  int max_codes = 0;
  hostctx::DevBuf<gnsscorr_e1t_chan> d_chan;   // the host wrappers' own
  hostctx::DevBuf<gnsscorr_e1t_epoch> d_ep;
  int packed = 0;                              // gnsscorr_e1t_set_packed
  int i16 = 0;                                 // gnsscorr_e1t_set_record_format(ctx, 2)
};

#define E1T_BAD_CONFIG                                                            \
  "e1t: bad config (file_type 1/2, code_length 4092, meandr_length 8184, "        \
  "0<=dll_spacing<1, 0<=sll_spacing<1, positive rates)"

static int check_cfg(const gnsscorr_e1t_cfg* cfg) {
  if (!cfg || (cfg->file_type != 1 && cfg->file_type != 2) || !(cfg->samp_rate > 0) ||
      !(cfg->code_freq_basis > 0) || !(cfg->meandr_freq_basis > 0) || cfg->code_length != kChips ||
      cfg->meandr_length != 2 * kChips || !(cfg->dll_spacing >= 0 && cfg->dll_spacing < 1) ||
      !(cfg->sll_spacing >= 0 && cfg->sll_spacing < 1) || cfg->max_codes < 0) {
    gnsscorr_set_error(E1T_BAD_CONFIG);
    return GNSSCORR_EINVAL;
  }
  if (cfg_mode(cfg) < 0) {
    gnsscorr_set_error(E1T_BAD_CONFIG ": epoch_ms 0/1/4, ambiguous 0/1 (got %d, %d)",
                       (int)cfg->epoch_ms, (int)cfg->ambiguous);
    return GNSSCORR_EINVAL;
  }
  return GNSSCORR_OK;
}
#undef E1T_BAD_CONFIG

extern "C" void gnsscorr_e1t_loop_coefs(const gnsscorr_e1t_cfg* cfg, double* tau1c, double* tau2c,
                                        double* tau1m, double* tau2m, double* k1, double* k2,
                                        double* k3) {
  const int mode = cfg_mode(cfg) < 0 ? 0 : cfg_mode(cfg);
  calc_loop_coef(cfg->dll_noise_bw, cfg->dll_damping, tau1c, tau2c);
  if (mode & 2) *tau1m = *tau2m = 0.0;   // no subcarrier loop
  else calc_loop_coef(cfg->sll_noise_bw, cfg->sll_damping, tau1m, tau2m);
  calc_fll_pll_loop_coef(cfg->pll_noise_bw, cfg->fll_noise_bw, k1, k2, k3, pdi_carr(mode));
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
  if (cfg->ambiguous) {
    o->code_freq = 2 * cfg->code_freq_basis;   // amb_1ms:157, amb_4ms:151; no subcarrier NCO
  } else {
    o->code_freq = cfg->code_freq_basis;
    o->meandr_freq = cfg->meandr_freq_basis;
  }
  o->carr_freq = o->carr_freq_basis = acq_freq;
  o->i1 = o->q1 = 0.001;               // tracking.sci:205
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_e1t_destroy(gnsscorr_e1t_ctx* c) { return ftrack::destroy(c); }

extern "C" int gnsscorr_e1t_set_packed(gnsscorr_e1t_ctx* c, int packed) {
  return ftrack::set_packed(__func__, c, packed);
}
extern "C" int gnsscorr_e1t_set_record_format(gnsscorr_e1t_ctx* c, int fmt) {
  return ftrack::set_record_format(__func__, c, fmt);
}

// the stream and room for the code rows (gnsscorr_e1t_set_codes fills them)
static int init_device(gnsscorr_e1t_ctx* c) {
  HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  HIP_TRY(hipMalloc(&c->d_codes,
                    sizeof(uint32_t) * (size_t)c->max_codes * (size_t)code_words(c->mode)));
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
  c->mode = cfg_mode(cfg);
  c->max_codes = cfg->max_codes > 0 ? cfg->max_codes : 50;   // settings.NumberOfE1BCodes
  const bool amb = (c->mode & 2) != 0;
  E1tParams& p = c->p;
  p.file_type = cfg->file_type;
  // GNSSCORR_E1T_CHUNK=0: the per-sample path only (A/B and tests)
  const char* chk = getenv("GNSSCORR_E1T_CHUNK");
  p.chunked = !(chk && chk[0] == '0');
  p.n_codes = 0;
  p.fs = cfg->samp_rate;
  p.code_basis = amb ? 2 * cfg->code_freq_basis : cfg->code_freq_basis;   // amb_1ms:202
  p.meandr_basis = cfg->meandr_freq_basis;
  p.if_freq = cfg->if_freq;
  p.dspc = cfg->dll_spacing;
  p.sspc = cfg->sll_spacing;
  p.code_len = (double)(amb ? 2 * cfg->code_length : cfg->code_length);   // amb_1ms:91
  gnsscorr_e1t_loop_coefs(cfg, &p.tau1c, &p.tau2c, &p.tau1m, &p.tau2m, &p.k1, &p.k2, &p.k3);
  rc = init_device(c);
  if (rc) {
    gnsscorr_e1t_destroy(c);
    return rc;
  }
  *out = c;
  return GNSSCORR_OK;
}

// The padded rows of one code as bits (1 = entry -1), each the window
// [len s - 1, len s + len] of the circular sequence (0-based), len entries per epoch:
//   mode 0  tracking.sci:157-160: row s = [c(1023 s) c(1023 s + 1 : 1023 s + 1023)
//           c(1023 s + 1024)], 1-based with c(0) = c(4092), c(4093) = c(1)
//   mode 1  4ms:159: [c($) c c(1)]
//   mode 2  amb_1ms:148-151: rows of ca = kron(c, [1 1]) .* [+1 -1 ...] (:141-145)
//   mode 3  amb_4ms:146: [ca($) ca ca(1)]
template <int MODE>
static void build_rows(const int8_t* code, uint32_t* dst) {
  using M = Mode<MODE>;
  constexpr int kSeq = M::kAmb ? 2 * kChips : kChips;
  for (int s = 0; s < M::kRows; s++) {
    uint32_t* row = dst + s * M::kRowWords;
    for (int j = 0; j < M::kRowLen; j++) {
      const int i = (s * M::kEpochLen + j - 1 + kSeq) % kSeq;
      // ca(i) = c(i / 2), negated on the second half of the chip
      const bool neg = M::kAmb ? ((code[i >> 1] < 0) != ((i & 1) != 0)) : code[i] < 0;
      if (neg) row[j >> 5] |= 1u << (j & 31);
    }
  }
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
  const size_t words = (size_t)code_words(c->mode);
  uint32_t* h = (uint32_t*)calloc((size_t)n_codes * words, sizeof(uint32_t));
  if (!h) return GNSSCORR_EINVAL;
  for (int r = 0; r < n_codes; r++) {
    const int8_t* code = chips + (size_t)r * kChips;
    uint32_t* dst = h + (size_t)r * words;
    switch (c->mode) {
      case 0: build_rows<0>(code, dst); break;
      case 1: build_rows<1>(code, dst); break;
      case 2: build_rows<2>(code, dst); break;
      default: build_rows<3>(code, dst); break;
    }
  }
  hipError_t e = hipSetDevice(c->cfg.device);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // no launch still reads the old rows
  if (e == hipSuccess)
    e = hipMemcpy(c->d_codes, h, sizeof(uint32_t) * (size_t)n_codes * words,
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
  if (!rc) rc = check_packed_aligned(__func__, c, d_if, stride);
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
#define E1T_LAUNCH(MD, FT, CL)                                                                \
  do {                                                                                        \
    if (T == 64)                                                                              \
      hipLaunchKernelGGL((e1t_track_kernel<MD, FT, CL, 64>), grid, block, 0, c->stream,      \
                         c->p, d_if, stride, n_samples, c->d_codes, d_chan, n_epochs, d_ep);  \
    else                                                                                      \
      hipLaunchKernelGGL((e1t_track_kernel<MD, FT, CL, 256>), grid, block, 0, c->stream,     \
                         c->p, d_if, stride, n_samples, c->d_codes, d_chan, n_epochs, d_ep);  \
  } while (0)
#define E1T_LAUNCH_FT(MD, FT)                 \
  do {                                        \
    if (closed_loop) E1T_LAUNCH(MD, FT, true);   \
    else E1T_LAUNCH(MD, FT, false);           \
  } while (0)
  // (packed records: the kernels of FT + kPacked; int16 records: FT + kInt16)
#define E1T_LAUNCH_MODE(MD)                   \
  do {                                        \
    if (c->cfg.file_type == 2) {              \
      if (c->packed) E1T_LAUNCH_FT(MD, 2 + kPacked);  \
      else if (c->i16) E1T_LAUNCH_FT(MD, 2 + kInt16);  \
      else E1T_LAUNCH_FT(MD, 2);              \
    } else {                                  \
      if (c->packed) E1T_LAUNCH_FT(MD, 1 + kPacked);  \
      else if (c->i16) E1T_LAUNCH_FT(MD, 1 + kInt16);  \
      else E1T_LAUNCH_FT(MD, 1);              \
    }                                         \
  } while (0)
  switch (c->mode) {
    case 0: E1T_LAUNCH_MODE(0); break;
    case 1: E1T_LAUNCH_MODE(1); break;
    case 2: E1T_LAUNCH_MODE(2); break;
    default: E1T_LAUNCH_MODE(3); break;
  }
#undef E1T_LAUNCH_MODE
#undef E1T_LAUNCH_FT
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
  if (!c) return bad_arguments(__func__);
  auto* kernel = c->mode == 0 ? e1t_replay_kernel<0> : c->mode == 1 ? e1t_replay_kernel<1>
               : c->mode == 2 ? e1t_replay_kernel<2> : e1t_replay_kernel<3>;
  return ftrack::replay_dev(__func__, c, kernel, n_ch, d_chan, n_epochs, d_sums, d_ep);
}

extern "C" int gnsscorr_e1t_replay(gnsscorr_e1t_ctx* c, int n_ch, gnsscorr_e1t_chan* h_chan,
                                   int n_epochs, const double* h_sums, gnsscorr_e1t_epoch* h_ep) {
  return ftrack::replay<10>(__func__, c, n_ch, h_chan, n_epochs, h_sums, h_ep,
                            [&](gnsscorr_e1t_chan* d_chan, double* d_sums, gnsscorr_e1t_epoch* d_ep) {
                              return gnsscorr_e1t_replay_dev(c, n_ch, d_chan, n_epochs, d_sums, d_ep);
                            });
}
