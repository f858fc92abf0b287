// acq64.hip -- parallel code-phase acquisition at the reference's precision
// (fp64), on gfx950.
//
// Reference: POSTPROCESSING_SCILAB_RECEIVERS/GPS/L1/acquisition.sci:46-192
// (GLONASS: GLONASS/L1/acquisition.sci:46-198), which Scilab evaluates in
// doubles:  X = fft(exp(i f 2 pi t) .* block), |ifft(X .* conj(fft(code)))|^2,
// keep the block with the larger maximum, then peak / code phase / second
// peak outside +-1 chip.  This file computes every one of those steps in fp64
// (wipe-off, forward transforms, products, inverse transform, powers and the
// comparisons), so rows agree with an fp64 evaluation to ~1e-13 relative.
//
// MI355X design
//  * A 1-ms row of N complex doubles (256 KiB at N = 16368) does not fit the
//    160 KiB LDS, so it lives in REGISTERS: T threads hold ~N/T complex values
//    each, and every FFT stage is a batch of small in-register DFTs.  Between
//    stages the row is exchanged through LDS in two halves -- the real parts
//    (N doubles = 128 KiB), then the imaginary parts -- so the LDS only ever
//    holds one fp64 plane of the row.
//  * Three stages N = R1 * R2 * R3 per plan, two exchanges per transform:
//      N = 16368 (16.368 Msps, BASELINE config 2): 16 x 33 x 31, Good-Thomas
//        prime-factor (pairwise coprime): no twiddles at all; the Ruritanian
//        input map and the CRT output map are folded into addressing, and the
//        spectra are stored pre-permuted so the hot loads stay coalesced;
//        512 threads, the 16 radix-31 groups beyond 512 are done as direct
//        31-term sums from a side copy;
//      N = 16000 (16 Msps, the Scilab receivers' initSettings.sci:69 default):
//        40 x 40 x 10 Cooley-Tukey (decimation in frequency), 400 threads,
//        every stage balanced (40 values per thread); inter-stage twiddles
//        W^(k m) are generated per group from one table load by a complex
//        recurrence (error ~1e-15).
//  * Small DFTs are compile-time compositions: symmetric prime kernels
//    (X_m = A_m - i B_m, X_{P-m} = A_m + i B_m), Good-Thomas for coprime
//    splits (33 = 3 x 11, 40 = 8 x 5, 10 = 2 x 5), Cooley-Tukey for prime
//    powers (16 = 4 x 4, 8 = 2 x 4); twiddle constants are constexpr-evaluated.
//  * The inverse FFT is a forward FFT of conj(Y): |ifft(Y)|^2 = |fft(conj Y)|^2 / N^2.
//  * The correlation kernel fuses conj(X)*F (with the bin's circular shift on
//    the fs/N grid folded into the X load), the three stages, |.|^2, the
//    non-coherent sum over blocks, and exact row statistics (acq_peak.h) in two
//    register passes.
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include "acq64_dft.h"
#include "acq_ctx.h"
#include "if2.h"
#include "if16.h"

// Diagnostic hook: tools/acq64_stamps.hip defines ACQ64_STAMP(i) to record
// s_memtime at the barriers of the correlation kernel; nothing in the library.
#ifndef ACQ64_STAMP
#define ACQ64_STAMP(i)
#endif
// a stamp taken once the scalar v is known (a tool may pin v before the stamp)
#ifndef ACQ64_STAMP_AFTER
#define ACQ64_STAMP_AFTER(i, v) ACQ64_STAMP(i)
#endif

namespace {

// LDS one workgroup may allocate on the build's offload arch: the library is
// built for gfx950 only (Makefile ARCH), where a workgroup may take the CU's
// whole 160 KiB.  acq64_corr_kernel sizes its parked non-coherent sums from it.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "acq64.hip sizes its LDS for gfx950 (160 KiB per workgroup)"
#endif
constexpr int kLdsBudget = 160 * 1024;

// ---- plans -----------------------------------------------------------------------
// N = R1 R2 R3.  Positions between stages (same for both kinds):
//   after stage 1: k1*G1 + g,       g = n2*R3 + n3   (G1 = R2*R3 = stage-1 groups)
//   after stage 2: (k1*R2 + k2)*R3 + n3
// stage 2 groups g2 = k1*R3 + n3 (G2 = R1*R3), stage 3 groups g3 = k1*R2 + k2.
// PFA: input n = (n1 Q1 + n2 Q2 + n3 Q3) mod N, output k = (k1 E1 + k2 E2 + k3 E3) mod N,
//      spectra stored at n1*G1 + n2*R3 + n3 (digits n_i = (n mod R_i) INV_i mod R_i).
// CT:  input n = n1*G1 + n2*R3 + n3, output k = k1 + R1 k2 + R1 R2 k3, twiddles
//      W_N^(k1 g) after stage 1 and W_G1^(k2 n3) after stage 2; natural storage.
template <int N_, int R1_, int R2_, int R3_, int T_, bool PFA_>
struct Plan {
  static constexpr int N = N_, R1 = R1_, R2 = R2_, R3 = R3_, T = T_;
  static constexpr bool PFA = PFA_;
  static constexpr int TB = (T + 63) / 64 * 64;   // launched threads (whole waves)
  static constexpr int NW = TB / 64;
  static constexpr int G1 = N / R1, G2 = N / R2, G3 = N / R3;
  static constexpr int K1 = (G1 + T - 1) / T, K2 = (G2 + T - 1) / T;
  static constexpr int K3 = G3 / T, L = G3 - K3 * T;   // leftover stage-3 groups
  static constexpr int LS = L * R3 > 0 ? L * R3 : 1;
  // LDS exchange layouts.  PFA plans (PlanA) keep the natural positions.  Cooley-Tukey
  // plans pad them so that every exchange read and write is free of bank conflicts
  // (PlanB at natural positions: 46 % of its LDS cycles were conflicts, PMC
  // profiles/r6/pmc_gps_scilab_r6d.json):
  //  exchange 1: stage-1 output (k1, g) at k1 LG1 + g.  Stage-2 group g2 = t reads
  //    (t / R3) LG1 + t % R3 + n2 R3: with LG1 = R3 (mod 32) a 32-lane ds_read_b64 group
  //    hits the double banks t + c (mod 32), all distinct; the writes are runs of g.
  //  exchange 2: (k1, k2, n3) at k1 LB2 + k2 + n3 S3 (S3 = R2 + 1: injective).  The
  //    writes (fixed k2, lanes (t / R3, t % R3)) hit S3 t (mod 16) with S3 odd; the
  //    stage-3 reads (fixed n3, lanes k1 = t / R3, k2 = t % R3 + R3 j) hit LB2 (t / R3)
  //    + t % R3 = t (mod 32) with LB2 = R3 (mod 32).
  //  (MI355X_MICROARCH.md LDS table: ds_read_b64 2 x 32 lanes, bank (a/4) mod 64;
  //  ds_write_b64 4 x 16 lanes, bank (a/4) mod 32.)
  static constexpr int pad_to(int v, int m, int r) { return v + (((r - v) % m) + m) % m; }
  static constexpr int LG1 = PFA_ ? N / R1 : pad_to(N / R1, 32, R3);
  static constexpr int S2 = PFA_ ? R3 : 1;
  static constexpr int S3 = PFA_ ? 1 : pad_to(R2 + 1, 8, 1) | 1;
  static constexpr int LB2 = PFA_ ? R2 * R3 : pad_to(R2 * S2 + (R3 - 1) * S3 + 1, 32, R3);
  static constexpr int LX = PFA_ ? N : (R1 * LG1 > R1 * LB2 ? R1 * LG1 : R1 * LB2);
  static constexpr int Q1 = N / R1, Q2 = N / R2, Q3 = N / R3;
  static constexpr int INV1 = PFA ? cinv(Q1 % R1, R1) : 0;
  static constexpr int INV2 = PFA ? cinv(Q2 % R2, R2) : 0;
  static constexpr int INV3 = PFA ? cinv(Q3 % R3, R3) : 0;
  static constexpr int E1 = PFA ? (int)((long)Q1 * INV1 % N) : 0;
  static constexpr int E2 = PFA ? (int)((long)Q2 * INV2 % N) : 0;
  static constexpr int E3 = PFA ? (int)((long)Q3 * INV3 % N) : 0;
  static_assert(R1 * R2 * R3 == N, "plan factors");
  static_assert(L * R3 <= T, "leftover stage-3 inputs must fit one per thread");
  // leftover stage-3 groups run as symmetric tasks (group, m), m = 0..(R3-1)/2:
  // task t computes outputs m and R3-m (m > 0) of group K3*T + t % L
  static constexpr int LT = L * ((R3 + 1) / 2);
  static_assert(LT <= T, "leftover tasks must fit one per thread");
  __device__ static __forceinline__ bool lvalid(int t, int j) {
    return t < LT && (j == 0 || t >= L);
  }
  __device__ static __forceinline__ int lslot(int t, int j) {
    return j == 0 ? t / L : R3 - t / L;
  }
  static_assert(!PFA || (cgcd(R1, R2) == 1 && cgcd(R1, R3) == 1 && cgcd(R2, R3) == 1),
                "PFA needs coprime factors");
  // Code spectra are spectra of real sequences, F[-k] = conj(F[k]).  In PFA
  // digits negation is digit-wise, so with two stage-1 groups per thread a
  // thread can own a group and its negative and load F once for both:
  // SYM plans pair the 1023 radix-16 groups as (g, -g) -- 511 pairs + group 0.
  static constexpr bool SYM = PFA && K1 == 2 && R2 == 33 && R3 == 31 && T == 512;
  // stage-3 group of main slot j of thread t.  CT plans with several groups
  // per thread give a thread groups (k1, k2 + j R2/K3) so that ALL its outputs
  // (natural k1 + R1 k2 + R1 R2 k3) lie at least N/(R3 K3) apart.
  __device__ static __forceinline__ int group3(int t, int j) {
    if constexpr (!PFA && K3 > 1 && L == 0 && R2 % K3 == 0 && T == R1 * (R2 / K3)) {
      constexpr int W = R2 / K3;
      return (t / W) * R2 + t % W + W * j;
    } else {
      return t + j * T;
    }
  }
  // a thread's main stage-3 outputs are at least this far apart (circularly):
  // any window of fewer samples holds at most one of them
  static constexpr int SPACING =
      (!PFA && K3 > 1 && L == 0 && R2 % K3 == 0 && T == R1 * (R2 / K3)) ? N / (R3 * K3)
                                                                      : (K3 == 1 ? N / R3 : 1);
  // stage-1 group of slot j of thread t (SYM: the pair (g, -g)), -1 if none
  __device__ static __forceinline__ int group1(int t, int j) {
    if constexpr (SYM) {
      // slot 0 takes whole rows n2 = 1..16 (every n3) and row 0's n3 = 1..15;
      // the mirrors (rows 32..17, row 0's n3 = 30..16) are slot 1.  A wave's
      // slot-0 (and slot-1) groups are then ~2 consecutive 31-group rows:
      // each of its 16-byte loads covers ~1 KB of contiguous storage
      // (circularly shifted by the bin), not ~5 runs of 15 groups
      int g;
      if (t < 496) g = (1 + t / R3) * R3 + t % R3;    // n2 = 1..16, n3 = 0..30
      else if (t < 511) g = t - 495;                  // n2 = 0, n3 = 1..15
      else g = t == 511 ? 0 : -1;                     // group 0 pairs with itself
      if (j == 0 || g <= 0) return j == 0 ? g : -1;
      const int n2 = g / R3, n3 = g % R3;
      return ((R2 - n2) % R2) * R3 + (R3 - n3) % R3;
    } else {
      const int g = t + j * T;
      return (t < T && g < G1) ? g : -1;
    }
  }
  // natural input index of stage-1 element (n1, g)
  __device__ static __forceinline__ int in_index(int n1, int g) {
    if constexpr (PFA) {
      const int n2 = g / R3, n3 = g % R3;
      int n = n1 * Q1 + n2 * Q2;          // < 2N
      n -= n >= N ? N : 0;
      n += n3 * Q3;                        // < 2N
      return n >= N ? n - N : n;
    } else {
      return n1 * G1 + g;
    }
  }
  // natural output index of stage-3 slot k3 of group g3: base + k3*step (mod N)
  __device__ static __forceinline__ void out_base(int g3, int& base, int& step) {
    const int k1 = g3 / R2, k2 = g3 % R2;
    if constexpr (PFA) {
      base = (k1 * E1 + k2 * E2) % N;      // < R1*N + R2*N < 2^31
      step = E3;
    } else {
      base = k1 + R1 * k2;
      step = R1 * R2;
    }
  }
  // storage position of stage-3 output k3 of group g3: sbase(g3) + soff(k3).
  // PFA: the natural index k = CRT(k1, k2, k3) has k mod R_i = k_i, so its
  // storage digits are k_i * INV_i mod R_i -- no division per value.
  __device__ static __forceinline__ int sbase(int g3) {
    const int k1 = g3 / R2, k2 = g3 % R2;
    if constexpr (PFA) return (k1 * INV1 % R1) * G1 + (k2 * INV2 % R2) * R3;
    else return k1 + R1 * k2;
  }
  static constexpr int soff(int k3) { return PFA ? (k3 * INV3 % R3) : R1 * R2 * k3; }
  // storage position of natural index k in a spectrum row
  __device__ static __forceinline__ int store_index(int k) {
    if constexpr (PFA) {
      const int n1 = (k % R1) * INV1 % R1, n2 = (k % R2) * INV2 % R2, n3 = (k % R3) * INV3 % R3;
      return n1 * G1 + n2 * R3 + n3;
    } else {
      return k;
    }
  }
};
static_assert((long)16 * 15345 + (long)33 * 16368 < (1L << 31), "int index maps");

typedef Plan<16368, 16, 33, 31, 512, true> PlanA;   // 16.368 Msps
typedef Plan<16000, 40, 40, 10, 400, false> PlanB;  // 16 Msps

// multiply x[k] (k = 1..R-1) by w^k, w = W_M^m from the table; two interleaved
// recurrences (odd / even powers) halve the dependency chain
template <int R>
__device__ __forceinline__ void twiddle_run(v2d (&x)[R], v2d w) {
  const v2d w2 = cmul(w, w);
  v2d po = w, pe = w2;
#pragma unroll
  for (int k = 1; k < R; k++) {
    if (k & 1) {
      x[k] = cmul(x[k], po);
      if (k + 2 < R) po = cmul(po, w2);
    } else {
      x[k] = cmul(x[k], pe);
      if (k + 2 < R) pe = cmul(pe, w2);
    }
  }
}

__device__ __forceinline__ double part(v2d v, int p) { return p ? v.y : v.x; }
__device__ __forceinline__ void set_part(v2d& v, int p, double d) {
  if (p)
    v.y = d;
  else
    v.x = d;
}

// The transform from stage-1 inputs v1 (loaded by the caller) to stage-3
// outputs v3 (main groups g3 = t + j*T) and vl[j] (leftover outputs where
// P::lvalid(t, j): slot P::lslot(t, j) of group K3*T + t % L).  lds: N doubles; side: the
// LS real parts of the leftover groups' stage-3 inputs (their imaginary parts stay in
// the plane after exchange 2: the leftover tasks read lds[K3*T*R3 ..] after fft_core's
// last barrier, so a caller that writes the plane next must pass a barrier first);
// twN: W_N^j (global, CT plans only).
// Keeps the exchange reads as single ds_read_b64 (256 B/clk per CU): the
// load/store optimizer otherwise pairs them into ds_read2_b64, which the LDS
// serves at 128 B/clk (MI355X_MICROARCH.md, LDS table).
__device__ __forceinline__ void lds_read_fence() { __builtin_amdgcn_sched_barrier(0); }

// the lane id by mbcnt, opaque to the compiler (recomputed where it is used,
// never hoisted or kept live across a loop)
__device__ __forceinline__ int lane_id_opaque() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

struct NoHook {
  __device__ void operator()() const {}
};
template <class P, class Hook = NoHook, bool kStage3 = true, bool kPinStage1 = false>
__device__ __forceinline__ void fft_core(double* lds, double* side,
                                         const v2d* __restrict__ twN, int t,
                                         v2d (&v1)[P::K1][P::R1], v2d (&v3)[P::K3][P::R3],
                                         v2d (&vl)[2], const Hook& before_exchange = Hook()) {
  constexpr int R1 = P::R1, R2 = P::R2, R3 = P::R3, T = P::T, G2 = P::G2;
  const bool act = t < T;
  // ---- stage 1
#pragma unroll
  for (int j = 0; j < P::K1; j++) {
    dft<R1>(v1[j]);
    if constexpr (!P::PFA) {
      const int g = P::group1(t, j);
      if (g >= 0) twiddle_run<R1>(v1[j], twN[g]);
    }
  }
  if constexpr (kPinStage1) {
    // stage 1 completes before the hook: its results pass through empty asm
    // statements, the hook's loads stay behind a compiler memory barrier
#pragma unroll
    for (int j = 0; j < P::K1; j++)
#pragma unroll
      for (int k = 0; k < R1; k++) asm volatile("" : "+v"(v1[j][k].x), "+v"(v1[j][k].y));
    asm volatile("" ::: "memory");
  }
  before_exchange();   // the caller may still use the LDS up to here
  // ---- exchange 1: re then im
  v2d v2[P::K2][R2];
#pragma unroll
  for (int p = 0; p < 2; p++) {
#pragma unroll
    for (int j = 0; j < P::K1; j++) {
      const int g = P::group1(t, j);
      if (g >= 0) {
#pragma unroll
        for (int k1 = 0; k1 < R1; k1++) lds[k1 * P::LG1 + g] = part(v1[j][k1], p);
      }
    }
    __syncthreads();
    ACQ64_STAMP(1 + 2 * p);
#pragma unroll
    for (int j = 0; j < P::K2; j++) {
      const int g2 = t + j * T;
      if (act && g2 < G2) {
        const int base = (g2 / R3) * P::LG1 + g2 % R3;
#pragma unroll
        for (int n2 = 0; n2 < R2; n2++) {
          set_part(v2[j][n2], p, lds[base + n2 * R3]);
          lds_read_fence();
        }
      }
    }
    __syncthreads();
    ACQ64_STAMP(2 + 2 * p);
  }
  // ---- stage 2
#pragma unroll
  for (int j = 0; j < P::K2; j++) {
    dft<R2>(v2[j]);
    if constexpr (!P::PFA) {
      const int g2 = t + j * T;
      if (act && g2 < G2) twiddle_run<R2>(v2[j], twN[(g2 % R3) * R1]);   // W_G1^n3 = W_N^(n3 R1)
    }
  }
  // ---- exchange 2
#pragma unroll
  for (int p = 0; p < 2; p++) {
#pragma unroll
    for (int j = 0; j < P::K2; j++) {
      const int g2 = t + j * T;
      if (act && g2 < G2) {
        const int k1 = g2 / R3, n3 = g2 % R3;
#pragma unroll
        for (int k2 = 0; k2 < R2; k2++) lds[k1 * P::LB2 + k2 * P::S2 + n3 * P::S3] = part(v2[j][k2], p);
      }
    }
    __syncthreads();
    ACQ64_STAMP(5 + 2 * p);
#pragma unroll
    for (int j = 0; j < P::K3; j++) {
      const int g3 = act ? P::group3(t, j) : 0;
      const int b3 = (g3 / R2) * P::LB2 + (g3 % R2) * P::S2;
#pragma unroll
      for (int n3 = 0; n3 < R3; n3++) {
        set_part(v3[j][n3], p, lds[b3 + n3 * P::S3]);
        lds_read_fence();
      }
    }
    if constexpr (P::L > 0) {
      // PFA layout: leftover group K3*T + lg, input n3 at (K3*T + lg)*R3 + n3
      static_assert(P::PFA, "leftover groups assume the PFA exchange layout");
      if (p == 0 && t < P::L * R3) side[t] = lds[P::K3 * T * R3 + t];
    }
    __syncthreads();
    ACQ64_STAMP(6 + 2 * p);
  }
  // ---- stage 3 (main groups: left to the caller when !kStage3)
  if constexpr (kStage3) {
#pragma unroll
    for (int j = 0; j < P::K3; j++) dft<R3>(v3[j]);
  }
  if constexpr (P::L > 0) {
    // leftover groups: the symmetric prime DFT (dft_prime) split by output
    // pair, real parts from the side copy, imaginary parts from the plane
    // (exchange 2's last phase), W^(jm) from the constant table kTw (cos, -sin;
    // an LDS copy took the 400 B that the non-coherent kernel's sums need)
    if (t < P::LT) {
      constexpr int H = (R3 - 1) / 2;
      const int lg = t % P::L, m = t / P::L;
      const double* xr = side + lg * R3;
      const double* xi = lds + P::K3 * T * R3 + lg * R3;
      v2d A = (v2d){xr[0], xi[0]}, B = (v2d){0.0, 0.0};
      int q = m;
#pragma unroll
      for (int j = 1; j <= H; j++) {
        const v2d a = (v2d){xr[j], xi[j]}, b = (v2d){xr[R3 - j], xi[R3 - j]};
        const v2d w = (v2d){kTw<R3>.c[q], -kTw<R3>.s[q]};
        const v2d sj = a + b, dj = a - b;
        A = (v2d){fma(w.x, sj.x, A.x), fma(w.x, sj.y, A.y)};
        B = (v2d){fma(-w.y, dj.x, B.x), fma(-w.y, dj.y, B.y)};
        q += m;
        q -= q >= R3 ? R3 : 0;
      }
      vl[0] = (v2d){A.x + B.y, A.y - B.x};   // A - iB
      vl[1] = (v2d){A.x - B.y, A.y + B.x};   // A + iB (slot R3 - m)
    }
  }
}

// ---- forward transforms ------------------------------------------------------------
// Inputs are written in the plan's storage order (element n at store_index(n)),
// so the forward FFT reads its stage-1 groups with coalesced loads at constant
// offsets, exactly like the correlation kernel reads the spectra.
// IF rows: x[n] = sum_{p<coh} IF[blk][n + pN] * exp(i f ((n+pN)*2)*pi*ts), evaluated as
// acquisition.sci:61-62,107 does (phasePoints = (0:L-1)*2*%pi*ts; exp(%i*f*phasePoints))
// at the class frequency f = cfreq[cls]; row = cls * n_blocks + blk.  With
// fuse_n > 0 (short frequency tables) every workgroup first classifies the
// table itself (acq64_classify_kernel's job) and workgroup 0 publishes it.
// I16: the record is GNSSCORR_IF_INT16 (if16.h): an I,Q pair is one dword load, a real
// sample one 16-bit load, both halves converted from their full 16 bits.  A kernel of
// its own: the int8 / packed one keeps its code.
constexpr int kFuseClass = 64;
template <class P, bool I16 = false>
__global__ __launch_bounds__(256) void acq64_wipe_kernel(
    const int8_t* __restrict__ src, int iq, int n_blocks, int coh, const double* __restrict__ cfreq_in,
    const int* __restrict__ n_cls_dev, double ts, v2d* __restrict__ out, int fuse_n,
    const double* __restrict__ freqs, double delta, int2* __restrict__ fmap_out,
    double* __restrict__ cfreq_out, int* __restrict__ nclass_out) {
  constexpr int N = P::N;
  __shared__ double s_r[kFuseClass], s_cf[kFuseClass];
  __shared__ int s_l[kFuseClass], s_nc;
  const double* cfreq = cfreq_in;
  int n_cls;
  if (fuse_n > 0) {
    const int t = threadIdx.x;
    if (t < fuse_n) s_r[t] = grid_residue(freqs[t], delta);
    __syncthreads();
    if (t < fuse_n) {
      int l = t;
      for (int j = 0; j < t; j++)
        if (s_r[j] == s_r[t]) { l = j; break; }
      s_l[t] = l;
    }
    __syncthreads();
    if (t < fuse_n) {
      const int l = s_l[t];
      int cls = 0;
      for (int k = 0; k < l; k++) cls += s_l[k] == k;
      if (l == t) s_cf[cls] = s_r[t];
      if (blockIdx.x == 0) {
        const double q = rint((freqs[t] - s_r[t]) / delta);
        int mN = fabs(q) < 1e9 ? (int)fmod(q, (double)N) : 0;
        mN += mN < 0 ? N : 0;
        fmap_out[t] = make_int2(cls, mN);
        if (l == t) cfreq_out[cls] = s_r[t];
      }
    }
    if (t == 0) {
      int cnt = 0;
      for (int k = 0; k < fuse_n; k++) cnt += s_l[k] == k;
      s_nc = cnt;
      if (blockIdx.x == 0) *nclass_out = cnt;
    }
    __syncthreads();
    n_cls = s_nc;
  } else {
    n_cls = *n_cls_dev;
  }
  const long total = (long)n_cls * n_blocks * N;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int row = (int)(i / N), n = (int)(i % N);
    const int cls = row / n_blocks, blk = row % n_blocks;
    // (an LDS / global pointer select would make this a flat load)
    const double f = fuse_n > 0 ? s_cf[cls] : cfreq[cls];
    const bool cplx = iq & GNSSCORR_IF_IQ, pk = iq & GNSSCORR_IF_PACKED2;
    const int ne = cplx ? 2 : 1;
    const long e0 = (long)blk * coh * N * ne;   // first element of the block
    double re = 0.0, im = 0.0;
    for (int p = 0; p < coh; p++) {
      const long m = n + (long)p * N;
      double I, Q;
      if constexpr (I16) {
        const int w = cplx ? if16_sample<2>(reinterpret_cast<const uint8_t*>(src), (e0 >> 1) + m)
                           : if16_sample<1>(reinterpret_cast<const uint8_t*>(src), e0 + m);
        I = cplx ? (double)if16_half(w, 0) : (double)w;
        Q = cplx ? (double)if16_half(w, 16) : 0.0;
      } else {
        I = (double)if_elem(src, e0 + ne * m, pk);
        Q = cplx ? (double)if_elem(src, e0 + 2 * m + 1, pk) : 0.0;
      }
      const double th = f * ((((double)m * 2.0) * M_PI) * ts);
      double sn, cs;
      sincos(th, &sn, &cs);
      re += I * cs - Q * sn;
      im += I * sn + Q * cs;
    }
    out[(long)row * N + P::store_index(n)] = (v2d){re, im};
  }
}

template <class P>
__global__ __launch_bounds__(256) void acq64_codes_kernel(const int8_t* __restrict__ codes,
                                                          long n, v2d* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i - i % P::N + P::store_index((int)(i % P::N))] = (v2d){(double)codes[i], 0.0};
}

// Rows in storage order -> spectra in storage order.
template <class P>
__global__ __launch_bounds__(P::TB) void acq64_fwd_kernel(const v2d* __restrict__ in,
                                                          const int* __restrict__ n_cls_dev,
                                                          int per_cls, int n_rows,
                                                          v2d* __restrict__ out, int rs,
                                                          const v2d* __restrict__ twN) {
  __shared__ double lds[P::LX];
  __shared__ double side[P::LS];
  const int t = threadIdx.x;
  // rows grid-strided over a capped grid (n_rows is an upper bound of the
  // rows when the class count is on the device); fft_core ends on a barrier
  // after its last exchange read, but the leftover tasks (P::L > 0) read the
  // plane after it: the next row's exchange-1 writes wait for a barrier
  const int rows = n_cls_dev ? *n_cls_dev * per_cls : n_rows;
  for (int w = blockIdx.x; w < rows; w += gridDim.x) {
    const v2d* src = in + (long)w * P::N;
    v2d v1[P::K1][P::R1];
#pragma unroll
    for (int j = 0; j < P::K1; j++) {
      const int g0 = P::group1(t, j), g = g0 < 0 ? 0 : g0;
#pragma unroll
      for (int n1 = 0; n1 < P::R1; n1++) v1[j][n1] = src[n1 * P::G1 + g];
    }
    v2d v3[P::K3][P::R3], vl[2] = {(v2d){0.0, 0.0}, (v2d){0.0, 0.0}};
    fft_core<P>(lds, side, twN, t, v1, v3, vl);
    v2d* o = out + (long)w * rs;
    if (t < P::T) {
#pragma unroll
      for (int j = 0; j < P::K3; j++) {
        const int sb = P::sbase(P::group3(t, j));
#pragma unroll
        for (int k3 = 0; k3 < P::R3; k3++) o[sb + P::soff(k3)] = v3[j][k3];
      }
    }
    if constexpr (P::L > 0) {
#pragma unroll
      for (int j = 0; j < 2; j++)
        if (P::lvalid(t, j)) {
          int base, step;
          P::out_base(P::K3 * P::T + t % P::L, base, step);
          o[P::store_index((base + P::lslot(t, j) * step) % P::N)] = vl[j];
        }
      __syncthreads();   // leftover tasks' plane reads before the next row's writes
    }
  }
}

// ---- forward transforms of prime-factor plans in two launches --------------------
// Stage 1 (radix R1 over the G1 groups) in place: element n1*G1 + g of a row
// becomes k1*G1 + g -- each thread reads and writes the same R1 positions.
template <class P>
__global__ __launch_bounds__(256) void acq64_fwd1_kernel(v2d* __restrict__ io,
                                                         const int* __restrict__ n_cls_dev,
                                                         int per_cls, int n_rows) {
  // grid-stride: the launch is sized for the host's upper bound on the rows
  // (classes <= frequencies), capped; the actual count is read here
  const int rows = n_cls_dev ? *n_cls_dev * per_cls : n_rows;
  const long total = (long)rows * P::G1;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int row = (int)(i / P::G1), g = (int)(i % P::G1);
    v2d* r = io + (long)row * P::N;
    v2d v[P::R1];
#pragma unroll
    for (int n1 = 0; n1 < P::R1; n1++) v[n1] = r[n1 * P::G1 + g];
    dft<P::R1>(v);
#pragma unroll
    for (int k1 = 0; k1 < P::R1; k1++) r[k1 * P::G1 + g] = v[k1];
  }
}

// Stages 2 and 3 of one (row, k1): the G1 = R2 x R3 values k1*G1 + n2*R3 + n3
// are an independent R2 x R3 prime-factor transform.  One output per thread
// as direct DFT sums (R2, then R3 complex MACs) through LDS; the results go to
// the plan's storage positions sbase(k1*R2 + k2) + soff(k3).
constexpr int kFwd23Threads = 1024;
template <class P>
__global__ __launch_bounds__(kFwd23Threads) void acq64_fwd23_kernel(
    const v2d* __restrict__ in, const int* __restrict__ n_cls_dev, int per_cls, int n_rows,
    v2d* __restrict__ out, int rs) {
  constexpr int R2 = P::R2, R3 = P::R3, G1 = P::G1;
  static_assert(G1 <= kFwd23Threads, "one output per thread");
  __shared__ v2d s_a[G1], s_b[G1];
  __shared__ v2d w2[R2], w3[R3];
  // grid-stride over (row, k1) (see acq64_fwd1_kernel)
  const int rows = n_cls_dev ? *n_cls_dev * per_cls : n_rows;
  const int t = threadIdx.x;
  if (t < R2) w2[t] = (v2d){kTw<R2>.c[t], -kTw<R2>.s[t]};
  if (t < R3) w3[t] = (v2d){kTw<R3>.c[t], -kTw<R3>.s[t]};
  for (int u = blockIdx.x; u < rows * P::R1; u += gridDim.x) {
  const int row = u / P::R1, k1 = u % P::R1;
  if (t < G1) s_a[t] = in[(long)row * P::N + k1 * G1 + t];
  __syncthreads();
  // (four partial sums: the latency of one dependent chain, not the FMA
  // rate, bounds these single-wave-per-SIMD sums)
  if (t < G1) {   // stage 2: output (k2, n3) = sum_n2 a[n2][n3] W_R2^(n2 k2)
    const int k2 = t / R3, n3 = t % R3;
    v2d acc[4] = {(v2d){0.0, 0.0}, (v2d){0.0, 0.0}, (v2d){0.0, 0.0}, (v2d){0.0, 0.0}};
    // W^(n2 k2) by recurrence from one table read (a per-lane gather of the
    // table at every step conflicts in LDS); error ~R2 ulp
    const v2d wk = w2[k2];
    v2d w = (v2d){1.0, 0.0};
#pragma unroll
    for (int n2 = 0; n2 < R2; n2++) {
      acc[n2 & 3] += cmul(s_a[n2 * R3 + n3], w);
      w = cmul(w, wk);
    }
    s_b[t] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  }
  __syncthreads();
  if (t < G1) {   // stage 3: output (k2, k3) = sum_n3 b[k2][n3] W_R3^(n3 k3)
    const int k2 = t / R3, k3 = t % R3;
    v2d acc[4] = {(v2d){0.0, 0.0}, (v2d){0.0, 0.0}, (v2d){0.0, 0.0}, (v2d){0.0, 0.0}};
    const v2d wk = w3[k3];
    v2d w = (v2d){1.0, 0.0};
#pragma unroll
    for (int n3 = 0; n3 < R3; n3++) {
      acc[n3 & 3] += cmul(s_b[k2 * R3 + n3], w);
      w = cmul(w, wk);
    }
    out[(long)row * rs + P::sbase(k1 * R2 + k2) + P::soff(k3)] =
        (acc[0] + acc[1]) + (acc[2] + acc[3]);
  }
  __syncthreads();   // s_a / s_b are refilled by the next (row, k1)
  }
}

// ---- unit descriptors ---------------------------------------------------------------
// One descriptor per launched workgroup of acq64_corr_kernel, in launch order (the order
// permutation applied).  Rebuilt by every correlate call: group_code, group_freq,
// group_rec and the frequency map are the caller's device buffers, whose contents may
// change from call to call behind the same pointers.
template <class P>
__global__ __launch_bounds__(256) void acq64_unit_desc_kernel(
    int n_units, int rs, int n_blocks, bool nc, const int* __restrict__ group_code,
    const int* __restrict__ group_freq, int n_bins, const int* __restrict__ order,
    const int2* __restrict__ fmap, int gpr, int nbT, const int* __restrict__ group_rec,
    acq64_unit_desc* __restrict__ desc) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= n_units) return;
  const auto [rowid, blk0] = unit_row(order[w], n_blocks, nc);
  // records (gnsscorr_acq_set_records): virtual group gv = rec * gpr + g reads
  // blocks rec * n_blocks .. of the nbT resident blocks per class
  // (gnsscorr_acq_set_group_records: group g searches record group_rec[g] only)
  const int gv = rowid / n_bins, bin = rowid % n_bins;
  // a per-group record outside [0, nbT / n_blocks) is clamped: never a read past the spectra
  const int rec = group_rec ? min(max(group_rec[gv], 0), nbT / n_blocks - 1) : gv / gpr;
  const int g = group_rec ? gv : gv - rec * gpr;
  const int2 fm = fmap[group_freq[g * n_bins + bin]];
  const int m = fm.y;
  acq64_unit_desc d;
  d.x_ofs = ((long)fm.x * nbT + rec * n_blocks + blk0) * rs;
  d.f_ofs = (long)group_code[g] * rs;
  if constexpr (P::PFA) {
    // digits of the shift: X_f[k] = X_r[k - m], negation of m digit-wise
    constexpr int R1 = P::R1, R2 = P::R2, R3 = P::R3;
    const int m1 = (m % R1) * P::INV1 % R1, m2 = (m % R2) * P::INV2 % R2,
              m3 = (m % R3) * P::INV3 % R3;
    d.shift = m1 | m2 << 8 | m3 << 16;
  } else {
    d.shift = m;
  }
  d.rowid = rowid;
  d.blk0 = blk0;
  d.slot = rowid * n_blocks + blk0;
  desc[w] = d;
}

// ---- the correlation kernel -------------------------------------------------------
// One workgroup = one unit: BEST_OF_BLOCKS -> (row, block); NONCOHERENT -> row,
// |.|^2 summed over the blocks in registers.  fmap[fid] = {class, m}: the bin's
// spectrum is the class spectrum circularly shifted by m (X_f[k] = X_r[k - m]).
template <class P, int MODE, bool DUMP>
__global__ __launch_bounds__(P::TB) void acq64_corr_kernel(
    const v2d* __restrict__ X, const v2d* __restrict__ F, int rs, int n_blocks, int spc,
    gnsscorr_acq_row* __restrict__ stats, double* __restrict__ dump, int dump_block,
    const acq64_unit_desc* __restrict__ desc, const v2d* __restrict__ twN) {
  constexpr int N = P::N, R1 = P::R1, R3 = P::R3, T = P::T, K3 = P::K3, L = P::L;
  constexpr bool kNC = MODE == GNSSCORR_ACQ_NONCOHERENT;
  // non-coherent: a thread's first kE running sums live in the LDS left over
  // beside the exchange plane for the whole row (the others are parked in the
  // plane between blocks, see start_sums)
  constexpr int kLdsOther = P::LX * 8 + P::LS * 8 + P::NW * 20;
  constexpr int kE0 = kNC ? (kLdsBudget - kLdsOther) / (8 * T) : 0;
  // one s_extra row holds the leftover outputs' sums (pwl) when there are any
  constexpr int kPwlRow = (kNC && L > 0 && kE0 > 0) ? 1 : 0;
  static_assert(!kPwlRow || 2 * P::LT <= T, "leftover sums fit one s_extra row");
  constexpr int kE = kE0 - kPwlRow < K3 * R3 ? kE0 - kPwlRow : K3 * R3;
  __shared__ double lds[P::LX + (kE + kPwlRow) * T];   // the exchange plane, then s_extra
  __shared__ double side[P::LS];
  __shared__ double s_v[P::NW], s_m[P::NW];
  __shared__ int s_k[P::NW];
  static_assert(sizeof(double) * (P::LX + (kE + kPwlRow) * T + P::LS) +
                        (2 * sizeof(double) + sizeof(int)) * P::NW <= (size_t)kLdsBudget,
                "acq64_corr_kernel: static LDS over the gfx950 budget");
  double* const s_extra = lds + P::LX;
  // non-coherent: threadIdx.x is rebuilt inside and after the block loop from the
  // wave's base (uniform: an SGPR) and the lane id, so no per-lane copy of it stays
  // live across the loop (that copy was the kernel's last spill to scratch)
  const int wave_base = __builtin_amdgcn_readfirstlane(threadIdx.x & ~63);
  int t = threadIdx.x;
  const bool act = t < T;
  ACQ64_STAMP(0);
  // the unit's rows and shift, resolved by acq64_unit_desc_kernel: scalar loads of one
  // 32-byte record (blockIdx.x-indexed, issued together: one round trip) ahead of the
  // X / F addresses
  const acq64_unit_desc ud = desc[blockIdx.x];
  const int rowid = ud.rowid, blk0 = ud.blk0;
  const int nblk = kNC ? n_blocks : 1;
  const double inv_n2 = 1.0 / ((double)N * (double)N);
  ACQ64_STAMP_AFTER(11, ud.shift);

  double pw[K3][R3], pwl[2] = {-1.0, -1.0};   // pwl: leftover outputs (P::lvalid)

  for (int i = 0; i < nblk; i++) {
    const int blk = blk0 + i;
    const v2d* Xb = X + (ud.x_ofs + (long)i * rs);
    // the code row is the same for every block: keep the compiler from
    // hoisting its loads out of the block loop (they would stay live in
    // registers across the whole transform)
    // (the offset, not the pointer, goes through the asm: an opaque pointer
    // loses its global address space, and the code loads became flat loads,
    // whose completion the waitcnt logic can only wait for all at once)
    long fofs = ud.f_ofs;
    asm volatile("" : "+s"(fofs));
    const v2d* Fc = F + fofs;
    // likewise every thread-dependent address: t is opaque per block, so the
    // index arithmetic is redone per block instead of held across it
    int t;
    if constexpr (kNC) {
      t = wave_base + lane_id_opaque();
    } else {
      t = threadIdx.x;
      asm volatile("" : "+v"(t));
    }
    // stage-1 inputs: conj(X[k - m]) * F[k]  (= conj(X * conj(F)), acquisition.sci:116).
    // Slots of groups a thread does not own are left as garbage: fft_core never
    // stores them.
    v2d v1[P::K1][R1];
    if constexpr (P::PFA) {
      constexpr int R2 = P::R2;
      // digits of the shift: X_f[k] = X_r[k - m], negation of m digit-wise
      const int m1 = ud.shift & 0xff, m2 = (ud.shift >> 8) & 0xff, m3 = ud.shift >> 16;
      auto shifted = [&](int g) {
        int n2 = g / R3 - m2, n3 = g % R3 - m3;
        n2 += n2 < 0 ? R2 : 0;
        n3 += n3 < 0 ? R3 : 0;
        return n2 * R3 + n3;
      };
      auto plane = [&](int n1) {
        int a = n1 - m1;
        return (a < 0 ? a + R1 : a) * P::G1;
      };
      if constexpr (P::SYM) {
        // slot 0: group ga; slot 1: gb = -ga, whose code value at plane -n1 is
        // conj(F[ga] at plane n1): one F load serves both
        const int ga0 = P::group1(t, 0), ga = ga0 < 0 ? 0 : ga0;
        const int gb0 = P::group1(t, 1), gb = gb0 < 0 ? ga : gb0;
        const int sa = shifted(ga), sb = shifted(gb);
#pragma unroll
        for (int n1 = 0; n1 < R1; n1++) {
          const int nn = (R1 - n1) % R1;
          const v2d f = Fc[n1 * P::G1 + ga];
          const v2d xa = Xb[plane(n1) + sa], xb = Xb[plane(nn) + sb];
          v1[0][n1] = (v2d){fma(xa.x, f.x, xa.y * f.y), fma(xa.x, f.y, -(xa.y * f.x))};
          v1[1][nn] = (v2d){fma(xb.x, f.x, -(xb.y * f.y)), -fma(xb.x, f.y, xb.y * f.x)};
        }
      } else {
#pragma unroll
        for (int j = 0; j < P::K1; j++) {
          const int g0 = P::group1(t, j), g = g0 < 0 ? 0 : g0;
          const int gs = shifted(g);
#pragma unroll
          for (int n1 = 0; n1 < R1; n1++) {
            const v2d x = Xb[plane(n1) + gs], f = Fc[n1 * P::G1 + g];
            v1[j][n1] = (v2d){fma(x.x, f.x, x.y * f.y), fma(x.x, f.y, -(x.y * f.x))};
          }
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < P::K1; j++) {
        const int g0 = P::group1(t, j), g = g0 < 0 ? 0 : g0;
#pragma unroll
        for (int n1 = 0; n1 < R1; n1++) {
          const int n = n1 * P::G1 + g;
          int s = n - ud.shift;
          s += s < 0 ? N : 0;
          const v2d x = Xb[s], f = Fc[n];
          v1[j][n1] = (v2d){fma(x.x, f.x, x.y * f.y), fma(x.x, f.y, -(x.y * f.x))};
        }
      }
    }
    v2d v3[K3][R3], vl[2] = {(v2d){0.0, 0.0}, (v2d){0.0, 0.0}};
    // non-coherent: the running sums are parked in the LDS between blocks
    // (stored after a block's stage 3, when the exchange plane is idle) and
    // come back after this block's stage 1, just before the exchange needs the
    // plane: they are not live across the load phase, whose in-flight X / F
    // loads take the registers (held in registers, they were spilled there).
    auto start_sums = [&]() {
      if constexpr (kNC) {
        // branch-free (a branch here lets the compiler sink stage 1 below the
        // reads, back into the load phase); at i == 0 the plane's content is
        // read but not used
        const bool first = i == 0;
        const int tt = min(t, T - 1);
#pragma unroll
        for (int j = 0; j < K3; j++)
#pragma unroll
          for (int k = 0; k < R3; k++) {
            if (j * R3 + k < kE) continue;   // in s_extra: read just before stage 3
            const double v = lds[(j * R3 + k) * T + tt];
            pw[j][k] = first ? 0.0 : v;
          }
        if constexpr (!kPwlRow) {
          pwl[0] = first ? (P::lvalid(t, 0) ? 0.0 : -1.0) : pwl[0];
          pwl[1] = first ? (P::lvalid(t, 1) ? 0.0 : -1.0) : pwl[1];
        }
        __syncthreads();   // exchange 1 overwrites the parked sums
      }
    };
    // |.|^2 / N^2 (|ifft(Y)|^2 = |fft(conj Y)|^2 / N^2); a prime radix-R3
    // stage is fused with the powers
    constexpr bool kFuse = is_prime(R3);
    fft_core<P, decltype(start_sums), !kFuse, kNC>(lds, side, twN, t, v1, v3, vl,
                                                   start_sums);
    // the first kE running sums are added to in place in s_extra, each read
    // just before its output is formed: they take no registers in stage 3
#pragma unroll
    for (int j = 0; j < K3; j++) {
      auto put_power = [&](int k3, double p) {
        const int f = j * R3 + k3;
        if (kNC && f < kE) {
          if (act) {
            double* const a = s_extra + f * T + t;
            *a = (i == 0 ? 0.0 : *a) + p;
          }
        } else {
          pw[j][k3] = kNC ? pw[j][k3] + p : p;
        }
      };
      if constexpr (kFuse) {
        dft_prime_power<R3>(v3[j], put_power, inv_n2);
      } else {
#pragma unroll
        for (int k3 = 0; k3 < R3; k3++)
          put_power(k3, fma(v3[j][k3].x, v3[j][k3].x, v3[j][k3].y * v3[j][k3].y) * inv_n2);
      }
    }
    if constexpr (L > 0) {
#pragma unroll
      for (int j = 0; j < 2; j++)
        if (P::lvalid(t, j)) {
          const double p = fma(vl[j].x, vl[j].x, vl[j].y * vl[j].y) * inv_n2;
          if constexpr (kPwlRow) {   // in place in the s_extra row after the kE sums
            double* const a = s_extra + kE * T + j * P::LT + t;
            *a = (i == 0 ? 0.0 : *a) + p;
          } else {
            pwl[j] = kNC ? pwl[j] + p : p;
          }
        }
    }
    static_assert(!(DUMP && kNC), "power dumps are coherent-mode only");
    if (DUMP && blk == dump_block && act) {
#pragma unroll
      for (int j = 0; j < K3; j++) {
        int base, step;
        P::out_base(P::group3(t, j), base, step);
        int k = base;
#pragma unroll
        for (int k3 = 0; k3 < R3; k3++) {
          dump[(long)rowid * N + k] = pw[j][k3];
          k += step;
          if (k >= N) k -= N;
        }
      }
      if constexpr (L > 0) {
#pragma unroll
        for (int j = 0; j < 2; j++)
          if (P::lvalid(t, j)) {
            int base, step;
            P::out_base(K3 * T + t % P::L, base, step);
            dump[(long)rowid * N + (base + P::lslot(t, j) * step) % N] = pwl[j];
          }
      }
    }
    if constexpr (kNC) {
      // park the sums (exchange 2's reads ended with a barrier: the plane is idle)
      static_assert(K3 * R3 * T <= N, "parked sums fit the exchange plane");
      if (i + 1 < nblk && act) {
#pragma unroll
        for (int j = 0; j < K3; j++)
#pragma unroll
          for (int k = 0; k < R3; k++) {
            const int f = j * R3 + k;
            if (f >= kE) lds[f * T + t] = pw[j][k];   // f < kE: already in s_extra
          }
      }
    }
  }
  if constexpr (kNC) t = wave_base + lane_id_opaque();
  if constexpr (kE > 0) {
    const int tt = min(t, T - 1);
#pragma unroll
    for (int f = 0; f < kE; f++) pw[f / R3][f % R3] = s_extra[f * T + tt];
  }
  if constexpr (kPwlRow) {
#pragma unroll
    for (int j = 0; j < 2; j++)
      pwl[j] = P::lvalid(t, j) ? s_extra[kE * T + j * P::LT + t] : -1.0;
  }
  // ---- row statistics (acq_peak.h).  The thread's outputs lie at least
  // SPACING = N/R3 samples apart: the stride of top2_exact for its top-2.  Wider
  // windows take an exact second pass over the registers.
  auto wrap_add = [](int k, int d) {   // (k + d) mod N for k, d in [0, N)
    const unsigned u = (unsigned)(k + d);
    return (int)min(u, u - (unsigned)N);
  };
  // (Top2::push and store_row written out here: called, they reorder this kernel's
  // instructions)
  double a1 = -1.0, a2 = -1.0;
  int ak = INT_MAX;
#pragma unroll
  for (int j = 0; j < K3; j++) {
    int base, step;
    P::out_base(act ? P::group3(t, j) : 0, base, step);
    int k = base;
#pragma unroll
    for (int k3 = 0; k3 < R3; k3++) {
      const double v = pw[j][k3];
      const bool take = better(v, k, a1, ak);
      a2 = fmax(a2, fmin(a1, v));
      ak = take ? k : ak;
      a1 = fmax(a1, v);
      k = wrap_add(k, step);
    }
  }
  if (!act) { a1 = -1.0; a2 = -1.0; ak = INT_MAX; }
  double bv = a1;
  int bk = ak;
  int kl[2] = {INT_MAX, INT_MAX};
  if constexpr (L > 0) {
#pragma unroll
    for (int j = 0; j < 2; j++)
      if (P::lvalid(t, j)) {
        int base, step;
        P::out_base(K3 * T + t % P::L, base, step);
        kl[j] = (base + P::lslot(t, j) * step) % N;
        if (better(pwl[j], kl[j], bv, bk)) { bv = pwl[j]; bk = kl[j]; }
      }
  }
  block_argmax<P::NW>(bv, bk, s_v, s_k, t);
  ACQ64_STAMP(9);
  double sv = -1.0;
  if (top2_exact(P::SPACING, spc)) {
    sv = outside_window(ak, bk, spc, N) ? a1 : a2;
  } else if (act) {
#pragma unroll
    for (int j = 0; j < K3; j++) {
      int base, step;
      P::out_base(P::group3(t, j), base, step);
      int k = base;
#pragma unroll
      for (int k3 = 0; k3 < R3; k3++) {
        if (outside_window(k, bk, spc, N)) sv = fmax(sv, pw[j][k3]);
        k = wrap_add(k, step);
      }
    }
  }
  if constexpr (L > 0) {
#pragma unroll
    for (int j = 0; j < 2; j++)
      if (P::lvalid(t, j) && outside_window(kl[j], bk, spc, N)) sv = fmax(sv, pwl[j]);
  }
  sv = block_max0<P::NW>(sv, s_m, t);
  ACQ64_STAMP(10);
  if (t == 0) {
    gnsscorr_acq_row r;
    r.peak = bv;
    r.second = sv;
    r.argmax = bk;
    r.block = kNC ? -1 : blk0;
    stats[ud.slot] = r;
  }
  ACQ64_STAMP(12);
}

// Frequencies -> spectrum classes on the fs/N grid: class = canonical residue
// r = f mod fs/N (one forward FFT per class and block); bin f = r + m fs/N
// reads the class spectrum shifted by m.  fmap[i] = {class, m mod N}.
__global__ __launch_bounds__(1024) void acq64_classify_kernel(const double* __restrict__ freqs,
                                                              int n, double delta, int N,
                                                              int2* __restrict__ fmap,
                                                              double* __restrict__ cfreq,
                                                              int* __restrict__ n_classes,
                                                              double* __restrict__ resid,
                                                              int* __restrict__ lead) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) resid[i] = grid_residue(freqs[i], delta);
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const double r = resid[i];
    int l = i;
    for (int j = 0; j < i; j++)
      if (resid[j] == r) { l = j; break; }
    lead[i] = l;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int l = lead[i];
    int cls = 0;
    for (int k = 0; k < l; k++) cls += lead[k] == k;
    const double q = rint((freqs[i] - resid[i]) / delta);
    int mN = (fabs(q) < 1e9 ? (int)fmod(q, (double)N) : 0);
    mN += mN < 0 ? N : 0;
    fmap[i] = make_int2(cls, mN);
    if (l == i) cfreq[cls] = resid[i];
  }
  // class count: every thread counts its own entries (one serial thread over
  // the whole table took ~100 us at full-sky sizes, a dependent load per entry)
  __shared__ int s_cnt;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  int mine = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) mine += lead[i] == i;
  atomicAdd(&s_cnt, mine);
  __syncthreads();
  if (threadIdx.x == 0) *n_classes = s_cnt;
}

// ---- launch helpers ---------------------------------------------------------------
template <class P>
int fwd_launch(gnsscorr_acq_ctx* c, const v2d* in, const int* n_cls_dev, int per_cls,
               int n_rows, v2d* out) {
  if constexpr (P::PFA) {
    // two launches spread over the whole GPU (a config-2 search has only 4
    // rows: one workgroup per row would leave 252 CUs idle): stage 1 in place,
    // then the 16 independent 1023-point (33 x 31) transforms of every row
    v2d* io = const_cast<v2d*>(in);
    // n_rows is an upper bound when the class count is on the device (a
    // full-sky GLONASS part: 574 frequencies x 10 blocks for 2 classes x 10):
    // capped grids, grid-stride kernels (92 k mostly-empty workgroups cost
    // ~190 us of launch alone)
    const long groups = (long)n_rows * P::G1;
    const long g1 = (groups + 255) / 256, g23 = (long)n_rows * P::R1;
    hipLaunchKernelGGL((acq64_fwd1_kernel<P>), dim3((unsigned)(g1 < 4096 ? g1 : 4096)), dim3(256),
                       0, c->stream, io, n_cls_dev, per_cls, n_rows);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((acq64_fwd23_kernel<P>), dim3((unsigned)(g23 < 2048 ? g23 : 2048)),
                       dim3(kFwd23Threads), 0, c->stream, (const v2d*)io, n_cls_dev, per_cls,
                       n_rows, out, c->rs64);
  } else {
    hipLaunchKernelGGL((acq64_fwd_kernel<P>), dim3(n_rows < 512 ? n_rows : 512), dim3(P::TB), 0,
                       c->stream, in,
                       n_cls_dev, per_cls, n_rows, out, c->rs64, (const v2d*)c->d_twN);
  }
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

template <class P>
int corr_launch(gnsscorr_acq_ctx* c, int n_blocks, int mode, int n_units, int n_bins,
                const int32_t* d_gcode, const int32_t* d_gfreq, int spc, double* d_dump,
                int dump_block, int gpr) {
  const int nbT = n_blocks * c->spec_recs;
  // a descriptor names its stats record with an int
  if ((size_t)n_units * (mode == GNSSCORR_ACQ_NONCOHERENT ? n_blocks : 1) > (size_t)INT_MAX) {
    gnsscorr_set_error("gnsscorr_acq_correlate: %d units x %d blocks: too many row records",
                       n_units, n_blocks);
    return GNSSCORR_EINVAL;
  }
  int rc = hostctx::grow(c->d_udesc, (size_t)n_units);
  if (rc) return rc;
  hipLaunchKernelGGL((acq64_unit_desc_kernel<P>), dim3((n_units + 255) / 256), dim3(256), 0,
                     c->stream, n_units, c->rs64, n_blocks, mode == GNSSCORR_ACQ_NONCOHERENT,
                     d_gcode, d_gfreq, n_bins, (const int*)c->d_order.p,
                     (const int2*)c->d_fmap64, gpr, nbT, c->d_group_rec, c->d_udesc.p);
  HIP_TRY(hipGetLastError());

#define ACQ64_LAUNCH(M, D)                                                                  \
  hipLaunchKernelGGL((acq64_corr_kernel<P, M, D>), dim3(n_units), dim3(P::TB), 0, c->stream, \
                     (const v2d*)c->d_X64.p, (const v2d*)c->d_F64, c->rs64, n_blocks, spc,     \
                     c->d_stats.p, d_dump, dump_block,                                        \
                     (const acq64_unit_desc*)c->d_udesc.p, (const v2d*)c->d_twN)
  if (d_dump)
    ACQ64_LAUNCH(GNSSCORR_ACQ_BEST_OF_BLOCKS, true);
  else if (mode == GNSSCORR_ACQ_NONCOHERENT)
    ACQ64_LAUNCH(GNSSCORR_ACQ_NONCOHERENT, false);
  else
    ACQ64_LAUNCH(GNSSCORR_ACQ_BEST_OF_BLOCKS, false);
#undef ACQ64_LAUNCH
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

template <class P>
int set_codes_launch(gnsscorr_acq_ctx* c, const int8_t* d_codes, int n_codes) {
  const long n = (long)n_codes * P::N;
  hipLaunchKernelGGL(acq64_codes_kernel<P>, dim3((n + 255) / 256), dim3(256), 0, c->stream,
                     d_codes, n, (v2d*)c->d_in64.p);
  HIP_TRY(hipGetLastError());
  return fwd_launch<P>(c, (const v2d*)c->d_in64.p, nullptr, 1, n_codes, (v2d*)c->d_F64);
}

template <class P>
int spectra_launch(gnsscorr_acq_ctx* c, const int8_t* d_if, int iq, int n_blocks, int n_freqs,
                   const double* d_freqs) {
  constexpr int N = P::N;
  const int rows = n_freqs * n_blocks;   // upper bound: classes <= frequencies
  const double delta = c->cfg.samp_rate / N;
  const int fuse = n_freqs <= kFuseClass ? n_freqs : 0;
  if (!fuse) {
    const int rc = acq64_classify_launch(c, d_freqs, n_freqs);
    if (rc) return rc;
  }
  const long work = (long)rows * N;
  const int grid = (int)((work + 255) / 256 < 2048 ? (work + 255) / 256 : 2048);
  if (iq & GNSSCORR_IF_INT16)
    hipLaunchKernelGGL((acq64_wipe_kernel<P, true>), dim3(grid), dim3(256), 0, c->stream, d_if, iq,
                       n_blocks, c->coh, c->d_cfreq, c->d_nclass, 1.0 / c->cfg.samp_rate,
                       (v2d*)c->d_in64.p, fuse, d_freqs, delta, c->d_fmap64, c->d_cfreq,
                       c->d_nclass);
  else
  hipLaunchKernelGGL(acq64_wipe_kernel<P>, dim3(grid), dim3(256), 0, c->stream, d_if, iq,
                     n_blocks, c->coh, c->d_cfreq, c->d_nclass, 1.0 / c->cfg.samp_rate,
                     (v2d*)c->d_in64.p, fuse, d_freqs, delta, c->d_fmap64, c->d_cfreq,
                     c->d_nclass);
  HIP_TRY(hipGetLastError());
  return fwd_launch<P>(c, (const v2d*)c->d_in64.p, c->d_nclass, n_blocks, rows, (v2d*)c->d_X64.p);
}

}  // namespace

int acq64_plan_for(int n_samples) {
  // GNSSCORR_ACQ_GENERIC=1: the generic engine (acq64_gen.hip) for every N (cross-checks)
  const char* fg = getenv("GNSSCORR_ACQ_GENERIC");
  const int force_generic = fg ? atoi(fg) : 0;
  if (!force_generic && n_samples == PlanA::N) return 1;
  if (!force_generic && n_samples == PlanB::N) return 2;
  if (n_samples >= 64 && n_samples <= (1 << 19)) return 3;
  return 0;
}

int acq64_init(gnsscorr_acq_ctx* c) {
  c->plan64 = acq64_plan_for(c->cfg.n_samples);
  if (!c->plan64) {
    gnsscorr_set_error("acq64: n_samples %d outside [64, %d] (compiled plans: %d, %d; "
                       "Bluestein otherwise)", c->cfg.n_samples, 1 << 19, PlanA::N, PlanB::N);
    return GNSSCORR_EINVAL;
  }
  const int N = c->cfg.n_samples;
  c->rs64 = (N + 63) & ~63;
  HIP_TRY(hipMalloc(&c->d_F64, sizeof(double2) * (size_t)c->rs64 * c->cfg.max_codes));
  HIP_TRY(hipMemset(c->d_F64, 0, sizeof(double2) * (size_t)c->rs64 * c->cfg.max_codes));
  HIP_TRY(hipMalloc(&c->d_fmap64, sizeof(int2) * c->cfg.max_freqs));
  HIP_TRY(hipMalloc(&c->d_lead64, sizeof(int) * c->cfg.max_freqs));
  if (c->plan64 == 3) return acq64_gen_init(c);
  HIP_TRY(hipMalloc(&c->d_twN, sizeof(double2) * N));
  double2* tw = (double2*)malloc(sizeof(double2) * N);
  if (!tw) return GNSSCORR_ENOMEM;
  for (int j = 0; j < N; j++) {
    // W_N^j = exp(-2 pi i j / N), argument reduced to [0, pi/4]-accurate libm calls
    const double a = 2.0 * M_PI * ((double)j / (double)N);
    tw[j] = make_double2(cos(a), -sin(a));
  }
  hipError_t e = hipMemcpy(c->d_twN, tw, sizeof(double2) * N, hipMemcpyHostToDevice);
  free(tw);
  HIP_TRY(e);
  return GNSSCORR_OK;
}

void acq64_free(gnsscorr_acq_ctx* c) {
  hostctx::release(c->d_F64, c->d_X64, c->d_in64, c->d_twN, c->d_fmap64, c->d_lead64, c->d_udesc);
  acq64_gen_free(c);
}

int acq64_classify_launch(gnsscorr_acq_ctx* c, const double* d_freqs, int n_freqs) {
  const int N = c->cfg.n_samples;
  hipLaunchKernelGGL(acq64_classify_kernel, dim3(1), dim3(1024), 0, c->stream, d_freqs, n_freqs,
                     c->cfg.samp_rate / N, N, c->d_fmap64, c->d_cfreq, c->d_nclass, c->d_resid,
                     c->d_lead64);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

// Once per context (gnsscorr_acq_create): the input buffer of max_codes code
// transforms, and this file's code object loaded on the device (HIP loads a
// translation unit's kernels on their first use: ~3 ms on the first
// set_prn_codes of a process otherwise; hipFuncGetAttributes loads it).  The generic
// engine's kernels are a code object of their own, loaded only by a context on it.
int acq64_preload(gnsscorr_acq_ctx* c) {
  int rc = hostctx::grow(c->d_in64, (size_t)c->cfg.max_codes * c->cfg.n_samples);
  if (rc) return rc;
  hipFuncAttributes a;
  HIP_TRY(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&acq64_classify_kernel)));
  return c->plan64 == 3 ? acq64_gen_preload(c) : GNSSCORR_OK;
}

int acq64_set_codes(gnsscorr_acq_ctx* c, const int8_t* d_codes, int n_codes, int code_len) {
  int rc = hostctx::grow(c->d_in64, (size_t)n_codes * c->cfg.n_samples);
  if (rc) return rc;
  if (c->plan64 == 3) return acq64_gen_set_codes(c, d_codes, n_codes, code_len);
  return c->plan64 == 1 ? set_codes_launch<PlanA>(c, d_codes, n_codes)
                        : set_codes_launch<PlanB>(c, d_codes, n_codes);
}

int acq64_set_zero_padded(gnsscorr_acq_ctx* c, int keep) {
  return c->plan64 == 3 ? acq64_gen_set_zero_padded(c, keep) : GNSSCORR_OK;
}

int acq64_spectra(gnsscorr_acq_ctx* c, const int8_t* d_if, int iq, int n_blocks, int n_freqs,
                  const double* d_freqs) {
  const size_t rows = (size_t)n_freqs * n_blocks;
  int rc = hostctx::grow(c->d_in64, rows * c->cfg.n_samples);
  if (rc) return rc;
  rc = hostctx::grow(c->d_X64, rows * c->rs64);
  if (rc) return rc;
  if (c->plan64 == 3) return acq64_gen_spectra(c, d_if, iq, n_blocks, n_freqs, d_freqs);
  return c->plan64 == 1 ? spectra_launch<PlanA>(c, d_if, iq, n_blocks, n_freqs, d_freqs)
                        : spectra_launch<PlanB>(c, d_if, iq, n_blocks, n_freqs, d_freqs);
}

int acq64_correlate(gnsscorr_acq_ctx* c, int n_blocks, int mode, int n_groups, int n_bins,
                    const int32_t* d_gcode, const int32_t* d_gfreq, int spc, double* d_dump,
                    int dump_block) {
  // n_groups per record; the units of every record of the resident spectra run
  // in one launch (virtual groups rec * n_groups + g)
  const int upr = mode == GNSSCORR_ACQ_NONCOHERENT ? 1 : n_blocks;
  const int n_units = (c->d_group_rec ? 1 : c->spec_recs) * n_groups * n_bins * upr;
  if (c->plan64 == 3)
    return acq64_gen_correlate(c, n_blocks, mode, n_groups, n_bins, d_gcode, d_gfreq, spc,
                               d_dump, dump_block);
  return c->plan64 == 1 ? corr_launch<PlanA>(c, n_blocks, mode, n_units, n_bins, d_gcode, d_gfreq,
                                             spc, d_dump, dump_block, n_groups)
                        : corr_launch<PlanB>(c, n_blocks, mode, n_units, n_bins, d_gcode, d_gfreq,
                                             spc, d_dump, dump_block, n_groups);
}
