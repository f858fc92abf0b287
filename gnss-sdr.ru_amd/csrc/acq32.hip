// acq32.hip -- the fp32 acquisition engine (GNSSCORR_ACQ_F32, N = 16368 only) behind the
// acq32_* interface of acq_ctx.h.  The front (acq.hip) owns the C ABI, the checks, the tile
// order and the per-group selection; this file owns the fp32 spectra and their kernels.
//
// MI355X design
//  * N = samplesPerCode = 16368 = 16 * 3 * 11 * 31.  The four factors are
//    pairwise coprime, so the DFT is done as a Good-Thomas prime-factor FFT:
//    a 4-D DFT of shape 16 x 3 x 11 x 31 with NO inter-stage twiddles.  The
//    Ruritanian input map n(p) and CRT output map k(p) are pure index
//    permutations; they are folded into where data is read and written.
//  * One 1-ms row (16368 complex fp32 = 128 KiB) lives in LDS for the whole
//    transform; 528 work-items (9 wavefronts) each own one radix-16, one
//    3x11 or one radix-31 butterfly per pass: 3 LDS passes per transform.
//  * The IFFT is computed as a forward FFT of conj(Y) (|ifft(Y)| = |fft(conj Y)|/N),
//    so one kernel body serves both directions.
//  * Forward spectra of the wiped-off IF (shared by all codes) and of every
//    code replica are written to HBM already permuted into the correlation
//    kernel's LDS order (sigma = n^-1 o k), so the hot kernel streams both
//    operands with fully coalesced 8-byte loads and needs no gathers.
//  * The hot kernel fuses: conj(X)*F, 3 FFT passes, |.|^2, the row statistics
//    (acq_peak.h), and the best-of-blocks or non-coherent combine over
//    blocks -- the 16368-point power row never leaves registers.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "acq_ctx.h"
#include "acq_peak.h"
#include "if2.h"

// Diagnostic hook: tools/acq_pstamps.hip defines it to record s_memtime at the
// pipelined kernel's phase boundaries; in the library it compiles to nothing.
#ifndef ACQ_PSTAMP          // pipelined kernel: (unit iteration, stamp id), tools/acq_pstamps.hip
#define ACQ_PSTAMP(it, i)
#endif

namespace {

constexpr int N = 16368;
constexpr int M16 = N / 16, M3 = N / 3, M11 = N / 11, M31 = N / 31;  // 1023 5456 1488 528
// CRT idempotents e_i = 1 mod N_i, 0 mod N_j (checked on the host at create)
constexpr int E16 = 15345, E3 = 10912, E11 = 5952, E31 = 528;
constexpr int kThreads = 512;           // 8 wavefronts -> up to 256 VGPRs each
// Spectra rows in HBM are padded to 16 planes x 1024 complex (128 KiB) so the
// radix-16 loads are 16-byte aligned: LDS position a*1023+g <-> a*1024+g.
constexpr int kPlane = 1024;
constexpr int NPAD = 16 * kPlane;
constexpr int kGroups31 = N / 31;       // 528 radix-31 groups
constexpr int kLeft = kGroups31 - kThreads;  // 16 groups done as direct dot products

constexpr float kCos11[11] = {1.000000000e+00f, 8.412535328e-01f, 4.154150130e-01f, -1.423148383e-01f, -6.548607339e-01f, -9.594929736e-01f, -9.594929736e-01f, -6.548607339e-01f, -1.423148383e-01f, 4.154150130e-01f, 8.412535328e-01f};
constexpr float kSin11[11] = {0.000000000e+00f, 5.406408175e-01f, 9.096319954e-01f, 9.898214419e-01f, 7.557495744e-01f, 2.817325568e-01f, -2.817325568e-01f, -7.557495744e-01f, -9.898214419e-01f, -9.096319954e-01f, -5.406408175e-01f};
constexpr float kCos31[31] = {1.000000000e+00f, 9.795299413e-01f, 9.189578116e-01f, 8.207634412e-01f, 6.889669191e-01f, 5.289640103e-01f, 3.473052528e-01f, 1.514277775e-01f, -5.064916884e-02f, -2.506525323e-01f, -4.403941516e-01f, -6.121059825e-01f, -7.587581227e-01f, -8.743466161e-01f, -9.541392564e-01f, -9.948693234e-01f, -9.948693234e-01f, -9.541392564e-01f, -8.743466161e-01f, -7.587581227e-01f, -6.121059825e-01f, -4.403941516e-01f, -2.506525323e-01f, -5.064916884e-02f, 1.514277775e-01f, 3.473052528e-01f, 5.289640103e-01f, 6.889669191e-01f, 8.207634412e-01f, 9.189578116e-01f, 9.795299413e-01f};
constexpr float kSin31[31] = {0.000000000e+00f, 2.012985201e-01f, 3.943558551e-01f, 5.712682151e-01f, 7.247927872e-01f, 8.486442575e-01f, 9.377521321e-01f, 9.884683243e-01f, 9.987165072e-01f, 9.680771189e-01f, 8.978045396e-01f, 7.907757369e-01f, 6.513724827e-01f, 4.853019625e-01f, 2.993631230e-01f, 1.011683220e-01f, -1.011683220e-01f, -2.993631230e-01f, -4.853019625e-01f, -6.513724827e-01f, -7.907757369e-01f, -8.978045396e-01f, -9.680771189e-01f, -9.987165072e-01f, -9.884683243e-01f, -9.377521321e-01f, -8.486442575e-01f, -7.247927872e-01f, -5.712682151e-01f, -3.943558551e-01f, -2.012985201e-01f};
constexpr float kCos16[16] = {1.0f, 9.238795325e-01f, 7.071067812e-01f, 3.826834324e-01f, 0.0f, -3.826834324e-01f, -7.071067812e-01f, -9.238795325e-01f, -1.0f, -9.238795325e-01f, -7.071067812e-01f, -3.826834324e-01f, 0.0f, 3.826834324e-01f, 7.071067812e-01f, 9.238795325e-01f};
constexpr float kSin16[16] = {0.0f, 3.826834324e-01f, 7.071067812e-01f, 9.238795325e-01f, 1.0f, 9.238795325e-01f, 7.071067812e-01f, 3.826834324e-01f, 0.0f, -3.826834324e-01f, -7.071067812e-01f, -9.238795325e-01f, -1.0f, -9.238795325e-01f, -7.071067812e-01f, -3.826834324e-01f};
constexpr float kSqrt3_2 = 8.660254038e-01f;

// Complex values live in packed fp32 pairs (v2f): gfx950 executes v_pk_fma_f32 /
// v_pk_add_f32 on both halves in one instruction, and re/im swaps and sign
// flips fold into the op_sel / neg modifiers, so the DFTs below are written
// with explicit swaps instead of scalar re/im arithmetic.
typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2f swp(v2f v) { return __builtin_shufflevector(v, v, 1, 0); }
__device__ __forceinline__ v2f bc(float c) { return (v2f){c, c}; }
// -i v = (v.y, -v.x)
__device__ __forceinline__ v2f mul_mi(v2f v) { return swp(v) * (v2f){1.f, -1.f}; }
// v * (c + i s) for constants c, s
__device__ __forceinline__ v2f cmulc(v2f v, float c, float s) {
  return v * bc(c) + swp(v) * (v2f){-s, s};
}
__device__ __forceinline__ v2f ld2(const float2& f) { return (v2f){f.x, f.y}; }
__device__ __forceinline__ float2 st2(v2f v) { return make_float2(v.x, v.y); }

// ---- small forward DFTs (W = exp(-2 pi i / P)) --------------------------------
__device__ __forceinline__ void dft4(v2f& a, v2f& b, v2f& c, v2f& d) {
  const v2f t0 = a + c, t1 = a - c, t2 = b + d, t3 = b - d;
  a = t0 + t2;
  c = t0 - t2;
  const v2f s3 = swp(t3);
  b = __builtin_elementwise_fma(s3, (v2f){1.f, -1.f}, t1);   // t1 - i t3
  d = __builtin_elementwise_fma(s3, (v2f){-1.f, 1.f}, t1);   // t1 + i t3
}

// In place: on return x[k] = X[k].
__device__ __forceinline__ void dft16(v2f (&x)[16]) {
#pragma unroll
  for (int n2 = 0; n2 < 4; n2++) dft4(x[n2], x[4 + n2], x[8 + n2], x[12 + n2]);
#pragma unroll
  for (int k1 = 1; k1 < 4; k1++)
#pragma unroll
    for (int n2 = 1; n2 < 4; n2++) {
      const int m = n2 * k1;
      x[4 * k1 + n2] = cmulc(x[4 * k1 + n2], kCos16[m], -kSin16[m]);
    }
#pragma unroll
  for (int k1 = 0; k1 < 4; k1++) dft4(x[4 * k1], x[4 * k1 + 1], x[4 * k1 + 2], x[4 * k1 + 3]);
  // X[k1 + 4 k2] sits in slot 4 k1 + k2: transpose the 4x4 block (register renaming)
  v2f y[16];
#pragma unroll
  for (int i = 0; i < 16; i++) y[i] = x[i];
#pragma unroll
  for (int k1 = 0; k1 < 4; k1++)
#pragma unroll
    for (int k2 = 0; k2 < 4; k2++) x[k1 + 4 * k2] = y[4 * k1 + k2];
}

__device__ __forceinline__ void dft3(v2f& x0, v2f& x1, v2f& x2) {
  const v2f s = x1 + x2, d = x1 - x2;
  const v2f t = x0 - bc(0.5f) * s;
  x0 = x0 + s;
  const v2f sd = swp(d);   // -/+ i sqrt(3)/2 (x1 - x2)
  x1 = __builtin_elementwise_fma(sd, (v2f){kSqrt3_2, -kSqrt3_2}, t);
  x2 = __builtin_elementwise_fma(sd, (v2f){-kSqrt3_2, kSqrt3_2}, t);
}

template <int P>
__device__ __forceinline__ float ctab(int k) { return P == 11 ? kCos11[k] : kCos31[k]; }
template <int P>
__device__ __forceinline__ float stab(int k) { return P == 11 ? kSin11[k] : kSin31[k]; }

// Symmetric prime-length DFT: X_m = A_m - i B_m, X_{P-m} = A_m + i B_m with
// A_m = x0 + sum_j cos(2 pi jm/P)(x_j + x_{P-j}), B_m = sum_j sin(..)(x_j - x_{P-j}).
template <int P>
__device__ __forceinline__ void dftp(v2f (&x)[P]) {
  constexpr int H = (P - 1) / 2;
  v2f s[H + 1], d[H + 1];
#pragma unroll
  for (int j = 1; j <= H; j++) {
    s[j] = x[j] + x[P - j];
    d[j] = x[j] - x[P - j];
  }
  const v2f x0 = x[0];
  v2f X0 = x0;
#pragma unroll
  for (int j = 1; j <= H; j++) X0 += s[j];
  x[0] = X0;
#pragma unroll
  for (int m = 1; m <= H; m++) {
    v2f A = x0, B = (v2f){0.f, 0.f};
#pragma unroll
    for (int j = 1; j <= H; j++) {
      const int q = (j * m) % P;
      A += bc(ctab<P>(q)) * s[j];
      B += bc(stab<P>(q)) * d[j];
    }
    const v2f sb = swp(B);
    x[m] = __builtin_elementwise_fma(sb, (v2f){1.f, -1.f}, A);        // A - i B
    x[P - m] = __builtin_elementwise_fma(sb, (v2f){-1.f, 1.f}, A);    // A + i B
  }
}

// ---- index maps --------------------------------------------------------------
// LDS position p = a*1023 + (b*11 + c)*31 + d
__device__ __forceinline__ int in_index(int p) {  // Ruritanian input map n(p)
  const int d = p % 31, c = (p / 31) % 11, b = (p / 341) % 3, a = p / 1023;
  int n = a * M16 + b * M3 + c * M11 + d * M31;
  n %= N;
  return n;
}

// ---- the three in-LDS passes (16, 3x11, 31) ----------------------------------
// Correlation-kernel first pass straight from HBM/L2: every thread owns the
// two adjacent radix-16 groups g = 2t, 2t+1 and reads them as ONE 16-byte
// buffer load per plane a (scalar plane offset a*8 KiB, 32-bit lane offset),
// forms D = conj(X) * F, runs both DFT16s in registers and writes LDS once.
typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));

// Frequency bins on the fs/N grid share one spectrum: X_f[k] = X_f0[k - m]
// for f = f0 + m*fs/N (exact circular shift).  In prime-factor coordinates a
// shift by m subtracts (15m mod 16, 2m mod 3, 4m mod 11, m mod 31) from the
// (a, b, c, d) of every position, so the X read below is still one plane per
// a and an (almost always) contiguous pair of groups.
struct Shift { int a, b, c, d; };

__device__ __forceinline__ int shift_group(int g, const Shift& s) {
  const int d = g % 31, bc = g / 31, c = bc % 11, b = bc / 11;
  int b2 = b - s.b, c2 = c - s.c, d2 = d - s.d;
  b2 += b2 < 0 ? 3 : 0;
  c2 += c2 < 0 ? 11 : 0;
  d2 += d2 < 0 ? 31 : 0;
  return (b2 * 11 + c2) * 31 + d2;
}

__device__ __forceinline__ void load_mul_pass16(const float2* __restrict__ Xb,
                                                const float2* __restrict__ Fc, float2* lds,
                                                int t, const Shift& sh) {
  const auto rx = __builtin_amdgcn_make_buffer_rsrc((void*)Xb, 0, NPAD * 8, 0x00020000);
  const auto rf = __builtin_amdgcn_make_buffer_rsrc((void*)Fc, 0, NPAD * 8, 0x00020000);
  const int g0 = 2 * t;
  const int voff = g0 * 8;
  v2f x0[16], x1[16];
  if (sh.a == 0 && sh.b == 0 && sh.c == 0 && sh.d == 0) {   // uniform branch
#pragma unroll
    for (int a = 0; a < 16; a++) {
      const f4v u = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rx, voff, a * kPlane * 8, 0));
      const f4v f = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rf, voff, a * kPlane * 8, 0));
      // conj(u) * f = u.re * f + u.im * (f.im, -f.re)
      const v2f f0 = (v2f){f.x, f.y}, f1 = (v2f){f.z, f.w};
      x0[a] = bc(u.x) * f0 + bc(u.y) * mul_mi(f0);
      x1[a] = bc(u.z) * f1 + bc(u.w) * mul_mi(f1);
    }
  } else {
    const int v0 = shift_group(g0 < M16 ? g0 : 0, sh) * 8;
    const int v1 = shift_group(g0 + 1 < M16 ? g0 + 1 : 0, sh) * 8;
#pragma unroll
    for (int a = 0; a < 16; a++) {
      const int pa = ((a - sh.a) & 15) * kPlane * 8;
      const f2v u0 = __builtin_bit_cast(f2v, __builtin_amdgcn_raw_buffer_load_b64(rx, v0, pa, 0));
      const f2v u1 = __builtin_bit_cast(f2v, __builtin_amdgcn_raw_buffer_load_b64(rx, v1, pa, 0));
      const f4v f = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rf, voff, a * kPlane * 8, 0));
      const v2f f0 = (v2f){f.x, f.y}, f1 = (v2f){f.z, f.w};
      x0[a] = bc(u0.x) * f0 + bc(u0.y) * mul_mi(f0);
      x1[a] = bc(u1.x) * f1 + bc(u1.y) * mul_mi(f1);
    }
  }
  dft16(x0);
  dft16(x1);
  const bool two = g0 + 1 < M16;
#pragma unroll
  for (int a = 0; a < 16; a++) {
    lds[a * M16 + g0] = st2(x0[a]);
    if (two) lds[a * M16 + g0 + 1] = st2(x1[a]);
  }
}

__device__ __forceinline__ void pass33(float2* lds, int t) {
  if (t >= 16 * 31) return;
  const int a = t / 31, d = t % 31;
  float2* base = lds + a * M16 + d;
  v2f v[3][11];
#pragma unroll
  for (int b = 0; b < 3; b++)
#pragma unroll
    for (int c = 0; c < 11; c++) v[b][c] = ld2(base[(b * 11 + c) * 31]);
#pragma unroll
  for (int c = 0; c < 11; c++) dft3(v[0][c], v[1][c], v[2][c]);
#pragma unroll
  for (int b = 0; b < 3; b++) dftp<11>(v[b]);
#pragma unroll
  for (int b = 0; b < 3; b++)
#pragma unroll
    for (int c = 0; c < 11; c++) base[(b * 11 + c) * 31] = st2(v[b][c]);
}

// dim-31 pass, leftover groups 512..527: thread t < 496 computes output m of
// group 512 + t/31 as a direct 31-term DFT sum (twiddles from an LDS table).
__device__ __forceinline__ float2 dft31_single(const float2* lds, const float2* tw, int t) {
  const int grp = kThreads + t / 31, m = t % 31;
  const float2* x = lds + grp * 31;
  float re = 0.f, im = 0.f;
  int q = 0;
#pragma unroll
  for (int j = 0; j < 31; j++) {
    const float2 v = x[j], w = tw[q];  // w = exp(-2 pi i q / 31)
    re = fmaf(v.x, w.x, fmaf(-v.y, w.y, re));
    im = fmaf(v.x, w.y, fmaf(v.y, w.x, im));
    q += m;
    if (q >= 31) q -= 31;
  }
  return make_float2(re, im);
}

__device__ __forceinline__ void init_tw31(float2* tw) {
  if (threadIdx.x < 31) tw[threadIdx.x] = make_float2(kCos31[threadIdx.x], -kSin31[threadIdx.x]);
}

// natural output index of LDS position t*31 + d': k = (a E16 + b E3 + c E11 + d' E31) mod N
__device__ __forceinline__ int out_base(int t) {
  const int a = t / 33, bc = t % 33, b = bc / 11, c = bc % 11;
  return (a * E16 + b * E3 + c * E11) % N;  // < 2^31: 32-bit modulo
}

// ---- forward spectra: wiped-off IF rows and code rows --------------------------
// The forward transforms are latency-bound (82 rows for a GPS search), so each
// row is split over many small workgroups with the prime-factor structure:
//   K1: wipe-off + radix-16 pass, 4 workgroups x 256 groups per row -> HBM
//       staging T[row][a'][1024]
//   K2: the 16 independent 1023-point (3 x 11 x 31) sub-transforms of a row,
//       one wavefront each, written straight to the correlation layout (sigma).
// mode 0: IF row = (freq_id, block); x[n] = IF[block][n] * exp(i f ((n*2)*pi)*ts)
//         with coh > 1 a block is coh code periods and x[n] = sum over p < coh of
//         the wiped-off sample n + p*N (phase index n + p*N): the coh*N-point
//         spectrum of acquisition.sci's settings.acqCohIntegration-ms blocks
//         against repmat(code, coh) is nonzero only at multiples of coh, where it
//         equals this folded N-point spectrum times coh x the 1-ms code spectrum,
//         and its inverse is the same N-periodic power row (GLONASS
//         acquisition.sci:52-72, 113-135: "The rest are copies of the first 1msec")
// mode 1: code row c; x[n] = code[c][n]
constexpr int kFuseClass = 64;   // frequency tables this short are classified inside fwd16
constexpr int kFwd1Threads = 256;
constexpr int kFwd1G = kFwd1Threads / 16;   // radix-16 columns g per workgroup
// One workgroup = 16 columns g of one row: every thread makes ONE input sample
// (a, g) -- the wipe-off's fp64 sincos spread over 64 workgroups per row, not
// 16 per thread -- then 16 threads run the radix-16 of their column.
__global__ __launch_bounds__(kFwd1Threads) void acq_fwd16_kernel(
    const int8_t* __restrict__ src, int iq, int n_blocks, const double* __restrict__ freqs,
    double ts, int mode, float2* __restrict__ stage, const double* __restrict__ cfreqs,
    const int* __restrict__ n_rows_dev, int coh, int n_rows, int fuse_n, double delta,
    int4* __restrict__ fmap_out, double* __restrict__ cfreq_out, int* __restrict__ nclass_out) {
  __shared__ float2 xs[kFwd1G][17];
  __shared__ double s_r[kFuseClass], s_cf[kFuseClass];
  __shared__ int s_l[kFuseClass], s_nc;
  const int chunks = (M16 + kFwd1G - 1) / kFwd1G;
  int n_cls_rows = n_rows_dev ? -1 : n_rows;
  if (fuse_n > 0) {
    // acq_classify_kernel folded in for short frequency tables: every workgroup
    // classifies the table in LDS (fuse_n <= kFuseClass lanes), workgroup 0
    // publishes the map for the later kernels
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
        int mN = (fabs(q) < 1e8 ? (int)q : 0) % N;
        mN += mN < 0 ? N : 0;
        fmap_out[t] = make_int4(cls, (15 * mN) & 15, (2 * mN) % 3, ((4 * mN) % 11) * 32 + mN % 31);
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
    n_cls_rows = s_nc * n_blocks;
    cfreqs = s_cf;
  } else if (n_rows_dev) {
    n_cls_rows = *n_rows_dev * n_blocks;
  }
  // grid-stride over (row, chunk): only the spectrum-class rows exist
  const int total = n_cls_rows * chunks;
  for (int w = blockIdx.x; w < total; w += gridDim.x) {
  const int row = w / chunks, g0 = (w % chunks) * kFwd1G;
  const int a = threadIdx.x >> 4, gl = threadIdx.x & 15, g = g0 + gl;
  if (g < M16) {
    const int n0 = in_index(a * M16 + g);
    float2 v;
    if (mode == 0) {
      const int cls = row / n_blocks, blk = row % n_blocks;
      const double f = cfreqs[cls];
      const bool cplx = iq & GNSSCORR_IF_IQ, pk = iq & GNSSCORR_IF_PACKED2;
      const int ne = cplx ? 2 : 1;
      const long e0 = (long)blk * coh * N * ne;   // first element of the block
      double re = 0.0, im = 0.0;
      for (int p = 0; p < coh; p++) {
        const int n = n0 + p * N;
        const double I = (double)if_elem(src, e0 + (long)ne * n, pk);
        const double Q = cplx ? (double)if_elem(src, e0 + 2L * n + 1, pk) : 0.0;
        // acquisition.sci:61-62, 107: phasePoints = (0:coh*N-1)*2*%pi*ts; exp(i f pp)
        const double th = f * ((((double)n * 2.0) * M_PI) * ts);
        double sn, cs;
        sincos(th, &sn, &cs);
        re += I * cs - Q * sn;
        im += I * sn + Q * cs;
      }
      v = make_float2((float)re, (float)im);
    } else {
      v = make_float2((float)src[(long)row * N + n0], 0.f);
    }
    xs[gl][a] = v;
  }
  __syncthreads();
  if (threadIdx.x < kFwd1G && g0 + threadIdx.x < M16) {
    const int gg = g0 + threadIdx.x;
    v2f x[16];
#pragma unroll
    for (int k = 0; k < 16; k++) x[k] = ld2(xs[threadIdx.x][k]);
    dft16(x);
    float2* o = stage + (long)row * NPAD + gg;
#pragma unroll
    for (int k = 0; k < 16; k++) o[k * kPlane] = st2(x[k]);
  }
  __syncthreads();   // xs is rewritten by the next item
  }
}

// The 1023-point (3 x 11 x 31) sub-transform of plane a of a row, 512 threads:
// dft3 over b for the 341 (c, d) columns, dft11 over c for the 93 (b, d)
// columns, then the 33 radix-31 groups split into their 16 output pairs
// (X_0 and X_m / X_{31-m} of the symmetric form): 528 tasks, one round.  The
// scatter targets (sigma) are fetched before the first barrier.
constexpr int kFwd2Threads = 512;
__global__ __launch_bounds__(kFwd2Threads) void acq_fwd1023_kernel(
    const float2* __restrict__ stage, const int* __restrict__ sigma, float2* __restrict__ out,
    int n_blocks, const int* __restrict__ n_rows_dev, int n_rows) {
  __shared__ float2 sub[M16 + 1];
  const int total = (n_rows_dev ? *n_rows_dev * n_blocks : n_rows) * 16;
  const int t = threadIdx.x;
  for (int w = blockIdx.x; w < total; w += gridDim.x) {
    const int row = w >> 4, a = w & 15;
    // radix-31 tasks of this thread: k = t and t + 512 (k < 528)
    int dst0[2], dst1[2];
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const int k = t + r * kFwd2Threads;
      dst0[r] = dst1[r] = 0;
      if (k < 33 * 16) {
        const int grp = k >> 4, m = k & 15, p0 = a * M16 + grp * 31;
        dst0[r] = sigma[p0 + m];
        dst1[r] = m ? sigma[p0 + 31 - m] : 0;
      }
    }
    const float2* in = stage + (long)row * NPAD + a * kPlane;
    for (int i = t; i < M16; i += kFwd2Threads) sub[i] = in[i];
    __syncthreads();
    if (t < 11 * 31) {   // radix 3 over b, column (c, d)
      const int c = t / 31, d = t % 31;
      v2f x0 = ld2(sub[c * 31 + d]), x1 = ld2(sub[(11 + c) * 31 + d]),
          x2 = ld2(sub[(22 + c) * 31 + d]);
      dft3(x0, x1, x2);
      sub[c * 31 + d] = st2(x0);
      sub[(11 + c) * 31 + d] = st2(x1);
      sub[(22 + c) * 31 + d] = st2(x2);
    }
    __syncthreads();
    if (t < 3 * 31) {    // radix 11 over c, column (b, d)
      const int b = t / 31, d = t % 31;
      v2f v[11];
#pragma unroll
      for (int c = 0; c < 11; c++) v[c] = ld2(sub[(b * 11 + c) * 31 + d]);
      dftp<11>(v);
#pragma unroll
      for (int c = 0; c < 11; c++) sub[(b * 11 + c) * 31 + d] = st2(v[c]);
    }
    __syncthreads();
    float2* o = out + (long)row * NPAD;
#pragma unroll
    for (int r = 0; r < 2; r++) {   // radix 31: (group, output pair m)
      const int k = t + r * kFwd2Threads;
      if (k >= 33 * 16) break;
      const int grp = k >> 4, m = k & 15;
      const float2* x = &sub[grp * 31];
      const v2f x0 = ld2(x[0]);
      if (m == 0) {
        v2f X0 = x0;
#pragma unroll
        for (int j = 1; j <= 15; j++) X0 += ld2(x[j]) + ld2(x[31 - j]);
        o[dst0[r]] = st2(X0);
      } else {
        v2f A = x0, B = (v2f){0.f, 0.f};
        int q = m;
#pragma unroll
        for (int j = 1; j <= 15; j++) {   // q = j*m mod 31
          const v2f xj = ld2(x[j]), xn = ld2(x[31 - j]);
          A += bc(kCos31[q]) * (xj + xn);
          B += bc(kSin31[q]) * (xj - xn);
          q += m;
          if (q >= 31) q -= 31;
        }
        const v2f sb = swp(B);
        o[dst0[r]] = st2(__builtin_elementwise_fma(sb, (v2f){1.f, -1.f}, A));   // A - i B
        o[dst1[r]] = st2(__builtin_elementwise_fma(sb, (v2f){-1.f, 1.f}, A));   // A + i B
      }
    }
    __syncthreads();   // sub is reloaded by the next item
  }
}

// Spectrum classes: frequencies with the same residue r = f mod fs/N share one
// forward spectrum, computed AT r; bin f = r + m*fs/N reads it circularly
// shifted by m (exact identity: exp(i 2 pi m n / N) modulation).  The class
// spectrum depends on r alone, so results do not depend on which other
// frequencies are in the list (sharding / ordering invariant).
// fmap[i] = {class, 15m mod 16, 2m mod 3, (4m mod 11) * 32 + m mod 31};
// cfreq[class] = r.

constexpr int kClassLds = 2048;   // frequencies classified in LDS (larger tables: global scratch)
__global__ __launch_bounds__(1024) void acq_classify_kernel(const double* __restrict__ freqs,
                                                            int n, double delta,
                                                            int4* __restrict__ fmap,
                                                            double* __restrict__ cfreq,
                                                            int* __restrict__ n_classes,
                                                            double* __restrict__ resid) {
  extern __shared__ double s_cls[];   // [n] residues, then [n] int4 (n <= kClassLds)
  const bool lds = n <= kClassLds;
  double* R = lds ? s_cls : resid;
  int4* F = lds ? reinterpret_cast<int4*>(s_cls + ((n + 1) & ~1)) : fmap;
  // pass 0: every residue once (fmod is a long fp64 sequence)
  for (int i = threadIdx.x; i < n; i += blockDim.x) R[i] = grid_residue(freqs[i], delta);
  __syncthreads();
  // pass 1: leader = first j with the same residue; shift m = (f - r) / delta
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const double f = freqs[i], r = R[i];
    int l = i;
    for (int j = 0; j < i; j++)
      if (R[j] == r) { l = j; break; }
    const double q = rint((f - r) / delta);
    F[i] = make_int4(l, fabs(q) < 1e8 ? (int)q : 0, 0, 0);
  }
  __syncthreads();
  // pass 2: class id = number of leaders before the leader
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int4 v = F[i];
    int cls = 0;
    for (int k = 0; k < v.x; k++) cls += F[k].x == k;
    int mN = v.y % N;
    mN += mN < 0 ? N : 0;
    F[i].z = cls;
    F[i].w = mN;
  }
  // class count: every thread counts its own entries (one thread walking the
  // table was a dependent LDS/global load per entry)
  __shared__ int s_cnt;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  int mine = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) mine += F[i].x == i;
  atomicAdd(&s_cnt, mine);
  __syncthreads();
  if (threadIdx.x == 0) *n_classes = s_cnt;
  // pass 3: class frequencies and the packed shift coordinates
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int4 v = F[i];
    if (v.x == i) cfreq[v.z] = R[i];
    const int mN = v.w;
    fmap[i] = make_int4(v.z, (15 * mN) & 15, (2 * mN) % 3, ((4 * mN) % 11) * 32 + mN % 31);
  }
}

// ---- block-level reductions ---------------------------------------------------
struct PeakSlot {
  float v;
  int k;
};

// max value, smallest natural index among equals; result broadcast to all
// threads.  One barrier: the scratch slots are next written after at least
// one more barrier (the next block / unit), so no trailing barrier is needed.
__device__ __forceinline__ void block_argmax(float& v, int& k, PeakSlot* scratch) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(v, o, 64);
    const int k2 = __shfl_xor(k, o, 64);
    if (better(v2, k2, v, k)) { v = v2; k = k2; }
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) scratch[w] = PeakSlot{v, k};
  __syncthreads();
  v = scratch[0].v;
  k = scratch[0].k;
#pragma unroll
  for (int i = 1; i < kThreads / 64; i++)
    if (better(scratch[i].v, scratch[i].k, v, k)) { v = scratch[i].v; k = scratch[i].k; }
}

// max over the workgroup, valid in thread 0 only (one barrier, as above)
__device__ __forceinline__ float block_max0(float v, float* scratch) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) scratch[w] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 1; i < kThreads / 64; i++) v = fmaxf(v, scratch[i]);
  }
  return v;
}

// ---- the one-unit correlation kernel --------------------------------------------
// Serves the non-coherent searches (<NONCOHERENT, false>), the power-row dump
// of gnsscorr_acq_power_row (<BEST_OF_BLOCKS, true>) and every search whose
// second-peak window can hold two outputs of one thread (WIDE: !top2_exact(528, spc),
// see the row statistics below); every other best-of-blocks search runs
// acq_corr_pipe_kernel below.
// One workgroup = one work unit: BEST_OF_BLOCKS -> unit = (row, block), the
// statistics of that block go to stats[unit]; NONCOHERENT -> unit = row, |.|^2
// summed over the blocks in registers, stats to stats[row * n_blocks].
// (Row-sized units would leave the last of ~5 rounds of workgroups 1/8 full.)
// Every thread owns radix-31 group t (positions t*31 .. t*31+30) and threads
// t < 496 also own one output of the 16 leftover groups (position 512*31 + t).
template <int MODE, bool DUMP, bool WIDE>
__global__ __launch_bounds__(kThreads) void acq_corr_kernel(
    const float2* __restrict__ X, const float2* __restrict__ F, int n_blocks,
    const int* __restrict__ group_code, const int* __restrict__ group_freq, int n_bins,
    int spc, gnsscorr_acq_row* __restrict__ stats, double* __restrict__ dump_power,
    int dump_block, const int* __restrict__ order, const int4* __restrict__ fmap) {
  __shared__ float2 lds[N];
  __shared__ float2 tw[32];
  __shared__ PeakSlot s_pk[kThreads / 64];
  __shared__ float s_mx[kThreads / 64];
  constexpr bool kNonCoh = MODE == GNSSCORR_ACQ_NONCOHERENT;
  const int unit = order[blockIdx.x];
  const auto [rowid, blk0] = unit_row(unit, n_blocks, kNonCoh);
  const int nblk = kNonCoh ? n_blocks : 1;
  const int g = rowid / n_bins, bin = rowid % n_bins;
  const int code = group_code[g];
  const int fid = group_freq[g * n_bins + bin];
  const int4 fm = fmap[fid];
  const Shift sh{fm.y, fm.z, fm.w >> 5, fm.w & 31};
  const int t = threadIdx.x;
  const float inv_n2 = 1.0f / ((float)N * (float)N);
  const bool extra = t < kLeft * 31;
  const int kb = out_base(t);
  // natural index of the leftover output owned by this thread
  const int kx = (out_base(kThreads + t / 31) + (t % 31) * E31) % N;
  init_tw31(tw);

  constexpr int kAcc = kNonCoh ? 32 : 1;
  float pacc[kAcc];
#pragma unroll
  for (int d = 0; d < kAcc; d++) pacc[d] = 0.f;
  float best_pk = -1.f, best_sec = 0.f;
  int best_k = 0;

  const float2* Fc = F + (long)code * NPAD;
  for (int i = 0; i < nblk; i++) {
    const int blk = blk0 + i;
    const float2* Xb = X + ((long)fm.x * n_blocks + blk) * NPAD;
    // D = conj(X) * F  (= conj(X * conj(F)), acquisition.sci:116), then radix-16
    load_mul_pass16(Xb, Fc, lds, t, sh);
    __syncthreads();
    pass33(lds, t);
    __syncthreads();
    float pw[32];  // pw[31] = this thread's leftover output (or -1)
    const float2 y = extra ? dft31_single(lds, tw, t) : make_float2(0.f, 0.f);
    pw[31] = extra ? (y.x * y.x + y.y * y.y) * inv_n2 : -1.f;
    v2f x[31];
#pragma unroll
    for (int d = 0; d < 31; d++) x[d] = ld2(lds[t * 31 + d]);
    dftp<31>(x);
#pragma unroll
    for (int d = 0; d < 31; d++) pw[d] = (x[d].x * x[d].x + x[d].y * x[d].y) * inv_n2;
    if (DUMP && blk == dump_block) {
      int k = kb;
#pragma unroll
      for (int d = 0; d < 31; d++) {
        dump_power[(long)rowid * N + k] = pw[d];
        k += E31;
        if (k >= N) k -= N;
      }
      if (extra) dump_power[(long)rowid * N + kx] = pw[31];
    }
    if (kNonCoh) {
#pragma unroll
      for (int d = 0; d < 32; d++) pacc[d % kAcc] += pw[d];
      __syncthreads();  // LDS is rewritten by the next block
      if (i + 1 < nblk) continue;
#pragma unroll
      for (int d = 0; d < 31; d++) pw[d] = pacc[d % kAcc];
      pw[31] = extra ? pacc[31 % kAcc] : -1.f;
    }
    // Row statistics (acq_peak.h).  Thread t's 31 strided outputs sit at natural
    // indices kb + 528 d (mod N): stride E31 = 528 for top2_exact, and the per-thread
    // top-2 (slot order) answers in one pass.  WIDE: an exact second pass over the
    // registers instead.  The leftover output (kx) is handled on its own.
    Top2<float> own{-1.f, -1.f, 0};   // (ak: the slot until the loop ends)
#pragma unroll
    for (int d = 0; d < 31; d++) push_slot_order(pw[d], d, own.a1, own.a2, own.ak);
    own.ak = kb + own.ak * E31;
    if (own.ak >= N) own.ak -= N;
    float v = own.a1;
    int kk = own.ak;
    if (extra && better(pw[31], kx, v, kk)) { v = pw[31]; kk = kx; }
    block_argmax(v, kk, s_pk);
    float sv = own.second(kk, spc, N);
    if (WIDE) {
      sv = -1.f;
      int k = kb;
#pragma unroll
      for (int d = 0; d < 31; d++) {
        if (outside_window(k, kk, spc, N)) sv = fmaxf(sv, pw[d]);
        k += E31;
        if (k >= N) k -= N;
      }
    }
    if (extra && outside_window(kx, kk, spc, N)) sv = fmaxf(sv, pw[31]);
    sv = block_max0(sv, s_mx);
    best_pk = v;
    best_k = kk;
    best_sec = sv;
  }
  if (t == 0) store_row(stats, rowid, blk0, n_blocks, kNonCoh, best_pk, best_k, best_sec);
}

// ---- the pipelined (persistent, two-role) correlation kernel -------------------
// Serves every best-of-blocks search with top2_exact(528, spc) (no dump, no non-coherent
// sum, no window wider than its top-2 statistics allow: those stay with
// acq_corr_kernel above).
// One workgroup per CU (the 128 KiB row fills the LDS), 1024 threads:
//   waves 0-7  ("compute"): the in-LDS passes of unit u -- 3x11, radix-31 --
//              and the row statistics;
//   waves 8-15 ("stream"):  the HBM/L2 loads, conj(X)*F and radix-16 of unit
//              u+G in registers while the compute waves work, the LDS write
//              of that row once the compute waves hold their radix-31 inputs,
//              and the 16 leftover radix-31 groups of unit u.
// Per unit:  P1 [3x11 | loads+radix-16]  S1  P2 [radix-31 inputs -> regs |
// leftover inputs -> side buffer]  S2  P3 [radix-31 + top-2 | row write +
// leftover outputs]  S3 (argmax)  P4 [second peak]  S4.
// Both roles keep their per-thread working set in the SAME register array r,
// so the stream role's 32 loaded values and the compute role's 31-33 values
// share VGPRs (the 1024-thread launch bound allows 128 per thread).
constexpr int kPipeThreads = 1024;
constexpr int kRole = 512;   // threads per role

template <int O>
__device__ __forceinline__ void dft16_r(v2f (&r)[33]) {
  v2f x[16];
#pragma unroll
  for (int i = 0; i < 16; i++) x[i] = r[O + i];
  dft16(x);
#pragma unroll
  for (int i = 0; i < 16; i++) r[O + i] = x[i];
}

// conj(X) * F for radix-16 groups g0 = tl and g1 = tl + 512 into r[0..15],
// r[16..31] (8-byte loads: consecutive lanes read consecutive columns, and the
// LDS writes of store16_r are bank-conflict free).  g1 = 1023 (tl = 511) is the
// zero pad column of the HBM rows; it is loaded but never stored.
// Column pairs of the stream role.  A code is real, so its spectrum is
// conjugate-symmetric: F[-k] = conj(F[k]).  Negation acts on the PFA slot
// coordinates one by one ((a, b, c, d) -> (-a, -b, -c, -d), the input map is
// linear), so stream thread tl owns group g = pair_group(tl) and its negative
// neg_group(g): 511 such pairs plus group 0 (self-paired, tl = 511, written
// twice with the same values) cover the 1023 groups, and only the 16 code
// values of g are loaded (acq_symmetrize_kernel makes the stored F exactly
// symmetric, so the derived half equals the stored one bit for bit).
__device__ __forceinline__ int pair_group(int tl) {
  if (tl < 495) return (tl / 15) * 31 + 1 + tl % 15;   // d = 1..15, every (b, c)
  if (tl < 510) {                                      // d = 0, c = 1..5, every b
    const int j = tl - 495;
    return ((j / 5) * 11 + 1 + j % 5) * 31;
  }
  return tl == 510 ? 341 : 0;                          // (1, 0, 0), then group 0
}

__device__ __forceinline__ int neg_group(int g) {
  const int d = g % 31, bc = g / 31, c = bc % 11, b = bc / 11;
  return (((3 - b) % 3) * 11 + (11 - c) % 11) * 31 + (31 - d) % 31;
}

__device__ __forceinline__ void load_mul_r(const float2* __restrict__ Xb,
                                           const float2* __restrict__ Fc, int tl,
                                           const Shift& sh, v2f (&r)[33]) {
  const auto rx = __builtin_amdgcn_make_buffer_rsrc((void*)Xb, 0, NPAD * 8, 0x00020000);
  const auto rf = __builtin_amdgcn_make_buffer_rsrc((void*)Fc, 0, NPAD * 8, 0x00020000);
  // tl is made opaque so that the group arithmetic is recomputed per unit
  // instead of being hoisted out of the unit loop
  int t0 = tl;
  asm volatile("" : "+v"(t0));
  const int ga = pair_group(t0), gb = neg_group(ga);
  const int foff = ga * 8;
  // Planes in groups of kLdGroup: all loads of a group are issued before any
  // of its products (sched_group_barrier pins the VMEM reads first), so a
  // unit costs 16 / kLdGroup L2 round trips instead of one per plane.
  // Column ga takes plane a with F[a]; column gb takes plane -a with conj(F[a]).
  // One group of all 48 loads measured 115.5 us against 118.8.
  constexpr int kLdGroup = 16;
  int x0off = foff, x1off = gb * 8;
  int pa_shift = 0;
  if (!(sh.a == 0 && sh.b == 0 && sh.c == 0 && sh.d == 0)) {   // uniform branch
    x0off = shift_group(ga, sh) * 8;
    x1off = shift_group(gb, sh) * 8;
    pa_shift = sh.a;
  }
#pragma unroll
  for (int a0 = 0; a0 < 16; a0 += kLdGroup) {
    f2v U0[kLdGroup], U1[kLdGroup], F0[kLdGroup];
#pragma unroll
    for (int a = 0; a < kLdGroup; a++) {
      const int an = (16 - (a0 + a)) & 15;
      const int pa = ((a0 + a - pa_shift) & 15) * kPlane * 8;
      const int pn = ((an - pa_shift) & 15) * kPlane * 8;
      const int pf = (a0 + a) * kPlane * 8;
      U0[a] = __builtin_bit_cast(f2v, __builtin_amdgcn_raw_buffer_load_b64(rx, x0off, pa, 0));
      U1[a] = __builtin_bit_cast(f2v, __builtin_amdgcn_raw_buffer_load_b64(rx, x1off, pn, 0));
      F0[a] = __builtin_bit_cast(f2v, __builtin_amdgcn_raw_buffer_load_b64(rf, foff, pf, 0));
    }
    __builtin_amdgcn_sched_group_barrier(0x020, 3 * kLdGroup, 0);
#pragma unroll
    for (int a = 0; a < kLdGroup; a++) {
      const int an = (16 - (a0 + a)) & 15;
      const v2f f0 = (v2f){F0[a].x, F0[a].y}, f1 = (v2f){F0[a].x, -F0[a].y};
      r[a0 + a] = bc(U0[a].x) * f0 + bc(U0[a].y) * mul_mi(f0);
      r[16 + an] = bc(U1[a].x) * f1 + bc(U1[a].y) * mul_mi(f1);
    }
  }
  dft16_r<0>(r);
  dft16_r<16>(r);
  // pin the radix-16 results here (P1): without this the arithmetic is sunk
  // past the barriers to its only use, the LDS write in P3
#pragma unroll
  for (int i = 0; i < 32; i++) asm volatile("" : "+v"(r[i]));
}

__device__ __forceinline__ void store16_r(float2* lds, int tl, const v2f (&r)[33]) {
  int t0 = tl;
  asm volatile("" : "+v"(t0));   // per-unit address arithmetic, not hoisted VGPRs
  const int ga = pair_group(t0), gb = neg_group(ga);
#pragma unroll
  for (int a = 0; a < 16; a++) {
    lds[a * M16 + ga] = st2(r[a]);
    lds[a * M16 + gb] = st2(r[16 + a]);
  }
}

// Threads t >= 496 compute a copy of task 0 and store nothing: r is then
// redefined on every lane (a lane that kept its old r would keep it live
// around the whole unit loop).
__device__ __forceinline__ void pass33_r(float2* lds, int t, v2f (&r)[33]) {
  const bool own = t < 16 * 31;
  const int tt = own ? t : 0;
  const int a = tt / 31, d = tt % 31;
  float2* base = lds + a * M16 + d;
#pragma unroll
  for (int i = 0; i < 33; i++) r[i] = ld2(base[i * 31]);
#pragma unroll
  for (int c = 0; c < 11; c++) dft3(r[c], r[11 + c], r[22 + c]);
#pragma unroll
  for (int b = 0; b < 3; b++) {
    v2f x[11];
#pragma unroll
    for (int c = 0; c < 11; c++) x[c] = r[b * 11 + c];
    dftp<11>(x);
#pragma unroll
    for (int c = 0; c < 11; c++) r[b * 11 + c] = x[c];
  }
  if (own) {
#pragma unroll
    for (int i = 0; i < 33; i++) base[i * 31] = st2(r[i]);
  }
}

// Radix-31 of r[0..30] reduced on the fly to this thread's top-2 powers
// |X_d|^2 * scale: the sums/differences overwrite r in place and each output
// pair is squared and folded into (m1, d1, m2) as soon as it exists, so no
// outputs are held (VGPR budget of the 1024-thread kernel).  Slots are visited
// in the order 0, 1, 30, 2, 29, ..., 15, 16; an exact tie keeps the earlier
// visited slot (push_slot_order).
__device__ __forceinline__ void dft31_top2(v2f (&r)[33], float scale, float& m1, float& m2,
                                           int& d1) {
  constexpr int P = 31, H = 15;
  const v2f x0 = r[0];
  v2f X0 = x0;
#pragma unroll
  for (int j = 1; j <= H; j++) {
    const v2f s = r[j] + r[P - j], d = r[j] - r[P - j];
    r[j] = s;
    r[P - j] = d;
    X0 += s;
  }
  m1 = (X0.x * X0.x + X0.y * X0.y) * scale;
  m2 = -1.f;
  d1 = 0;
#pragma unroll
  for (int m = 1; m <= H; m++) {
    v2f A = x0, B = (v2f){0.f, 0.f};
#pragma unroll
    for (int j = 1; j <= H; j++) {
      const int q = (j * m) % P;
      A += bc(kCos31[q]) * r[j];
      B += bc(kSin31[q]) * r[P - j];
    }
    // X_m = A - i B and X_{P-m} = A + i B, held as (re_m, re_{P-m}), (im_m, im_{P-m})
    // so that both powers come out of three packed instructions
    const v2f re = __builtin_elementwise_fma(bc(B.y), (v2f){1.f, -1.f}, bc(A.x));
    const v2f im = __builtin_elementwise_fma(bc(B.x), (v2f){-1.f, 1.f}, bc(A.y));
    const v2f pw = __builtin_elementwise_fma(im, im, re * re) * bc(scale);
    push_slot_order(pw.x, m, m1, m2, d1);
    push_slot_order(pw.y, P - m, m1, m2, d1);
  }
}

// One output pair (m, 31 - m) -- or X_0 for m = 0 -- of leftover radix-31
// group 512 + g, g = t / 16, m = t % 16, from the side copy of its inputs;
// twiddles from tw16[j][m] = (cos, sin)(2 pi jm / 31), j = 1..15.  Returns the
// pair's top-2 powers and the natural index of the larger.
__device__ __forceinline__ void leftover_pair(const float2* side, const float2* tw16, int t,
                                              float scale, float& m1, float& m2, int& k1) {
  const int g = t >> 4, m = t & 15;
  const float2* x = side + g * 31;
  const v2f x0 = ld2(x[0]);
  v2f A = x0, B = (v2f){0.f, 0.f};
#pragma unroll
  for (int j = 1; j <= 15; j++) {
    const v2f a = ld2(x[j]), b = ld2(x[31 - j]);
    const float2 w = tw16[j * 16 + m];
    A += bc(w.x) * (a + b);
    B += bc(w.y) * (a - b);
  }
  const v2f sb = swp(B);
  const v2f lo = __builtin_elementwise_fma(sb, (v2f){1.f, -1.f}, A);    // X_m
  const v2f hi = __builtin_elementwise_fma(sb, (v2f){-1.f, 1.f}, A);    // X_{31-m}
  const float pl = (lo.x * lo.x + lo.y * lo.y) * scale;
  const float ph = m ? (hi.x * hi.x + hi.y * hi.y) * scale : -1.f;
  const int d1 = ph > pl ? 31 - m : m;
  m1 = fmaxf(pl, ph);
  m2 = fminf(pl, ph);
  k1 = out_base(kThreads + g) + d1 * E31;
  k1 = k1 >= N ? k1 - N : k1;
  k1 = k1 >= N ? k1 - N : k1;
}

// Wave reductions with ds_swizzle (xor 1..16 within each 32-lane half, the
// pattern is an immediate: no per-lane address VGPRs to keep live); the two
// half-wave results go to separate scratch slots.
template <int X>
__device__ __forceinline__ float swz_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x1f | (X << 10)));
}
template <int X>
__device__ __forceinline__ int swz_i(int v) {
  return __builtin_amdgcn_ds_swizzle(v, 0x1f | (X << 10));
}

__device__ __forceinline__ void pick(float& v, int& k, float v2, int k2) {
  if (better(v2, k2, v, k)) { v = v2; k = k2; }
}

// (v, k) argmax over the workgroup (value max, smallest natural index among
// equals), broadcast to every thread: swizzle steps within 32-lane halves,
// the two halves via readlane, one slot per wave, one barrier, then a
// depth-4 tree over the NT/64 slots.
template <int NT>
__device__ __forceinline__ void block_argmax_n(float& v, int& k, PeakSlot* scratch) {
  pick(v, k, swz_f<1>(v), swz_i<1>(k));
  pick(v, k, swz_f<2>(v), swz_i<2>(k));
  pick(v, k, swz_f<4>(v), swz_i<4>(k));
  pick(v, k, swz_f<8>(v), swz_i<8>(k));
  pick(v, k, swz_f<16>(v), swz_i<16>(k));
  float va = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
  int ka = __builtin_amdgcn_readlane(k, 0);
  pick(va, ka, __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32)),
       __builtin_amdgcn_readlane(k, 32));
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = PeakSlot{va, ka};
  __syncthreads();
  constexpr int S = NT / 64;
  float sv[S];
  int sk[S];
#pragma unroll
  for (int i = 0; i < S; i++) { sv[i] = scratch[i].v; sk[i] = scratch[i].k; }
#pragma unroll
  for (int w = 1; w < S; w *= 2)
#pragma unroll
    for (int i = 0; i + w < S; i += 2 * w) pick(sv[i], sk[i], sv[i + w], sk[i + w]);
  v = sv[0];
  k = sk[0];
}

// max over the workgroup, valid in thread 0 only (one barrier)
template <int NT>
__device__ __forceinline__ float block_max0_n(float v, float* scratch) {
  v = fmaxf(v, swz_f<1>(v));
  v = fmaxf(v, swz_f<2>(v));
  v = fmaxf(v, swz_f<4>(v));
  v = fmaxf(v, swz_f<8>(v));
  v = fmaxf(v, swz_f<16>(v));
  const float h = fmaxf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0)),
                        __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32)));
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = h;
  __syncthreads();
  if (threadIdx.x == 0) {
    constexpr int S = NT / 64;
    float m[S];
#pragma unroll
    for (int i = 0; i < S; i++) m[i] = scratch[i];
#pragma unroll
    for (int w = 1; w < S; w *= 2)
#pragma unroll
      for (int i = 0; i + w < S; i += 2 * w) m[i] = fmaxf(m[i], m[i + w]);
    v = m[0];
  }
  return v;
}

struct UnitInfo {
  int rowid, blk, code;
  int4 fm;
};

__device__ __forceinline__ UnitInfo unit_info(int u, const int* __restrict__ order, int n_blocks,
                                              int n_bins, const int* __restrict__ group_code,
                                              const int* __restrict__ group_freq,
                                              const int4* __restrict__ fmap) {
  UnitInfo ui;
  const int unit = order[u];
  ui.rowid = unit / n_blocks;
  ui.blk = unit % n_blocks;
  const int g = ui.rowid / n_bins, bin = ui.rowid % n_bins;
  ui.code = group_code[g];
  ui.fm = fmap[group_freq[g * n_bins + bin]];
  return ui;
}

// Per-unit statistics of the pipelined kernel, carried across the next
// unit's barriers by the compute role.
struct RowCand {
  Top2<float> own, left;   // own group top-2, leftover pair top-2
};

// DPP lane exchanges (quad_perm 1032 / 2301, row_half_mirror, row_mirror):
// four steps leave every lane of each 16-lane row holding the row result;
// the four rows are combined through readlane.  Pure VALU, no LDS round trips.
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, dpp_i<CTRL>(__builtin_bit_cast(int, v)));
}
__device__ __forceinline__ float rl_f(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// wave-level (v, k) argmax -> one slot per wave
__device__ __forceinline__ void wave_argmax_slot(float v, int k, PeakSlot* slots) {
  pick(v, k, dpp_f<0xB1>(v), dpp_i<0xB1>(k));
  pick(v, k, dpp_f<0x4E>(v), dpp_i<0x4E>(k));
  pick(v, k, dpp_f<0x141>(v), dpp_i<0x141>(k));
  pick(v, k, dpp_f<0x140>(v), dpp_i<0x140>(k));
  float va = rl_f(v, 0);
  int ka = __builtin_amdgcn_readlane(k, 0);
  pick(va, ka, rl_f(v, 16), __builtin_amdgcn_readlane(k, 16));
  pick(va, ka, rl_f(v, 32), __builtin_amdgcn_readlane(k, 32));
  pick(va, ka, rl_f(v, 48), __builtin_amdgcn_readlane(k, 48));
  if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = PeakSlot{va, ka};
}

template <int S>
__device__ __forceinline__ PeakSlot read_argmax(const PeakSlot* slots) {
  float sv[S];
  int sk[S];
#pragma unroll
  for (int i = 0; i < S; i++) { sv[i] = slots[i].v; sk[i] = slots[i].k; }
#pragma unroll
  for (int w = 1; w < S; w *= 2)
#pragma unroll
    for (int i = 0; i + w < S; i += 2 * w) pick(sv[i], sk[i], sv[i + w], sk[i + w]);
  return PeakSlot{sv[0], sk[0]};
}

// second-peak candidate of this thread given the row argmax kk.  The slots of either
// set lie E31 = 528 samples apart: exact where top2_exact(E31, spc) only
// (correlate_launch sends wider windows to acq_corr_kernel<.., WIDE>)
// Top2::second spelled locally as !outside_window: through the header's wrap the
// compiler gives this kernel another instruction sequence, which measured slower.
__device__ __forceinline__ float second_cand(const RowCand& c, int kk, int spc) {
  auto in_win = [&](int k) {
    int dist = k - kk;
    if (dist < 0) dist += N;
    return dist < spc || dist > N - spc;
  };
  return fmaxf(in_win(c.own.ak) ? c.own.a2 : c.own.a1, in_win(c.left.ak) ? c.left.a2 : c.left.a1);
}

__device__ __forceinline__ void wave_max_slot(float v, float* slots) {
  v = fmaxf(v, dpp_f<0xB1>(v));
  v = fmaxf(v, dpp_f<0x4E>(v));
  v = fmaxf(v, dpp_f<0x141>(v));
  v = fmaxf(v, dpp_f<0x140>(v));
  const float h = fmaxf(fmaxf(rl_f(v, 0), rl_f(v, 16)), fmaxf(rl_f(v, 32), rl_f(v, 48)));
  if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = h;
}

template <int S>
__device__ __forceinline__ float read_max(const float* slots) {
  float m[S];
#pragma unroll
  for (int i = 0; i < S; i++) m[i] = slots[i];
#pragma unroll
  for (int w = 1; w < S; w *= 2)
#pragma unroll
    for (int i = 0; i + w < S; i += 2 * w) m[i] = fmaxf(m[i], m[i + w]);
  return m[0];
}

__device__ __forceinline__ void write_stats(gnsscorr_acq_row* stats, const UnitInfo& uc,
                                            int n_blocks, float peak, int argmax, float second) {
  store_row(stats, uc.rowid, uc.blk, n_blocks, false, peak, argmax, second);
}

// BEST_OF_BLOCKS statistics only (unit = (row, block)); launched with at most
// one workgroup per CU, each looping over units u = blockIdx.x + k * gridDim.x.
// Three barriers per unit:
//   P1 [compute: argmax of the previous unit from its slots, its second-peak
//       wave maxima, 3x11 pass | stream: loads + radix-16 of unit u+G]   S1
//   P2 [compute: radix-31 inputs -> regs, leftover inputs -> side copy;
//       thread 0: second peak + stats of the previous unit]              S2
//   P3 [compute: radix-31 + top-2, leftover pair, wave argmax slots |
//       stream: row write of unit u+G]                                   S3
// so the row statistics ride on the next unit's barriers.
__global__ __launch_bounds__(kPipeThreads) void acq_corr_pipe_kernel(
    const float2* __restrict__ X, const float2* __restrict__ F, int n_blocks,
    const int* __restrict__ group_code, const int* __restrict__ group_freq, int n_bins,
    int spc, gnsscorr_acq_row* __restrict__ stats, const int* __restrict__ order,
    const int4* __restrict__ fmap, int n_units) {
  constexpr int S = kRole / 64;   // statistics slots: one per compute wave
  __shared__ float2 lds[N];
  __shared__ float2 side[kLeft * 31];
  __shared__ float2 tw16[16 * 16];
  __shared__ PeakSlot s_pk[S];
  __shared__ float s_mx[S];
  const int t = threadIdx.x;
  // wave-uniform role, made visibly uniform (SGPR) so that the buffer
  // descriptors built inside role branches stay scalar
  const bool stream = __builtin_amdgcn_readfirstlane(t >> 9) != 0;
  const int tl = t & (kRole - 1);
  const int G = gridDim.x;
  const float inv_n2 = 1.0f / ((float)N * (float)N);
  int u = blockIdx.x;
  if (u >= n_units) return;
  if (t < 256) {
    const int j = t >> 4, m = t & 15, q = (j * m) % 31;   // tw16[j][m]: lanes m read 16 consecutive
    tw16[t] = make_float2(kCos31[q], kSin31[q]);
  }
  const int kb = out_base(tl);   // natural index of slot 0 of radix-31 group tl

  v2f r[33];
#pragma unroll
  for (int i = 0; i < 33; i++) r[i] = (v2f){0.f, 0.f};
  if (stream) {   // prologue: the first unit's radix-16 pass
    const UnitInfo un = unit_info(u, order, n_blocks, n_bins, group_code, group_freq, fmap);
    const Shift sh{un.fm.y, un.fm.z, un.fm.w >> 5, un.fm.w & 31};
    load_mul_r(X + ((long)un.fm.x * n_blocks + un.blk) * NPAD, F + (long)un.code * NPAD, tl, sh, r);
    store16_r(lds, tl, r);
  }
  __syncthreads();

  RowCand prev{{-1.f, -1.f, 0}, {-1.f, -1.f, 0}};
  PeakSlot pk{-1.f, 0};
  int it = 0;
  for (; u < n_units; u += G, it++) {
    const int un_next = u + G;
    const bool nxt = un_next < n_units;
    ACQ_PSTAMP(it, 0);
    // P1
    if (!stream) {
      if (it > 0) {   // previous unit: row argmax, then second-peak wave maxima
        pk = read_argmax<S>(s_pk);
        wave_max_slot(second_cand(prev, pk.k, spc), s_mx);
      }
      pass33_r(lds, tl, r);
    } else if (nxt) {
      const UnitInfo un = unit_info(un_next, order, n_blocks, n_bins, group_code, group_freq, fmap);
      const Shift sh{un.fm.y, un.fm.z, un.fm.w >> 5, un.fm.w & 31};
      load_mul_r(X + ((long)un.fm.x * n_blocks + un.blk) * NPAD, F + (long)un.code * NPAD, tl, sh, r);
    } else {
#pragma unroll
      for (int i = 0; i < 33; i++) r[i] = (v2f){0.f, 0.f};   // r is redefined on every path
    }
    ACQ_PSTAMP(it, 1);
    __syncthreads();   // S1
    ACQ_PSTAMP(it, 2);
    // P2
    if (!stream) {
#pragma unroll
      for (int d = 0; d < 31; d++) r[d] = ld2(lds[tl * 31 + d]);
      if (tl < kLeft * 31) side[tl] = lds[kThreads * 31 + tl];   // leftover inputs
      if (t == 0 && it > 0)
        write_stats(stats, unit_info(u - G, order, n_blocks, n_bins, group_code, group_freq, fmap),
                    n_blocks, pk.v, pk.k, read_max<S>(s_mx));
    }
    ACQ_PSTAMP(it, 3);
    __syncthreads();   // S2: the row is free
    ACQ_PSTAMP(it, 4);
    // P3: compute role -- radix-31 group tl, then (tl < 256) one output pair of
    // the 16 leftover groups from the side copy; stream role -- the row write
    if (!stream) {
      RowCand c{{-1.f, -1.f, 0}, {-1.f, -1.f, 0}};
      int d1;
      dft31_top2(r, inv_n2, c.own.a1, c.own.a2, d1);
      c.own.ak = kb + d1 * E31;
      if (c.own.ak >= N) c.own.ak -= N;
      if (tl < kLeft * 16)
        leftover_pair(side, tw16, tl, inv_n2, c.left.a1, c.left.a2, c.left.ak);
      float v = c.own.a1;
      int k = c.own.ak;
      pick(v, k, c.left.a1, c.left.ak);
      wave_argmax_slot(v, k, s_pk);
      prev = c;
    } else if (nxt) {
      store16_r(lds, tl, r);
    }
    ACQ_PSTAMP(it, 5);
    __syncthreads();   // S3: next row written, argmax slots complete
    ACQ_PSTAMP(it, 6);
  }
  // epilogue: statistics of the last unit
  if (!stream) {
    pk = read_argmax<S>(s_pk);
    wave_max_slot(second_cand(prev, pk.k, spc), s_mx);
  }
  __syncthreads();
  if (t == 0)
    write_stats(stats, unit_info(u - G, order, n_blocks, n_bins, group_code, group_freq, fmap),
                n_blocks, pk.v, pk.k, read_max<S>(s_mx));
}

// ---- host-side index tables ---------------------------------------------------
static int host_in_index(int p) {
  const int d = p % 31, c = (p / 31) % 11, b = (p / 341) % 3, a = p / 1023;
  return (a * M16 + b * M3 + c * M11 + d * M31) % N;
}
static int host_out_index(int p) {
  const int d = p % 31, c = (p / 31) % 11, b = (p / 341) % 3, a = p / 1023;
  return (int)(((long)a * E16 + (long)b * E3 + (long)c * E11 + (long)d * E31) % N);
}

}  // namespace

// Code spectra are spectra of real sequences; make them exactly
// conjugate-symmetric (F[-k] = conj(F[k]), F real at k = 0 and N/2) so the
// pipelined kernel may derive half of them (pair_group).  Slot s = a*M16 + g
// keeps its value when it precedes its negative and writes the negative.
__global__ __launch_bounds__(256) void acq_symmetrize_kernel(float2* __restrict__ F,
                                                             int n_codes) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)n_codes * N) return;
  const int code = (int)(i / N), sl = (int)(i % N);
  const int a = sl / M16, g = sl % M16;
  const int sn = ((16 - a) & 15) * M16 + neg_group(g);
  float2* Fc = F + (long)code * NPAD;
  const float2 v = Fc[a * kPlane + g];
  if (sl == sn)
    Fc[a * kPlane + g] = make_float2(v.x, 0.f);
  else if (sl < sn)
    Fc[(sn / M16) * kPlane + sn % M16] = make_float2(v.x, -v.y);
}

// ---- the engine interface (acq_ctx.h) ---------------------------------------------------------

int acq32_supports(int n_samples) { return n_samples == N; }

// the fp32 path's spectra and its store permutation
int acq32_init(gnsscorr_acq_ctx* c) {
  // self-check of the prime-factor maps: both must be bijections
  static int checked = 0;
  if (!checked) {
    char* seen = (char*)calloc(2 * N, 1);
    if (!seen) return GNSSCORR_ENOMEM;
    for (int p = 0; p < N; p++) { seen[host_in_index(p)]++; seen[N + host_out_index(p)]++; }
    for (int i = 0; i < 2 * N; i++)
      if (seen[i] != 1) { free(seen); gnsscorr_set_error("PFA map check failed"); return GNSSCORR_EINVAL; }
    free(seen);
    checked = 1;
  }
  const gnsscorr_acq_cfg* cfg = &c->cfg;
  acq32_ctx& e = c->f32;
  if (hipDeviceGetAttribute(&e.n_cu, hipDeviceAttributeMultiprocessorCount, cfg->device) !=
          hipSuccess || e.n_cu < 1)
    e.n_cu = 256;
  const size_t nF = NPAD * (size_t)cfg->max_codes;
  const size_t nX = NPAD * (size_t)cfg->max_freqs * cfg->max_blocks;
  HIP_TRY(hipMalloc(&e.d_sigma, sizeof(int) * N));
  HIP_TRY(hipMalloc(&e.d_F, sizeof(float2) * nF));
  HIP_TRY(hipMalloc(&e.d_X, sizeof(float2) * nX));
  HIP_TRY(hipMemset(e.d_F, 0, sizeof(float2) * nF));
  HIP_TRY(hipMemset(e.d_X, 0, sizeof(float2) * nX));
  HIP_TRY(hipMalloc(&e.d_fmap, sizeof(int4) * cfg->max_freqs));
  // sigma(p) = n^-1(k(p)): where the forward FFT's output k(p) must be stored
  // so that the correlation kernel reads its input n(p') linearly
  int* inv_in = (int*)malloc(sizeof(int) * 2 * N);
  if (!inv_in) return GNSSCORR_ENOMEM;
  int* sigma = inv_in + N;
  for (int p = 0; p < N; p++) inv_in[host_in_index(p)] = p;
  for (int p = 0; p < N; p++) {
    const int q = inv_in[host_out_index(p)];          // LDS position in the correlation kernel
    sigma[p] = (q / M16) * kPlane + q % M16;          // padded HBM index
  }
  const hipError_t err = hipMemcpy(e.d_sigma, sigma, sizeof(int) * N, hipMemcpyHostToDevice);
  free(inv_in);
  HIP_TRY(err);
  return GNSSCORR_OK;
}

void acq32_free(gnsscorr_acq_ctx* c) {
  acq32_ctx& e = c->f32;
  hostctx::release(e.d_sigma, e.d_F, e.d_X, e.d_fmap, e.d_stage);
}

// Once per context (gnsscorr_acq_create): this file's code object loaded
// (hipFuncGetAttributes loads it), so that the context's first set_codes and first
// search cost what every later one does.
int acq32_preload(gnsscorr_acq_ctx* c) {
  hipFuncAttributes a;
  HIP_TRY(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&acq_fwd16_kernel)));
  return GNSSCORR_OK;
}

// forward transform of n_rows rows into dst (padded correlation layout)
static int forward_launch(gnsscorr_acq_ctx* c, const int8_t* src, int iq, int n_blocks,
                          const double* d_freqs, int mode, int n_rows, float2* dst,
                          const double* d_cfreq, const int* d_nrows, int fuse_n = 0) {
  int rc = hostctx::grow(c->f32.d_stage, (size_t)n_rows * NPAD);
  if (rc) return rc;
  // grid-stride kernels: the device-side class count bounds the work, the grid
  // only the parallelism (n_rows is an upper bound of the rows)
  const int g16 = min(n_rows * ((M16 + kFwd1G - 1) / kFwd1G), 4096);
  const int g1023 = min(n_rows * 16, 1024);
  hipLaunchKernelGGL(acq_fwd16_kernel, dim3(g16),
                     dim3(kFwd1Threads), 0, c->stream, src, iq,
                     n_blocks, d_freqs, 1.0 / c->cfg.samp_rate, mode, c->f32.d_stage.p, d_cfreq,
                     d_nrows, mode == 0 ? c->coh : 1, n_rows, fuse_n, c->cfg.samp_rate / N,
                     c->f32.d_fmap, c->d_cfreq, c->d_nclass);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(acq_fwd1023_kernel, dim3(g1023), dim3(kFwd2Threads), 0, c->stream,
                     c->f32.d_stage.p,
                     c->f32.d_sigma, dst, n_blocks, d_nrows, n_rows);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

// spectra of the n_codes int8 replicas at d_codes (device), kept resident, made exactly
// conjugate-symmetric.  code_len is not needed: the replicas are already zero above it.
int acq32_set_codes(gnsscorr_acq_ctx* c, const int8_t* d_codes, int n_codes, int code_len) {
  int rc = forward_launch(c, d_codes, 0, 1, nullptr, 1, n_codes, c->f32.d_F, nullptr, nullptr);
  if (rc) return rc;
  hipLaunchKernelGGL(acq_symmetrize_kernel, dim3((n_codes * N + 255) / 256), dim3(256), 0,
                     c->stream, c->f32.d_F, n_codes);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

int acq32_spectra(gnsscorr_acq_ctx* c, const int8_t* d_if, int iq, int n_blocks, int n_freqs,
                  const double* d_freqs) {
  // spectrum classes on the fs/N grid (one forward FFT per class and block)
  const int fuse = n_freqs <= kFuseClass ? n_freqs : 0;
  if (!fuse) {
    const size_t cls_lds =
        n_freqs <= kClassLds ? (size_t)((n_freqs + 1) & ~1) * 8 + (size_t)n_freqs * 16 : 0;
    hipLaunchKernelGGL(acq_classify_kernel, dim3(1), dim3(1024), cls_lds, c->stream, d_freqs,
                       n_freqs, c->cfg.samp_rate / N, c->f32.d_fmap, c->d_cfreq, c->d_nclass,
                       c->d_resid);
    HIP_TRY(hipGetLastError());
  }
  return forward_launch(c, d_if, iq, n_blocks, d_freqs, 0, n_freqs * n_blocks, c->f32.d_X,
                        c->d_cfreq, c->d_nclass, fuse);
}

// the front has sized d_stats and built d_order for these units (correlate_launch)
int acq32_correlate(gnsscorr_acq_ctx* c, int n_blocks, int mode, int n_groups, int n_bins,
                    const int32_t* d_gcode, const int32_t* d_gfreq, int spc, double* d_dump,
                    int dump_block) {
  const acq32_ctx& e = c->f32;
  const int n_units = n_groups * n_bins * (mode == GNSSCORR_ACQ_NONCOHERENT ? 1 : n_blocks);
#define ACQ_CORR_LAUNCH(M, D, W)                                                             \
  hipLaunchKernelGGL((acq_corr_kernel<M, D, W>), dim3(n_units), dim3(kThreads), 0, c->stream, \
                     e.d_X, e.d_F, n_blocks, d_gcode, d_gfreq, n_bins, spc, c->d_stats.p,      \
                     d_dump, dump_block, c->d_order.p, e.d_fmap)
  // a thread's outputs lie E31 = 528 apart; windows too wide for its top-2 take the
  // one-unit kernel's exact pass (the power-row dump searches at spc 16)
  const bool wide = !top2_exact(E31, spc);
  if (d_dump)
    ACQ_CORR_LAUNCH(GNSSCORR_ACQ_BEST_OF_BLOCKS, true, false);
  else if (mode == GNSSCORR_ACQ_NONCOHERENT && wide)
    ACQ_CORR_LAUNCH(GNSSCORR_ACQ_NONCOHERENT, false, true);
  else if (mode == GNSSCORR_ACQ_NONCOHERENT)
    ACQ_CORR_LAUNCH(GNSSCORR_ACQ_NONCOHERENT, false, false);
  else if (wide)
    ACQ_CORR_LAUNCH(GNSSCORR_ACQ_BEST_OF_BLOCKS, false, true);
  else
    hipLaunchKernelGGL(acq_corr_pipe_kernel, dim3(n_units < e.n_cu ? n_units : e.n_cu),
                       dim3(kPipeThreads), 0, c->stream, e.d_X, e.d_F, n_blocks, d_gcode,
                       d_gfreq, n_bins, spc, c->d_stats.p, c->d_order.p, e.d_fmap, n_units);
#undef ACQ_CORR_LAUNCH
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}
