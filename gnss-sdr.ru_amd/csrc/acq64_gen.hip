// acq64_gen.hip -- the generic-N engine of the fp64 acquisition (acq64.hip: the
// compiled plans), for any other samplesPerCode, e.g. acquisition.sci at fs = 5 or
// 38.192 MHz.  The same fp64 pipeline on rows in global memory, by three engines behind
// one set of host entry points (acq64_gen_*, acq_ctx.h) and one search driver
// (acq64_gen_correlate):
//  * Bluestein's chirp-z (g_* kernels, bz_* host code): every length-N DFT by the
//    identity  X_k = c_k sum_n (a_n c_n) conj(c_{k-n}),  c_n = exp(-i pi n^2 / N),
//    i.e. a cyclic convolution of length M = 2^q >= 2N - 1 (radix-16 Stockham
//    passes in global memory, the last one radix 2, 4 or 8 when q is not a
//    multiple of 4).  A fallback for sizes with a prime factor above 31: correct to
//    fp64 rounding, not tuned;
//  * the mixed-radix Stockham passes (mx_*), N a product of compiled radices;
//  * the four-step plan (m4_*) where one is compiled for N.
// The g_stats* kernels are the row statistics of all three.
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include "acq64_dft.h"
#include "acq_ctx.h"
#include "if2.h"
#include "if16.h"

namespace {

// pass modes, template arguments of mx_pass, of m4_cols2 (In) and of m4_rows2 (Out);
// plain ints, explained at the kernels
constexpr int kMxRows = 0, kMxCorrIn = 1, kMxPower = 2, kMxPowerKeep = 3, kMxPowerHalf = 4,
              kMxRowsZeroTail = 5;
constexpr int kM4InRows = 0, kM4InCorr = 1;
constexpr int kM4OutRows = 0, kM4OutPower = 2, kM4OutTop2 = 3;

// ---- Bluestein's kernels -------------------------------------------------------------
constexpr int kGThreads = 256;

// one radix-R Stockham pass (autosort), forward: Ns = product of the earlier
// passes' radices
template <int R>
__global__ __launch_bounds__(kGThreads) void g_fft_pass(const v2d* __restrict__ in,
                                                        v2d* __restrict__ out, int M, int Ns,
                                                        const v2d* __restrict__ twM) {
  const int j = blockIdx.x * kGThreads + threadIdx.x;   // < M / R
  const long row = (long)blockIdx.y * M;
  if (j >= M / R) return;
  const int k = j & (Ns - 1);
  const int tstep = k * (M / (R * Ns));                   // twiddle W_M^(r * tstep)
  v2d v[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    const v2d x = in[row + j + r * (M / R)];
    v[r] = r == 0 ? x : cmul(x, twM[(r * tstep) & (M - 1)]);
  }
  dft<R>(v);
  const int d = (j / Ns) * Ns * R + k;
#pragma unroll
  for (int r = 0; r < R; r++) out[row + d + r * Ns] = v[r];
}

// A[row] = (a_n c_n | 0...) from natural rows a (stride src_rs)
__global__ __launch_bounds__(kGThreads) void g_pre_kernel(const v2d* __restrict__ a, int src_rs,
                                                          const v2d* __restrict__ chirp, int N,
                                                          int M, v2d* __restrict__ A) {
  const int n = blockIdx.x * kGThreads + threadIdx.x;
  if (n >= M) return;
  const long r = blockIdx.y;
  A[r * M + n] = n < N ? cmul(a[r * src_rs + n], chirp[n]) : (v2d){0.0, 0.0};
}

// correlation rows of a chunk: Y_k = conj(X_cls,blk[k - m]) F_code[k] (as acq64_corr_kernel),
// times c_k, zero padded.  unit = u0 + blockIdx.y; block `blk` of it (-1: the unit's own).
__global__ __launch_bounds__(kGThreads) void g_corr_pre_kernel(
    const v2d* __restrict__ X, const v2d* __restrict__ F, int rs, int n_blocks, int nc_blk,
    const int* __restrict__ group_code, const int* __restrict__ group_freq, int n_bins,
    const int2* __restrict__ fmap, int u0, const v2d* __restrict__ chirp, int N, int M,
    v2d* __restrict__ A) {
  const int n = blockIdx.x * kGThreads + threadIdx.x;
  if (n >= M) return;
  const int unit = u0 + blockIdx.y;
  const int rowid = nc_blk >= 0 ? unit : unit / n_blocks;
  const int blk = nc_blk >= 0 ? nc_blk : unit % n_blocks;
  const int g = rowid / n_bins, bin = rowid % n_bins;
  v2d y = (v2d){0.0, 0.0};
  if (n < N) {
    const int2 fm = fmap[group_freq[g * n_bins + bin]];
    int s = n - fm.y;
    s += s < 0 ? N : 0;
    const v2d x = X[((long)fm.x * n_blocks + blk) * rs + s];
    const v2d f = F[(long)group_code[g] * rs + n];
    y = cmul((v2d){fma(x.x, f.x, x.y * f.y), fma(x.x, f.y, -(x.y * f.x))}, chirp[n]);
  }
  A[(long)blockIdx.y * M + n] = y;
}

// B = conj(A * Vf)   (IFFT_M(Z) = conj(FFT_M(conj Z)) / M)
__global__ __launch_bounds__(kGThreads) void g_mulv_kernel(const v2d* __restrict__ A,
                                                           const v2d* __restrict__ vf, int M,
                                                           v2d* __restrict__ B) {
  const int n = blockIdx.x * kGThreads + threadIdx.x;
  if (n >= M) return;
  const long i = (long)blockIdx.y * M + n;
  const v2d z = cmul(A[i], vf[n]);
  B[i] = (v2d){z.x, -z.y};
}

// spectra: out[k] = c_k conj(D_k) / M
__global__ __launch_bounds__(kGThreads) void g_post_kernel(const v2d* __restrict__ D,
                                                           const v2d* __restrict__ chirp, int N,
                                                           int M, v2d* __restrict__ out, int rs) {
  const int k = blockIdx.x * kGThreads + threadIdx.x;
  if (k >= N) return;
  const v2d d = D[(long)blockIdx.y * M + k];
  const double inv = 1.0 / (double)M;
  out[(long)blockIdx.y * rs + k] = cmul((v2d){d.x * inv, -d.y * inv}, chirp[k]);
}

// powers |DFT_N(Y)|^2 / N^2 = |D_k|^2 / (M N)^2, stored or added; lags k < n_out
// (N, or the kept lags of a zero-padded search) of rows of stride N
__global__ __launch_bounds__(kGThreads) void g_power_kernel(const v2d* __restrict__ D, int N,
                                                            int M, int acc,
                                                            double* __restrict__ pw, int n_out) {
  const int k = blockIdx.x * kGThreads + threadIdx.x;
  if (k >= n_out) return;
  const v2d d = D[(long)blockIdx.y * M + k];
  const double sc = 1.0 / ((double)M * (double)N);
  const double p = fma(d.x * sc, d.x * sc, (d.y * sc) * (d.y * sc));
  double* o = pw + (long)blockIdx.y * N + k;
  *o = acc ? *o + p : p;
}

// Row statistics of a power row (acq_peak.h), two kernels that differ in their scan.
// N: the lags searched, circular in N (the row length, or the kept lags of a
// zero-padded search: E1/acquisition.sci:121-145); rs: the stride of the rows of pw.
// Their common end: the power-row dump, the row record.
template <int NT>
__device__ __forceinline__ void g_stats_finish(const double* __restrict__ row, int N, int unit,
                                               int n_blocks, int nc, double bv, int bk, double sv,
                                               gnsscorr_acq_row* __restrict__ stats,
                                               double* __restrict__ dump, int dump_block) {
  const auto [rowid, blk0] = unit_row(unit, n_blocks, nc);
  if (dump && !nc && blk0 == dump_block)
    for (int k = threadIdx.x; k < N; k += NT) dump[(long)rowid * N + k] = row[k];
  if (threadIdx.x == 0) store_row(stats, rowid, blk0, n_blocks, nc, bv, bk, sv);
}

// two passes, exact for every window: the argmax, then the maximum outside the window
// (period = 0), or over the candidate range of GLONASS/L3/acquisition.sci:134-153 written
// on `period` samples (set_peak_period; acq_peak.h: in_period_range)
__global__ __launch_bounds__(kGThreads) void g_stats_kernel(const double* __restrict__ pw, int N,
                                                            int u0, int n_blocks, int nc, int spc,
                                                            gnsscorr_acq_row* __restrict__ stats,
                                                            double* __restrict__ dump,
                                                            int dump_block, int rs, int period) {
  __shared__ double s_v[kGThreads / 64], s_m[kGThreads / 64];
  __shared__ int s_k[kGThreads / 64];
  const double* row = pw + (long)blockIdx.x * rs;
  double bv = -1.0;
  int bk = INT_MAX;
  for (int k = threadIdx.x; k < N; k += kGThreads)
    if (row[k] > bv) { bv = row[k]; bk = k; }     // first index within the thread's stride
  block_argmax<kGThreads / 64>(bv, bk, s_v, s_k);
  double sv = -1.0;
  for (int k = threadIdx.x; k < N; k += kGThreads)
    if (period ? in_period_range(k, bk, spc, period) : outside_window(k, bk, spc, N))
      sv = fmax(sv, row[k]);
  sv = block_max0<kGThreads / 64>(sv, s_m);
  g_stats_finish<kGThreads>(row, N, u0 + blockIdx.x, n_blocks, nc, bv, bk, sv, stats, dump,
                            dump_block);
}

// One pass (the generic path's default): 1024 threads, thread t keeps the top-2 of
// k = t, t + 1024, ...  Same results as g_stats_kernel where stats1_exact holds; one
// read of the row.
constexpr int kStatsThreads = 1024;
// The stride of a thread's samples for top2_exact: kStatsThreads, except across the
// wrap, where thread t's last sample t + kStatsThreads q and its first lie
// N - kStatsThreads q apart, smallest (r = N - kStatsThreads floor((N - 1) / kStatsThreads))
// for the threads with the most samples (304 at N = 38192, 16 at N = 16400).
static inline bool stats1_exact(int N, int spc) {
  const int r = N <= kStatsThreads ? kStatsThreads : N - kStatsThreads * ((N - 1) / kStatsThreads);
  return top2_exact(r < kStatsThreads ? r : kStatsThreads, spc);
}
__global__ __launch_bounds__(kStatsThreads) void g_stats1_kernel(
    const double* __restrict__ pw, int N, int u0, int n_blocks, int nc, int spc,
    gnsscorr_acq_row* __restrict__ stats, double* __restrict__ dump, int dump_block, int rs) {
  __shared__ double s_v[kStatsThreads / 64], s_m[kStatsThreads / 64];
  __shared__ int s_k[kStatsThreads / 64];
  const double* row = pw + (long)blockIdx.x * rs;
  Top2<double> own;
  for (int k = threadIdx.x; k < N; k += kStatsThreads) own.push(row[k], k);
  double bv = own.a1;
  int bk = own.ak;
  block_argmax<kStatsThreads / 64>(bv, bk, s_v, s_k);
  const double sv = block_max0<kStatsThreads / 64>(own.second(bk, spc, N), s_m);
  g_stats_finish<kStatsThreads>(row, N, u0 + blockIdx.x, n_blocks, nc, bv, bk, sv, stats, dump,
                                dump_block);
}

// the row statistics of a chunk's nu power rows (units u0 ...) on stream st: the one
// pass where it is exact, else the two passes; always the two passes for the period
// rule of a zero-padded search (set_peak_period), which no thread's top-2 answers
int g_stats_launch(gnsscorr_acq_ctx* c, hipStream_t st, const double* pw, int NK, int nu, int u0,
                   int n_blocks, bool nc, int spc, double* d_dump, int dump_block) {
  const int period = c->keep ? c->peak_period : 0;
  if (!period && stats1_exact(NK, spc))
    hipLaunchKernelGGL(g_stats1_kernel, dim3(nu), dim3(kStatsThreads), 0, st, pw, NK, u0,
                       n_blocks, (int)nc, spc, c->d_stats.p, d_dump, dump_block,
                       c->cfg.n_samples);
  else
    hipLaunchKernelGGL(g_stats_kernel, dim3(nu), dim3(kGThreads), 0, st, pw, NK, u0, n_blocks,
                       (int)nc, spc, c->d_stats.p, d_dump, dump_block, c->cfg.n_samples, period);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

// Row statistics of a concatenated search (GNSSCORR_ACQ_CONCAT): the row of one (group,
// bin) is the kept lags of its n_blocks blocks laid end to end
// (COMPASS/B1/acquisition_7x3ms.sci:139-145), index q at lag q % keep of power row
// q / keep; the blocks' power rows are consecutive, rs apart.  One workgroup per
// (group, bin): the argmax over the n_blocks * keep lags (first index among equals, so
// the first of exactly equal blocks, :154-157), then the maximum over the candidates
// with n = n_blocks * keep -- outside the window circular in n, or with a period the
// range of :159-176 (acq_peak.h: in_period_range), scanned over its span only
// (period_span: at most period + 1 lags of the row, which may cross a block boundary).
__global__ __launch_bounds__(kGThreads) void g_stats_concat_kernel(
    const double* __restrict__ pw, int keep, int n_blocks, int r0, int spc,
    gnsscorr_acq_row* __restrict__ stats, int rs, int period) {
  __shared__ double s_v[kGThreads / 64], s_m[kGThreads / 64];
  __shared__ int s_k[kGThreads / 64];
  const double* rows = pw + (long)blockIdx.x * n_blocks * rs;
  const int n = n_blocks * keep;
  double bv = -1.0;
  int bk = INT_MAX;
  for (int b = 0; b < n_blocks; b++) {
    const double* row = rows + (long)b * rs;
    for (int k = threadIdx.x; k < keep; k += kGThreads)
      if (better(row[k], b * keep + k, bv, bk)) { bv = row[k]; bk = b * keep + k; }
  }
  block_argmax<kGThreads / 64>(bv, bk, s_v, s_k);
  double sv = -1.0;
  if (period) {
    const PeriodSpan sp = period_span(bk, spc, period);
    const int hi = sp.hi < n ? sp.hi : n - 1;
    for (int q = sp.lo + threadIdx.x; q <= hi; q += kGThreads)
      if (in_period_range(q, bk, spc, period))
        sv = fmax(sv, rows[(long)(q / keep) * rs + q % keep]);
  } else {
    for (int b = 0; b < n_blocks; b++) {
      const double* row = rows + (long)b * rs;
      for (int k = threadIdx.x; k < keep; k += kGThreads)
        if (outside_window(b * keep + k, bk, spc, n)) sv = fmax(sv, row[k]);
    }
  }
  sv = block_max0<kGThreads / 64>(sv, s_m);
  if (threadIdx.x == 0) {
    gnsscorr_acq_row r;
    r.peak = bv;
    r.second = sv;
    r.argmax = bk;
    r.block = bk / keep;
    stats[r0 + blockIdx.x] = r;   // one record per (group, bin): acq_select with one block
  }
}

// the statistics of a concatenated search's chunk: units u0 .. u0 + nu - 1 are whole
// rows (both a multiple of n_blocks), their power rows consecutive in pw
int g_stats_concat_launch(gnsscorr_acq_ctx* c, hipStream_t st, const double* pw, int nu, int u0,
                          int n_blocks, int spc) {
  hipLaunchKernelGGL(g_stats_concat_kernel, dim3(nu / n_blocks), dim3(kGThreads), 0, st, pw,
                     c->keep, n_blocks, u0 / n_blocks, spc, c->d_stats.p, c->cfg.n_samples,
                     c->peak_period);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

// wipe-off rows in natural order (acq64_wipe_kernel with a runtime N; I16 as there: the
// GNSSCORR_IF_INT16 kernel, the int8 / packed one keeps its code)
template <bool I16 = false>
__global__ __launch_bounds__(256) void g_wipe_kernel(const int8_t* __restrict__ src, int iq,
                                                     int n_blocks, int coh, long bstride,
                                                     const double* __restrict__ cfreq,
                                                     const int* __restrict__ n_cls_dev, double ts,
                                                     int N, v2d* __restrict__ out) {
  const long total = (long)(*n_cls_dev) * n_blocks * N;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int row = (int)(i / N), n = (int)(i % N);
    const int cls = row / n_blocks, blk = row % n_blocks;
    const double f = cfreq[cls];
    const bool cplx = iq & GNSSCORR_IF_IQ, pk = iq & GNSSCORR_IF_PACKED2;
    const int ne = cplx ? 2 : 1;
    // the block's first element: bstride samples after the previous block's (coh * N end
    // to end, or the block stride of set_block_stride: acquisition_7x3ms.sci:52-58)
    const long e0 = (long)blk * bstride * ne;
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
    out[(long)row * N + n] = (v2d){re, im};
  }
}

__global__ __launch_bounds__(256) void g_codes_kernel(const int8_t* __restrict__ codes, long n,
                                                      v2d* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (v2d){(double)codes[i], 0.0};
}

// ---------------------------------------------------------------------------------
// Mixed-radix Stockham FFT of length N (the generic path's default since round 5):
// N = R_1 ... R_P, every R_i a radix the kernels are compiled for (mix_factor).
// Pass i (Ns = R_1 ... R_{i-1}) reads elements j + r N/R_i (r < R_i) of a row,
// multiplies element r by W_{Ns R}^{r k} (k = j mod Ns; = W_N^{r k N/(Ns R)}, the
// table d_twN), runs a radix-R DFT in registers (dft<R>) and writes positions
// (j / Ns) Ns R + k + r Ns: autosort, natural order out, no bit reversal.
// Against Bluestein (two FFTs of length M = 2^q >= 2N - 1 per DFT plus the chirp
// passes, ~60 N x 16 B of row traffic per correlation row at N = 38 192) a
// correlation row moves ~5.5 N x 16 B: the product conj(X[k - m]) F[k] is formed
// inside the first pass and |.|^2 / N^2 inside the last (added over the blocks of a
// non-coherent search), so no pre / post passes run (acquisition.sci:107-132).
// ---------------------------------------------------------------------------------
constexpr int kMixThreads = 128;

struct MixCorr {
  const v2d* X;
  const v2d* F;
  int rs, n_blocks, nc_blk, n_bins, u0;
  const int* group_code;
  const int* group_freq;
  const int2* fmap;
  // records (gnsscorr_acq_set_records): virtual group g = rec * n_groups + g0 searches
  // group g0 on record rec, whose blocks are rec * n_blocks ... of the spectra's nbT
  int n_groups = 1 << 30, nbT = 0;
  int keep = 0;   // zero-padded search: the lags kept by the last pass (kMxPowerKeep / Half)
};

// a correlation unit's class spectrum row and code spectrum row (kMxCorrIn, kM4InCorr)
__device__ __forceinline__ void mix_unit_rows(const MixCorr& cp, int unit, const v2d*& Xr,
                                              const v2d*& Fr, int& shift) {
  const int rowid = cp.nc_blk >= 0 ? unit : unit / cp.n_blocks;
  const int blk = cp.nc_blk >= 0 ? cp.nc_blk : unit % cp.n_blocks;
  const int g = rowid / cp.n_bins, bin = rowid % cp.n_bins;
  const int rec = g / cp.n_groups, g0 = g - rec * cp.n_groups;
  const int2 fm = cp.fmap[cp.group_freq[g0 * cp.n_bins + bin]];
  Xr = cp.X + ((long)fm.x * cp.nbT + rec * cp.n_blocks + blk) * cp.rs;
  Fr = cp.F + (long)cp.group_code[g0] * cp.rs;
  shift = fm.y;
}

// kMxRows: rows in (stride in_rs) -> rows out (stride out_rs)
// kMxCorrIn: first pass of a correlation chunk: the input is y[n] = conj(X[n - m]) F[n] of
//         unit u0 + row (its bin's class spectrum shifted by m, acquisition.sci:116)
// kMxPower: last pass of a correlation chunk: |.|^2 / N^2 into pw (added when acc)
// kMxPowerKeep: kMxPower of a zero-padded search: only lags < cp.keep are squared, stored or
//         added (a bound check per output; any keep)
// kMxPowerHalf: kMxPower of a zero-padded search with keep = N/2 and an even last radix:
//         Ns = N/R, output r of butterfly k lands at lag k + r Ns, so the kept lags are the
//         outputs r < R/2 and only those are formed (dft_first_half); even R only
// kMxRowsZeroTail: kMxRows as the first pass (Ns = 1) of rows that are zero from element n_in
//         on (zero-extended codes; n_in is passed in `acc`): input r of every butterfly is
//         element j + r N/R, so the inputs r >= ceil(n_in / (N/R)) are zero for every j
//         and are not loaded
// occupancy: a pass is latency bound (strided row loads, one butterfly per thread),
// so the register allocator is held to 3 waves per SIMD up to radix 16 (the fused
// first pass otherwise keeps all 2R complex loads in flight: 244 VGPRs, 2 waves;
// at 4 waves radix 16 spills)
template <int R>
constexpr int mx_waves() { return R <= 16 ? 3 : 2; }
template <int R, int MODE>
__global__ __launch_bounds__(kMixThreads, mx_waves<R>()) void mx_pass(const v2d* __restrict__ in, int in_rs,
                                                       v2d* __restrict__ out, int out_rs, int N,
                                                       int Ns, const v2d* __restrict__ tw,
                                                       MixCorr cp, double* __restrict__ pw,
                                                       int acc) {
  const int j = blockIdx.x * kMixThreads + threadIdx.x;   // < N / R
  if (j >= N / R) return;
  const long row = blockIdx.y;
  const int NR = N / R;
  v2d v[R];
  if constexpr (MODE == kMxCorrIn) {
    const v2d *Xr, *Fr;
    int shift;
    mix_unit_rows(cp, cp.u0 + (int)row, Xr, Fr, shift);
#pragma unroll
    for (int r = 0; r < R; r++) {
      const int n = j + r * NR;
      int s = n - shift;
      s += s < 0 ? N : 0;
      const v2d x = Xr[s], f = Fr[n];
      v[r] = (v2d){fma(x.x, f.x, x.y * f.y), fma(x.x, f.y, -(x.y * f.x))};
    }
  } else if constexpr (MODE == kMxRowsZeroTail) {
    const int nz = (acc + NR - 1) / NR;   // inputs r >= nz are zero
#pragma unroll
    for (int r = 0; r < R; r++)
      v[r] = r < nz ? in[row * in_rs + j + r * NR] : (v2d){0.0, 0.0};
  } else {
#pragma unroll
    for (int r = 0; r < R; r++) v[r] = in[row * in_rs + j + r * NR];
  }
  const int k = j % Ns;
  const int ts = k * (N / (Ns * R));   // r ts < N
#pragma unroll
  for (int r = 1; r < R; r++) v[r] = cmul(v[r], tw[r * ts]);
  if constexpr (MODE == kMxPowerHalf) {
    // Ns = N/R: k = j is the butterfly's first output lag, and the kept lags
    // k + r Ns < N/2 are r < R/2
    static_assert(R % 2 == 0, "the half last pass needs an even radix");
    v2d h[R / 2];
    dft_first_half<R>(v, h);
    const double sc = 1.0 / ((double)N * (double)N);
    double* o = pw + row * N + k;
#pragma unroll
    for (int r = 0; r < R / 2; r++) {
      const double q = fma(h[r].x, h[r].x, h[r].y * h[r].y) * sc;
      o[r * Ns] = acc ? o[r * Ns] + q : q;
    }
    return;
  }
  dft<R>(v);
  const int d = (j / Ns) * Ns * R + k;
  if constexpr (MODE == kMxPowerKeep) {
    const double sc = 1.0 / ((double)N * (double)N);
    double* o = pw + row * N + d;
#pragma unroll
    for (int r = 0; r < R; r++)
      if (d + r * Ns < cp.keep) {
        const double q = fma(v[r].x, v[r].x, v[r].y * v[r].y) * sc;
        o[r * Ns] = acc ? o[r * Ns] + q : q;
      }
  } else if constexpr (MODE == kMxPower) {
    const double sc = 1.0 / ((double)N * (double)N);
    double* o = pw + row * N + d;
#pragma unroll
    for (int r = 0; r < R; r++) {
      const double q = fma(v[r].x, v[r].x, v[r].y * v[r].y) * sc;
      o[r * Ns] = acc ? o[r * Ns] + q : q;
    }
  } else {
#pragma unroll
    for (int r = 0; r < R; r++) out[row * out_rs + d + r * Ns] = v[r];
  }
}

// the radices mx_pass is compiled for, largest first within a power of two
#define MIX_RADICES(X) X(16) X(8) X(4) X(2) X(3) X(5) X(7) X(11) X(13) X(17) X(19) X(23) X(29) X(31)

// N -> radices (powers of two as 16s, then one 8 / 4 / 2; odd primes); 0 when a
// prime factor above 31 remains (Bluestein).  38192 -> 7, 16, 31, 11.
int mix_factor(int N, int* r) {
  int n = 0, m = N;
  while (m % 16 == 0 && n < 24) { r[n++] = 16; m /= 16; }
  if (m % 8 == 0) { r[n++] = 8; m /= 8; }
  else if (m % 4 == 0) { r[n++] = 4; m /= 4; }
  else if (m % 2 == 0) { r[n++] = 2; m /= 2; }
  const int odd[] = {3, 5, 7, 11, 13, 17, 19, 23, 29, 31};
  for (int p : odd)
    while (m % p == 0 && n < 24) { r[n++] = p; m /= p; }
  if (m != 1 || n < 2) return 0;
  // the fused passes take the smallest radices (fewest registers): the first (the
  // correlation product, 2R loads) the smallest, the last (|.|^2) the next one
  for (int a = 0; a < n; a++)
    for (int b = a + 1; b < n; b++)
      if (r[b] < r[a]) { const int t = r[a]; r[a] = r[b]; r[b] = t; }
  const int second = r[1];
  for (int a = 1; a + 1 < n; a++) r[a] = r[a + 1];
  r[n - 1] = second;
  return n;
}

// the order of a zero-padded search's correlation passes (set_zero_padded): the smallest
// even radix last, so that with keep = N/2 the last pass forms half of its outputs
// (mx_pass kMxPowerHalf); the first pass keeps the smallest of the others; r unchanged for an
// odd N.  128000 -> 5, 5, 5, 16, 16, 4 (unpadded: 4, 5, 5, 16, 16, 5).
void mix_order_padded(const int* r, int n, int* rp) {
  int t[24];
  for (int a = 0; a < n; a++) t[a] = r[a];
  for (int a = 0; a < n; a++)
    for (int b = a + 1; b < n; b++)
      if (t[b] < t[a]) { const int x = t[a]; t[a] = t[b]; t[b] = x; }
  int e = -1;
  for (int a = 0; a < n && e < 0; a++)
    if (t[a] % 2 == 0) e = a;
  if (e < 0) {
    for (int a = 0; a < n; a++) rp[a] = r[a];
    return;
  }
  int m = 0;
  for (int a = 0; a < n; a++)
    if (a != e) rp[m++] = t[a];
  rp[n - 1] = t[e];
}

template <int MODE>
int mx_launch(gnsscorr_acq_ctx* c, int R, const v2d* in, int in_rs, v2d* out, int out_rs, int rows,
              int Ns, const MixCorr& cp, double* pw, int acc) {
  const int N = c->cfg.n_samples;
  const dim3 grid((N / R + kMixThreads - 1) / kMixThreads, rows);
  const v2d* tw = (const v2d*)c->d_twN;
  switch (R) {
    // (kMxPowerHalf exists for even radices; mx_chunk asks for it only with one)
#define MIX_CASE(RR)                                                                           \
  case RR:                                                                                     \
    hipLaunchKernelGGL((mx_pass<RR, (MODE == kMxPowerHalf && RR % 2) ? kMxPowerKeep : MODE>),  \
                       grid, dim3(kMixThreads), 0, c->stream, in, in_rs, out, out_rs, N, Ns,   \
                       tw, cp, pw, acc);                                                       \
    break;
    MIX_RADICES(MIX_CASE)
#undef MIX_CASE
    default:
      gnsscorr_set_error("acq64 mixed radix: no kernel for radix %d", R);
      return GNSSCORR_EINVAL;
  }
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

// ---------------------------------------------------------------------------------
// Four-step plan (round 5): N = N1 N2 with N1 = A B and N2 = C D, each a pair of
// compiled radices.  X[k1 + N1 k2] = sum_n2 W_N2^(n2 k2) W_N^(n2 k1) sum_n1
// W_N1^(n1 k1) x[N2 n1 + n2].  m4_cols2 runs the N1-point DFTs of a tile of kM4T2
// columns n2 in LDS (A-point DFTs, twiddle W_N1^(q u), B-point DFTs: the standard
// two-factor split), multiplies by W_N^(n2 k1) and writes Y[k1 N2 + n2]; m4_rows
// (m4_rows2) runs the N2-point DFTs of kR2 rows k1 the same way and writes X[k1 + N1 k2].
// Two passes over the rows instead of the four of the mixed-radix plan at
// N = 38 192 = 112 x 341; the correlation product is formed in the first, |.|^2 /
// N^2 in the second (acquisition.sci:107-132), as in mx_pass.
// ---------------------------------------------------------------------------------
constexpr int kM4ColThreads = 128;   // m4_cols2 threads
constexpr int kM4T2 = 16;            // m4_cols2: columns n2 per workgroup
constexpr int kM4RowThreads = 64;    // m4_rows2 threads
// The intermediate rows Y[k1][n2] are stored at a pitch of N2 rounded up to whole
// m4_cols2 tiles (kM4T2 columns = 256 B): every tile writes whole, aligned 128-byte
// lines that no other workgroup touches (at the natural pitch N2 = 341 a tile's
// 256-byte runs straddled three lines shared with the neighbouring tiles, which run
// on other XCDs)
__host__ __device__ constexpr int m4_pitch(int n2) { return (n2 + kM4T2 - 1) / kM4T2 * kM4T2; }

// Per-column top-2 of a power row (kM4OutTop2 of m4_rows2): the column k1 holds the
// samples k1 + N1 k2, so N1 is the stride of top2_exact for a column's top-2
// (g_stats1_kernel's argument with columns for threads).
struct M4Top {
  double a1, a2;
  int ak, pad;
};

// one wave: the statistics of unit u0 + r from its per-column top-2 rows (the argmax
// over the columns, then the largest of the columns' candidates for `second`).  Same
// results as g_stats1_kernel on the power rows.
__device__ __forceinline__ void m4_stats_row(const M4Top* __restrict__ top, int r, int N1, int N,
                                             int u0, int n_blocks, int nc, int spc,
                                             gnsscorr_acq_row* __restrict__ stats) {
  const int lane = threadIdx.x % 64;
  const M4Top* t = top + (long)r * N1;
  const auto [rowid, blk0] = unit_row(u0 + r, n_blocks, nc);
  double bv = -1.0;
  int bk = INT_MAX;
  for (int c = lane; c < N1; c += 64)
    if (better(t[c].a1, t[c].ak, bv, bk)) { bv = t[c].a1; bk = t[c].ak; }
  wave_argmax(bv, bk);
  double sv = -1.0;
  for (int c = lane; c < N1; c += 64)
    sv = fmax(sv, Top2<double>{t[c].a1, t[c].a2, t[c].ak}.second(bk, spc, N));
  sv = wave_max(sv);
  if (lane == 0) store_row(stats, rowid, blk0, n_blocks, nc, bv, bk, sv);
}

__global__ __launch_bounds__(64) void m4_stats_kernel(const M4Top* __restrict__ top, int N1,
                                                      int N, int u0, int n_blocks, int nc,
                                                      int spc,
                                                      gnsscorr_acq_row* __restrict__ stats) {
  m4_stats_row(top, blockIdx.x, N1, N, u0, n_blocks, nc, spc, stats);
}

// A chunk's statistics pass carried by the next chunk's first m4_cols2 launch: extra
// rows of workgroups (one statistics row per wave) after the main grid.  Stream order
// puts them after the chunk's last m4_rows2 (which wrote top) and before the next
// chunk's (which overwrites it); it saves one launch and its tail per chunk.
struct M4StatsJob {
  const M4Top* top = nullptr;
  gnsscorr_acq_row* stats = nullptr;
  int n = 0, u0 = 0, N1 = 0, n_blocks = 1, nc = 0, spc = 0;
  int main_rows = 0;   // the launch's own rows (blockIdx.y below: the column pass)
};

// The column pass without its first and last LDS round trips (round 6): the A-point
// stage reads its inputs (or forms the correlation product) straight from global
// memory -- a lane's task is (q, t), 64 lanes cover 4 values of q x 16 consecutive
// columns, whole 256-byte runs -- and the B-point stage writes its outputs, times
// W_N^(n2 k1), straight to Y.  The LDS holds only the exchange between the stages, one
// fp64 plane at a time (real parts, then imaginary parts: 15.2 KB per tile, 126 VGPRs,
// 16 waves per CU; the complex exchange, 30.5 KB, held it to 10 and lost: DESIGN.md
// section 3).  The register allocator is held to those 4 waves per SIMD.
template <int A, int B, int MODE>
__global__ __launch_bounds__(kM4ColThreads) __attribute__((amdgpu_waves_per_eu(4)))
void m4_cols2(const v2d* __restrict__ in, int in_rs, v2d* __restrict__ out, int N,
              const v2d* __restrict__ tw, const v2d* __restrict__ tws, MixCorr cp,
              M4StatsJob sj) {
  constexpr int N1 = A * B;
  static_assert(kM4ColThreads % kM4T2 == 0, "m4_cols2: a lane keeps one column");
  if ((int)blockIdx.y >= sj.main_rows) {   // the previous chunk's statistics (whole workgroups)
    const int r = (((int)blockIdx.y - sj.main_rows) * (int)gridDim.x + (int)blockIdx.x) *
                      (kM4ColThreads / 64) + (int)threadIdx.x / 64;
    if (r < sj.n) m4_stats_row(sj.top, r, sj.N1, N, sj.u0, sj.n_blocks, sj.nc, sj.spc, sj.stats);
    return;
  }
  __shared__ double sp[N1][kM4T2 + 1];   // one fp64 plane: real parts, then imaginary
  const int N2 = N / N1;
  const int n2_0 = blockIdx.x * kM4T2;
  const long row = blockIdx.y;
  const int t = threadIdx.x % kM4T2, n2 = n2_0 + t;
  const bool col = n2 < N2;
  const v2d *Xr = nullptr, *Fr = nullptr;
  int shift = 0;
  if constexpr (MODE == kM4InCorr) mix_unit_rows(cp, cp.u0 + (int)row, Xr, Fr, shift);
  // ---- stage A: task (q, t), q = (task / kM4T2) < B: the A-point DFT over p of
  // x[B p + q], times W_N1^(q u), into LDS slot B u + q
  constexpr int kLanesQ = kM4ColThreads / kM4T2;   // values of q per pass
  constexpr int kItA = (B + kLanesQ - 1) / kLanesQ;
  double ai[kItA][A];
#pragma unroll
  for (int it = 0; it < kItA; it++) {
    const int q = threadIdx.x / kM4T2 + kLanesQ * it;
    if (q >= B) continue;
    v2d v[A];
#pragma unroll
    for (int p = 0; p < A; p++) {
      const int n = N2 * (B * p + q) + n2;
      if constexpr (MODE == kM4InCorr) {
        int sx = n - shift;
        sx += sx < 0 ? N : 0;
        const v2d xv = col ? Xr[sx] : (v2d){0.0, 0.0}, f = col ? Fr[n] : (v2d){0.0, 0.0};
        v[p] = (v2d){fma(xv.x, f.x, xv.y * f.y), fma(xv.x, f.y, -(xv.y * f.x))};   // conj(X) F
      } else {
        v[p] = col ? in[row * in_rs + n] : (v2d){0.0, 0.0};
      }
    }
    dft<A>(v);
#pragma unroll
    for (int u = 1; u < A; u++) v[u] = cmul(v[u], tws[q * u]);   // W_N1^(q u), q u < N1
#pragma unroll
    for (int u = 0; u < A; u++) {
      sp[B * u + q][t] = v[u].x;
      ai[it][u] = v[u].y;
    }
  }
  __syncthreads();
  // ---- stage B: task (u, t), u = threadIdx.x / kM4T2 < A: the B-point DFT over q;
  // output w is k1 = u + A w, times W_N^(n2 k1) = W_N^(n2 u) (W_N^(A n2))^w
  constexpr int kItB = (A + kLanesQ - 1) / kLanesQ;
  static_assert(kItB == 1, "m4_cols2: one B-point pass (the plane exchange)");
  v2d vb[B];
  {
    const int u = threadIdx.x / kM4T2;
#pragma unroll
    for (int q = 0; q < B; q++) vb[q].x = u < A ? sp[B * u + q][t] : 0.0;
  }
  __syncthreads();   // the imaginary parts overwrite the plane
#pragma unroll
  for (int it = 0; it < kItA; it++) {
    const int q = threadIdx.x / kM4T2 + kLanesQ * it;
    if (q < B) {
#pragma unroll
      for (int u = 0; u < A; u++) sp[B * u + q][t] = ai[it][u];
    }
  }
  __syncthreads();
  {
    const int u = threadIdx.x / kM4T2;
#pragma unroll
    for (int q = 0; q < B; q++) vb[q].y = u < A ? sp[B * u + q][t] : 0.0;
  }
#pragma unroll
  for (int it = 0; it < kItB; it++) {
    const int u = threadIdx.x / kM4T2 + kLanesQ * it;
    if (u >= A) continue;
    v2d (&v)[B] = vb;
    dft<B>(v);
    if (col) {
      v2d wc = tw[n2 * u], ws = tw[A * n2];   // n2 u < N, A n2 < N
      const long base = row * (long)N1 * m4_pitch(N2) + n2;
#pragma unroll
      for (int w = 0; w < B; w++) {
        out[base + (long)(u + A * w) * m4_pitch(N2)] = cmul(v[w], wc);
        wc = cmul(wc, ws);
      }
    }
  }
}

// m4_rows2 kM4OutRows: complex rows out (stride out_rs); kM4OutPower: |.|^2 / N^2 into pw
// (added to the running sums when ACC); kM4OutTop2: as kM4OutPower on a row's last block,
// per-column top-2 into top (the power row is not stored)
// The rows pass (round 6; the round-5 m4_rows kept complex rows in LDS, 21.9 KB per
// 4-row tile, 7 waves per CU): the C-point stage reads its inputs straight from Y
// (lanes cover 4 rows x 16 consecutive n2: whole lines), the exchange to the D-point
// stage goes through ONE fp64 plane at a time (real parts, then imaginary parts:
// 4 x (N2 + 1) doubles, 10.9 KB), and the prime D-point stage emits its outputs as
// they are formed (power, statistics or complex rows go out from registers, no LDS
// round trip).  164 VGPRs: 12 waves per CU.  The arithmetic is m4_rows' except the
// stage-A twiddles (a recurrence, <= C roundings of drift).  38.192 Msps search
// 1.14-1.15 -> 1.09-1.11 ms (profiles/r6/acq_generic_rows2_ab_r7b.log).
// Rows k1 per m4_rows2 workgroup (2: 150 VGPRs, 12 waves per CU, but 22 of 64 lanes in
// the 31-point stage: 1.21 against 1.10 ms; 5: 0.995-1.006 against 0.948-0.957 ms,
// DESIGN.md section 3)
constexpr int kR2 = 4;
// 3 waves per SIMD (164 VGPRs; 2: 1.09-1.11 against 1.05-1.07 ms)
template <int C, int D, int MODE, bool ACC>
__global__ __launch_bounds__(kM4RowThreads) __attribute__((amdgpu_waves_per_eu(3)))
void m4_rows2(const v2d* __restrict__ Y, v2d* __restrict__ out, int out_rs, int N,
              const v2d* __restrict__ tws, double* __restrict__ pw, int acc,
              M4Top* __restrict__ top) {
  constexpr int N2 = C * D, P2 = m4_pitch(C * D);
  static_assert(is_prime(D), "m4_rows2: the second stage emits a prime DFT's outputs");
  static_assert(kM4RowThreads == 64 && D * kR2 <= 3 * 64 && C * kR2 <= 64,
                "m4_rows2: up to three stage-A passes, one stage-B pass per wave");
  // plane pitch (doubles): LP = 8 mod 32, so the 32 lanes of a half-wave (4 rows x 8
  // consecutive q, or 4 rows x 8 values of u) fall on 32 distinct bank pairs (at
  // N2 + 1 = 342 the rows overlapped: 44 % of the LDS cycles were bank conflicts)
  constexpr int LP = N2 + 1 + ((8 - (N2 + 1)) % 32 + 32) % 32;
  static_assert(LP % 32 == 8 && LP > N2, "m4_rows2: plane pitch");
  __shared__ double sp[kR2][LP];
  const int N1 = N / N2;
  const int k1_0 = blockIdx.x * kR2;
  const long row = blockIdx.y;
  const int t = threadIdx.x;
  const v2d* Yt = Y + row * (long)N1 * P2 + (long)k1_0 * P2;
  // ---- stage A: task (q, r) = (task / kR2, task % kR2), the C-point DFT over p of
  // Y[k1_0 + r][D p + q], then W_N2^(q u).  One pass after the other, each pass's real
  // parts into the plane as soon as they exist: only the imaginary parts stay live
  // (the other waves of the CU hide the load latency)
  constexpr int kTA = D * kR2, kItA = (kTA + 63) / 64;
  // the passes as a loop that is NOT unrolled: unrolled, the scheduler overlapped
  // them (232 VGPRs, 2 waves per SIMD); as a loop, 164 VGPRs: 3 waves per SIMD
  double ai[kItA][C];
#pragma unroll 1
  for (int it = 0; it < kItA; it++) {
    const int task = t + 64 * it, q = task / kR2, r = task % kR2;
    const bool ok = task < kTA && k1_0 + r < N1;
    v2d v[C];
#pragma unroll
    for (int p = 0; p < C; p++) v[p] = ok ? Yt[(long)r * P2 + D * p + q] : (v2d){0.0, 0.0};
    dft<C>(v);
    // W_N2^(q u) = (W_N2^q)^u by recurrence: one table load per task instead of C - 1
    // (all hoisted, they doubled the pass's live registers); <= C roundings of drift
    const v2d w1 = tws[q < D ? q : 0];
    v2d wu = w1;
#pragma unroll
    for (int u = 1; u < C; u++) {
      v[u] = cmul(v[u], wu);
      wu = cmul(wu, w1);
    }
#pragma unroll
    for (int u = 0; u < C; u++) {
      if (task < kTA) sp[r][D * u + q] = v[u].x;
      if (it == 0) ai[0][u] = v[u].y;   // (constant register indices: uniform branches)
      else if (kItA < 3 || it == 1) ai[kItA > 1 ? 1 : 0][u] = v[u].y;
      else ai[kItA - 1][u] = v[u].y;
    }
    // the next pass's loads and arithmetic stay behind this one (interleaving the two
    // passes, the scheduler held both passes' working sets)
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  }
  // ---- exchange, one plane at a time; stage B: task (u, r) = (t / kR2, t % kR2)
  const int ub = t / kR2, rb = t % kR2;
  const bool actB = ub < C && k1_0 + rb < N1;
  // the exchange reads are not predicated: an inactive lane reads a valid slot (ub
  // clamped) and runs the D-point DFT on it, but emits nothing
  const int ubc = min(ub, C - 1);
  v2d x[D];
  __syncthreads();
#pragma unroll
  for (int w = 0; w < D; w++) x[w].x = sp[rb][D * ubc + w];
  __syncthreads();   // the imaginary parts overwrite the plane
#pragma unroll
  for (int it = 0; it < kItA; it++) {
    const int task = t + 64 * it, q = task / kR2, r = task % kR2;
    if (task < kTA) {
#pragma unroll
      for (int u = 0; u < C; u++) sp[r][D * u + q] = ai[it][u];
    }
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < D; w++) x[w].y = sp[rb][D * ubc + w];
  __builtin_amdgcn_sched_barrier(0);
  // ---- stage B: the D-point DFT; output w is element k2 = ub + C w of column k1
  const int k1 = k1_0 + rb;
  const double sc = 1.0 / ((double)N * (double)N);
  Top2<double> col;
  auto emit = [&](int w, v2d v) {
    if (!actB) return;
    const int d = k1 + N1 * (ub + C * w);   // < N
    if constexpr (MODE == kM4OutPower || MODE == kM4OutTop2) {
      const double q = fma(v.x, v.x, v.y * v.y) * sc;
      double* o = pw + row * N + d;
      const double val = ACC ? *o + q : q;   // (ACC: the running sums of earlier blocks)
      if constexpr (MODE == kM4OutPower) *o = val;
      else col.push(val, d);                 // (the row's power is not stored)
    } else {
      out[row * out_rs + d] = v;
    }
  };
  dft_prime_emit<D, true>(x, emit);
  if constexpr (MODE == kM4OutTop2) {
    // the column's C tasks sit in the lanes rb + kR2 u: a tree over u (step s merges
    // the disjoint lane ranges [u, u + s) and [u + s, u + 2 s) within the column)
#pragma unroll
    for (int st = 1; st < C; st <<= 1) {
      const Top2<double> o{__shfl_down(col.a1, kR2 * st, 64), __shfl_down(col.a2, kR2 * st, 64),
                           __shfl_down(col.ak, kR2 * st, 64)};
      if (ub + st < C) col.merge(o);
    }
    if (t < kR2 && k1_0 + t < N1) top[row * N1 + k1_0 + t] = M4Top{col.a1, col.a2, col.ak, 0};
  }
}

// the compiled four-step plans: {A, B, C, D}
constexpr int kM4Plans[][4] = {{0, 0, 0, 0}, {7, 16, 11, 31}, {3, 16, 11, 31}};

int m4_plan(int N) {
  for (int i = 1; i < (int)(sizeof kM4Plans / sizeof kM4Plans[0]); i++)
    if (N == kM4Plans[i][0] * kM4Plans[i][1] * kM4Plans[i][2] * kM4Plans[i][3]) return i;
  return 0;
}

// Chunk lane i of the four-step plan.  Lane 0 is the context's stream with the work and
// power rows that the Bluestein and mixed-radix passes share; lane 1 has its own.
acq_chunk_lane chunk_lane(const gnsscorr_acq_ctx* c, int i) {
  if (i) return c->gen.m4.lane1;
  return {c->stream, c->gen.d_A, c->gen.d_pw, c->gen.m4.d_top};
}

// rows [src] -> DFT rows or the correlation's power rows, one chunk of `rows` on lane ln
template <int MODE_IN, int MODE_OUT>
int m4_launch(gnsscorr_acq_ctx* c, const acq_chunk_lane& ln, const v2d* in, int in_rs, v2d* out,
              int out_rs, int rows, const MixCorr& cp, double* pw, int acc,
              const M4StatsJob* stats_job = nullptr, hipEvent_t after_cols = nullptr) {
  const int N = c->cfg.n_samples;
  M4StatsJob sj = stats_job ? *stats_job : M4StatsJob{};
  sj.main_rows = rows;
  const int* const pl = kM4Plans[c->gen.m4.plan];
  const int per_y = (N / (pl[0] * pl[1]) + kM4T2 - 1) / kM4T2 *
                    (kM4ColThreads / 64);   // statistics rows per extra grid row
  const int ey = sj.n > 0 ? (sj.n + per_y - 1) / per_y : 0;
  const v2d* tw = (const v2d*)c->d_twN;
  const v2d* tws1 = (const v2d*)c->gen.m4.d_tw;   // W_N1^j, then W_N2^j from + N1
  v2d* Y = (v2d*)ln.Y;
  M4Top* top = (M4Top*)ln.top;
  hipStream_t st = ln.stream;
  switch (c->gen.m4.plan) {
#define M4_CASE(I, A, B, C, D)                                                                 \
  case I:                                                                                      \
    hipLaunchKernelGGL((m4_cols2<A, B, MODE_IN>),                                              \
                       dim3((N / (A * B) + kM4T2 - 1) / kM4T2, rows + ey), dim3(kM4ColThreads), \
                       0, st, in, in_rs, Y, N, tw, tws1, cp, sj);                              \
    if (after_cols) HIP_TRY(hipEventRecord(after_cols, st));                                   \
    hipLaunchKernelGGL((acc ? m4_rows2<C, D, MODE_OUT, true> : m4_rows2<C, D, MODE_OUT, false>), \
                       dim3((A * B + kR2 - 1) / kR2, rows), dim3(kM4RowThreads), 0, st, Y, out, \
                       out_rs, N, tws1 + A * B, pw, acc, top);                                 \
    break;
    M4_CASE(1, 7, 16, 11, 31)
    M4_CASE(2, 3, 16, 11, 31)
#undef M4_CASE
    default:
      gnsscorr_set_error("acq64 four-step: no plan %d", c->gen.m4.plan);
      return GNSSCORR_EINVAL;
  }
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

// ---- host side: switches, chunk size ----------------------------------------------------
// The engine's switches, read once per context (acq64_gen_init), all for cross-checks and
// A/Bs: GNSSCORR_ACQ_BLUESTEIN=1 the chirp-z engine for every N, _MIX4=0
// no four-step plan, _M4LANES=1 one chunk lane, _M4STATS=0 the four-step plan keeps the
// separate statistics pass, _GCHUNK_MB MiB per work buffer (0: the engine's default)
struct GenEnv {
  bool bluestein, mix4, two_lanes, m4stats;
  long chunk_mb;
};
GenEnv gen_env() {
  const char *fb = getenv("GNSSCORR_ACQ_BLUESTEIN"), *f4 = getenv("GNSSCORR_ACQ_MIX4"),
             *gl = getenv("GNSSCORR_ACQ_M4LANES"), *fs = getenv("GNSSCORR_ACQ_M4STATS"),
             *gm = getenv("GNSSCORR_ACQ_GCHUNK_MB");
  return {fb && atoi(fb), !(f4 && f4[0] == '0'), !(gl && gl[0] == '1'), !(fs && fs[0] == '0'),
          gm && atol(gm) > 0 ? atol(gm) : 0L};
}

// rows per chunk of the generic engine: at most what one call of this context
// can run in one go (codes x frequencies x blocks covers the code spectra, the IF
// class spectra and a search's units), so small contexts keep small work buffers
// (ADVICE r5); 1 .. 4096
int chunk_cap(const gnsscorr_acq_ctx* c, int rows) {
  const long most = (long)c->cfg.max_codes * c->cfg.max_freqs * c->cfg.max_blocks;
  if (rows > most) rows = (int)(most < 4096 ? most : 4096);
  if (rows > 4096) rows = 4096;
  return rows < 1 ? 1 : rows;
}

// Rows per chunk of every engine: what `mib` MiB (the engine's default, or
// GNSSCORR_ACQ_GCHUNK_MB) hold of work rows of row_bytes each, within chunk_cap
int chunk_rows(const gnsscorr_acq_ctx* c, const GenEnv& env, long mib, long row_bytes) {
  if (env.chunk_mb) mib = env.chunk_mb;
  return chunk_cap(c, (int)((mib << 20) / row_bytes));
}

// ---- host side: Bluestein -----------------------------------------------------------------
// FFT_M of `rows` rows in place in A (B is the ping-pong buffer); result in *res
int bz_fft(gnsscorr_acq_ctx* c, v2d* A, v2d* B, int rows, v2d** res) {
  const int M = c->gen.bz.M;
  v2d *in = A, *out = B;
  int Ns = 1;
  while (Ns < M) {
    const int R = M / Ns >= 16 ? 16 : M / Ns;   // radix-16 passes, then one of 2, 4 or 8
    const dim3 grid((M / R + kGThreads - 1) / kGThreads, rows);
    const v2d* tw = (const v2d*)c->gen.bz.d_twM;
    auto* const pass = R == 16 ? g_fft_pass<16> : R == 8 ? g_fft_pass<8>
                       : R == 4 ? g_fft_pass<4> : g_fft_pass<2>;
    hipLaunchKernelGGL(pass, grid, dim3(kGThreads), 0, c->stream, in, out, M, Ns, tw);
    HIP_TRY(hipGetLastError());
    Ns *= R;
    v2d* t = in;
    in = out;
    out = t;
  }
  *res = in;
  return GNSSCORR_OK;
}

// The chirp-z convolution of the `rows` rows prepared in d_A (a pre kernel's output):
// FFT_M, times vf, FFT_M; the result rows are *D, one of the two work buffers
int bz_convolve(gnsscorr_acq_ctx* c, int rows, v2d** D) {
  const int M = c->gen.bz.M;
  v2d *A = (v2d*)c->gen.d_A, *B = (v2d*)c->gen.d_B;
  int rc = bz_fft(c, A, B, rows, D);
  if (rc) return rc;
  v2d* E = *D == A ? B : A;
  hipLaunchKernelGGL(g_mulv_kernel, dim3((M + kGThreads - 1) / kGThreads, rows), dim3(kGThreads),
                     0, c->stream, *D, (const v2d*)c->gen.bz.d_vf, M, E);
  HIP_TRY(hipGetLastError());
  return bz_fft(c, E, *D, rows, D);
}

// one chunk of gen_dft_rows: DFT_N of nr natural rows a (stride src_rs) -> out (stride rs)
int bz_dft_chunk(gnsscorr_acq_ctx* c, const v2d* a, int src_rs, int nr, v2d* out, int rs) {
  const int N = c->cfg.n_samples, M = c->gen.bz.M;
  const v2d* chirp = (const v2d*)c->gen.bz.d_chirp;
  hipLaunchKernelGGL(g_pre_kernel, dim3((M + kGThreads - 1) / kGThreads, nr), dim3(kGThreads), 0,
                     c->stream, a, src_rs, chirp, N, M, (v2d*)c->gen.d_A);
  HIP_TRY(hipGetLastError());
  v2d* D;
  const int rc = bz_convolve(c, nr, &D);
  if (rc) return rc;
  hipLaunchKernelGGL(g_post_kernel, dim3((N + kGThreads - 1) / kGThreads, nr), dim3(kGThreads), 0,
                     c->stream, D, chirp, N, M, out, rs);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

int bz_init(gnsscorr_acq_ctx* c, const GenEnv& env) {
  const long N = c->cfg.n_samples;
  int M = 16;
  while (M < 2 * N - 1) M *= 2;
  c->gen.bz.M = M;
  c->gen.chunk = chunk_rows(c, env, 64, (long)M * 16);   // ~64 MiB per work buffer
  HIP_TRY(hipMalloc(&c->gen.bz.d_chirp, sizeof(double2) * N));
  HIP_TRY(hipMalloc(&c->gen.bz.d_vf, sizeof(double2) * M));
  HIP_TRY(hipMalloc(&c->gen.bz.d_twM, sizeof(double2) * M));
  HIP_TRY(hipMalloc(&c->gen.d_A, sizeof(double2) * (size_t)M * c->gen.chunk));
  HIP_TRY(hipMalloc(&c->gen.d_B, sizeof(double2) * (size_t)M * c->gen.chunk));
  HIP_TRY(hipMalloc(&c->gen.d_pw, sizeof(double) * (size_t)N * c->gen.chunk));
  double2* h = (double2*)malloc(sizeof(double2) * M);
  if (!h) return GNSSCORR_ENOMEM;
  // exp(i pi_ n^2 / N), pi_ = -+pi: exact argument reduction n^2 mod 2N
  auto chirp = [N](long n, double pi_) {
    const double a = pi_ * ((double)((n * n) % (2 * N)) / (double)N);
    return make_double2(cos(a), sin(a));
  };
  for (long n = 0; n < N; n++) h[n] = chirp(n, -M_PI);
  hipError_t e = hipMemcpy(c->gen.bz.d_chirp, h, sizeof(double2) * N, hipMemcpyHostToDevice);
  // W_M^t with the angle reduced to the first octant by symmetry
  for (long t = 0; e == hipSuccess && t < M; t++) {
    const double a = -2.0 * M_PI * ((double)t / (double)M);
    h[t] = make_double2(cos(a), sin(a));
  }
  if (e == hipSuccess) e = hipMemcpy(c->gen.bz.d_twM, h, sizeof(double2) * M, hipMemcpyHostToDevice);
  // two-sided conjugate chirp v_m = conj(c_|m|), wrapped to M
  for (long m = 0; m < M; m++) h[m] = make_double2(0.0, 0.0);
  for (long m = 0; m < N; m++) {
    h[m] = chirp(m, M_PI);
    if (m > 0) h[M - m] = h[m];
  }
  if (e == hipSuccess) e = hipMemcpy(c->gen.d_A, h, sizeof(double2) * M, hipMemcpyHostToDevice);
  free(h);
  HIP_TRY(e);
  v2d* D;
  int rc = bz_fft(c, (v2d*)c->gen.d_A, (v2d*)c->gen.d_B, 1, &D);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->gen.bz.d_vf, D, sizeof(double2) * M, hipMemcpyDeviceToDevice,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return GNSSCORR_OK;
}

// ---- host side: mixed-radix passes and four-step plan ---------------------------------------
// one chunk of gen_dft_rows by the mixed-radix passes
int mx_dft_chunk(gnsscorr_acq_ctx* c, const v2d* src, int srs, int nr, v2d* out, int rs,
                 int n_in) {
  const int N = c->cfg.n_samples, P = c->gen.mix.nr;
  const MixCorr none{};
  v2d *A = (v2d*)c->gen.d_A, *B = (v2d*)c->gen.d_B;
  int Ns = 1;
  for (int i = 0; i < P; i++) {
    const bool last = i + 1 == P, tail = i == 0 && n_in < N;
    v2d* dst = last ? out : (i % 2 == 0 ? A : B);
    auto* const launch = tail ? mx_launch<kMxRowsZeroTail> : mx_launch<kMxRows>;
    const int rc = launch(c, c->gen.mix.r[i], src, srs, dst, last ? rs : N, nr, Ns, none, nullptr,
                          tail ? n_in : 0);
    if (rc) return rc;
    src = dst;
    srs = N;
    Ns *= c->gen.mix.r[i];
  }
  return GNSSCORR_OK;
}

int mx_init(gnsscorr_acq_ctx* c, const GenEnv& env) {
  const long N = c->cfg.n_samples;
  const int m4 = c->gen.m4.plan;
  const long N1 = m4 ? kM4Plans[m4][0] * kM4Plans[m4][1] : 0;
  // (the four-step plan's Y rows at the m4_pitch, a few % above N)
  const long ya = m4 ? N1 * m4_pitch((int)(N / N1)) : N;
  // Rows per chunk from the work buffer's size (DESIGN.md section 3 has the sweeps).  Large
  // chunks keep each pass at ~10 k workgroups (profiles/r5/acq_generic_chunk_ab_r5ao.log).
  // The four-step plan's Y is written by m4_cols2 and read back at once by m4_rows2: at
  // <= 232 MiB (385 rows at N = 38 192) it stays in the 256 MB memory-side cache between
  // the two passes (profiles/r6/acq_generic_chunk_sweep_r7h.log).  Two chunk lanes split
  // that budget, 116 MiB of Y each, so both lanes' Y stay in the cache together and one
  // chunk's column pass (memory-bound) overlaps the other's row pass (fp64-issue-bound):
  // 3 % on one search (profiles/r6/acq_generic_lanes_ab_r8f.log; other sizes per lane
  // slower); the search's set-up and selection still run alone before the fork and after
  // the join.
  c->gen.m4.lanes = m4 && env.two_lanes ? 2 : 1;
  c->gen.chunk = chunk_rows(c, env, m4 ? 232 / c->gen.m4.lanes : 256, ya * 16);
  HIP_TRY(hipMalloc(&c->d_twN, sizeof(double2) * N));
  HIP_TRY(hipMalloc(&c->gen.d_A, sizeof(double2) * (size_t)ya * c->gen.chunk));
  if (!m4)   // the four-step plan's passes need one work buffer (Y), the Stockham passes two
    HIP_TRY(hipMalloc(&c->gen.d_B, sizeof(double2) * (size_t)N * c->gen.chunk));
  HIP_TRY(hipMalloc(&c->gen.d_pw, sizeof(double) * (size_t)N * c->gen.chunk));
  const size_t top_bytes = sizeof(M4Top) * (size_t)N1 * c->gen.chunk;
  if (m4 && env.m4stats) HIP_TRY(hipMalloc(&c->gen.m4.d_top, top_bytes));
  if (c->gen.m4.lanes == 2) {
    acq_chunk_lane& l1 = c->gen.m4.lane1;
    HIP_TRY(hipMalloc(&l1.Y, sizeof(double2) * (size_t)ya * c->gen.chunk));
    HIP_TRY(hipMalloc(&l1.pw, sizeof(double) * (size_t)N * c->gen.chunk));
    if (c->gen.m4.d_top) HIP_TRY(hipMalloc(&l1.top, top_bytes));
    HIP_TRY(hipStreamCreateWithFlags(&l1.stream, hipStreamNonBlocking));
    for (hipEvent_t& ev : c->gen.m4.ev)
      HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  }
  double2* h = (double2*)malloc(sizeof(double2) * N);
  if (!h) return GNSSCORR_ENOMEM;
  for (long t = 0; t < N; t++) {   // W_N^t = exp(-2 pi i t / N)
    const double a = -2.0 * M_PI * ((double)t / (double)N);
    h[t] = make_double2(cos(a), sin(a));
  }
  hipError_t e = hipMemcpy(c->d_twN, h, sizeof(double2) * N, hipMemcpyHostToDevice);
  if (e == hipSuccess && m4) {
    // the passes' inner twiddles as compact tables (the same values as d_twN's)
    const long N2 = N / N1;
    double2* ht = (double2*)malloc(sizeof(double2) * (N1 + N2));
    if (!ht) { free(h); return GNSSCORR_ENOMEM; }
    for (long j = 0; j < N1; j++) ht[j] = h[j * N2];        // W_N1^j = W_N^(j N2)
    for (long j = 0; j < N2; j++) ht[N1 + j] = h[j * N1];   // W_N2^j = W_N^(j N1)
    e = hipMalloc(&c->gen.m4.d_tw, sizeof(double2) * (N1 + N2));
    if (e == hipSuccess)
      e = hipMemcpy(c->gen.m4.d_tw, ht, sizeof(double2) * (N1 + N2), hipMemcpyHostToDevice);
    free(ht);
  }
  free(h);
  HIP_TRY(e);
  return GNSSCORR_OK;
}

// DFT_N of `rows` natural rows a (stride src_rs) -> out (stride rs), a chunk at a time by
// the context's engine.  n_in: the rows are zero from that element on (n_in = N: nothing
// known; the mixed-radix first pass skips those loads)
int gen_dft_rows(gnsscorr_acq_ctx* c, const v2d* a, int src_rs, int rows, v2d* out, int rs,
                 int n_in) {
  const acq64_gen_ctx& g = c->gen;
  for (int r0 = 0; r0 < rows; r0 += g.chunk) {
    const int nr = rows - r0 < g.chunk ? rows - r0 : g.chunk;
    const v2d* src = a + (long)r0 * src_rs;
    v2d* dst = out + (long)r0 * rs;
    const int rc = g.m4.plan ? m4_launch<kM4InRows, kM4OutRows>(c, chunk_lane(c, 0), src, src_rs,
                                                                dst, rs, nr, MixCorr{}, nullptr, 0)
                   : g.mix.nr ? mx_dft_chunk(c, src, src_rs, nr, dst, rs, n_in)
                              : bz_dft_chunk(c, src, src_rs, nr, dst, rs);
    if (rc) return rc;
  }
  return GNSSCORR_OK;
}

// ---- the search: one chunk's block per engine ------------------------------------------------
// Units cp.u0 .. cp.u0 + nu - 1 (block cp.nc_blk of each in a non-coherent search, else the
// unit's own) -> their power rows, stored for b == 0 and added to for b > 0.

// chirp-z: the correlation product times the chirp, the convolution, the powers of the NK
// lags searched
int bz_chunk(gnsscorr_acq_ctx* c, const MixCorr& cp, int nu, int b, int NK) {
  const int N = c->cfg.n_samples, M = c->gen.bz.M;
  hipLaunchKernelGGL(g_corr_pre_kernel, dim3((M + kGThreads - 1) / kGThreads, nu),
                     dim3(kGThreads), 0, c->stream, cp.X, cp.F, cp.rs, cp.n_blocks, cp.nc_blk,
                     cp.group_code, cp.group_freq, cp.n_bins, cp.fmap, cp.u0,
                     (const v2d*)c->gen.bz.d_chirp, N, M, (v2d*)c->gen.d_A);
  HIP_TRY(hipGetLastError());
  v2d* D;
  const int rc = bz_convolve(c, nu, &D);
  if (rc) return rc;
  hipLaunchKernelGGL(g_power_kernel, dim3((NK + kGThreads - 1) / kGThreads, nu), dim3(kGThreads),
                     0, c->stream, D, N, M, b > 0, c->gen.d_pw, NK);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

// the mixed-radix passes: the product in the first, the powers in the last.  A zero-padded
// search (cp.keep) runs them in the padded order, the last one pruned to the kept lags
int mx_chunk(gnsscorr_acq_ctx* c, const MixCorr& cp, int nu, int b) {
  const int N = c->cfg.n_samples, P = c->gen.mix.nr, keep = cp.keep;
  const int* const radix = keep ? c->gen.mix.rp : c->gen.mix.r;
  const bool half = keep && 2 * keep == N && radix[P - 1] % 2 == 0;
  v2d *A = (v2d*)c->gen.d_A, *B = (v2d*)c->gen.d_B;
  const v2d* src = nullptr;
  int Ns = 1;
  for (int i = 0; i < P; i++) {
    v2d* dst = i % 2 == 0 ? A : B;
    const bool last = i + 1 == P;   // the last pass writes power rows, the others work rows
    auto* const launch = i == 0 ? mx_launch<kMxCorrIn> : !last ? mx_launch<kMxRows>
                         : !keep ? mx_launch<kMxPower>
                         : half  ? mx_launch<kMxPowerHalf> : mx_launch<kMxPowerKeep>;
    const int rc = launch(c, radix[i], src, i ? N : 0, last ? nullptr : dst, last ? 0 : N, nu, Ns,
                          cp, last ? c->gen.d_pw : nullptr, last && b > 0);
    if (rc) return rc;
    src = dst;
    Ns *= radix[i];
  }
  return GNSSCORR_OK;
}

// the four-step plan on lane ln: the product in the column pass, the powers in the rows
// pass; top2: the per-column top-2 instead (the row statistics ride on a row's last block).
// sj: the lane's previous chunk's statistics, carried by the column pass
int m4_chunk(gnsscorr_acq_ctx* c, const acq_chunk_lane& ln, const MixCorr& cp, int nu, int b,
             bool top2, const M4StatsJob* sj, hipEvent_t fork) {
  auto* const launch = top2 ? m4_launch<kM4InCorr, kM4OutTop2> : m4_launch<kM4InCorr, kM4OutPower>;
  return launch(c, ln, nullptr, 0, nullptr, 0, nu, cp, ln.pw, b > 0, sj, fork);
}

}  // namespace

// ---- entry points (acq_ctx.h) --------------------------------------------------------------
int acq64_gen_init(gnsscorr_acq_ctx* c) {
  const GenEnv env = gen_env();
  const int N = c->cfg.n_samples;
  // the mixed-radix plan unless N has a prime factor above 31 (or the chirp-z engine is
  // asked for), as the four-step plan where one is compiled for N
  c->gen.mix.nr = env.bluestein ? 0 : mix_factor(N, c->gen.mix.r);
  mix_order_padded(c->gen.mix.r, c->gen.mix.nr, c->gen.mix.rp);
  c->gen.m4.plan = c->gen.mix.nr && env.mix4 ? m4_plan(N) : 0;
  return c->gen.mix.nr ? mx_init(c, env) : bz_init(c, env);
}

void acq64_gen_free(gnsscorr_acq_ctx* c) {
  acq64_gen_ctx& g = c->gen;
  hostctx::release(g.bz.d_chirp, g.bz.d_vf, g.bz.d_twM, g.d_A, g.d_B, g.d_pw, g.m4.d_top,
                   g.m4.d_tw, g.m4.lane1.Y, g.m4.lane1.pw, g.m4.lane1.top);
  for (hipEvent_t& ev : g.m4.ev)
    if (ev) {
      (void)hipEventDestroy(ev);
      ev = nullptr;
    }
  if (g.m4.lane1.stream) (void)hipStreamDestroy(g.m4.lane1.stream);
  g.m4.lane1.stream = nullptr;
}

// this file's code object loaded on the device (acq64_preload)
int acq64_gen_preload(gnsscorr_acq_ctx*) {
  hipFuncAttributes a;
  HIP_TRY(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&g_codes_kernel)));
  return GNSSCORR_OK;
}

// d_codes: n_codes replicas of N int8 values, zero from code_len on (set_codes_padded)
int acq64_gen_set_codes(gnsscorr_acq_ctx* c, const int8_t* d_codes, int n_codes, int code_len) {
  const long n = (long)n_codes * c->cfg.n_samples;
  hipLaunchKernelGGL(g_codes_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, d_codes, n,
                     (v2d*)c->d_in64.p);
  HIP_TRY(hipGetLastError());
  return gen_dft_rows(c, (const v2d*)c->d_in64.p, c->cfg.n_samples, n_codes, (v2d*)c->d_F64,
                      c->rs64, code_len);
}

// A zero-padded search runs the plain mixed-radix passes; a context on a four-step plan
// has one work buffer (Y) and gets the passes' second one here, once.
int acq64_gen_set_zero_padded(gnsscorr_acq_ctx* c, int keep) {
  if (keep > 0 && c->gen.m4.plan && !c->gen.d_B)
    HIP_TRY(hipMalloc(&c->gen.d_B, sizeof(double2) * (size_t)c->cfg.n_samples * c->gen.chunk));
  return GNSSCORR_OK;
}

int acq64_gen_spectra(gnsscorr_acq_ctx* c, const int8_t* d_if, int iq, int n_blocks, int n_freqs,
                      const double* d_freqs) {
  const int N = c->cfg.n_samples;
  int rc = acq64_classify_launch(c, d_freqs, n_freqs);
  if (rc) return rc;
  const int rows = n_freqs * n_blocks;   // upper bound: classes <= frequencies
  const long work = (long)rows * N;
  const int grid = (int)((work + 255) / 256 < 2048 ? (work + 255) / 256 : 2048);
  if (iq & GNSSCORR_IF_INT16)
    hipLaunchKernelGGL(g_wipe_kernel<true>, dim3(grid), dim3(256), 0, c->stream, d_if, iq,
                       n_blocks, c->coh, c->bstride ? (long)c->bstride : (long)c->coh * N,
                       (const double*)c->d_cfreq, (const int*)c->d_nclass,
                       1.0 / c->cfg.samp_rate, N, (v2d*)c->d_in64.p);
  else
  hipLaunchKernelGGL(g_wipe_kernel<false>, dim3(grid), dim3(256), 0, c->stream, d_if, iq, n_blocks,
                     c->coh, c->bstride ? (long)c->bstride : (long)c->coh * N,
                     (const double*)c->d_cfreq, (const int*)c->d_nclass,
                     1.0 / c->cfg.samp_rate, N, (v2d*)c->d_in64.p);
  HIP_TRY(hipGetLastError());
  // transform only the class rows (the count is on the device: one small read
  // back; this generic path is synchronous here anyway)
  int n_cls = 0;
  HIP_TRY(hipMemcpyAsync(&n_cls, c->d_nclass, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return gen_dft_rows(c, (const v2d*)c->d_in64.p, N, n_cls * n_blocks, (v2d*)c->d_X64.p, c->rs64,
                      N);
}

// The search driver of all three engines: the units in equal chunks, every chunk's blocks
// by the engine's body (m4_chunk, mx_chunk or bz_chunk), then its row statistics.
int acq64_gen_correlate(gnsscorr_acq_ctx* c, int n_blocks, int mode, int n_groups, int n_bins,
                        const int32_t* d_gcode, const int32_t* d_gfreq, int spc, double* d_dump,
                        int dump_block) {
  const int N = c->cfg.n_samples;
  // zero-padded search (set_zero_padded): the plain passes, not the four-step plan, and the
  // statistics over the kept lags
  const int keep = c->keep, NK = keep ? keep : N;
  const int m4 = keep ? 0 : c->gen.m4.plan;
  const bool nc = mode == GNSSCORR_ACQ_NONCOHERENT;
  // records: every group on every record of the resident spectra (virtual groups; one
  // record on Bluestein, gnsscorr_acq_set_records)
  const int nrec = c->spec_recs;
  const int n_units = nrec * n_groups * n_bins * (nc ? 1 : n_blocks);
  // four-step plans: the row statistics ride on the last block's m4_rows2 (per-column
  // top-2 of samples N1 apart; its power rows are then not stored) unless the window is
  // too wide for that top-2 or the power rows are dumped
  const int N1 = m4 ? kM4Plans[m4][0] * kM4Plans[m4][1] : 0;
  const bool fused = m4 && c->gen.m4.d_top && top2_exact(N1, spc) && !d_dump;
  // equal chunks (7 x 375 rows rather than 6 x 385 + 314 at the bench's 2 624); with
  // two lanes an even count, chunk i on lane i % 2 (stream, Y, power rows, top-2 of
  // its own), forked from and joined back to the context stream
  const int lanes = m4 ? c->gen.m4.lanes : 1;
  // a concatenated search's units are per block, every chunk whole rows of n_blocks (the
  // equal step rounded up to one: still within the chunk, itself a multiple of n_blocks)
  const bool concat = mode == GNSSCORR_ACQ_CONCAT;
  const int chunk = concat ? c->gen.chunk - c->gen.chunk % n_blocks : c->gen.chunk;
  if (chunk < 1) {
    gnsscorr_set_error("gnsscorr_acq: GNSSCORR_ACQ_CONCAT needs a chunk of at least n_blocks "
                       "rows (%d < %d: max_codes x max_freqs x max_blocks too small)",
                       c->gen.chunk, n_blocks);
    return GNSSCORR_EINVAL;
  }
  int n_ch = (n_units + chunk - 1) / chunk;
  if (lanes == 2 && n_ch > 1 && n_ch % 2) n_ch++;
  int step = n_ch > 0 ? (n_units + n_ch - 1) / n_ch : chunk;
  if (concat) step = (step + n_blocks - 1) / n_blocks * n_blocks;
  // lane 1 starts after lane 0's first column pass, so from then on one lane's column
  // pass (memory-bound) runs beside the other's row pass (fp64-issue-bound); started
  // together, the lanes ran the same pass at the same time
  M4StatsJob pends[2];   // per lane: fused statistics of its previous chunk, not yet launched
  int ci = 0;
  for (int u0 = 0; u0 < n_units; u0 += step, ci++) {
    const int nu = n_units - u0 < step ? n_units - u0 : step;
    const int nb = nc ? n_blocks : 1;
    const int li = lanes == 2 ? ci % 2 : 0;
    const acq_chunk_lane ln = chunk_lane(c, li);
    M4StatsJob& pend = pends[li];
    if (lanes == 2 && ci == 1) HIP_TRY(hipStreamWaitEvent(ln.stream, c->gen.m4.ev[0], 0));
    for (int b = 0; b < nb; b++) {
      const MixCorr cp{(const v2d*)c->d_X64.p, (const v2d*)c->d_F64, c->rs64, n_blocks,
                       nc ? b : -1, n_bins, u0, d_gcode, d_gfreq, (const int2*)c->d_fmap64,
                       n_groups, n_blocks * nrec, keep};
      int rc;
      if (m4) {
        const M4StatsJob* sj = b == 0 && pend.n > 0 ? &pend : nullptr;
        hipEvent_t const fork = lanes == 2 && ci == 0 && b == 0 ? c->gen.m4.ev[0] : nullptr;
        rc = m4_chunk(c, ln, cp, nu, b, fused && b == nb - 1, sj, fork);
        if (!rc && sj) pend.n = 0;
      } else {
        rc = c->gen.mix.nr ? mx_chunk(c, cp, nu, b) : bz_chunk(c, cp, nu, b, NK);
      }
      if (rc) return rc;
    }
    if (fused) {   // carried by the lane's next column pass, or launched below
      pend = M4StatsJob{(const M4Top*)ln.top, c->d_stats.p, nu, u0, N1, n_blocks, (int)nc, spc};
    } else {
      const int rc = concat ? g_stats_concat_launch(c, ln.stream, ln.pw, nu, u0, n_blocks, spc)
                            : g_stats_launch(c, ln.stream, ln.pw, NK, nu, u0, n_blocks, nc, spc,
                                             d_dump, dump_block);
      if (rc) return rc;
    }
  }
  for (int l = 0; l < 2; l++)
    if (pends[l].n > 0) {   // each lane's last chunk's statistics
      hipLaunchKernelGGL(m4_stats_kernel, dim3(pends[l].n), dim3(64), 0, chunk_lane(c, l).stream,
                         pends[l].top, N1, N, pends[l].u0, n_blocks, (int)nc, spc, c->d_stats.p);
      HIP_TRY(hipGetLastError());
    }
  if (lanes == 2) {   // join lane 1 back to the context stream
    HIP_TRY(hipEventRecord(c->gen.m4.ev[1], c->gen.m4.lane1.stream));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->gen.m4.ev[1], 0));
  }
  return GNSSCORR_OK;
}

// Host only: the pass orders acq64_gen_init stores in mix.r / mix.rp for n_samples (the
// tests' view of mix_factor / mix_order_padded; no environment, no device)
extern "C" int gnsscorr_acq_mix_plan(int n_samples, int* radices, int* padded, int cap) {
  if (n_samples < 64 || n_samples > (1 << 19)) return 0;
  int r[24] = {}, rp[24] = {};
  const int n = mix_factor(n_samples, r);
  mix_order_padded(r, n, rp);
  for (int i = 0; i < n && i < cap; i++) {
    if (radices) radices[i] = r[i];
    if (padded) padded[i] = rp[i];
  }
  return n;
}
