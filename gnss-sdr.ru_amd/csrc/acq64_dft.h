// acq64_dft.h -- what the two fp64 acquisition translation units (acq64.hip: the
// compiled three-stage plans; acq64_gen.hip: the generic-N engine) build their
// transforms from: constexpr trigonometry and number theory, complex helpers, the
// in-register DFT codelets and the wave / workgroup reductions; all forced inline.
#ifndef GNSSCORR_ACQ64_DFT_H
#define GNSSCORR_ACQ64_DFT_H
#include <hip/hip_runtime.h>
#include <limits.h>
#include "acq_peak.h"

namespace {

typedef double v2d __attribute__((ext_vector_type(2)));

// ---- compile-time arithmetic -------------------------------------------------
constexpr double kPi = 3.14159265358979323846264338327950288;

constexpr double poly_sin(double x) {   // |x| <= pi/4, 1 ulp
  double x2 = x * x, term = x, sum = x;
  for (int i = 1; i < 12; i++) {
    term *= -x2 / (double)((2 * i) * (2 * i + 1));
    sum += term;
  }
  return sum;
}
constexpr double poly_cos(double x) {
  double x2 = x * x, term = 1.0, sum = 1.0;
  for (int i = 1; i < 12; i++) {
    term *= -x2 / (double)((2 * i - 1) * (2 * i));
    sum += term;
  }
  return sum;
}
struct CS { double c, s; };
// cos, sin of 2 pi j / R: exact octant reduction in integers, then a series
constexpr CS cs2pi(long j, long R) {
  j %= R;
  if (j < 0) j += R;
  const long q = (8 * j) / R, rem = 8 * j - q * R;   // angle = (q + rem/R) pi/4
  double c = 0, s = 0;
  if ((q & 1) == 0) {
    const double x = (double)rem / (double)R * (kPi / 4);
    c = poly_cos(x);
    s = poly_sin(x);
  } else {   // phi = pi/4 + x in [pi/4, pi/2): use pi/2 - phi = (R - rem)/R pi/4
    const double y = (double)(R - rem) / (double)R * (kPi / 4);
    c = poly_sin(y);
    s = poly_cos(y);
  }
  switch ((q >> 1) & 3) {
    case 0: return CS{c, s};
    case 1: return CS{-s, c};
    case 2: return CS{-c, -s};
    default: return CS{s, -c};
  }
}
template <int R>
struct TwTab {
  double c[R], s[R];
  constexpr TwTab() : c{}, s{} {
    for (int j = 0; j < R; j++) {
      const CS v = cs2pi(j, R);
      c[j] = v.c;
      s[j] = v.s;
    }
  }
};
template <int R>
constexpr TwTab<R> kTw{};

constexpr int cgcd(int a, int b) { return b == 0 ? a : cgcd(b, a % b); }
constexpr int cinv(int a, int m) {   // a^-1 mod m (gcd(a, m) = 1)
  a %= m;
  for (int x = 1; x < m; x++)
    if ((long)a * x % m == 1) return x;
  return m == 1 ? 0 : -1;
}
constexpr bool is_prime(int r) {
  if (r < 2) return false;
  for (int d = 2; d * d <= r; d++)
    if (r % d == 0) return false;
  return true;
}
constexpr int small_pf(int r) {
  for (int d = 2; d * d <= r; d++)
    if (r % d == 0) return d;
  return r;
}
// largest power of the smallest prime factor dividing r
constexpr int pf_power(int r) {
  const int p = small_pf(r);
  int q = 1;
  while (r % (q * p) == 0) q *= p;
  return q;
}

// ---- complex helpers -----------------------------------------------------------
__device__ __forceinline__ v2d mul_mi(v2d v) { return (v2d){v.y, -v.x}; }   // -i v
__device__ __forceinline__ v2d mul_pi(v2d v) { return (v2d){-v.y, v.x}; }   // +i v
__device__ __forceinline__ v2d cmul(v2d a, v2d b) {
  return (v2d){fma(a.x, b.x, -(a.y * b.y)), fma(a.x, b.y, a.y * b.x)};
}
// v * W_R^j, W = exp(-2 pi i / R); j is a compile-time constant after unrolling
template <int R>
__device__ __forceinline__ v2d twc(v2d v, int j) {
  j %= R;
  if (j == 0) return v;
  if (4 * j == R) return mul_mi(v);
  if (2 * j == R) return -v;
  if (4 * j == 3 * R) return mul_pi(v);
  const double c = kTw<R>.c[j], s = kTw<R>.s[j];   // W^j = c - i s
  return (v2d){fma(v.x, c, v.y * s), fma(v.y, c, -(v.x * s))};
}

// ---- small in-register DFTs (forward, natural order in and out) ---------------
template <int R>
__device__ __forceinline__ void dft(v2d (&x)[R]);

__device__ __forceinline__ void dft2(v2d (&x)[2]) {
  const v2d a = x[0], b = x[1];
  x[0] = a + b;
  x[1] = a - b;
}
__device__ __forceinline__ void dft4(v2d (&x)[4]) {
  const v2d t0 = x[0] + x[2], t1 = x[0] - x[2], t2 = x[1] + x[3], t3 = x[1] - x[3];
  x[0] = t0 + t2;
  x[2] = t0 - t2;
  x[1] = t1 + mul_mi(t3);
  x[3] = t1 + mul_pi(t3);
}
// symmetric prime-length DFT
template <int P>
__device__ __forceinline__ void dft_prime(v2d (&x)[P]) {
  constexpr int H = (P - 1) / 2;
  v2d s[H + 1], d[H + 1];
#pragma unroll
  for (int j = 1; j <= H; j++) {
    s[j] = x[j] + x[P - j];
    d[j] = x[j] - x[P - j];
  }
  const v2d x0 = x[0];
  v2d X0 = x0;
#pragma unroll
  for (int j = 1; j <= H; j++) X0 += s[j];
#pragma unroll
  for (int m = 1; m <= H; m++) {
    v2d A = x0, B = (v2d){0.0, 0.0};
#pragma unroll
    for (int j = 1; j <= H; j++) {
      const int q = (j * m) % P;
      const double c = kTw<P>.c[q], sn = kTw<P>.s[q];
      A = (v2d){fma(c, s[j].x, A.x), fma(c, s[j].y, A.y)};
      B = (v2d){fma(sn, d[j].x, B.x), fma(sn, d[j].y, B.y)};
    }
    x[m] = (v2d){A.x + B.y, A.y - B.x};       // A - i B
    x[P - m] = (v2d){A.x - B.y, A.y + B.x};   // A + i B
  }
  x[0] = X0;
}
// symmetric prime DFT that hands each output to emit(k, X_k) as its (m, P-m) pair
// is formed (s_j, d_j in place in x): the 31 complex outputs are never all live (register
// pressure of the non-coherent kernel, whose running sums stay live across the transform)
// SERIAL: one output pair at a time (a scheduling barrier after each): the compiler
// otherwise interleaves all (P-1)/2 accumulator pairs, 4 P more live registers
template <int P, bool SERIAL = false, class Emit>
__device__ __forceinline__ void dft_prime_emit(v2d (&x)[P], const Emit& emit) {
  constexpr int H = (P - 1) / 2;
#pragma unroll
  for (int j = 1; j <= H; j++) {
    const v2d a = x[j], b = x[P - j];
    x[j] = a + b;        // s_j
    x[P - j] = a - b;    // d_j
  }
  v2d X0 = x[0];
#pragma unroll
  for (int j = 1; j <= H; j++) X0 += x[j];
#pragma unroll
  for (int m = 1; m <= H; m++) {
    v2d A = x[0], B = (v2d){0.0, 0.0};
#pragma unroll
    for (int j = 1; j <= H; j++) {
      const int q = (j * m) % P;
      const double c = kTw<P>.c[q], sn = kTw<P>.s[q];
      A = (v2d){fma(c, x[j].x, A.x), fma(c, x[j].y, A.y)};
      B = (v2d){fma(sn, x[P - j].x, B.x), fma(sn, x[P - j].y, B.y)};
    }
    emit(m, (v2d){A.x + B.y, A.y - B.x});       // A - iB
    emit(P - m, (v2d){A.x - B.y, A.y + B.x});   // A + iB
    if constexpr (SERIAL) __builtin_amdgcn_sched_barrier(0);
  }
  emit(0, X0);
}
// dft_prime_emit fused with |.|^2 * scale: put_power(k, |X_k|^2 scale) for every output k
template <int P, class Put>
__device__ __forceinline__ void dft_prime_power(v2d (&x)[P], const Put& put_power, double scale) {
  dft_prime_emit<P>(x, [&](int k, v2d v) { put_power(k, fma(v.x, v.x, v.y * v.y) * scale); });
}

// Good-Thomas R = A * B, gcd(A, B) = 1: n = (a B + b A) mod R, k = CRT(ka, kb)
template <int A, int B>
__device__ __forceinline__ void dft_pfa(v2d (&x)[A * B]) {
  constexpr int R = A * B;
  constexpr int eA = B * cinv(B % A, A) % R, eB = A * cinv(A % B, B) % R;
  v2d y[A][B];
#pragma unroll
  for (int a = 0; a < A; a++)
#pragma unroll
    for (int b = 0; b < B; b++) y[a][b] = x[(a * B + b * A) % R];
#pragma unroll
  for (int b = 0; b < B; b++) {
    v2d t[A];
#pragma unroll
    for (int a = 0; a < A; a++) t[a] = y[a][b];
    dft<A>(t);
#pragma unroll
    for (int a = 0; a < A; a++) y[a][b] = t[a];
  }
#pragma unroll
  for (int a = 0; a < A; a++) dft<B>(y[a]);
#pragma unroll
  for (int a = 0; a < A; a++)
#pragma unroll
    for (int b = 0; b < B; b++) x[(a * eA + b * eB) % R] = y[a][b];
}
// Cooley-Tukey R = A * B (decimation in frequency): n = a B + b, k = ka + A kb
template <int A, int B>
__device__ __forceinline__ void dft_ct(v2d (&x)[A * B]) {
  constexpr int R = A * B;
  v2d y[A][B];
#pragma unroll
  for (int b = 0; b < B; b++) {
    v2d t[A];
#pragma unroll
    for (int a = 0; a < A; a++) t[a] = x[a * B + b];
    dft<A>(t);
#pragma unroll
    for (int a = 0; a < A; a++) y[a][b] = twc<R>(t[a], a * b);
  }
#pragma unroll
  for (int a = 0; a < A; a++) dft<B>(y[a]);
#pragma unroll
  for (int a = 0; a < A; a++)
#pragma unroll
    for (int b = 0; b < B; b++) x[a + A * b] = y[a][b];
}
template <int R>
__device__ __forceinline__ void dft(v2d (&x)[R]) {
  if constexpr (R == 1) {
  } else if constexpr (R == 2) {
    dft2(x);
  } else if constexpr (R == 4) {
    dft4(x);
  } else if constexpr (is_prime(R)) {
    dft_prime<R>(x);
  } else if constexpr (pf_power(R) != R) {
    constexpr int A = pf_power(R);
    dft_pfa<A, R / A>(x);
  } else {
    constexpr int A = (small_pf(R) == 2 && R >= 16) ? 4 : small_pf(R);
    dft_ct<A, R / A>(x);
  }
}

// outputs 0 .. R/2-1 of an even-length DFT, by decimation in time: X_k = E_k + W_R^k O_k
// (E, O the R/2-point DFTs of the even and the odd inputs); the other half,
// X_{k+R/2} = E_k - W_R^k O_k, is not formed
template <int R>
__device__ __forceinline__ void dft_first_half(const v2d (&x)[R], v2d (&o)[R / 2]) {
  static_assert(R % 2 == 0, "even length");
  v2d e[R / 2], d[R / 2];
#pragma unroll
  for (int n = 0; n < R / 2; n++) {
    e[n] = x[2 * n];
    d[n] = x[2 * n + 1];
  }
  dft<R / 2>(e);
  dft<R / 2>(d);
#pragma unroll
  for (int k = 0; k < R / 2; k++) o[k] = e[k] + twc<R>(d[k], k);
}

// ---- workgroup reductions --------------------------------------------------------
// Wave step: DPP row_shr 1/2/4/8 (a Hillis-Steele scan inside each 16-lane row,
// the identity shifted in) leaves each row's result in its lane 15; the four
// rows combine in scalar registers.  VALU only: no ds_bpermute round trips
// (a 64-bit __shfl_xor is two LDS-crossbar operations per step).  Every lane
// of the wave must be active.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double ident, double v) {
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(ident), __double2loint(v), CTRL, 0xF,
                                             0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(ident), __double2hiint(v), CTRL, 0xF,
                                             0xF, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_f64(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l),
                          __builtin_amdgcn_readlane(__double2loint(v), l));
}
template <int CTRL>
__device__ __forceinline__ void argmax_step(double& v, int& k) {
  const double v2 = dpp_f64<CTRL>(-1.0, v);
  const int k2 = __builtin_amdgcn_update_dpp(INT_MAX, k, CTRL, 0xF, 0xF, false);
  if (better(v2, k2, v, k)) { v = v2; k = k2; }
}
// argmax (largest value, first index on ties) of the wave; uniform result
__device__ __forceinline__ void wave_argmax(double& v, int& k) {
  argmax_step<0x111>(v, k);
  argmax_step<0x112>(v, k);
  argmax_step<0x114>(v, k);
  argmax_step<0x118>(v, k);
  double bv = readlane_f64(v, 15);
  int bk = __builtin_amdgcn_readlane(k, 15);
#pragma unroll
  for (int r = 31; r < 64; r += 16) {
    const double v2 = readlane_f64(v, r);
    const int k2 = __builtin_amdgcn_readlane(k, r);
    if (better(v2, k2, bv, bk)) { bv = v2; bk = k2; }
  }
  v = bv;
  k = bk;
}
__device__ __forceinline__ double wave_max(double v) {   // values >= -1
  v = fmax(v, dpp_f64<0x111>(-1.0, v));
  v = fmax(v, dpp_f64<0x112>(-1.0, v));
  v = fmax(v, dpp_f64<0x114>(-1.0, v));
  v = fmax(v, dpp_f64<0x118>(-1.0, v));
  return fmax(fmax(readlane_f64(v, 15), readlane_f64(v, 31)),
              fmax(readlane_f64(v, 47), readlane_f64(v, 63)));
}
// tid: the caller's thread index (default threadIdx.x)
template <int NW>
__device__ __forceinline__ void block_argmax(double& v, int& k, double* sv, int* sk,
                                             int tid = threadIdx.x) {
  wave_argmax(v, k);
  if ((tid & 63) == 0) { sv[tid >> 6] = v; sk[tid >> 6] = k; }
  __syncthreads();
  v = sv[0];
  k = sk[0];
#pragma unroll
  for (int i = 1; i < NW; i++)
    if (better(sv[i], sk[i], v, k)) { v = sv[i]; k = sk[i]; }
}
template <int NW>
__device__ __forceinline__ double block_max0(double v, double* sm, int tid = threadIdx.x) {
  v = wave_max(v);
  if ((tid & 63) == 0) sm[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int i = 1; i < NW; i++) v = fmax(v, sm[i]);
  }
  return v;
}

}  // namespace
#endif
