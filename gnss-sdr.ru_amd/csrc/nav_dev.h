// nav_dev.h -- device helpers that the GPS fix (navfix.hip), the GLONASS fix (navglo.hip)
// and the BeiDou fix (navb1.hip) compute identically: the wave reductions, one pass of
// tropo.sci, the LDL' factorisation of the normal equations with the library's rank rule,
// on the host the constants of tropo.sci's two passes; check_t and the reductions of the
// Kepler propagation (GPS, BeiDou); togeod and cart2geo with plain atan(y, x) (GLONASS,
// BeiDou).  Every file includes it under `#pragma clang fp contract(off)`: no operation
// here may be contracted.
#ifndef GNSSCORR_NAV_DEV_H
#define GNSSCORR_NAV_DEV_H
#include <hip/hip_runtime.h>
#include <math.h>

namespace navdev {

constexpr double kPi = 3.14159265358979323846;                 // %pi

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v = v + __shfl_xor(v, d);
  return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v = fmin(v, __shfl_xor(v, d));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v = max(v, __shfl_xor(v, d));
  return v;
}

// one pass of tropo.sci:59-86 with hsta = 0
static __device__ double tropo_pass(double sinel, double htop, double ref) {
  const double a_e = 6378.137, b0 = 7.839257e-5;
  double rtop = (a_e + htop) * (a_e + htop) - a_e * a_e * (1 - sinel * sinel);
  if (rtop < 0) rtop = 0;
  rtop = sqrt(rtop) - a_e * sinel;
  const double a = -sinel / htop;
  const double b = -b0 * (1 - sinel * sinel) / htop;
  const double a2 = a * a, b2 = b * b;
  double alpha[8] = {2 * a,
                     2 * a2 + 4 * b / 3,
                     a * (a2 + 3 * b),
                     a2 * a2 / 5 + 2.4 * a2 * b + 1.2 * b2,
                     2 * a * b * (a2 + 3 * b) / 3,
                     b2 * (6 * a2 + 4 * b) * 1.428571e-1,
                     0.0,
                     0.0};
  if (b2 > 1.0e-35) {
    alpha[6] = a * (b2 * b) / 2;
    alpha[7] = b2 * b2 / 9;
  }
  double rn = rtop * rtop, dot = 0.0;                          // rn(i) = rtop^(i + 1)
#pragma unroll
  for (int i = 0; i < 8; i++) {
    dot = dot + alpha[i] * rn;
    rn = rn * rtop;
  }
  const double dr = rtop + dot;
  return dr * ref * 1000;
}

// tropo.sci:34-56,94-96 for (hsta, p, tkel, hum, hp, htkel, hhum) =
// (0, 1013, 293, 50, 0, 0, 0): the two passes' htop and ref
inline void tropo_consts(double (&htop)[2], double (&ref)[2]) {
  const double tkel = 293.0, hum = 50.0, pr = 1013.0, tlapse = -6.5;
  const double tkhum = tkel + tlapse * (0.0 - 0.0);
  const double atkel = 7.5 * (tkhum - 273.15) / (237.3 + tkhum - 273.15);
  const double e0 = 0.0611 * hum * pow(10.0, atkel);
  const double tksea = tkel - tlapse * 0.0;
  const double em = -978.77 / (2.8704e6 * tlapse * 1.0e-5);
  const double tkelh = tksea + tlapse * 0.0;
  const double e0sea = e0 * pow(tksea / tkelh, 4 * em);
  const double tkelp = tksea + tlapse * 0.0;
  const double psea = pr * pow(tksea / tkelp, em);
  double refsea = 77.624e-6 / tksea;
  htop[0] = 1.1385e-5 / refsea;
  refsea = refsea * psea;
  ref[0] = refsea * pow((htop[0] - 0.0) / htop[0], 4);
  refsea = (371900.0e-6 / tksea - 12.92e-6) / tksea;
  htop[1] = 1.1385e-5 * (1255 / tksea + 0.05) / refsea;
  ref[1] = refsea * e0sea * pow((htop[1] - 0.0) / htop[1], 4);
}

// LDL' of the symmetric 4 x 4 N (lower triangle used), column order.  False when
// a pivot is not above 1e-12 of its column's diagonal entry of N (the rank rule).
struct Ldl { double l10, l20, l21, l30, l31, l32, d0, d1, d2, d3; };
static __device__ bool ldl_factor(const double (&N)[10], Ldl* f) {
  // N: 00 10 11 20 21 22 30 31 32 33
  const double tol = 1.e-12;
  f->d0 = N[0];
  if (!(f->d0 > tol * N[0])) return false;
  f->l10 = N[1] / f->d0;
  f->l20 = N[3] / f->d0;
  f->l30 = N[6] / f->d0;
  f->d1 = N[2] - f->l10 * f->l10 * f->d0;
  if (!(f->d1 > tol * N[2])) return false;
  f->l21 = (N[4] - f->l20 * f->l10 * f->d0) / f->d1;
  f->l31 = (N[7] - f->l30 * f->l10 * f->d0) / f->d1;
  f->d2 = N[5] - f->l20 * f->l20 * f->d0 - f->l21 * f->l21 * f->d1;
  if (!(f->d2 > tol * N[5])) return false;
  f->l32 = (N[8] - f->l30 * f->l20 * f->d0 - f->l31 * f->l21 * f->d1) / f->d2;
  f->d3 = N[9] - f->l30 * f->l30 * f->d0 - f->l31 * f->l31 * f->d1 - f->l32 * f->l32 * f->d2;
  if (!(f->d3 > tol * N[9])) return false;
  return true;
}
static __device__ void ldl_solve(const Ldl& f, double g0, double g1, double g2, double g3, double* x) {
  const double z0 = g0;
  const double z1 = g1 - f.l10 * z0;
  const double z2 = g2 - f.l20 * z0 - f.l21 * z1;
  const double z3 = g3 - f.l30 * z0 - f.l31 * z1 - f.l32 * z2;
  const double x3 = z3 / f.d3;
  const double x2 = z2 / f.d2 - f.l32 * x3;
  const double x1 = z1 / f.d1 - f.l21 * x2 - f.l31 * x3;
  const double x0 = z0 / f.d0 - f.l10 * x1 - f.l20 * x2 - f.l30 * x3;
  x[0] = x0;
  x[1] = x1;
  x[2] = x2;
  x[3] = x3;
}

// the GPS L1 and COMPASS B1 satpos.sci share these (check_t.sci:19-27 is one text)
__device__ __forceinline__ double check_t(double t) {          // check_t.sci:19-27
  const double half_week = 302400.0;
  if (t > half_week) return t - 2 * half_week;
  if (t < -half_week) return t + 2 * half_week;
  return t;
}
// x - fix(x ./ y) .* y
__device__ __forceinline__ double rem_fix(double x, double y) { return x - trunc(x / y) * y; }
// Scilab's two-argument atand, read as (180 / %pi) * atan(y, x)
__device__ __forceinline__ double atand2(double y, double x) { return (180.0 / kPi) * atan2(y, x); }

// GLONASS/L1 and COMPASS/B1 togeod.sci:31-110 (the same text, atan(y, x) called directly) for
// a = 6378137, finv = 298.257223563: latitude and longitude in degrees
inline __device__ void togeod_atan(double X, double Y, double Z, double* dphi_deg,
                                   double* dlambda_deg) {
  const double a = 6378137.0, finv = 298.257223563, tolsq = 1.e-10, rtd = 180 / kPi;
  const double esq = (2 - 1 / finv) / finv, oneesq = 1 - esq;
  const double P = sqrt(X * X + Y * Y);
  double dlambda = P > 1.e-20 ? atan2(Y, X) * rtd : 0.0;       // :52-56
  if (dlambda < 0) dlambda = dlambda + 360;
  const double r = sqrt(P * P + Z * Z);
  double sinphi = r > 1.e-20 ? Z / r : 0.0;
  double dphi = asin(sinphi);
  *dlambda_deg = dlambda;
  if (r < 1.e-20) {                                            // :75-78, dphi is 0 here
    *dphi_deg = dphi;
    return;
  }
  double h = r - a * (1 - sinphi * sinphi / finv);
  for (int i = 0; i < 10; i++) {
    sinphi = sin(dphi);
    const double cosphi = cos(dphi);
    const double N_phi = a / sqrt(1 - esq * sinphi * sinphi);
    const double dP = P - (N_phi + h) * cosphi;
    const double dZ = Z - (N_phi * oneesq + h) * sinphi;
    h = h + (sinphi * dZ + cosphi * dP);
    dphi = dphi + (cosphi * dZ - sinphi * dP) / (N_phi + h);
    if (dP * dP + dZ * dZ < tolsq) break;
  }
  *dphi_deg = dphi * rtd;
}

// GLONASS/L1 and COMPASS/B1 cart2geo.sci:20-45 with i = 5
inline __device__ void cart2geo5_atan(double X, double Y, double Z, double* phi_deg,
                                      double* lambda_deg, double* h_out) {
  const double a = 6378137.0, f = 1 / 298.257223563;
  const double lambda = atan2(Y, X);                           // :23
  const double ex2 = (2 - f) * f / ((1 - f) * (1 - f));
  const double c = a * sqrt(1 + ex2);
  const double p = sqrt(X * X + Y * Y);
  double phi = atan(Z / (p * (1 - (2 - f)) * f));
  double h = 0.1, oldh = 0;
  int iterations = 0;
  while (fabs(h - oldh) > 1.e-12) {
    oldh = h;
    const double cp = cos(phi);
    const double N = c / sqrt(1 + ex2 * (cp * cp));
    phi = atan(Z / (p * (1 - (2 - f) * f * N / (N + h))));
    h = p / cos(phi) - N;
    iterations = iterations + 1;
    if (iterations > 100) break;
  }
  *phi_deg = phi * 180 / kPi;
  *lambda_deg = lambda * 180 / kPi;
  *h_out = h;
}

}  // namespace navdev
#endif
