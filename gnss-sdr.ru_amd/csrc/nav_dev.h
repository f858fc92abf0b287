// nav_dev.h -- device helpers that the GPS fix (navfix.hip), the GLONASS fix (navglo.hip)
// and the BeiDou fix (navb1.hip) compute identically: the wave reductions, one pass of
// tropo.sci, the LDL' factorisation of the normal equations with the library's rank rule,
// on the host the constants of tropo.sci's two passes; togeod and cart2geo in their two texts
// (Fix); the Kepler propagation of satpos.sci with check_t and its reductions (GPS, BeiDou);
// bin2dec of an ephemeris field.  The measurement loop built from them is nav_fix.h.  Every
// file includes it under `#pragma clang fp contract(off)`: no operation here may be
// contracted.
#ifndef GNSSCORR_NAV_DEV_H
#define GNSSCORR_NAV_DEV_H
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

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

// The two texts of the shared geoFunctions.  kGps: GPS/L1 takes every angle of two arguments
// through atand and converts back; its leastSquarePos.sci starts the troposphere term at 2 m,
// divides the rows of A by the observation and forms omc as obs - range - dt - trop.
// kGloB1: GLONASS/L1 and COMPASS/B1 call atan(y, x) directly, start the term at 0, divide by
// the geometric range and form obs - dt - range - trop.
enum class Fix { kGps, kGloB1 };

template <Fix F>
__device__ __forceinline__ double atan_yx(double y, double x) {
  if constexpr (F == Fix::kGps) return atand2(y, x) / 180 * kPi;
  else return atan2(y, x);
}

// togeod.sci (GPS/L1 :32-113, GLONASS/L1 and COMPASS/B1 :31-110) for a = 6378137,
// finv = 298.257223563: latitude and longitude in degrees
template <Fix F>
__device__ void togeod(double X, double Y, double Z, double* dphi_deg, double* dlambda_deg) {
  const double a = 6378137.0, finv = 298.257223563, tolsq = 1.e-10, rtd = 180 / kPi;
  const double esq = (2 - 1 / finv) / finv, oneesq = 1 - esq;
  const double P = sqrt(X * X + Y * Y);
  double dlambda = P > 1.e-20 ? atan_yx<F>(Y, X) * rtd : 0.0;
  if (dlambda < 0) dlambda = dlambda + 360;
  const double r = sqrt(P * P + Z * Z);
  double sinphi = r > 1.e-20 ? Z / r : 0.0;
  double dphi = asin(sinphi);
  *dlambda_deg = dlambda;
  if (r < 1.e-20) {                                            // dphi is 0 here
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

// cart2geo.sci (GPS/L1 :22-53, GLONASS/L1 and COMPASS/B1 :20-45) with i = 5
template <Fix F>
__device__ void cart2geo5(double X, double Y, double Z, double* phi_deg, double* lambda_deg,
                          double* h_out) {
  const double a = 6378137.0, f = 1 / 298.257223563;
  const double lambda = atan_yx<F>(Y, X);
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

// GPS/L1 and COMPASS/B1 satpos.sci (:56-145, :53-136) are one text but for two constants and
// the names of four fields.  The elements as the file names them, a2 / a1 / a0 / T_GD for
// GPS's a_f2 / a_f1 / a_f0 / T_GD and BeiDou's a2 / a1 / a0 / T_GD_1.
constexpr double kEphPi = 3.1415926535898;     // gpsPi, BDPi: ephemeris.sci, satpos.sci
struct Kepler {
  double t_oc, a2, a1, a0, T_GD;
  double sqrtA, t_oe, deltan, M_0, e, omega, C_uc, C_us, C_rc, C_rs, i_0, iDot, C_ic, C_is;
  double omega_0, omegaDot;
};
// from a record E that names the orbit as the file does, and its own clock terms
template <class E>
__device__ __forceinline__ Kepler kepler_of(const E& e, double a2, double a1, double a0,
                                            double T_GD) {
  return {e.t_oc, a2, a1, a0, T_GD, e.sqrtA, e.t_oe, e.deltan, e.M_0, e.e, e.omega,
          e.C_uc, e.C_us, e.C_rc, e.C_rs, e.i_0, e.iDot, e.C_ic, e.C_is, e.omega_0, e.omegaDot};
}

struct SatPos { double x, y, z, clk; };

// satpos.sci for one satellite: ECEF position and clock correction at transmit_time
__device__ inline SatPos sat_pos(const Kepler& e, double Omegae_dot, double GM,
                                 double transmit_time) {
  const double F = -4.442807633e-10;
  const double two_pi = 2 * kEphPi;
  const double dt = check_t(transmit_time - e.t_oc);
  const double clk0 = ((e.a2 * dt + e.a1) * dt + e.a0) - e.T_GD;
  const double time = transmit_time - clk0;
  const double a = e.sqrtA * e.sqrtA;
  const double tk = check_t(time - e.t_oe);
  const double n0 = sqrt(GM / (a * a * a));
  const double n = n0 + e.deltan;
  double M = e.M_0 + n * tk;
  M = rem_fix(M + two_pi, two_pi);
  double E = M;
  for (int ii = 0; ii < 10; ii++) {
    const double E_old = E;
    E = M + e.e * sin(E);
    const double dE = rem_fix(E - E_old, two_pi);
    if (fabs(dE) < 1.e-12) break;
  }
  E = rem_fix(E + two_pi, two_pi);
  const double sinE = sin(E), cosE = cos(E);
  const double dtr = F * e.e * e.sqrtA * sinE;
  const double nu = atand2(sqrt(1 - e.e * e.e) * sinE, cosE - e.e) / 180 * kPi;
  double phi = nu + e.omega;
  phi = rem_fix(phi, two_pi);
  const double c2 = cos(2 * phi), s2 = sin(2 * phi);
  const double u = phi + e.C_uc * c2 + e.C_us * s2;
  const double r = a * (1 - e.e * cosE) + e.C_rc * c2 + e.C_rs * s2;
  const double i = e.i_0 + e.iDot * tk + e.C_ic * c2 + e.C_is * s2;
  double Omega = e.omega_0 + (e.omegaDot - Omegae_dot) * tk - Omegae_dot * e.t_oe;
  Omega = rem_fix(Omega + two_pi, two_pi);
  const double cu = cos(u), su = sin(u), cO = cos(Omega), sO = sin(Omega);
  SatPos s;
  s.x = cu * r * cO - su * r * cos(i) * sO;
  s.y = cu * r * sO + su * r * cos(i) * cO;
  s.z = su * r * sin(i);
  s.clk = ((e.a2 * dt + e.a1) * dt + e.a0) - e.T_GD + dtr;
  return s;
}

// the unsigned value of n values from 1-based position s of a subframe (bin2dec)
__device__ __forceinline__ uint64_t bits_value(const uint8_t* sub, int s, int n) {
  uint64_t v = 0;
  for (int i = 0; i < n; i++) v = v << 1 | sub[s - 1 + i];
  return v;
}

}  // namespace navdev
#endif
