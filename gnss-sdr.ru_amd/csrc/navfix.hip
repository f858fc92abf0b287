// navfix.hip -- the GPS L1 receiver after the data bits, on the device ("nav"):
// ephemeris fields and TOW from the 1500 bits of gnsscorr_nav_gps_frames, then the
// measurement loop: pseudoranges, satellite positions, least-squares position.
//   GPS/L1/include/ephemeris.sci:82-226
//   GPS/L1/postNavigation.sci:117-282, GPS/L1/calculatePseudoranges.sci:55-72
//   GPS/L1/geoFunctions/satpos.sci:49-147, check_t.sci:19-27, leastSquarePos.sci:32-111,
//   e_r_corr.sci:21-32, topocent.sci:24-58, togeod.sci:32-113, tropo.sci:34-97,
//   cart2geo.sci:22-53
// The whole file is compiled without contraction: the field values and the raw
// pseudoranges are bit-exact ("nav fix").
//
// nav_gps_eph_kernel: one wave per channel.  The 1500 bits go to LDS once; lane f
// owns field f of the table below and walks the five subframes in order, so a
// later subframe with the same ID overwrites an earlier one.
//
// nav_gps_fix_kernel: one wave64 per receiver, lane = channel, the measurement
// loop inside the kernel (measurements are serial through satElev).  Per lane:
// pseudorange, Kepler, rotation, topocentric angles, troposphere.  Across lanes:
// the min of the travel times, the ballots that form the channel sets, and the
// fourteen sums of the normal equations A'A x = A'omc (xor butterflies: every lane
// ends with the same bits), which every lane then solves by an unrolled LDL'
// factorisation.  Lanes outside the active set contribute zeros to the sums and
// +inf to the min; no reduction sits inside a divergent branch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "gnsscorr_internal.h"
#include "hostctx.h"
#include "nav_host.h"

#pragma clang fp contract(off)
#include "nav_dev.h"

namespace {

using namespace navdev;

constexpr int kGpsBits = 1500;
constexpr double kGpsPi = 3.1415926535898;             // ephemeris.sci:65, satpos.sci:34

// ---------------------------------------------------------------------------
// ephemeris.sci:82-226.  Bit positions are the file's (1-based, inside a subframe).
// ---------------------------------------------------------------------------
struct EphField {
  uint8_t sf;              // subframe ID that carries it
  uint16_t s1;             // first bit of the first range
  uint8_t l1;              // its length
  uint16_t s2;             // first bit of the second range (0: none)
  uint8_t l2;
  uint8_t sgn;             // the file subtracts first bit * 2^length
  int8_t exp2;             // * 2^exp2
  uint8_t pi;              // then * gpsPi
  uint8_t is_int;          // an int32 field (idx counts from weekNumber)
  uint8_t idx;
  int16_t add;             // weekNumber: + 1024
};
constexpr int kEphFields = 27;
__constant__ EphField kEph[kEphFields] = {
    // subframe 1 (:92-119)
    {1, 61, 10, 0, 0, 0, 0, 0, 1, 0, 1024},            // weekNumber
    {1, 73, 4, 0, 0, 0, 0, 0, 1, 1, 0},                // accuracy
    {1, 77, 6, 0, 0, 0, 0, 0, 1, 2, 0},                // health
    {1, 197, 8, 0, 0, 1, -31, 0, 0, 0, 0},             // T_GD
    {1, 83, 2, 197, 8, 0, 0, 0, 1, 3, 0},              // IODC
    {1, 219, 16, 0, 0, 0, 4, 0, 0, 1, 0},              // t_oc
    {1, 241, 8, 0, 0, 1, -55, 0, 0, 2, 0},             // a_f2
    {1, 249, 16, 0, 0, 1, -43, 0, 0, 3, 0},            // a_f1
    {1, 271, 22, 0, 0, 1, -31, 0, 0, 4, 0},            // a_f0
    // subframe 2 (:121-159)
    {2, 61, 8, 0, 0, 0, 0, 0, 1, 4, 0},                // IODE_sf2
    {2, 69, 16, 0, 0, 1, -5, 0, 0, 5, 0},              // C_rs
    {2, 91, 16, 0, 0, 1, -43, 1, 0, 6, 0},             // deltan
    {2, 107, 8, 121, 24, 1, -31, 1, 0, 7, 0},          // M_0
    {2, 151, 16, 0, 0, 1, -29, 0, 0, 8, 0},            // C_uc
    {2, 167, 8, 181, 24, 0, -33, 0, 0, 9, 0},          // e
    {2, 211, 16, 0, 0, 1, -29, 0, 0, 10, 0},           // C_us
    {2, 227, 8, 241, 24, 0, -19, 0, 0, 11, 0},         // sqrtA
    {2, 271, 16, 0, 0, 0, 4, 0, 0, 12, 0},             // t_oe
    // subframe 3 (:161-205)
    {3, 61, 16, 0, 0, 1, -29, 0, 0, 13, 0},            // C_ic
    {3, 77, 8, 91, 24, 1, -31, 1, 0, 14, 0},           // omega_0
    {3, 121, 16, 0, 0, 1, -29, 0, 0, 15, 0},           // C_is
    {3, 137, 8, 151, 24, 1, -31, 1, 0, 16, 0},         // i_0
    {3, 181, 16, 0, 0, 1, -5, 0, 0, 17, 0},            // C_rc
    {3, 197, 8, 211, 24, 1, -31, 1, 0, 18, 0},         // omega
    {3, 241, 24, 0, 0, 1, -43, 1, 0, 19, 0},           // omegaDot
    {3, 271, 8, 0, 0, 0, 0, 0, 1, 5, 0},               // IODE_sf3
    {3, 279, 14, 0, 0, 1, -43, 1, 0, 20, 0},           // iDot
};
static_assert(sizeof(gnsscorr_gps_eph) == 21 * 8 + 10 * 4, "gnsscorr_gps_eph layout");
static_assert(offsetof(gnsscorr_gps_eph, weekNumber) == 21 * 8, "gnsscorr_gps_eph layout");

// the unsigned value of n bits from 1-based position s of a subframe (bin2dec)
__device__ __forceinline__ uint64_t bits_value(const uint8_t* sub, int s, int n) {
  uint64_t v = 0;
  for (int i = 0; i < n; i++) v = v << 1 | sub[s - 1 + i];
  return v;
}

__global__ __launch_bounds__(64) void nav_gps_eph_kernel(
    const uint8_t* __restrict__ bits, const int32_t* __restrict__ n_bits,
    const int32_t* __restrict__ first_subframe, gnsscorr_gps_eph* __restrict__ eph) {
  __shared__ uint8_t b[kGpsBits];
  const int ch = blockIdx.x, lane = threadIdx.x;
  const uint8_t* in = bits + (int64_t)ch * kGpsBits;
  double* out_d = (double*)(eph + ch);
  int32_t* out_i = (int32_t*)(out_d + 21);
  const bool is_short = n_bits[ch] < kGpsBits || first_subframe[ch] < 0;
  int undecided = 0;
  if (!is_short)
    for (int i = lane; i < kGpsBits; i += 64) {
      const uint8_t v = in[i];
      b[i] = v;
      undecided |= v > 1;
    }
  const int refused = __syncthreads_or(undecided) || is_short;
  int have = 0;
  if (!refused)
    for (int i = 0; i < 5; i++) {
      const int id = (int)bits_value(b + 300 * i, 50, 3);      // :85
      if (id >= 1 && id <= 3) have |= 1 << (id - 1);
    }
  if (lane < kEphFields) {
    const EphField f = kEph[lane];
    double vd = 0.0;
    int32_t vi = 0;
    if (!refused)
      for (int i = 0; i < 5; i++) {
        const uint8_t* sub = b + 300 * i;
        if ((int)bits_value(sub, 50, 3) != f.sf) continue;
        uint64_t u = bits_value(sub, f.s1, f.l1);
        if (f.l2) u = u << f.l2 | bits_value(sub, f.s2, f.l2);
        int64_t v = (int64_t)u;
        if (f.sgn) v -= (int64_t)sub[f.s1 - 1] << (f.l1 + f.l2);
        if (f.is_int) {
          vi = (int32_t)v + f.add;
        } else {
          vd = (double)v * ldexp(1.0, f.exp2);
          if (f.pi) vd = vd * kGpsPi;
        }
      }
    if (f.is_int) out_i[f.idx] = vi;
    else out_d[f.idx] = vd;
  } else if (lane == kEphFields) {                             // :226, the fifth subframe
    out_i[6] = refused ? 0 : (int32_t)bits_value(b + 1200, 31, 17) * 6 - 30;
  } else if (lane == kEphFields + 1) {
    out_i[7] = have;
    out_i[8] = is_short ? GNSSCORR_GPS_EPH_SHORT
                        : refused ? GNSSCORR_GPS_EPH_UNDECIDED : GNSSCORR_GPS_EPH_OK;
    out_i[9] = 0;
  }
}

// ---------------------------------------------------------------------------
// the measurement loop
// ---------------------------------------------------------------------------
struct FixArgs {
  double samples_per_code, start_offset, c, elevation_mask;
  int nav_sol_period, use_trop, max_meas, n_epochs;
  double htop[2], ref[2];        // navdev::tropo_consts
};

struct SatPos { double x, y, z, clk; };

// satpos.sci:56-145 for one satellite
__device__ SatPos sat_pos(const gnsscorr_gps_eph& e, double transmit_time) {
  const double Omegae_dot = 7.2921151467e-5, GM = 3.986005e14, F = -4.442807633e-10;
  const double two_pi = 2 * kGpsPi;
  const double dt = check_t(transmit_time - e.t_oc);
  const double clk0 = ((e.a_f2 * dt + e.a_f1) * dt + e.a_f0) - e.T_GD;
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
  s.clk = ((e.a_f2 * dt + e.a_f1) * dt + e.a_f0) - e.T_GD + dtr;
  return s;
}

// togeod.sci:32-113 for a = 6378137, finv = 298.257223563: latitude and longitude in degrees
__device__ void togeod(double X, double Y, double Z, double* dphi_deg, double* dlambda_deg) {
  const double a = 6378137.0, finv = 298.257223563, tolsq = 1.e-10, rtd = 180 / kPi;
  const double esq = (2 - 1 / finv) / finv, oneesq = 1 - esq;
  const double P = sqrt(X * X + Y * Y);
  double dlambda = P > 1.e-20 ? (atand2(Y, X) / 180 * kPi) * rtd : 0.0;
  if (dlambda < 0) dlambda = dlambda + 360;
  const double r = sqrt(P * P + Z * Z);
  double sinphi = r > 1.e-20 ? Z / r : 0.0;
  double dphi = asin(sinphi);
  *dlambda_deg = dlambda;
  if (r < 1.e-20) {                                            // :77-80, dphi is 0 here
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

// cart2geo.sci:22-53 with i = 5
__device__ void cart2geo5(double X, double Y, double Z, double* phi_deg, double* lambda_deg,
                          double* h_out) {
  const double a = 6378137.0, f = 1 / 298.257223563;
  const double lambda = atand2(Y, X) / 180 * kPi;
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

__global__ __launch_bounds__(64) void nav_gps_fix_kernel(
    const gnsscorr_gps_eph* __restrict__ eph, const int32_t* __restrict__ first_subframe,
    const char* __restrict__ abs_sample, int64_t epoch_stride, int64_t chan_stride,
    const int32_t* __restrict__ rx_first, FixArgs p, int32_t* __restrict__ n_meas_out,
    gnsscorr_gps_fix_sol* __restrict__ sol, gnsscorr_gps_fix_chan* __restrict__ chan) {
  const int rx = blockIdx.x, lane = threadIdx.x;
  const int c0 = rx_first[rx], n_ch = rx_first[rx + 1] - c0;
  const bool valid = lane < n_ch;
  const int ch = c0 + (valid ? lane : 0);
  const gnsscorr_gps_eph e = eph[ch];                          // once, into registers
  const int fs = valid ? first_subframe[ch] : -1;
  const bool decodable = valid && fs >= 0 && e.status == GNSSCORR_GPS_EPH_OK;
  const bool ready = decodable && e.have == 7;                 // postNavigation.sci:120-126
  const int n_ready = __popcll(__ballot(ready));
  const int p_max = wave_max(fs);
  const uint64_t seeds = __ballot(decodable);
  int64_t n_meas = 0;
  if (n_ready >= 4)                                            // :130, :163
    n_meas = min((int64_t)p.max_meas, ((int64_t)p.n_epochs - (p_max + 1)) / p.nav_sol_period);
  if (n_meas < 0) n_meas = 0;
  if (lane == 0) n_meas_out[rx] = (int32_t)n_meas;
  if (n_meas == 0) return;

  // :117,152: the TOW the file's channel loop leaves behind is its last channel's
  double transmit_time = (double)__shfl(e.TOW, 63 - __clzll((long long)seeds));
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  const double dtr = kPi / 180;
  double sat_elev = inf;                                       // :144
  const char* my_abs = abs_sample + (int64_t)ch * chan_stride;
  gnsscorr_gps_fix_chan* my_chan = chan + (int64_t)ch * p.max_meas;
  gnsscorr_gps_fix_sol* my_sol = sol + (int64_t)rx * p.max_meas;

  for (int m = 0; m < (int)n_meas; m++) {
    const bool active = ready && sat_elev >= p.elevation_mask;  // :167
    const int n_act = __popcll(__ballot(active));
    double el = nan, az = nan;                                 // :176-177

    // calculatePseudoranges.sci:55-72
    double travel = inf;
    if (active)
      travel = *(const double*)(my_abs + ((int64_t)fs + (int64_t)p.nav_sol_period * m) *
                                             epoch_stride) / p.samples_per_code;
    const double minimum = floor(wave_min(travel));
    const double raw_p = (travel - minimum + p.start_offset) * (p.c / 1000);

    SatPos s = {0, 0, 0, 0};                                   // :189-191, the active list only
    if (active) s = sat_pos(e, transmit_time);
    const double obs = raw_p + s.clk * p.c;                    // :201-202

    int status = GNSSCORR_GPS_FIX_OK;
    double pos0 = 0, pos1 = 0, pos2 = 0, pos3 = 0;
    double dop[5] = {0, 0, 0, 0, 0};
    double lat = nan, lon = nan, height = nan, corr_p = 0.0;
    if (n_act < 4) {                                           // :245-269
      status = GNSSCORR_GPS_FIX_FEW;
      pos0 = pos1 = pos2 = pos3 = nan;
    } else {                                                   // leastSquarePos.sci:32-111
      double N[10];
      Ldl f;
      for (int iter = 0; iter < 7; iter++) {
        double r0 = s.x, r1 = s.y, r2 = s.z, trop = 2;
        if (iter > 0) {
          const double rho2 = (s.x - pos0) * (s.x - pos0) + (s.y - pos1) * (s.y - pos1) +
                              (s.z - pos2) * (s.z - pos2);
          const double omegatau = 7.292115147e-5 * (sqrt(rho2) / p.c);   // e_r_corr.sci:21-24
          const double co = cos(omegatau), so = sin(omegatau);
          r0 = co * s.x + so * s.y;
          r1 = -so * s.x + co * s.y;
          double phi, lambda;                                  // topocent.sci:26-58
          togeod(pos0, pos1, pos2, &phi, &lambda);
          const double cl = cos(lambda * dtr), sl = sin(lambda * dtr);
          const double cb = cos(phi * dtr), sb = sin(phi * dtr);
          const double d0 = r0 - pos0, d1 = r1 - pos1, d2 = r2 - pos2;
          const double E = -sl * d0 + cl * d1 + 0 * d2;
          const double Nn = -sb * cl * d0 + -sb * sl * d1 + cb * d2;
          const double U = cb * cl * d0 + cb * sl * d1 + sb * d2;
          const double hor_dis = sqrt(E * E + Nn * Nn);
          if (hor_dis < 1.e-20) {
            az = 0;
            el = 90;
          } else {
            az = (atand2(E, Nn) / 180 * kPi) / dtr;
            el = (atand2(U, hor_dis) / 180 * kPi) / dtr;
          }
          if (az < 0) az = az + 360;
          trop = 0;
          if (p.use_trop == 1) {                               // tropo.sci:47-49,58-97
            double sinel = sin(el * dtr);
            if (sinel < 0) sinel = 0;
            trop = 0 + tropo_pass(sinel, p.htop[0], p.ref[0]);
            trop = trop + tropo_pass(sinel, p.htop[1], p.ref[1]);
          }
        }
        const double d0 = r0 - pos0, d1 = r1 - pos1, d2 = r2 - pos2;
        const double range = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        const double omc = active ? obs - range - pos3 - trop : 0.0;
        const double a0 = active ? -d0 / obs : 0.0;
        const double a1 = active ? -d1 / obs : 0.0;
        const double a2 = active ? -d2 / obs : 0.0;
        const double a3 = active ? 1.0 : 0.0;
        N[0] = wave_sum(a0 * a0);
        N[1] = wave_sum(a1 * a0);
        N[2] = wave_sum(a1 * a1);
        N[3] = wave_sum(a2 * a0);
        N[4] = wave_sum(a2 * a1);
        N[5] = wave_sum(a2 * a2);
        N[6] = wave_sum(a3 * a0);
        N[7] = wave_sum(a3 * a1);
        N[8] = wave_sum(a3 * a2);
        N[9] = wave_sum(a3 * a3);
        const double g0 = wave_sum(a0 * omc), g1 = wave_sum(a1 * omc);
        const double g2 = wave_sum(a2 * omc), g3 = wave_sum(a3 * omc);
        if (!ldl_factor(N, &f)) {                              // :85-88
          status = GNSSCORR_GPS_FIX_RANK;
          break;
        }
        double x[4];
        ldl_solve(f, g0, g1, g2, g3, x);                       // :91
        pos0 = pos0 + x[0];
        pos1 = pos1 + x[1];
        pos2 = pos2 + x[2];
        pos3 = pos3 + x[3];
      }
      if (status == GNSSCORR_GPS_FIX_RANK) {
        pos0 = pos1 = pos2 = pos3 = 0;
        lat = lon = height = 0;
        el = az = nan;
      } else {
        double q[4], Q00, Q11, Q22, Q33;                       // :105-111
        ldl_solve(f, 1, 0, 0, 0, q);
        Q00 = q[0];
        ldl_solve(f, 0, 1, 0, 0, q);
        Q11 = q[1];
        ldl_solve(f, 0, 0, 1, 0, q);
        Q22 = q[2];
        ldl_solve(f, 0, 0, 0, 1, q);
        Q33 = q[3];
        dop[0] = sqrt(Q00 + Q11 + Q22 + Q33);
        dop[1] = sqrt(Q00 + Q11 + Q22);
        dop[2] = sqrt(Q00 + Q11);
        dop[3] = sqrt(Q22);
        dop[4] = sqrt(Q33);
        if (!active) el = az = nan;
        sat_elev = el;                                         // postNavigation.sci:217
        if (active) corr_p = raw_p + s.clk * p.c + pos3;       // :220-222
        cart2geo5(pos0, pos1, pos2, &lat, &lon, &height);      // :227-233
      }
    }
    if (valid) {
      gnsscorr_gps_fix_chan o;
      o.el = el;
      o.az = az;
      o.rawP = raw_p;
      o.corrP = corr_p;
      o.used = active;
      o.reserved = 0;
      my_chan[m] = o;
    }
    if (lane == 0) {
      gnsscorr_gps_fix_sol o;
      o.X = pos0;
      o.Y = pos1;
      o.Z = pos2;
      o.dt = pos3;
      for (int k = 0; k < 5; k++) o.DOP[k] = dop[k];
      o.lat = lat;
      o.lon = lon;
      o.height = height;
      o.status = status;
      o.n_used = n_act;
      my_sol[m] = o;
    }
    transmit_time = transmit_time + (double)p.nav_sol_period / 1000;   // :280
  }
}

}  // namespace

// ============================================================================
// host side
// ============================================================================
using navhost::bad_arguments;
using navhost::check_series;
using navhost::series_bytes;

extern "C" void gnsscorr_nav_gps_fix_cfg_init(gnsscorr_gps_fix_cfg* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof *cfg);
  cfg->samplesPerCode = 16000.0;      // initSettings.sci:69-73: 16e6 / (1.023e6 / 1023)
  cfg->startOffset = 68.802;          // :125
  cfg->c = 299792458.0;               // :124
  cfg->elevationMask = 10.0;          // :106
  cfg->navSolPeriod = 500;            // :103
  cfg->useTropCorr = 1;               // :108
  cfg->max_meas = 1;
}

static int check_eph(const char* fn, const gnsscorr_nav_ctx* c, const void* bits,
                     const void* n_bits, const void* first, int n_ch, const void* eph) {
  if (!c || !bits || !n_bits || !first || !eph) return bad_arguments(fn, "null pointer");
  if (n_ch < 1) return bad_arguments(fn, "n_ch >= 1");
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_gps_ephemeris_dev(gnsscorr_nav_ctx* c, const uint8_t* d_bits,
                                              const int32_t* d_n_bits,
                                              const int32_t* d_first_subframe, int n_ch,
                                              gnsscorr_gps_eph* d_eph) {
  int rc = check_eph(__func__, c, d_bits, d_n_bits, d_first_subframe, n_ch, d_eph);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  hipLaunchKernelGGL(nav_gps_eph_kernel, dim3(n_ch), dim3(64), 0, c->stream, d_bits, d_n_bits,
                     d_first_subframe, d_eph);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_gps_ephemeris(gnsscorr_nav_ctx* c, const uint8_t* h_bits,
                                          const int32_t* h_n_bits,
                                          const int32_t* h_first_subframe, int n_ch,
                                          gnsscorr_gps_eph* h_eph) {
  int rc = check_eph(__func__, c, h_bits, h_n_bits, h_first_subframe, n_ch, h_eph);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  const size_t n = (size_t)n_ch;
  hostctx::Staging st(c->stream);
  const uint8_t* d_bits = st.in(h_bits, n * kGpsBits);
  const int32_t* d_n_bits = st.in(h_n_bits, n);
  const int32_t* d_first_subframe = st.in(h_first_subframe, n);
  gnsscorr_gps_eph* d_eph = st.out(h_eph, n);
  if (st.status()) return st.status();
  rc = gnsscorr_nav_gps_ephemeris_dev(c, d_bits, d_n_bits, d_first_subframe, n_ch, d_eph);
  return rc ? rc : st.finish();
}

static int check_fix(const char* fn, const gnsscorr_nav_ctx* c, const void* eph,
                     const void* first, const void* abs_sample, int64_t epoch_stride,
                     int64_t chan_stride, int n_epochs, int n_rx, const int32_t* rx_first,
                     const gnsscorr_gps_fix_cfg* cfg, const void* n_meas, const void* sol,
                     const void* chan) {
  if (!c || !eph || !first || !abs_sample || !rx_first || !cfg || !n_meas || !sol || !chan)
    return bad_arguments(fn, "null pointer");
  if (n_rx < 1) return bad_arguments(fn, "n_rx >= 1");
  if (rx_first[0] != 0) return bad_arguments(fn, "rx_first[0] == 0");
  for (int i = 0; i < n_rx; i++) {
    const int64_t n = (int64_t)rx_first[i + 1] - rx_first[i];
    if (n < 1) return bad_arguments(fn, "rx_first ascending");
    if (n > 64) return bad_arguments(fn, "at most 64 channels in a receiver");
  }
  int rc = check_series(fn, c, abs_sample, epoch_stride, chan_stride, n_epochs, rx_first[n_rx]);
  if (rc) return rc;
  if (cfg->navSolPeriod < 1) return bad_arguments(fn, "navSolPeriod >= 1");
  if (!(cfg->samplesPerCode > 0)) return bad_arguments(fn, "samplesPerCode > 0");
  if (cfg->max_meas < 1) return bad_arguments(fn, "max_meas >= 1");
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_gps_fix_dev(gnsscorr_nav_ctx* c, const gnsscorr_gps_eph* d_eph,
                                        const int32_t* d_first_subframe,
                                        const void* d_abs_sample, int64_t epoch_stride_bytes,
                                        int64_t chan_stride_bytes, int n_epochs, int n_rx,
                                        const int32_t* rx_first,
                                        const gnsscorr_gps_fix_cfg* cfg, int32_t* d_n_meas,
                                        gnsscorr_gps_fix_sol* d_sol,
                                        gnsscorr_gps_fix_chan* d_chan) {
  int rc = check_fix(__func__, c, d_eph, d_first_subframe, d_abs_sample, epoch_stride_bytes,
                     chan_stride_bytes, n_epochs, n_rx, rx_first, cfg, d_n_meas, d_sol, d_chan);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  rc = hostctx::grow(c->d_rx_first, (size_t)n_rx + 1);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->d_rx_first.p, rx_first, ((size_t)n_rx + 1) * sizeof(int32_t),
                         hipMemcpyHostToDevice, c->stream));
  FixArgs p;
  p.samples_per_code = cfg->samplesPerCode;
  p.start_offset = cfg->startOffset;
  p.c = cfg->c;
  p.elevation_mask = cfg->elevationMask;
  p.nav_sol_period = cfg->navSolPeriod;
  p.use_trop = cfg->useTropCorr;
  p.max_meas = cfg->max_meas;
  p.n_epochs = n_epochs;
  navdev::tropo_consts(p.htop, p.ref);
  hipLaunchKernelGGL(nav_gps_fix_kernel, dim3(n_rx), dim3(64), 0, c->stream, d_eph,
                     d_first_subframe, (const char*)d_abs_sample, epoch_stride_bytes,
                     chan_stride_bytes, c->d_rx_first.p, p, d_n_meas, d_sol, d_chan);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_gps_fix(gnsscorr_nav_ctx* c, const gnsscorr_gps_eph* h_eph,
                                    const int32_t* h_first_subframe, const void* h_abs_sample,
                                    int64_t epoch_stride_bytes, int64_t chan_stride_bytes,
                                    int n_epochs, int n_rx, const int32_t* rx_first,
                                    const gnsscorr_gps_fix_cfg* cfg, int32_t* h_n_meas,
                                    gnsscorr_gps_fix_sol* h_sol, gnsscorr_gps_fix_chan* h_chan) {
  int rc = check_fix(__func__, c, h_eph, h_first_subframe, h_abs_sample, epoch_stride_bytes,
                     chan_stride_bytes, n_epochs, n_rx, rx_first, cfg, h_n_meas, h_sol, h_chan);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  const size_t n_ch = (size_t)rx_first[n_rx], mm = (size_t)cfg->max_meas;
  const size_t n_in = series_bytes(epoch_stride_bytes, chan_stride_bytes, n_epochs, (int)n_ch);
  hostctx::Staging st(c->stream);
  const gnsscorr_gps_eph* d_eph = st.in(h_eph, n_ch);
  const int32_t* d_first_subframe = st.in(h_first_subframe, n_ch);
  int32_t* d_n_meas = st.out(h_n_meas, (size_t)n_rx);
  const char* d_abs_sample = st.in((const char*)h_abs_sample, n_in);
  // uploaded too: rows past n_meas stay as the caller has them
  gnsscorr_gps_fix_sol* d_sol = st.inout(h_sol, (size_t)n_rx * mm);
  gnsscorr_gps_fix_chan* d_chan = st.inout(h_chan, n_ch * mm);
  if (st.status()) return st.status();
  rc = gnsscorr_nav_gps_fix_dev(c, d_eph, d_first_subframe, d_abs_sample, epoch_stride_bytes,
                                chan_stride_bytes, n_epochs, n_rx, rx_first, cfg, d_n_meas, d_sol,
                                d_chan);
  return rc ? rc : st.finish();
}
