// nav_fix.h -- the measurement loop that the fix kernels of navfix.hip (GPS L1), navglo.hip
// (GLONASS L1OF) and navb1.hip (BeiDou B1I) share: one wave64 per receiver, lane = channel.
// The receiver's channels and its number of measurements, the pseudorange step, the seven
// iterations of leastSquarePos.sci in its two texts (navdev::Fix), the DOP values and the two
// output records.  What a constellation does differently stays in its own kernel: which
// channels are ready and active, the transmit time, the satellite, and what happens to the
// solution afterwards.  Included under `#pragma clang fp contract(off)`, as nav_dev.h.
//
// Per lane: pseudorange, rotation, topocentric angles, troposphere.  Across lanes: the min of
// the travel times and the fourteen sums of the normal equations A'A x = A'omc (xor
// butterflies: every lane ends with the same bits), which every lane then solves by an
// unrolled LDL' factorisation.  Lanes outside the active set contribute zeros to the sums and
// +inf to the min; no reduction sits inside a divergent branch.
#ifndef GNSSCORR_NAV_FIX_H
#define GNSSCORR_NAV_FIX_H
#include "gnsscorr_internal.h"
#include "nav_dev.h"

namespace navdev {

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ double infinity() { return __longlong_as_double(0x7ff0000000000000ll); }

struct Tropo { double htop[2], ref[2]; };      // tropo_consts

// this lane's channel of receiver blockIdx.x: lanes past the receiver's last channel read its
// first one and are not valid
struct FixLane {
  bool valid;
  int ch;
};
__device__ __forceinline__ FixLane fix_lane(const int32_t* __restrict__ rx_first) {
  const int rx = blockIdx.x, lane = threadIdx.x;
  const int c0 = rx_first[rx], n_ch = rx_first[rx + 1] - c0;
  FixLane l;
  l.valid = lane < n_ch;
  l.ch = c0 + (l.valid ? lane : 0);
  return l;
}

// the receiver's measurements, postNavigation.sci: none with fewer than 4 ready channels, else
// one per navSolPeriod after the latest first subframe, max_meas at the most.  Lane 0 writes
// the count; the rows this lane writes.
struct FixRows {
  int64_t n_meas;
  const char* my_abs;
  gnsscorr_gps_fix_chan* my_chan;
  gnsscorr_gps_fix_sol* my_sol;
};
__device__ __forceinline__ FixRows fix_rows(const FixLane& l, int fs, int n_ready, int max_meas,
                                            int n_epochs, int nav_sol_period,
                                            const char* abs_sample, int64_t chan_stride,
                                            int32_t* __restrict__ n_meas_out,
                                            gnsscorr_gps_fix_sol* sol,
                                            gnsscorr_gps_fix_chan* chan) {
  const int rx = blockIdx.x;
  const int p_max = wave_max(fs);
  int64_t n_meas = 0;
  if (n_ready >= 4)
    n_meas = min((int64_t)max_meas, ((int64_t)n_epochs - (p_max + 1)) / nav_sol_period);
  if (n_meas < 0) n_meas = 0;
  if (threadIdx.x == 0) n_meas_out[rx] = (int32_t)n_meas;
  FixRows r;
  r.n_meas = n_meas;
  r.my_abs = abs_sample + (int64_t)l.ch * chan_stride;
  r.my_chan = chan + (int64_t)l.ch * max_meas;
  r.my_sol = sol + (int64_t)rx * max_meas;
  return r;
}

// calculatePseudoranges.sci: the channel's absoluteSample at measurement m in code periods,
// and a travel time less the whole code periods of the wave's earliest arrival (+inf on the
// lanes that take no part).  The caller scales and offsets as its file does.
__device__ __forceinline__ double code_periods(const char* my_abs, int fs, int nav_sol_period,
                                               int m, int64_t epoch_stride,
                                               double samples_per_code) {
  return *(const double*)(my_abs + ((int64_t)fs + (int64_t)nav_sol_period * m) * epoch_stride) /
         samples_per_code;
}
__device__ __forceinline__ double since_earliest(double travel) {
  return travel - floor(wave_min(travel));
}

// leastSquarePos.sci with e_r_corr.sci, topocent.sci, togeod.sci and tropo.sci: seven
// iterations from the origin.  s*: this lane's satellite; obs: its corrected pseudorange.
// Returns GNSSCORR_GPS_FIX_OK with the position and clock in pos, the factorisation of the
// last normal matrix in f and this lane's angles in degrees (NaN off the active set), or
// GNSSCORR_GPS_FIX_RANK (the library's rank rule) with pos zero and the angles NaN.
template <Fix F>
__device__ int least_squares(double sx, double sy, double sz, double obs, bool active, double c,
                             int use_trop, const Tropo& tr, double (&pos)[4], Ldl& f,
                             double& el, double& az) {
  const double nan = quiet_nan(), dtr = kPi / 180;
  int status = GNSSCORR_GPS_FIX_OK;
  pos[0] = pos[1] = pos[2] = pos[3] = 0;
  el = az = nan;
  for (int iter = 0; iter < 7; iter++) {
    double r0 = sx, r1 = sy, r2 = sz, trop = F == Fix::kGps ? 2 : 0;
    if (iter > 0) {
      const double rho2 = (sx - pos[0]) * (sx - pos[0]) + (sy - pos[1]) * (sy - pos[1]) +
                          (sz - pos[2]) * (sz - pos[2]);
      const double omegatau = 7.292115147e-5 * (sqrt(rho2) / c);       // e_r_corr.sci
      const double co = cos(omegatau), so = sin(omegatau);
      r0 = co * sx + so * sy;
      r1 = -so * sx + co * sy;
      double phi, lambda;                                      // topocent.sci
      togeod<F>(pos[0], pos[1], pos[2], &phi, &lambda);
      const double cl = cos(lambda * dtr), sl = sin(lambda * dtr);
      const double cb = cos(phi * dtr), sb = sin(phi * dtr);
      const double d0 = r0 - pos[0], d1 = r1 - pos[1], d2 = r2 - pos[2];
      const double E = -sl * d0 + cl * d1 + 0 * d2;
      const double Nn = -sb * cl * d0 + -sb * sl * d1 + cb * d2;
      const double U = cb * cl * d0 + cb * sl * d1 + sb * d2;
      const double hor_dis = sqrt(E * E + Nn * Nn);
      if (hor_dis < 1.e-20) {
        az = 0;
        el = 90;
      } else {
        az = atan_yx<F>(E, Nn) / dtr;
        el = atan_yx<F>(U, hor_dis) / dtr;
      }
      if (az < 0) az = az + 360;
      trop = 0;
      if (use_trop == 1) {                                     // tropo.sci
        double sinel = sin(el * dtr);
        if (sinel < 0) sinel = 0;
        trop = 0 + tropo_pass(sinel, tr.htop[0], tr.ref[0]);
        trop = trop + tropo_pass(sinel, tr.htop[1], tr.ref[1]);
      }
    }
    const double d0 = r0 - pos[0], d1 = r1 - pos[1], d2 = r2 - pos[2];
    const double range = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
    double omc, div;
    if constexpr (F == Fix::kGps) {
      omc = active ? obs - range - pos[3] - trop : 0.0;
      div = obs;
    } else {
      omc = active ? obs - pos[3] - range - trop : 0.0;
      div = range;
    }
    const double a0 = active ? -d0 / div : 0.0;
    const double a1 = active ? -d1 / div : 0.0;
    const double a2 = active ? -d2 / div : 0.0;
    const double a3 = active ? 1.0 : 0.0;
    double N[10];
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
    if (!ldl_factor(N, &f)) {
      status = GNSSCORR_GPS_FIX_RANK;
      break;
    }
    double x[4];
    ldl_solve(f, g0, g1, g2, g3, x);
    pos[0] = pos[0] + x[0];
    pos[1] = pos[1] + x[1];
    pos[2] = pos[2] + x[2];
    pos[3] = pos[3] + x[3];
  }
  if (status == GNSSCORR_GPS_FIX_RANK) {
    pos[0] = pos[1] = pos[2] = pos[3] = 0;
    el = az = nan;
  } else if (!active) {
    el = az = nan;
  }
  return status;
}

// leastSquarePos.sci: GDOP, PDOP, HDOP, VDOP, TDOP from the diagonal of inv(A'A)
__device__ __forceinline__ void dop_from(const Ldl& f, double (&dop)[5]) {
  double q[4];
  ldl_solve(f, 1, 0, 0, 0, q);
  const double Q00 = q[0];
  ldl_solve(f, 0, 1, 0, 0, q);
  const double Q11 = q[1];
  ldl_solve(f, 0, 0, 1, 0, q);
  const double Q22 = q[2];
  ldl_solve(f, 0, 0, 0, 1, q);
  const double Q33 = q[3];
  dop[0] = sqrt(Q00 + Q11 + Q22 + Q33);
  dop[1] = sqrt(Q00 + Q11 + Q22);
  dop[2] = sqrt(Q00 + Q11);
  dop[3] = sqrt(Q22);
  dop[4] = sqrt(Q33);
}

// one measurement's rows: every valid lane its channel's, lane 0 the receiver's
__device__ __forceinline__ void write_fix_records(
    bool valid, gnsscorr_gps_fix_chan* my_chan, gnsscorr_gps_fix_sol* my_sol, double el,
    double az, double raw_p, double corr_p, bool used, const double (&pos)[4],
    const double (&dop)[5], double lat, double lon, double height, int status, int n_used) {
  if (valid) {
    gnsscorr_gps_fix_chan o;
    o.el = el;
    o.az = az;
    o.rawP = raw_p;
    o.corrP = corr_p;
    o.used = used;
    o.reserved = 0;
    *my_chan = o;
  }
  if (threadIdx.x == 0) {
    gnsscorr_gps_fix_sol o;
    o.X = pos[0];
    o.Y = pos[1];
    o.Z = pos[2];
    o.dt = pos[3];
    for (int k = 0; k < 5; k++) o.DOP[k] = dop[k];
    o.lat = lat;
    o.lon = lon;
    o.height = height;
    o.status = status;
    o.n_used = n_used;
    *my_sol = o;
  }
}

}  // namespace navdev
#endif
