// navb1.hip -- the BeiDou B1I receiver after the data bits, on the device ("nav"):
// ephemeris fields and SOW from the five deinterleaved subframes of
// gnsscorr_nav_b1_subframes, then the measurement loop: pseudoranges, Kepler satellite
// positions, least-squares position.
//   COMPASS/B1/include/ephemeris.sci:28-123
//   COMPASS/B1/postNavigation.sci:129-272, calculatePseudoranges.sci
//   COMPASS/B1/geoFunctions/satpos.sci:45-137, check_t.sci, leastSquarePos.sci,
//   e_r_corr.sci, topocent.sci, togeod.sci, tropo.sci, cart2geo.sci
// The whole file is compiled without contraction: the field values and the raw
// pseudoranges are bit-exact.
//
// nav_b1_eph_kernel: one wave per channel.  The 1065 values go to LDS once; lanes 0..4 each
// look one slot over for a 2 and leave its subframe ID in LDS; lane f < 35 owns field f of
// the table below and walks the slots in order, so a later slot with the same ID overwrites
// an earlier one.
//
// nav_b1_fix_kernel: one wave64 per receiver, lane = channel, the measurement loop inside
// the kernel, as nav_gps_fix_kernel (navfix.hip) and nav_glo_fix_kernel (navglo.hip).  The
// satellite position is the GPS file's Kepler propagation with BeiDou's constants and field
// names, so sat_pos is written out here; the least squares is the GLONASS file's.  There is
// no elevation mask: the set of used channels is fixed for the whole call.
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

constexpr int kB1Slots = 5, kB1SlotBits = 213;
constexpr int kB1Bits = kB1Slots * kB1SlotBits;
constexpr double kBdPi = 3.1415926535898;              // ephemeris.sci:25, satpos.sci:30
constexpr int kEphDoubles = 31, kEphInts = 8;

// ---------------------------------------------------------------------------
// ephemeris.sci:45-107.  Bit positions are the file's (1-based, inside decoded_sbfrm).
// ---------------------------------------------------------------------------
enum : uint8_t { kPlain = 0, kTimesPi = 1, kTgd = 2, kInt = 3 };
struct B1Field {
  uint8_t sf;              // subframe ID that carries it
  uint8_t s, n;            // first bit and length
  uint8_t sgn;             // the file subtracts bit(sgn) * 2^n (0: nothing)
  int8_t exp2;             // * 2^exp2
  uint8_t kind;            // then * BDPi; T_GD_1's * 0.1 * 1e-9; an int32 field
  uint8_t idx;             // index among the doubles / among the int32s
};
constexpr int kB1Fields = 35;
__constant__ B1Field kB1[kB1Fields] = {
    // subframe 1 (:45-74)
    {1, 28, 1, 0, 0, kInt, 0},                                 // SatH1
    {1, 29, 5, 0, 0, kInt, 1},                                 // IODC
    {1, 34, 4, 0, 0, kInt, 2},                                 // URAI
    {1, 38, 13, 0, 0, kInt, 3},                                // WN
    {1, 51, 17, 0, 3, kPlain, 1},                              // t_oc
    {1, 68, 10, 68, 0, kTgd, 0},                               // T_GD_1
    {1, 88, 8, 88, -30, kPlain, 5},                            // alpha0
    {1, 96, 8, 96, -27, kPlain, 6},                            // alpha1
    {1, 104, 8, 104, -24, kPlain, 7},                          // alpha2
    {1, 112, 8, 88, -24, kPlain, 8},                           // alpha3: bit 88, as the file
    {1, 120, 8, 120, 11, kPlain, 9},                           // beta0
    {1, 128, 8, 120, 14, kPlain, 10},                          // beta1: bit 120, as the file
    {1, 136, 8, 136, 16, kPlain, 11},                          // beta2
    {1, 144, 8, 144, 16, kPlain, 12},                          // beta3
    {1, 152, 11, 152, -66, kPlain, 2},                         // a2
    {1, 163, 24, 163, -33, kPlain, 3},                         // a0
    {1, 187, 22, 187, -50, kPlain, 4},                         // a1
    {1, 209, 5, 0, 0, kInt, 4},                                // IODE
    // subframe 2 (:76-91)
    {2, 28, 16, 28, -43, kTimesPi, 13},                        // deltan
    {2, 44, 18, 44, -31, kPlain, 14},                          // C_uc
    {2, 62, 32, 62, -31, kTimesPi, 15},                        // M_0
    {2, 94, 32, 94, -33, kPlain, 16},                          // e: signed, as the file
    {2, 126, 18, 126, -31, kPlain, 17},                        // C_us
    {2, 144, 18, 144, -6, kPlain, 18},                         // C_rc
    {2, 162, 18, 162, -6, kPlain, 19},                         // C_rs
    {2, 180, 32, 0, -19, kPlain, 20},                          // sqrtA: unsigned
    {2, 212, 2, 0, 18, kPlain, 21},                            // t_oe_msb: * 2^15 * 2^3
    // subframe 3 (:93-107)
    {3, 28, 15, 0, 3, kPlain, 22},                             // t_oe_lsb
    {3, 43, 32, 43, -31, kTimesPi, 23},                        // i_0
    {3, 75, 18, 75, -31, kPlain, 24},                          // C_ic
    {3, 93, 24, 93, -43, kTimesPi, 25},                        // omegaDot
    {3, 117, 18, 117, -31, kPlain, 26},                        // C_is
    {3, 135, 14, 135, -43, kTimesPi, 27},                      // iDot
    {3, 149, 32, 149, -31, kTimesPi, 28},                      // omega_0
    {3, 181, 32, 181, -31, kTimesPi, 29},                      // omega
};
static_assert(sizeof(gnsscorr_b1_eph) == kEphDoubles * 8 + kEphInts * 4, "gnsscorr_b1_eph");
static_assert(offsetof(gnsscorr_b1_eph, t_oe) == 30 * 8, "gnsscorr_b1_eph layout");
static_assert(offsetof(gnsscorr_b1_eph, SatH1) == kEphDoubles * 8, "gnsscorr_b1_eph layout");
static_assert(offsetof(gnsscorr_b1_eph, status) == kEphDoubles * 8 + 7 * 4, "gnsscorr_b1_eph");

// the unsigned value of n values from 1-based position s of a slot (bin2dec)
__device__ __forceinline__ uint64_t bits_value(const uint8_t* sub, int s, int n) {
  uint64_t v = 0;
  for (int i = 0; i < n; i++) v = v << 1 | sub[s - 1 + i];
  return v;
}

__global__ __launch_bounds__(64) void nav_b1_eph_kernel(
    const uint8_t* __restrict__ bits, const int32_t* __restrict__ n_subframes,
    const int32_t* __restrict__ first, gnsscorr_b1_eph* __restrict__ eph) {
  __shared__ uint8_t b[kB1Bits];
  __shared__ int8_t s_id[kB1Slots];                            // -1: skipped or short
  const int ch = blockIdx.x, lane = threadIdx.x;
  const uint8_t* in = bits + (int64_t)ch * kB1Bits;
  double* out_d = (double*)(eph + ch);
  int32_t* out_i = (int32_t*)(out_d + kEphDoubles);
  const bool is_short = n_subframes[ch] < kB1Slots || first[ch] < 0;
  if (!is_short)
    for (int i = lane; i < kB1Bits; i += 64) b[i] = in[i];
  __syncthreads();
  if (lane < kB1Slots) {                                       // :36-41
    int id = -1;
    if (!is_short) {
      const uint8_t* sub = b + kB1SlotBits * lane;
      bool skip = false;
      for (int k = 0; k < kB1SlotBits; k++) skip |= sub[k] > 1;
      if (!skip) id = (int)bits_value(sub, 5, 3);
    }
    s_id[lane] = (int8_t)id;
  }
  __syncthreads();
  int have = 0;
  for (int i = 0; i < kB1Slots; i++) {
    const int id = s_id[i];
    if (id >= 1 && id <= 3) have |= 1 << (id - 1);
  }
  if (lane < kB1Fields) {
    const B1Field f = kB1[lane];
    double vd = 0.0;
    int32_t vi = 0;
    for (int i = 0; i < kB1Slots; i++) {
      if (s_id[i] != f.sf) continue;
      const uint8_t* sub = b + kB1SlotBits * i;
      int64_t v = (int64_t)bits_value(sub, f.s, f.n);
      if (f.sgn) v -= (int64_t)sub[f.sgn - 1] << f.n;
      if (f.kind == kInt) {
        vi = (int32_t)v;
      } else if (f.kind == kTgd) {                             // :50-51
        vd = (double)v * 0.1 * 1e-9;
      } else {
        vd = (double)v * ldexp(1.0, f.exp2);
        if (f.kind == kTimesPi) vd = vd * kBdPi;
      }
    }
    if (f.kind == kInt) out_i[f.idx] = vi;
    else out_d[f.idx] = vd;
  } else if (lane == kB1Fields) {                              // :118
    double t_oe = 0.0;
    if ((have & 6) == 6) {
      double msb = 0.0, lsb = 0.0;
      for (int i = 0; i < kB1Slots; i++) {
        const uint8_t* sub = b + kB1SlotBits * i;
        if (s_id[i] == 2) msb = (double)bits_value(sub, 212, 2) * ldexp(1.0, 18);
        if (s_id[i] == 3) lsb = (double)bits_value(sub, 28, 15) * ldexp(1.0, 3);
      }
      t_oe = msb + lsb;
    }
    out_d[30] = t_oe;
  } else if (lane == kB1Fields + 1) {                          // :123, the fifth slot
    int sow = 0, status = is_short ? GNSSCORR_B1_EPH_SHORT : GNSSCORR_B1_EPH_OK;
    if (!is_short) {
      const uint8_t* sub = b + kB1SlotBits * 4;
      bool undecided = false;
      for (int k = 8; k <= 27; k++) undecided |= sub[k - 1] > 1;
      if (undecided) status = GNSSCORR_B1_EPH_NO_SOW;
      else sow = (int)bits_value(sub, 8, 20) - 24;
    }
    out_i[5] = sow;
    out_i[6] = have;
    out_i[7] = status;
  }
}

// ---------------------------------------------------------------------------
// the measurement loop
// ---------------------------------------------------------------------------
struct B1FixArgs {
  double samples_per_code, data_size, c;
  int nav_sol_period, use_trop, max_meas, n_epochs;
  double htop[2], ref[2];        // navdev::tropo_consts
};

struct SatPos { double x, y, z, clk; };

// satpos.sci:53-136 for one satellite
__device__ SatPos sat_pos(const gnsscorr_b1_eph& e, double transmit_time) {
  const double Omegae_dot = 7.2921150e-5, GM = 3.986004418e14, F = -4.442807633e-10;
  const double two_pi = 2 * kBdPi;
  const double dt = check_t(transmit_time - e.t_oc);
  const double clk0 = ((e.a2 * dt + e.a1) * dt + e.a0) - e.T_GD_1;
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
  s.clk = ((e.a2 * dt + e.a1) * dt + e.a0) - e.T_GD_1 + dtr;
  return s;
}

__global__ __launch_bounds__(64) void nav_b1_fix_kernel(
    const gnsscorr_b1_eph* __restrict__ eph, const int32_t* __restrict__ first,
    const char* __restrict__ abs_sample, int64_t epoch_stride, int64_t chan_stride,
    const int32_t* __restrict__ rx_first, B1FixArgs p, int32_t* __restrict__ n_meas_out,
    gnsscorr_gps_fix_sol* __restrict__ sol, gnsscorr_gps_fix_chan* __restrict__ chan) {
  const int rx = blockIdx.x, lane = threadIdx.x;
  const int c0 = rx_first[rx], n_ch = rx_first[rx + 1] - c0;
  const bool valid = lane < n_ch;
  const int ch = c0 + (valid ? lane : 0);
  const gnsscorr_b1_eph e = eph[ch];                           // once, into registers
  const int fs = valid ? first[ch] : -1;
  // postNavigation.sci:117-118 are disabled in the file; the library drops these channels
  const bool used = valid && fs >= 0 && e.status == GNSSCORR_B1_EPH_OK && e.have == 7;
  const uint64_t used_set = __ballot(used);
  const int n_used = __popcll(used_set);
  const int p_max = wave_max(fs);
  int64_t n_meas = 0;
  if (n_used >= 4)                                             // :121, :152
    n_meas = min((int64_t)p.max_meas, ((int64_t)p.n_epochs - (p_max + 1)) / p.nav_sol_period);
  if (n_meas < 0) n_meas = 0;
  if (lane == 0) n_meas_out[rx] = (int32_t)n_meas;
  if (n_meas == 0) return;

  double transmit_time = (double)__shfl(e.SOW, __ffsll((long long)used_set) - 1);   // :145
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  const double dtr = kPi / 180;
  const char* my_abs = abs_sample + (int64_t)ch * chan_stride;
  gnsscorr_gps_fix_chan* my_chan = chan + (int64_t)ch * p.max_meas;
  gnsscorr_gps_fix_sol* my_sol = sol + (int64_t)rx * p.max_meas;

  for (int m = 0; m < (int)n_meas; m++) {
    double el = nan, az_deg = nan;                             // :165-166

    // calculatePseudoranges.sci
    double travel = inf;
    if (used)
      travel = *(const double*)(my_abs + ((int64_t)fs + (int64_t)p.nav_sol_period * m) *
                                             epoch_stride) / p.samples_per_code / p.data_size;
    const double minimum = floor(wave_min(travel));
    const double raw_p = (travel - minimum) * (p.c / 1000);

    SatPos s = {0, 0, 0, 0};                                   // :175-177
    if (used) s = sat_pos(e, transmit_time);
    const double obs = raw_p + s.clk * p.c;                    // :187-188

    // leastSquarePos.sci, the GLONASS L1 text
    int status = GNSSCORR_GPS_FIX_OK;
    double pos0 = 0, pos1 = 0, pos2 = 0, pos3 = 0;
    double dop[5] = {0, 0, 0, 0, 0};
    double lat = 0, lon = 0, height = 0, corr_p = 0.0;
    double N[10];
    Ldl f;
    for (int iter = 0; iter < 7; iter++) {
      double r0 = s.x, r1 = s.y, r2 = s.z, trop = 0;
      if (iter > 0) {
        const double rho2 = (s.x - pos0) * (s.x - pos0) + (s.y - pos1) * (s.y - pos1) +
                            (s.z - pos2) * (s.z - pos2);
        const double omegatau = 7.292115147e-5 * (sqrt(rho2) / p.c);   // e_r_corr.sci
        const double co = cos(omegatau), so = sin(omegatau);
        r0 = co * s.x + so * s.y;
        r1 = -so * s.x + co * s.y;
        double phi, lambda;                                    // topocent.sci
        togeod_atan(pos0, pos1, pos2, &phi, &lambda);
        const double cl = cos(lambda * dtr), sl = sin(lambda * dtr);
        const double cb = cos(phi * dtr), sb = sin(phi * dtr);
        const double d0 = r0 - pos0, d1 = r1 - pos1, d2 = r2 - pos2;
        const double E = -sl * d0 + cl * d1 + 0 * d2;
        const double Nn = -sb * cl * d0 + -sb * sl * d1 + cb * d2;
        const double U = cb * cl * d0 + cb * sl * d1 + sb * d2;
        const double hor_dis = sqrt(E * E + Nn * Nn);
        if (hor_dis < 1.e-20) {
          az_deg = 0;
          el = 90;
        } else {
          az_deg = atan2(E, Nn) / dtr;
          el = atan2(U, hor_dis) / dtr;
        }
        if (az_deg < 0) az_deg = az_deg + 360;
        if (p.use_trop == 1) {                                 // tropo.sci
          double sinel = sin(el * dtr);
          if (sinel < 0) sinel = 0;
          trop = 0 + tropo_pass(sinel, p.htop[0], p.ref[0]);
          trop = trop + tropo_pass(sinel, p.htop[1], p.ref[1]);
        }
      }
      const double d0 = r0 - pos0, d1 = r1 - pos1, d2 = r2 - pos2;
      const double dist = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
      const double F = used ? obs - pos3 - dist - trop : 0.0;
      const double a0 = used ? -d0 / dist : 0.0;
      const double a1 = used ? -d1 / dist : 0.0;
      const double a2 = used ? -d2 / dist : 0.0;
      const double a3 = used ? 1.0 : 0.0;
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
      const double g0 = wave_sum(a0 * F), g1 = wave_sum(a1 * F);
      const double g2 = wave_sum(a2 * F), g3 = wave_sum(a3 * F);
      if (!ldl_factor(N, &f)) {                                // the library's rank rule
        status = GNSSCORR_GPS_FIX_RANK;
        break;
      }
      double x[4];
      ldl_solve(f, g0, g1, g2, g3, x);
      pos0 = pos0 + x[0];
      pos1 = pos1 + x[1];
      pos2 = pos2 + x[2];
      pos3 = pos3 + x[3];
    }
    if (status == GNSSCORR_GPS_FIX_RANK) {
      pos0 = pos1 = pos2 = pos3 = 0;
      el = az_deg = nan;
    } else {
      double q[4], Q00, Q11, Q22, Q33;
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
      if (!used) el = az_deg = nan;
      if (used) corr_p = raw_p - s.clk * p.c + pos3;           // postNavigation.sci:212-214
      cart2geo5_atan(pos0, pos1, pos2, &lat, &lon, &height);   // :219-225
    }
    if (valid) {
      gnsscorr_gps_fix_chan o;
      o.el = el;
      o.az = az_deg;
      o.rawP = raw_p;
      o.corrP = corr_p;
      o.used = used;
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
      o.n_used = n_used;
      my_sol[m] = o;
    }
    transmit_time = transmit_time + (double)p.nav_sol_period / 1000;   // :270
  }
}

}  // namespace

// ============================================================================
// host side
// ============================================================================
using navhost::bad_arguments;
using navhost::check_series;
using navhost::series_bytes;

extern "C" void gnsscorr_nav_b1_fix_cfg_init(gnsscorr_b1_fix_cfg* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof *cfg);
  cfg->samplesPerCode = 16000.0;      // initSettings.sci:71-75: 16e6 / (2.046e6 / 2046)
  cfg->dataTypeSizeInBytes = 1.0;     // :59
  cfg->c = 299792458.0;               // :129
  cfg->navSolPeriod = 500;            // :109
  cfg->useTropCorr = 0;               // :114
  cfg->max_meas = 1;
}

static int check_eph(const char* fn, const gnsscorr_nav_ctx* c, const void* bits,
                     const void* n_subframes, const void* first, int n_ch, const void* eph) {
  if (!c || !bits || !n_subframes || !first || !eph) return bad_arguments(fn, "null pointer");
  if (n_ch < 1) return bad_arguments(fn, "n_ch >= 1");
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_b1_ephemeris_dev(gnsscorr_nav_ctx* c, const uint8_t* d_bits,
                                             const int32_t* d_n_subframes,
                                             const int32_t* d_first, int n_ch,
                                             gnsscorr_b1_eph* d_eph) {
  int rc = check_eph(__func__, c, d_bits, d_n_subframes, d_first, n_ch, d_eph);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  hipLaunchKernelGGL(nav_b1_eph_kernel, dim3(n_ch), dim3(64), 0, c->stream, d_bits,
                     d_n_subframes, d_first, d_eph);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_b1_ephemeris(gnsscorr_nav_ctx* c, const uint8_t* h_bits,
                                         const int32_t* h_n_subframes, const int32_t* h_first,
                                         int n_ch, gnsscorr_b1_eph* h_eph) {
  int rc = check_eph(__func__, c, h_bits, h_n_subframes, h_first, n_ch, h_eph);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  const size_t n = (size_t)n_ch;
  hostctx::Staging st(c->stream);
  const uint8_t* d_bits = st.in(h_bits, n * kB1Bits);
  const int32_t* d_n_subframes = st.in(h_n_subframes, n);
  const int32_t* d_first = st.in(h_first, n);
  gnsscorr_b1_eph* d_eph = st.out(h_eph, n);
  if (st.status()) return st.status();
  rc = gnsscorr_nav_b1_ephemeris_dev(c, d_bits, d_n_subframes, d_first, n_ch, d_eph);
  return rc ? rc : st.finish();
}

static int check_fix(const char* fn, const gnsscorr_nav_ctx* c, const void* eph,
                     const void* first, const void* abs_sample, int64_t epoch_stride,
                     int64_t chan_stride, int n_epochs, int n_rx, const int32_t* rx_first,
                     const gnsscorr_b1_fix_cfg* cfg, const void* n_meas, const void* sol,
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
  if (!(cfg->dataTypeSizeInBytes > 0)) return bad_arguments(fn, "dataTypeSizeInBytes > 0");
  if (cfg->max_meas < 1) return bad_arguments(fn, "max_meas >= 1");
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_b1_fix_dev(gnsscorr_nav_ctx* c, const gnsscorr_b1_eph* d_eph,
                                       const int32_t* d_first, const void* d_abs_sample,
                                       int64_t epoch_stride_bytes, int64_t chan_stride_bytes,
                                       int n_epochs, int n_rx, const int32_t* rx_first,
                                       const gnsscorr_b1_fix_cfg* cfg, int32_t* d_n_meas,
                                       gnsscorr_gps_fix_sol* d_sol,
                                       gnsscorr_gps_fix_chan* d_chan) {
  int rc = check_fix(__func__, c, d_eph, d_first, d_abs_sample, epoch_stride_bytes,
                     chan_stride_bytes, n_epochs, n_rx, rx_first, cfg, d_n_meas, d_sol, d_chan);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  rc = hostctx::grow(c->d_rx_first, (size_t)n_rx + 1);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->d_rx_first.p, rx_first, ((size_t)n_rx + 1) * sizeof(int32_t),
                         hipMemcpyHostToDevice, c->stream));
  B1FixArgs p;
  p.samples_per_code = cfg->samplesPerCode;
  p.data_size = cfg->dataTypeSizeInBytes;
  p.c = cfg->c;
  p.nav_sol_period = cfg->navSolPeriod;
  p.use_trop = cfg->useTropCorr;
  p.max_meas = cfg->max_meas;
  p.n_epochs = n_epochs;
  navdev::tropo_consts(p.htop, p.ref);
  hipLaunchKernelGGL(nav_b1_fix_kernel, dim3(n_rx), dim3(64), 0, c->stream, d_eph, d_first,
                     (const char*)d_abs_sample, epoch_stride_bytes, chan_stride_bytes,
                     c->d_rx_first.p, p, d_n_meas, d_sol, d_chan);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_b1_fix(gnsscorr_nav_ctx* c, const gnsscorr_b1_eph* h_eph,
                                   const int32_t* h_first, const void* h_abs_sample,
                                   int64_t epoch_stride_bytes, int64_t chan_stride_bytes,
                                   int n_epochs, int n_rx, const int32_t* rx_first,
                                   const gnsscorr_b1_fix_cfg* cfg, int32_t* h_n_meas,
                                   gnsscorr_gps_fix_sol* h_sol, gnsscorr_gps_fix_chan* h_chan) {
  int rc = check_fix(__func__, c, h_eph, h_first, h_abs_sample, epoch_stride_bytes,
                     chan_stride_bytes, n_epochs, n_rx, rx_first, cfg, h_n_meas, h_sol, h_chan);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  const size_t n_ch = (size_t)rx_first[n_rx], mm = (size_t)cfg->max_meas;
  const size_t n_in = series_bytes(epoch_stride_bytes, chan_stride_bytes, n_epochs, (int)n_ch);
  hostctx::Staging st(c->stream);
  const gnsscorr_b1_eph* d_eph = st.in(h_eph, n_ch);
  const int32_t* d_first = st.in(h_first, n_ch);
  int32_t* d_n_meas = st.out(h_n_meas, (size_t)n_rx);
  const char* d_abs_sample = st.in((const char*)h_abs_sample, n_in);
  // uploaded too: rows past n_meas stay as the caller has them
  gnsscorr_gps_fix_sol* d_sol = st.inout(h_sol, (size_t)n_rx * mm);
  gnsscorr_gps_fix_chan* d_chan = st.inout(h_chan, n_ch * mm);
  if (st.status()) return st.status();
  rc = gnsscorr_nav_b1_fix_dev(c, d_eph, d_first, d_abs_sample, epoch_stride_bytes,
                               chan_stride_bytes, n_epochs, n_rx, rx_first, cfg, d_n_meas, d_sol,
                               d_chan);
  return rc ? rc : st.finish();
}
