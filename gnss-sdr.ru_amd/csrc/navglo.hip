// navglo.hip -- the GLONASS L1OF receiver after the data bits, on the device ("nav"):
// ephemeris fields and frame time from the 15 strings of gnsscorr_nav_glo_strings, the
// satellite state at the first measurement by Runge-Kutta integration from t_b, then the
// measurement loop: pseudoranges, one integration step per fix, least-squares position,
// PZ-90.02 -> WGS-84.
//   GLONASS/L1/include/ephemeris.sci:25-98
//   GLONASS/L1/postNavigation.sci:89-123,142-284, calculatePseudoranges.sci:55-72
//   GLONASS/L1/geoFunctions/satposg.sci:38-132,299-310, deltasatposg.sci:66-137,
//   leastSquarePos.sci:45-100, e_r_corr.sci:20-31, topocent.sci:22-54, togeod.sci:31-110,
//   tropo.sci:32-95, cart2geo.sci:20-45
// The file is compiled without contraction: the field values, the frame time, deltat, the
// three loop counts, the clock term and the raw pseudoranges are bit-exact.  Only the body of
// the Runge-Kutta step (rk4_step) lets the compiler contract.
//
// nav_glo_eph_kernel: one wave per channel.  The 1275 bits go to LDS once; lanes 0..14 each
// look one string over for an undecided bit and leave its number in LDS, lane f < 33 owns field f of
// the table below and walks the strings in order, so a later string with the same number
// overwrites an earlier one.
//
// nav_glo_satpos_kernel: one lane per channel over all channels of all receivers, 64-lane
// blocks.  Sequential fp64 work per satellite: up to about 1100 steps of rk4_step (90 of
// 10 s, 9 of 1 s, 999 of 1 ms for a frame 15 minutes from t_b).  One loop over the three step
// sizes, so the step's code is there once.
//
// nav_glo_fix_kernel: one wave64 per receiver, lane = channel, the measurement loop inside
// the kernel, out of the steps of nav_fix.h with the GLONASS/L1 text of the least squares
// (Fix::kGloB1).  Every lane keeps and advances its own satellite state; the solution goes
// from PZ-90.02 to WGS-84 before it is written.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "gnsscorr_internal.h"
#include "hostctx.h"
#include "nav_host.h"

#pragma clang fp contract(off)
#include "nav_fix.h"

namespace {

using namespace navdev;

constexpr int kGloStrings = 15, kGloStringBits = 85;
constexpr int kGloBits = kGloStrings * kGloStringBits;
constexpr int kEphDoubles = 15, kEphInts = 24;

// ---------------------------------------------------------------------------
// ephemeris.sci:47-91.  decoded_str(hi:-1:lo), 1-based: the bit at hi is the MSB.
// ---------------------------------------------------------------------------
struct GloField {
  uint8_t str;             // string number that carries it
  uint8_t hi, lo;
  uint8_t sgn;             // position of the (-1)^bit factor (0: none)
  int8_t exp2;             // * 2^exp2
  uint8_t mul;             // an int32 field: * mul
  uint8_t is_int;
  uint8_t idx;             // index among the doubles / among the int32s
};
constexpr int kGloFields = 33;
__constant__ GloField kGlo[kGloFields] = {
    // string 1 (:49-55)
    {1, 78, 77, 0, 0, 1, 1, 0},                                // P1
    {1, 76, 72, 0, 0, 1, 1, 1},                                // tk_h
    {1, 71, 66, 0, 0, 1, 1, 2},                                // tk_m
    {1, 65, 65, 0, 0, 30, 1, 3},                               // tk_s
    {1, 63, 41, 64, -20, 0, 0, 3},                             // xdot
    {1, 39, 36, 40, -30, 0, 0, 6},                             // xdotdot
    {1, 34, 9, 35, -11, 0, 0, 0},                              // x
    // string 2 (:60-65)
    {2, 80, 80, 0, 0, 4, 1, 4},                                // Bn
    {2, 65, 65, 0, 0, 1, 1, 5},                                // P2
    {2, 76, 70, 0, 0, 15, 1, 6},                               // tb
    {2, 63, 41, 64, -20, 0, 0, 4},                             // ydot
    {2, 39, 36, 40, -30, 0, 0, 7},                             // ydotdot
    {2, 34, 9, 35, -11, 0, 0, 1},                              // y
    // string 3 (:68-74)
    {3, 80, 80, 0, 0, 1, 1, 7},                                // P3
    {3, 78, 69, 79, -40, 0, 0, 9},                             // gamman
    {3, 67, 66, 0, 0, 1, 1, 8},                                // P
    {3, 65, 65, 0, 0, 1, 1, 9},                                // In3
    {3, 63, 41, 64, -20, 0, 0, 5},                             // zdot
    {3, 39, 36, 40, -30, 0, 0, 8},                             // zdotdot
    {3, 34, 9, 35, -11, 0, 0, 2},                              // z
    // string 4 (:77-84)
    {4, 79, 59, 80, -30, 0, 0, 10},                            // taun
    {4, 57, 54, 58, -30, 0, 0, 11},                            // deltataun
    {4, 53, 49, 0, 0, 1, 1, 10},                               // En
    {4, 34, 34, 0, 0, 1, 1, 11},                               // P4
    {4, 33, 30, 0, 0, 1, 1, 12},                               // Ft
    {4, 26, 16, 0, 0, 1, 1, 13},                               // Nt
    {4, 15, 11, 0, 0, 1, 1, 14},                               // n
    {4, 10, 9, 0, 0, 1, 1, 15},                                // M
    // string 5 (:86-90)
    {5, 80, 70, 0, 0, 1, 1, 16},                               // NA
    {5, 68, 38, 69, -31, 0, 0, 12},                            // tauc
    {5, 36, 32, 0, 0, 1, 1, 17},                               // N4
    {5, 30, 10, 31, -30, 0, 0, 13},                            // tauGPS
    {5, 9, 9, 0, 0, 1, 1, 18},                                 // In5
};
static_assert(sizeof(gnsscorr_glo_eph) == kEphDoubles * 8 + kEphInts * 4, "gnsscorr_glo_eph");
static_assert(offsetof(gnsscorr_glo_eph, P1) == kEphDoubles * 8, "gnsscorr_glo_eph layout");
static_assert(offsetof(gnsscorr_glo_eph, status) == kEphDoubles * 8 + 22 * 4, "gnsscorr_glo_eph");
static_assert(sizeof(gnsscorr_glo_sat) == 11 * 8 + 4 * 4, "gnsscorr_glo_sat layout");

// bin2dec(decoded_str(hi:-1:lo)) of one string
__device__ __forceinline__ uint32_t str_value(const uint8_t* s, int hi, int lo) {
  uint32_t v = 0;
  for (int k = hi; k >= lo; k--) v = v << 1 | s[k - 1];
  return v;
}

__global__ __launch_bounds__(64) void nav_glo_eph_kernel(
    const uint8_t* __restrict__ bits, const int32_t* __restrict__ n_strings,
    const int32_t* __restrict__ first_mark, gnsscorr_glo_eph* __restrict__ eph) {
  __shared__ uint8_t b[kGloBits];
  __shared__ int8_t s_num[kGloStrings];                        // 0: skipped or short
  __shared__ uint8_t s_skip[kGloStrings];
  const int ch = blockIdx.x, lane = threadIdx.x;
  const uint8_t* in = bits + (int64_t)ch * kGloBits;
  double* out_d = (double*)(eph + ch);
  int32_t* out_i = (int32_t*)(out_d + kEphDoubles);
  const bool is_short = n_strings[ch] < kGloStrings || first_mark[ch] < 0;   // postNavigation.sci:89-93
  if (!is_short)
    for (int i = lane; i < kGloBits; i += 64) b[i] = in[i];
  __syncthreads();
  if (lane < kGloStrings) {                                    // :38-43
    bool skip = false;
    int num = 0;
    if (!is_short) {
      const uint8_t* s = b + kGloStringBits * lane;
      for (int k = 0; k < kGloStringBits; k++) skip |= s[k] > 1;
      if (!skip) num = (int)str_value(s, 84, 81);
    }
    s_num[lane] = (int8_t)num;
    s_skip[lane] = skip;
  }
  __syncthreads();
  int have = 0, string_1_pos = 0;
  uint32_t skipped = 0;
  for (int i = 0; i < kGloStrings; i++) {
    const int n = s_num[i];
    skipped |= (uint32_t)s_skip[i] << i;
    if (n >= 1 && n <= 5) have |= 1 << (n - 1);
    if (n == 1) string_1_pos = i + 1;                          // :56
  }
  if (lane < kGloFields) {
    const GloField f = kGlo[lane];
    double vd = 0.0;
    int32_t vi = 0;
    for (int i = 0; i < kGloStrings; i++) {
      if (s_num[i] != f.str) continue;
      const uint8_t* s = b + kGloStringBits * i;
      const uint32_t u = str_value(s, f.hi, f.lo);
      if (f.is_int) {
        vi = (int32_t)u * f.mul;
      } else {                                                 // u * ((-1)^sign) * (2^exp2)
        vd = (double)u * (s[f.sgn - 1] ? -1.0 : 1.0) * ldexp(1.0, f.exp2);
      }
    }
    if (f.is_int) out_i[f.idx] = vi;
    else out_d[f.idx] = vd;
  } else if (lane == kGloFields) {                             // :95-98
    double t = 0.0;
    if (!is_short) {
      int tk = 0;
      if (string_1_pos) {
        const uint8_t* s = b + kGloStringBits * (string_1_pos - 1);
        tk = (int)str_value(s, 76, 72) * 60 * 60 + (int)str_value(s, 71, 66) * 60 +
             (int)str_value(s, 65, 65) * 30;
      }
      t = (double)(tk - (string_1_pos - 1) * 2) - 0.3;
    }
    out_d[14] = t;
  } else if (lane == kGloFields + 1) {
    out_i[19] = string_1_pos;
    out_i[20] = have;
    out_i[21] = (int32_t)skipped;
    out_i[22] = is_short ? GNSSCORR_GLO_EPH_SHORT : GNSSCORR_GLO_EPH_OK;
    out_i[23] = 0;
  }
}

// ---------------------------------------------------------------------------
// satposg.sci:67-132 = deltasatposg.sci:67-126: one classical Runge-Kutta step of the
// state (position, velocity) in the rotating frame, with r taken once per step as the
// files take it.  r^3 and r^5 come from 1 / r^2 and one more division.
// ---------------------------------------------------------------------------
struct GloState { double x, y, z, vx, vy, vz; };

__device__ __forceinline__ void rk4_step(GloState& w, double ax, double ay, double az, double h) {
#pragma clang fp contract(fast)
  const double mu = 398600.44e9, c20 = -1082.63e-6, ae = 6378.136e3, we = 0.7292115e-4;
  const double r2 = w.x * w.x + w.y * w.y + w.z * w.z;
  const double r = sqrt(r2);
  const double ir2 = 1 / r2, ir3 = ir2 / r;
  const double a = -mu * ir3;                                  // -mu/(r^3)
  const double b = 3.0 / 2 * c20 * mu * (ae * ae) * (ir3 * ir2);   // 3/2*c20*mu*(ae^2)/(r^5)
  const double c5 = 5 * ir2;                                   // 5/(r^2)
  const double we2 = we * we, we_2 = 2 * we;
  auto fx = [&](double x, double z, double vy) {
    return a * x + b * x * (1 - c5 * (z * z)) + we2 * x + we_2 * vy + ax;
  };
  auto fy = [&](double y, double z, double vx) {
    return a * y + b * y * (1 - c5 * (z * z)) + we2 * y - we_2 * vx + ay;
  };
  auto fz = [&](double z) { return a * z + b * z * (3 - c5 * (z * z)) + az; };
  const double k11 = h * w.vx, k12 = h * w.vy, k13 = h * w.vz;
  const double k14 = h * fx(w.x, w.z, w.vy), k15 = h * fy(w.y, w.z, w.vx), k16 = h * fz(w.z);
  const double k21 = h * (w.vx + 0.5 * k14), k22 = h * (w.vy + 0.5 * k15);
  const double k23 = h * (w.vz + 0.5 * k16);
  const double k24 = h * fx(w.x + 0.5 * k11, w.z + 0.5 * k13, w.vy + 0.5 * k15);
  const double k25 = h * fy(w.y + 0.5 * k12, w.z + 0.5 * k13, w.vx + 0.5 * k14);
  const double k26 = h * fz(w.z + 0.5 * k13);
  const double k31 = h * (w.vx + 0.5 * k24), k32 = h * (w.vy + 0.5 * k25);
  const double k33 = h * (w.vz + 0.5 * k26);
  const double k34 = h * fx(w.x + 0.5 * k21, w.z + 0.5 * k23, w.vy + 0.5 * k25);
  const double k35 = h * fy(w.y + 0.5 * k22, w.z + 0.5 * k23, w.vx + 0.5 * k24);
  const double k36 = h * fz(w.z + 0.5 * k23);
  const double k41 = h * (w.vx + k34), k42 = h * (w.vy + k35), k43 = h * (w.vz + k36);
  const double k44 = h * fx(w.x + k31, w.z + k33, w.vy + k35);
  const double k45 = h * fy(w.y + k32, w.z + k33, w.vx + k34);
  const double k46 = h * fz(w.z + k33);
  const double sixth = 1.0 / 6;
  w.x = w.x + sixth * (k11 + 2 * k21 + 2 * k31 + k41);
  w.y = w.y + sixth * (k12 + 2 * k22 + 2 * k32 + k42);
  w.z = w.z + sixth * (k13 + 2 * k23 + 2 * k33 + k43);
  w.vx = w.vx + sixth * (k14 + 2 * k24 + 2 * k34 + k44);
  w.vy = w.vy + sixth * (k15 + 2 * k25 + 2 * k35 + k45);
  w.vz = w.vz + sixth * (k16 + 2 * k26 + 2 * k36 + k46);
}

// |deltat| of a record that stage 1 wrote stays below 1.2e8 ms (tk_h <= 31, tb <= 1905 min);
// a record beyond this bound is not ready, so the loop counts below always fit
constexpr double kMaxDeltat = 134217728.0;                     // 2^27 ms

__global__ __launch_bounds__(64) void nav_glo_satpos_kernel(
    const gnsscorr_glo_eph* __restrict__ eph, int n_ch, double step,
    gnsscorr_glo_sat* __restrict__ sat) {
  const int ch = blockIdx.x * 64 + threadIdx.x;
  if (ch >= n_ch) return;
  const gnsscorr_glo_eph* e = eph + ch;
  gnsscorr_glo_sat o;
  memset(&o, 0, sizeof o);
  // postNavigation.sci:107-123,160 and satposg.sci:38-44: single IEEE operations.  Plain
  // operators under this file's contract(off); the __dmul_rn / __dsub_rn of the HIP headers
  // are inlined with their own contraction permission and fuse into one fma here.
  const double deltat = (e->t - step) * 1000 - (double)e->tb * 60 * 1000;
  const bool ready = e->status == GNSSCORR_GLO_EPH_OK && (e->have & 15) == 15 && e->Bn != 4 &&
                     e->In3 != 1 && fabs(deltat) < kMaxDeltat;
  if (ready) {
    const double deltat10 = trunc(deltat / 10000);
    const double remdeltat10 = deltat - trunc(deltat / 10000) * 10000;
    const double deltat1 = trunc(remdeltat10 / 1000);
    const double deltat001 = remdeltat10 - trunc(remdeltat10 / 1000) * 1000;
    const int n10 = (int)fabs(deltat10), n1 = (int)fabs(deltat1);
    const int n001 = (int)floor(fabs(deltat001));              // 1:abs(x) runs floor(abs(x)) times
    const double sgn = deltat > 0 ? 1.0 : deltat < 0 ? -1.0 : 0.0;
    GloState w = {e->x * 1000, e->y * 1000, e->z * 1000,       // :54-62
                  e->xdot * 1000, e->ydot * 1000, e->zdot * 1000};
    const double ax = e->xdotdot * 1000, ay = e->ydotdot * 1000, az = e->zdotdot * 1000;
    const int total = n10 + n1 + n001;
    for (int i = 0; i < total; i++) {                          // :64,:142,:223
      const double h = (i < n10 ? 10.0 : i < n10 + n1 ? 1.0 : 0.001) * sgn;
      rk4_step(w, ax, ay, az, h);
    }
    o.pos[0] = w.x;
    o.pos[1] = w.y;
    o.pos[2] = w.z;
    o.vel[0] = w.vx;
    o.vel[1] = w.vy;
    o.vel[2] = w.vz;
    o.acc[0] = ax;
    o.acc[1] = ay;
    o.acc[2] = az;
    o.clk = e->taun - e->gamman * (deltat / 1000);             // :310
    o.deltat = deltat;
    o.n10 = n10;
    o.n1 = n1;
    o.n001 = n001;
    o.ready = 1;
  }
  sat[ch] = o;
}

// ---------------------------------------------------------------------------
// the measurement loop
// ---------------------------------------------------------------------------
struct GloFixArgs {
  double samples_per_code, data_size, c, elevation_mask, step;
  int nav_sol_period, use_trop, max_meas, n_epochs;
  Tropo trop;
};

__global__ __launch_bounds__(64) void nav_glo_fix_kernel(
    const gnsscorr_glo_eph* __restrict__ eph, const gnsscorr_glo_sat* __restrict__ sat,
    const int32_t* __restrict__ first_mark, const char* __restrict__ abs_sample,
    int64_t epoch_stride, int64_t chan_stride, const int32_t* __restrict__ rx_first,
    GloFixArgs p, int32_t* __restrict__ n_meas_out, gnsscorr_gps_fix_sol* __restrict__ sol,
    gnsscorr_gps_fix_chan* __restrict__ chan) {
  const FixLane l = fix_lane(rx_first);
  const int fs = l.valid ? first_mark[l.ch] : -1;
  const gnsscorr_glo_sat* my_sat = sat + l.ch;
  const bool ready = l.valid && fs >= 0 && my_sat->ready == 1;   // postNavigation.sci:107-123
  const int n_ready = __popcll(__ballot(ready));
  const FixRows r = fix_rows(l, fs, n_ready, p.max_meas, p.n_epochs, p.nav_sol_period,   // :128, :167
                             abs_sample, chan_stride, n_meas_out, sol, chan);
  if (r.n_meas == 0) return;

  GloState w = {my_sat->pos[0], my_sat->pos[1], my_sat->pos[2],
                my_sat->vel[0], my_sat->vel[1], my_sat->vel[2]};
  const double ax = my_sat->acc[0], ay = my_sat->acc[1], az = my_sat->acc[2];
  double clk = my_sat->clk;
  const double gamman = eph[l.ch].gamman;
  const double nan = quiet_nan();
  double sat_elev = infinity();                                // :142
  for (int m = 0; m < (int)r.n_meas; m++) {
    const bool active = ready && sat_elev >= p.elevation_mask;  // :170
    const int n_act = __popcll(__ballot(active));

    double travel = infinity();                                // calculatePseudoranges.sci:55-72
    if (active)
      travel = code_periods(r.my_abs, fs, p.nav_sol_period, m, epoch_stride,
                            p.samples_per_code) / p.data_size;
    const double raw_p = since_earliest(travel) * (p.c / 1000);

    if (active) {                                              // deltasatposg.sci:66-137
      rk4_step(w, ax, ay, az, p.step);
      clk = clk - gamman * p.step;
    }
    const double obs = raw_p - clk * p.c;                      // postNavigation.sci:202-203

    int status = GNSSCORR_GPS_FIX_FEW;
    double pos[4] = {nan, nan, nan, nan}, el = nan, az_deg = nan;   // :179-180
    double dop[5] = {0, 0, 0, 0, 0};
    double lat = nan, lon = nan, height = nan, corr_p = 0.0;
    if (n_act >= 4) {                                          // else :249-271
      Ldl f;                                                   // leastSquarePos.sci:45-100
      status = least_squares<Fix::kGloB1>(w.x, w.y, w.z, obs, active, p.c, p.use_trop, p.trop,
                                          pos, f, el, az_deg);
      if (status == GNSSCORR_GPS_FIX_RANK) {
        lat = lon = height = 0;
      } else {
        dop_from(f, dop);                                      // :94-100
        // PZ-90.02 -> WGS-84, postNavigation.sci:206-208
        const double t0 = 1 * pos[0] + -0.82e-6 * pos[1] + 0 * pos[2];
        const double t1 = 0.82e-6 * pos[0] + 1 * pos[1] + 0 * pos[2];
        const double t2 = 0 * pos[0] + 0 * pos[1] + 1 * pos[2];
        pos[0] = -1.1 + (1 - 0.12e-6) * t0;
        pos[1] = -0.3 + (1 - 0.12e-6) * t1;
        pos[2] = -0.9 + (1 - 0.12e-6) * t2;
        sat_elev = el;                                         // :221
        if (active) corr_p = raw_p - clk * p.c + pos[3];       // :224-226
        cart2geo5<Fix::kGloB1>(pos[0], pos[1], pos[2], &lat, &lon, &height);   // :231-237
      }
    }
    write_fix_records(l.valid, r.my_chan + m, r.my_sol + m, el, az_deg, raw_p, corr_p, active,
                      pos, dop, lat, lon, height, status, n_act);
  }
}

}  // namespace

// ============================================================================
// host side
// ============================================================================
using navhost::bad_arguments;

extern "C" void gnsscorr_nav_glo_fix_cfg_init(gnsscorr_glo_fix_cfg* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof *cfg);
  cfg->samplesPerCode = 16000.0;      // initSettings.sci:69-81: round(16e6 / (0.511e6 / 511))
  cfg->dataTypeSizeInBytes = 1.0;     // :59
  cfg->c = 299792458.0;               // :136
  cfg->elevationMask = 0.0;           // :118
  cfg->navSolPeriod = 500;            // :115
  cfg->useTropCorr = 1;               // :120
  cfg->max_meas = 1;
}

extern "C" int gnsscorr_nav_glo_ephemeris_dev(gnsscorr_nav_ctx* c, const uint8_t* d_bits,
                                              const int32_t* d_n_strings,
                                              const int32_t* d_first_mark, int n_ch,
                                              gnsscorr_glo_eph* d_eph) {
  return navhost::ephemeris_dev(__func__, c, nav_glo_eph_kernel, d_bits, d_n_strings,
                                d_first_mark, n_ch, d_eph);
}

extern "C" int gnsscorr_nav_glo_ephemeris(gnsscorr_nav_ctx* c, const uint8_t* h_bits,
                                          const int32_t* h_n_strings,
                                          const int32_t* h_first_mark, int n_ch,
                                          gnsscorr_glo_eph* h_eph) {
  return navhost::ephemeris_host(__func__, c, nav_glo_eph_kernel, kGloBits, h_bits, h_n_strings,
                                 h_first_mark, n_ch, h_eph);
}

static int check_satpos(const char* fn, const gnsscorr_nav_ctx* c, const void* eph, int n_ch,
                        const gnsscorr_glo_fix_cfg* cfg, const void* sat) {
  if (!c || !eph || !cfg || !sat) return bad_arguments(fn, "null pointer");
  if (n_ch < 1) return bad_arguments(fn, "n_ch >= 1");
  if (cfg->navSolPeriod < 1) return bad_arguments(fn, "navSolPeriod >= 1");
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_glo_satpos_dev(gnsscorr_nav_ctx* c, const gnsscorr_glo_eph* d_eph,
                                           int n_ch, const gnsscorr_glo_fix_cfg* cfg,
                                           gnsscorr_glo_sat* d_sat) {
  int rc = check_satpos(__func__, c, d_eph, n_ch, cfg, d_sat);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  const double step = (double)cfg->navSolPeriod / 1000;
  hipLaunchKernelGGL(nav_glo_satpos_kernel, dim3((n_ch + 63) / 64), dim3(64), 0, c->stream, d_eph,
                     n_ch, step, d_sat);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_glo_satpos(gnsscorr_nav_ctx* c, const gnsscorr_glo_eph* h_eph,
                                       int n_ch, const gnsscorr_glo_fix_cfg* cfg,
                                       gnsscorr_glo_sat* h_sat) {
  int rc = check_satpos(__func__, c, h_eph, n_ch, cfg, h_sat);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  hostctx::Staging st(c->stream);
  const gnsscorr_glo_eph* d_eph = st.in(h_eph, (size_t)n_ch);
  gnsscorr_glo_sat* d_sat = st.out(h_sat, (size_t)n_ch);
  if (st.status()) return st.status();
  rc = gnsscorr_nav_glo_satpos_dev(c, d_eph, n_ch, cfg, d_sat);
  return rc ? rc : st.finish();
}

extern "C" int gnsscorr_nav_glo_fix_dev(gnsscorr_nav_ctx* c, const gnsscorr_glo_eph* d_eph,
                                        const gnsscorr_glo_sat* d_sat,
                                        const int32_t* d_first_mark, const void* d_abs_sample,
                                        int64_t epoch_stride_bytes, int64_t chan_stride_bytes,
                                        int n_epochs, int n_rx, const int32_t* rx_first,
                                        const gnsscorr_glo_fix_cfg* cfg, int32_t* d_n_meas,
                                        gnsscorr_gps_fix_sol* d_sol,
                                        gnsscorr_gps_fix_chan* d_chan) {
  int rc = navhost::check_fix_common(__func__, c, {d_eph, d_sat}, d_first_mark, d_abs_sample,
                                     epoch_stride_bytes, chan_stride_bytes, n_epochs, n_rx,
                                     rx_first, cfg, &gnsscorr_glo_fix_cfg::dataTypeSizeInBytes,
                                     d_n_meas, d_sol, d_chan);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  rc = navhost::upload_rx_first(c, rx_first, n_rx);
  if (rc) return rc;
  GloFixArgs p;
  p.samples_per_code = cfg->samplesPerCode;
  p.data_size = cfg->dataTypeSizeInBytes;
  p.c = cfg->c;
  p.elevation_mask = cfg->elevationMask;
  p.step = (double)cfg->navSolPeriod / 1000;
  p.nav_sol_period = cfg->navSolPeriod;
  p.use_trop = cfg->useTropCorr;
  p.max_meas = cfg->max_meas;
  p.n_epochs = n_epochs;
  navdev::tropo_consts(p.trop.htop, p.trop.ref);
  hipLaunchKernelGGL(nav_glo_fix_kernel, dim3(n_rx), dim3(64), 0, c->stream, d_eph, d_sat,
                     d_first_mark, (const char*)d_abs_sample, epoch_stride_bytes,
                     chan_stride_bytes, c->d_rx_first.p, p, d_n_meas, d_sol, d_chan);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_glo_fix(gnsscorr_nav_ctx* c, const gnsscorr_glo_eph* h_eph,
                                    const gnsscorr_glo_sat* h_sat, const int32_t* h_first_mark,
                                    const void* h_abs_sample, int64_t epoch_stride_bytes,
                                    int64_t chan_stride_bytes, int n_epochs, int n_rx,
                                    const int32_t* rx_first, const gnsscorr_glo_fix_cfg* cfg,
                                    int32_t* h_n_meas, gnsscorr_gps_fix_sol* h_sol,
                                    gnsscorr_gps_fix_chan* h_chan) {
  int rc = navhost::check_fix_common(__func__, c, {h_eph, h_sat}, h_first_mark, h_abs_sample,
                                     epoch_stride_bytes, chan_stride_bytes, n_epochs, n_rx,
                                     rx_first, cfg, &gnsscorr_glo_fix_cfg::dataTypeSizeInBytes,
                                     h_n_meas, h_sol, h_chan);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  hostctx::Staging st(c->stream);
  const gnsscorr_glo_eph* d_eph = st.in(h_eph, (size_t)rx_first[n_rx]);
  const gnsscorr_glo_sat* d_sat = st.in(h_sat, (size_t)rx_first[n_rx]);
  const navhost::FixStaged d =
      navhost::stage_fix(st, h_first_mark, h_abs_sample, epoch_stride_bytes, chan_stride_bytes,
                         n_epochs, n_rx, rx_first, cfg->max_meas, h_n_meas, h_sol, h_chan);
  if (st.status()) return st.status();
  rc = gnsscorr_nav_glo_fix_dev(c, d_eph, d_sat, d.first, d.abs_sample, epoch_stride_bytes,
                                chan_stride_bytes, n_epochs, n_rx, rx_first, cfg, d.n_meas, d.sol,
                                d.chan);
  return rc ? rc : st.finish();
}
