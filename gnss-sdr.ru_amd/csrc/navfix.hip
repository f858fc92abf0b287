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
// loop inside the kernel (measurements are serial through satElev), out of the steps
// of nav_fix.h: the ballots that form the channel sets, the TOW seed, navdev::sat_pos
// with GPS's constants and clock fields, the GPS/L1 text of the least squares
// (Fix::kGps) and the branch for fewer than 4 active channels.
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

constexpr int kGpsBits = 1500;

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
          if (f.pi) vd = vd * kEphPi;
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
  Tropo trop;
};

__global__ __launch_bounds__(64) void nav_gps_fix_kernel(
    const gnsscorr_gps_eph* __restrict__ eph, const int32_t* __restrict__ first_subframe,
    const char* __restrict__ abs_sample, int64_t epoch_stride, int64_t chan_stride,
    const int32_t* __restrict__ rx_first, FixArgs p, int32_t* __restrict__ n_meas_out,
    gnsscorr_gps_fix_sol* __restrict__ sol, gnsscorr_gps_fix_chan* __restrict__ chan) {
  const FixLane l = fix_lane(rx_first);
  const gnsscorr_gps_eph e = eph[l.ch];                        // once, into registers
  const int fs = l.valid ? first_subframe[l.ch] : -1;
  const bool decodable = l.valid && fs >= 0 && e.status == GNSSCORR_GPS_EPH_OK;
  const bool ready = decodable && e.have == 7;                 // postNavigation.sci:120-126
  const int n_ready = __popcll(__ballot(ready));
  const FixRows r = fix_rows(l, fs, n_ready, p.max_meas, p.n_epochs, p.nav_sol_period,   // :130, :163
                             abs_sample, chan_stride, n_meas_out, sol, chan);
  const uint64_t seeds = __ballot(decodable);
  if (r.n_meas == 0) return;

  // :117,152: the TOW the file's channel loop leaves behind is its last channel's
  double transmit_time = (double)__shfl(e.TOW, 63 - __clzll((long long)seeds));
  const Kepler k = kepler_of(e, e.a_f2, e.a_f1, e.a_f0, e.T_GD);
  const double nan = quiet_nan();
  double sat_elev = infinity();                                // :144
  for (int m = 0; m < (int)r.n_meas; m++) {
    const bool active = ready && sat_elev >= p.elevation_mask;  // :167
    const int n_act = __popcll(__ballot(active));

    double travel = infinity();                                // calculatePseudoranges.sci:55-72
    if (active)
      travel = code_periods(r.my_abs, fs, p.nav_sol_period, m, epoch_stride, p.samples_per_code);
    const double raw_p = (since_earliest(travel) + p.start_offset) * (p.c / 1000);

    SatPos s = {0, 0, 0, 0};                // :189-191, the active list only; satpos.sci:56-145
    if (active) s = sat_pos(k, 7.2921151467e-5, 3.986005e14, transmit_time);
    const double obs = raw_p + s.clk * p.c;                    // :201-202

    int status = GNSSCORR_GPS_FIX_FEW;
    double pos[4] = {nan, nan, nan, nan}, el = nan, az = nan;   // :176-177
    double dop[5] = {0, 0, 0, 0, 0};
    double lat = nan, lon = nan, height = nan, corr_p = 0.0;
    if (n_act >= 4) {                                          // else :245-269
      Ldl f;                                                   // leastSquarePos.sci:32-111
      status = least_squares<Fix::kGps>(s.x, s.y, s.z, obs, active, p.c, p.use_trop, p.trop,
                                        pos, f, el, az);
      if (status == GNSSCORR_GPS_FIX_RANK) {
        lat = lon = height = 0;
      } else {
        dop_from(f, dop);                                      // :105-111
        sat_elev = el;                                         // postNavigation.sci:217
        if (active) corr_p = raw_p + s.clk * p.c + pos[3];     // :220-222
        cart2geo5<Fix::kGps>(pos[0], pos[1], pos[2], &lat, &lon, &height);   // :227-233
      }
    }
    write_fix_records(l.valid, r.my_chan + m, r.my_sol + m, el, az, raw_p, corr_p, active, pos,
                      dop, lat, lon, height, status, n_act);
    transmit_time = transmit_time + (double)p.nav_sol_period / 1000;   // :280
  }
}

}  // namespace

// ============================================================================
// host side
// ============================================================================
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

extern "C" int gnsscorr_nav_gps_ephemeris_dev(gnsscorr_nav_ctx* c, const uint8_t* d_bits,
                                              const int32_t* d_n_bits,
                                              const int32_t* d_first_subframe, int n_ch,
                                              gnsscorr_gps_eph* d_eph) {
  return navhost::ephemeris_dev(__func__, c, nav_gps_eph_kernel, d_bits, d_n_bits,
                                d_first_subframe, n_ch, d_eph);
}

extern "C" int gnsscorr_nav_gps_ephemeris(gnsscorr_nav_ctx* c, const uint8_t* h_bits,
                                          const int32_t* h_n_bits,
                                          const int32_t* h_first_subframe, int n_ch,
                                          gnsscorr_gps_eph* h_eph) {
  return navhost::ephemeris_host(__func__, c, nav_gps_eph_kernel, kGpsBits, h_bits, h_n_bits,
                                 h_first_subframe, n_ch, h_eph);
}

extern "C" int gnsscorr_nav_gps_fix_dev(gnsscorr_nav_ctx* c, const gnsscorr_gps_eph* d_eph,
                                        const int32_t* d_first_subframe,
                                        const void* d_abs_sample, int64_t epoch_stride_bytes,
                                        int64_t chan_stride_bytes, int n_epochs, int n_rx,
                                        const int32_t* rx_first,
                                        const gnsscorr_gps_fix_cfg* cfg, int32_t* d_n_meas,
                                        gnsscorr_gps_fix_sol* d_sol,
                                        gnsscorr_gps_fix_chan* d_chan) {
  int rc = navhost::check_fix_common(__func__, c, {d_eph}, d_first_subframe, d_abs_sample,
                                     epoch_stride_bytes, chan_stride_bytes, n_epochs, n_rx,
                                     rx_first, cfg, (double gnsscorr_gps_fix_cfg::*)nullptr,
                                     d_n_meas, d_sol, d_chan);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  rc = navhost::upload_rx_first(c, rx_first, n_rx);
  if (rc) return rc;
  FixArgs p;
  p.samples_per_code = cfg->samplesPerCode;
  p.start_offset = cfg->startOffset;
  p.c = cfg->c;
  p.elevation_mask = cfg->elevationMask;
  p.nav_sol_period = cfg->navSolPeriod;
  p.use_trop = cfg->useTropCorr;
  p.max_meas = cfg->max_meas;
  p.n_epochs = n_epochs;
  navdev::tropo_consts(p.trop.htop, p.trop.ref);
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
  int rc = navhost::check_fix_common(__func__, c, {h_eph}, h_first_subframe, h_abs_sample,
                                     epoch_stride_bytes, chan_stride_bytes, n_epochs, n_rx,
                                     rx_first, cfg, (double gnsscorr_gps_fix_cfg::*)nullptr,
                                     h_n_meas, h_sol, h_chan);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  hostctx::Staging st(c->stream);
  const gnsscorr_gps_eph* d_eph = st.in(h_eph, (size_t)rx_first[n_rx]);
  const navhost::FixStaged d =
      navhost::stage_fix(st, h_first_subframe, h_abs_sample, epoch_stride_bytes,
                         chan_stride_bytes, n_epochs, n_rx, rx_first, cfg->max_meas, h_n_meas,
                         h_sol, h_chan);
  if (st.status()) return st.status();
  rc = gnsscorr_nav_gps_fix_dev(c, d_eph, d.first, d.abs_sample, epoch_stride_bytes,
                                chan_stride_bytes, n_epochs, n_rx, rx_first, cfg, d.n_meas, d.sol,
                                d.chan);
  return rc ? rc : st.finish();
}
