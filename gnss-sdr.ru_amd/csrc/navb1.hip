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
// the kernel, out of the steps of nav_fix.h.  The satellite position is navdev::sat_pos with
// BeiDou's constants and clock fields; the least squares is the GLONASS/L1 text
// (Fix::kGloB1).  There is no elevation mask: the set of used channels is fixed for the whole
// call.
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

constexpr int kB1Slots = 5, kB1SlotBits = 213;
constexpr int kB1Bits = kB1Slots * kB1SlotBits;
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
        if (f.kind == kTimesPi) vd = vd * kEphPi;
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
  Tropo trop;
};

__global__ __launch_bounds__(64) void nav_b1_fix_kernel(
    const gnsscorr_b1_eph* __restrict__ eph, const int32_t* __restrict__ first,
    const char* __restrict__ abs_sample, int64_t epoch_stride, int64_t chan_stride,
    const int32_t* __restrict__ rx_first, B1FixArgs p, int32_t* __restrict__ n_meas_out,
    gnsscorr_gps_fix_sol* __restrict__ sol, gnsscorr_gps_fix_chan* __restrict__ chan) {
  const FixLane l = fix_lane(rx_first);
  const gnsscorr_b1_eph e = eph[l.ch];                         // once, into registers
  const int fs = l.valid ? first[l.ch] : -1;
  // postNavigation.sci:117-118 are disabled in the file; the library drops these channels
  const bool used = l.valid && fs >= 0 && e.status == GNSSCORR_B1_EPH_OK && e.have == 7;
  const uint64_t used_set = __ballot(used);
  const int n_used = __popcll(used_set);
  const FixRows r = fix_rows(l, fs, n_used, p.max_meas, p.n_epochs, p.nav_sol_period,      // :121, :152
                             abs_sample, chan_stride, n_meas_out, sol, chan);
  if (r.n_meas == 0) return;

  double transmit_time = (double)__shfl(e.SOW, __ffsll((long long)used_set) - 1);   // :145
  const Kepler k = kepler_of(e, e.a2, e.a1, e.a0, e.T_GD_1);
  for (int m = 0; m < (int)r.n_meas; m++) {
    double travel = infinity();                                // calculatePseudoranges.sci
    if (used)
      travel = code_periods(r.my_abs, fs, p.nav_sol_period, m, epoch_stride,
                            p.samples_per_code) / p.data_size;
    const double raw_p = since_earliest(travel) * (p.c / 1000);

    SatPos s = {0, 0, 0, 0};                                   // :175-177, satpos.sci:53-136
    if (used) s = sat_pos(k, 7.2921150e-5, 3.986004418e14, transmit_time);
    const double obs = raw_p + s.clk * p.c;                    // :187-188

    double pos[4], el, az, dop[5] = {0, 0, 0, 0, 0};           // :165-166
    double lat = 0, lon = 0, height = 0, corr_p = 0.0;
    Ldl f;
    const int status = least_squares<Fix::kGloB1>(s.x, s.y, s.z, obs, used, p.c, p.use_trop,
                                                  p.trop, pos, f, el, az);
    if (status != GNSSCORR_GPS_FIX_RANK) {
      dop_from(f, dop);
      if (used) corr_p = raw_p - s.clk * p.c + pos[3];         // :212-214, the sign as the file
      cart2geo5<Fix::kGloB1>(pos[0], pos[1], pos[2], &lat, &lon, &height);   // :219-225
    }
    write_fix_records(l.valid, r.my_chan + m, r.my_sol + m, el, az, raw_p, corr_p, used, pos,
                      dop, lat, lon, height, status, n_used);
    transmit_time = transmit_time + (double)p.nav_sol_period / 1000;   // :270
  }
}

}  // namespace

// ============================================================================
// host side
// ============================================================================
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

extern "C" int gnsscorr_nav_b1_ephemeris_dev(gnsscorr_nav_ctx* c, const uint8_t* d_bits,
                                             const int32_t* d_n_subframes,
                                             const int32_t* d_first, int n_ch,
                                             gnsscorr_b1_eph* d_eph) {
  return navhost::ephemeris_dev(__func__, c, nav_b1_eph_kernel, d_bits, d_n_subframes, d_first,
                                n_ch, d_eph);
}

extern "C" int gnsscorr_nav_b1_ephemeris(gnsscorr_nav_ctx* c, const uint8_t* h_bits,
                                         const int32_t* h_n_subframes, const int32_t* h_first,
                                         int n_ch, gnsscorr_b1_eph* h_eph) {
  return navhost::ephemeris_host(__func__, c, nav_b1_eph_kernel, kB1Bits, h_bits, h_n_subframes,
                                 h_first, n_ch, h_eph);
}

extern "C" int gnsscorr_nav_b1_fix_dev(gnsscorr_nav_ctx* c, const gnsscorr_b1_eph* d_eph,
                                       const int32_t* d_first, const void* d_abs_sample,
                                       int64_t epoch_stride_bytes, int64_t chan_stride_bytes,
                                       int n_epochs, int n_rx, const int32_t* rx_first,
                                       const gnsscorr_b1_fix_cfg* cfg, int32_t* d_n_meas,
                                       gnsscorr_gps_fix_sol* d_sol,
                                       gnsscorr_gps_fix_chan* d_chan) {
  int rc = navhost::check_fix_common(__func__, c, {d_eph}, d_first, d_abs_sample,
                                     epoch_stride_bytes, chan_stride_bytes, n_epochs, n_rx,
                                     rx_first, cfg, &gnsscorr_b1_fix_cfg::dataTypeSizeInBytes,
                                     d_n_meas, d_sol, d_chan);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  rc = navhost::upload_rx_first(c, rx_first, n_rx);
  if (rc) return rc;
  B1FixArgs p;
  p.samples_per_code = cfg->samplesPerCode;
  p.data_size = cfg->dataTypeSizeInBytes;
  p.c = cfg->c;
  p.nav_sol_period = cfg->navSolPeriod;
  p.use_trop = cfg->useTropCorr;
  p.max_meas = cfg->max_meas;
  p.n_epochs = n_epochs;
  navdev::tropo_consts(p.trop.htop, p.trop.ref);
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
  int rc = navhost::check_fix_common(__func__, c, {h_eph}, h_first, h_abs_sample,
                                     epoch_stride_bytes, chan_stride_bytes, n_epochs, n_rx,
                                     rx_first, cfg, &gnsscorr_b1_fix_cfg::dataTypeSizeInBytes,
                                     h_n_meas, h_sol, h_chan);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  hostctx::Staging st(c->stream);
  const gnsscorr_b1_eph* d_eph = st.in(h_eph, (size_t)rx_first[n_rx]);
  const navhost::FixStaged d =
      navhost::stage_fix(st, h_first, h_abs_sample, epoch_stride_bytes, chan_stride_bytes,
                         n_epochs, n_rx, rx_first, cfg->max_meas, h_n_meas, h_sol, h_chan);
  if (st.status()) return st.status();
  rc = gnsscorr_nav_b1_fix_dev(c, d_eph, d.first, d.abs_sample, epoch_stride_bytes,
                               chan_stride_bytes, n_epochs, n_rx, rx_first, cfg, d.n_meas, d.sol,
                               d.chan);
  return rc ? rc : st.finish();
}
