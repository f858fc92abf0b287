// osg_chan.h -- the per-channel GP2021 arithmetic that both OSG tracking kernels
// share (osg_stream_kernel, track.hip; osg_track_kernel, track_real.hip): a
// call's NCO words and dump schedule in closed form, the per-sample step of the
// reference recurrence and the per-channel epilogue.  track.hip's head comment
// maps it onto Sim_GP2021_int (correlator.c:148-316).  Device code, internal to
// libgnsscorr.
#ifndef GNSSCORR_OSG_CHAN_H
#define GNSSCORR_OSG_CHAN_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "gnsscorr_internal.h"

namespace osgchan {

constexpr uint64_t kNever = ~0ull;

// epochs one call of nsamp samples can touch (an epoch is D >= 2046 half-chips
// of at least one sample each): the words of a call's epoch sums in LDS and
// the dumps a call can report (gnsscorr_track_max_dumps)
__host__ __device__ constexpr int epoch_cap(int nsamp) { return nsamp / GNSSCORR_OSG_ROW + 2; }

// 8-phase LO (correlator.c:203-204) as 4-bit two's-complement nibbles.
constexpr uint32_t kLutI = 0xEEF1221Fu;  // i_lo = {-1, 1, 2, 2, 1,-1,-2,-2}
constexpr uint32_t kLutQ = 0x1FEEF122u;  // q_lo = { 2, 2, 1,-1,-2,-2,-1, 1}

struct Chan {
  uint32_t P0, K0, cinc, kinc2, hc0, D;
  uint64_t j1;       // rollover index of the first dump (kNever: none)
  int base;          // prn * 2046 into the packed table
};

// Half-chip counter, table load index and epoch after r rollovers; div(m, e, q):
// m = e * D + q, the rollovers since the first dump over the epoch length.
template <typename DivD>
__device__ __forceinline__ void hc_rule(const Chan& c, uint64_t r, uint32_t& hc, uint32_t& ld,
                                        uint32_t& epoch, DivD div) {
  if (r < c.j1) {
    epoch = 0;
    hc = (uint32_t)((c.hc0 + r) & 0xFFFFu);
    ld = hc;
  } else {
    const uint32_t m = (uint32_t)(r - c.j1);
    uint32_t e, q;
    div(m, e, q);
    epoch = 1 + e;
    hc = q;
    ld = q ? q : (m == 0 ? (uint32_t)((c.hc0 + c.j1) & 0xFFFFu) : c.D);
  }
}
__device__ __forceinline__ void hc_after(const Chan& c, uint64_t r, uint32_t& hc, uint32_t& ld,
                                         uint32_t& epoch) {
  hc_rule(c, r, hc, ld, epoch, [&](uint32_t m, uint32_t& e, uint32_t& q) {
    e = m / c.D;
    q = m % c.D;
  });
}

__device__ __forceinline__ uint32_t n_dumps_after(const Chan& c, uint64_t r) {
  return r >= c.j1 ? 1 + (uint32_t)(r - c.j1) / c.D : 0u;
}

__device__ __forceinline__ void msbit_step(int& ms, int& bit) {
  // correlator.c:275-280
  ms++;
  if (ms == 20) bit = (bit + 1) % 50;
  ms %= 20;
}

__device__ __forceinline__ int sbyte(int x, int b) { return __builtin_amdgcn_sbfe(x, 8 * b, 8); }

struct Acc {
  uint32_t a[6];
};

// One sample of the reference recurrence (correlator.c:200-283) in three steps;
// what a code carry does (half-chip, dump, new bits) is each kernel's own.
// The LO of the sample's carrier phase
__device__ __forceinline__ void sample_lo(uint32_t phase, int& il, int& ql) {
  const uint32_t off = (phase >> 27) & 0x1Cu;
  il = __builtin_amdgcn_sbfe((int)kLutI, off, 4);
  ql = __builtin_amdgcn_sbfe((int)kLutQ, off, 4);
}
// ... its mixed sample onto the six sums (correlator.c:225-241)
__device__ __forceinline__ void sample_acc(int ival, int qval, int lb, int pb, int eb, Acc& acc) {
  acc.a[0] += (uint32_t)(lb * ival);
  acc.a[1] += (uint32_t)(lb * qval);
  acc.a[2] += (uint32_t)(pb * ival);
  acc.a[3] += (uint32_t)(pb * qval);
  acc.a[4] += (uint32_t)(eb * ival);
  acc.a[5] += (uint32_t)(eb * qval);
}
// ... and both NCOs to the next sample; true on a code carry (correlator.c:243-246)
__device__ __forceinline__ bool sample_nco(const Chan& c, uint32_t& phase, uint32_t& kph) {
  phase += c.cinc;
  const uint32_t nk = kph + c.kinc2;
  const bool carry = nk < kph;
  kph = nk;
  return carry;
}

// E/P/L bits of one half-chip as three 2-bit two's-complement fields
// (late | prompt << 2 | early << 4; values -1 / 0 / +1), see pack8_table()
__device__ __forceinline__ void unpack8(uint32_t w, int& lb, int& pb, int& eb) {
  lb = __builtin_amdgcn_sbfe((int)w, 0, 2);
  pb = __builtin_amdgcn_sbfe((int)w, 2, 2);
  eb = __builtin_amdgcn_sbfe((int)w, 4, 2);
}
// ... and as the three int8 of a word of the 32-bit table (gnsscorr_osg_packed_table)
__device__ __forceinline__ void unpack_pk(uint32_t w, int& lb, int& pb, int& eb) {
  lb = (int)(int8_t)(w & 0xFFu);
  pb = (int)(int8_t)((w >> 8) & 0xFFu);
  eb = (int)(int8_t)((w >> 16) & 0xFFu);
}

// Per-channel epilogue of a call (one thread): dumps, ms/bit counters, TIC latch,
// carrier cycles and the new channel state (correlator.c:243-316).  sum(i):
// the call's epoch sums, word i = epoch * 6 + k (LDS or global).  st_out (if
// given) receives the new state as well.
template <typename SumAt>
__device__ __forceinline__ gnsscorr_track_result channel_epilogue(
    const Chan& c, const gnsscorr_nco_cmd& cmd, gnsscorr_chan_state st, int chn, bool active,
    uint32_t ndump, uint64_t Rtot, int nsamp, int64_t tic_count, SumAt sum,
    gnsscorr_track_result* __restrict__ res, gnsscorr_chan_state* __restrict__ state,
    int32_t* __restrict__ all_dumps, int max_dumps, gnsscorr_chan_state* st_out = nullptr) {
  if (!active) {   // idle channel: only the epoch load (correlator.c:177-185)
    gnsscorr_track_result r;
    memset(&r, 0, sizeof r);
    r.n_dumps = cmd.prn > 32 ? -1 : 0;
    r.msbit_reg = st.msbit_reg;
    res[chn] = r;
    state[chn] = st;
    if (st_out) *st_out = st;
    return r;
  }
  gnsscorr_track_result r;
  memset(&r, 0, sizeof r);
  r.n_dumps = (int)ndump;
  int ms = st.ms_counter, bit = st.bit_counter, msbit = st.msbit_reg;

  const bool tic_here = tic_count >= 0 && tic_count < nsamp;
  uint32_t nd_tic = 0;
  uint64_t Rt = 0;
  if (tic_here) {
    Rt = ((uint64_t)c.K0 + (uint64_t)(tic_count + 1) * c.kinc2) >> 32;
    nd_tic = n_dumps_after(c, Rt);
  }
  int msbit_at_tic = msbit;
  for (uint32_t d = 0; d < ndump; d++) {
    uint32_t v[6];
#pragma unroll
    for (int k = 0; k < 6; k++)
      v[k] = sum(d * 6 + k) + (d == 0 ? (uint32_t)st.acc[k] : 0u);
    if (all_dumps && (int)d < max_dumps)
      for (int k = 0; k < 6; k++) all_dumps[((int64_t)chn * max_dumps + d) * 6 + k] = (int32_t)v[k];
    if (d + 1 == ndump)
      for (int k = 0; k < 6; k++) r.dump[k] = (int32_t)v[k];
    msbit_step(ms, bit);
    msbit = ms + (bit << 8);
    if (d + 1 == nd_tic) msbit_at_tic = msbit;
  }
  uint32_t nacc[6];
  for (int k = 0; k < 6; k++)
    nacc[k] = sum(ndump * 6 + k) + (ndump == 0 ? (uint32_t)st.acc[k] : 0u);

  const uint64_t Wtot = ((uint64_t)c.P0 + (uint64_t)nsamp * c.cinc) >> 32;
  uint32_t cycle_end;
  if (tic_here) {  // TIC latch after sample tic_count (correlator.c:286-303)
    const uint64_t t1 = (uint64_t)tic_count + 1;
    const uint64_t Wt = ((uint64_t)c.P0 + t1 * c.cinc) >> 32;
    const uint32_t cyc = st.carrier_cycle + (uint32_t)Wt;
    uint32_t hct, ldt, ept;
    hc_after(c, Rt, hct, ldt, ept);
    r.tic = 1;
    r.tic_regs[0] = (int32_t)hct;
    r.tic_regs[1] = (int32_t)(cyc & 0xffffu);
    r.tic_regs[2] = (int32_t)((c.P0 + (uint32_t)t1 * c.cinc) >> 22);
    r.tic_regs[3] = msbit_at_tic;
    r.tic_regs[4] = (int32_t)((uint32_t)((uint64_t)c.K0 + t1 * c.kinc2) >> 22);
    r.tic_regs[5] = (int32_t)(cyc >> 16);
    cycle_end = (uint32_t)(Wtot - Wt);
  } else {
    cycle_end = st.carrier_cycle + (uint32_t)Wtot;
  }
  uint32_t hce, lde, epe;
  hc_after(c, Rtot, hce, lde, epe);

  r.msbit_reg = msbit;
  res[chn] = r;

  st.carrier_phase = c.P0 + (uint32_t)nsamp * c.cinc;
  st.carrier_cycle = cycle_end;
  st.code_phase = (uint32_t)((uint64_t)c.K0 + (uint64_t)nsamp * c.kinc2);
  st.half_chip = hce;
  for (int k = 0; k < 6; k++) st.acc[k] = (int32_t)nacc[k];
  st.ms_counter = ms;
  st.bit_counter = bit;
  st.msbit_reg = msbit;
  state[chn] = st;
  if (st_out) *st_out = st;
  return r;
}

// channel state and NCO words of one call (correlator.c:177-189)
__device__ __forceinline__ bool chan_setup(const gnsscorr_nco_cmd& cmd, gnsscorr_chan_state& st,
                                           Chan& c) {
  if (cmd.epoch_load >= 0) {  // epoch set, correlator.c:177-182
    const int v = cmd.epoch_load & 0xFFFF;
    st.msbit_reg = v;
    st.ms_counter = v & 0xff;
    st.bit_counter = v >> 8;
  }
  const bool active = cmd.prn > 0 && cmd.prn <= 32;   // correlator.c:185
  c.P0 = st.carrier_phase;
  c.K0 = st.code_phase;
  c.cinc = cmd.carrier_incr;
  c.kinc2 = cmd.code_incr << 1;
  c.hc0 = st.half_chip & 0xFFFFu;
  c.D = (cmd.slew & 0xFFFFu) + 2046u;
  const uint32_t h1 = (c.hc0 + 1u) & 0xFFFFu;
  if (h1 >= c.D) c.j1 = 1;
  else if (c.D <= 0xFFFFu) c.j1 = 1ull + (c.D - h1);
  else c.j1 = kNever;  // uint16 half-chip can never reach D
  c.base = (active ? cmd.prn : 0) * GNSSCORR_OSG_ROW;
  return active;
}

}  // namespace osgchan
#endif
