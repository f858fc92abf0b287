// track.hip -- GP2021-semantics E/P/L tracking correlator on gfx950.
//
// Replaces the per-sample loop of Sim_GP2021_int
// (reference osgnss_next_step/src/correlator/correlator.c:148-316) with a
// closed-form, sample-parallel formulation that is bit-exact with it:
//
//  * carrier NCO: phase before sample n = P0 + n*cinc (mod 2^32); the 8-phase
//    LO index is its top 3 bits (correlator.c:203-215).
//  * code NCO: rollovers before sample n = (K0 + n*kinc2) >> 32 in 64-bit
//    (kinc2 = code_incr << 1, correlator.c:245), so every thread can start
//    its run of samples anywhere without walking the previous ones.
//  * half-chip / dump logic (correlator.c:246-283) is a function of the
//    rollover count r: until the first dump the half-chip is hc0 + r (uint16);
//    the first dump comes at rollover j1, then every D = slew + 2046
//    rollovers.  The E/P/L bits after the dump rollover are loaded from the
//    PRE-reset index (>= 2046, the reference's row over-read) and half-chip 0
//    of the new epoch keeps them (no reload), which hc_after() reproduces.
//  * accumulation is int32 two's-complement, so partial sums can be combined
//    in any order: per epoch in LDS, from lanes (here) or threads
//    (track_real.hip) that each hold the sums of the epoch they are in.
//
// Two kernels share that arithmetic (osg_chan.h): osg_stream_kernel in this
// file, the IQ stream engine (one wavefront per channel, every interleaved I,Q
// stream), and osg_track_kernel in track_real.hip (thread groups of 64-sample
// runs, real-sample streams).  The context and the C ABI in front of both:
// track_host.hip, through track_ctx.h.
#include <hip/hip_runtime.h>
#include <type_traits>
#include <string.h>
#include "gnsscorr_internal.h"
#include "if2.h"
#include "osg_chan.h"
#include "osg_isr.h"
#include "track_ctx.h"

// Diagnostic hook of osg_stream_kernel (tools/trk_stream_stamps.hip; a no-op here)
#ifndef STREAM_PSTAMP
#define STREAM_PSTAMP(i) \
  do {                   \
  } while (0)
#endif

namespace {
using namespace osgchan;

constexpr int kPk8Stage = 3088;       // LDS bytes of the E/P/L row (D <= 3071: slew <= 1025) + 3 of misalignment

// ---- IQ streams (osg_stream_kernel): segment sums with v_dot4 ---------------
// Between two code-NCO carries (one half-chip, ~8 samples) the E/P/L bits are
// constant, so acc_X += bit_X * ival(n) over the segment equals bit_X times the
// segment sum S = sum ival(n) (int32 wrap keeps it exact).  ival/qval of a
// pair of samples (n, n+1) is ONE v_dot4_i32_i8 of the IF word {I0,Q0,I1,Q1}
// with the LO word {il(a), ql(a), il(b), ql(b)} resp. {ql(a), -il(a), ql(b),
// -il(b)} (correlator.c:213-215), a / b the 8-phase LO indices of the two
// samples; the 64 (a, b) LO word pairs sit in LDS.  A carry between the two
// samples splits the pair with byte masks.
__device__ __forceinline__ int dot4(uint32_t a, uint32_t b, int c) {
  return __builtin_amdgcn_sdot4((int)a, (int)b, c, false);
}

// |segment sum| < 2^23 and bits are -1/0/+1: the 24-bit multiply is exact
// (int32 wrap on the accumulator, as the reference).  __mul24 (llvm.amdgcn.mul.i24)
// + add is selected as v_mad_i32_i24; a plain `c + a * b` becomes a 64-bit
// v_mad_u64_u32.  This used to be an inline-asm v_mad_i32_i24: an INLINEASM
// carries no implicit EXEC operand, so machine passes were free to move it
// across the exec-mask writes of divergent branches, where it then wrote
// lanes of a reused register that the branch had masked off -- the cause of
// the wrong sums DESIGN.md recorded for reordered IF loads in round 2.
__device__ __forceinline__ uint32_t mad24(int a, int b, uint32_t c) {
  return c + (uint32_t)__mul24(a, b);
}
__device__ __forceinline__ void seg_flush(int si, int sq, int lb, int pb, int eb, Acc& cur) {
  cur.a[0] = mad24(lb, si, cur.a[0]);
  cur.a[1] = mad24(lb, sq, cur.a[1]);
  cur.a[2] = mad24(pb, si, cur.a[2]);
  cur.a[3] = mad24(pb, sq, cur.a[3]);
  cur.a[4] = mad24(eb, si, cur.a[4]);
  cur.a[5] = mad24(eb, sq, cur.a[5]);
}

// ============================================================================
// Branch-free segment sums for interleaved I,Q streams (int8 or 2-bit packed):
// the piece and interval form that osg_stream_kernel runs.
//
// Why: a lane that walks its samples one by one takes a code-carry branch
// about once per 8 samples, at a different sample in every lane, so a wave
// executes the carry path (segment flush, bit reload, epoch switch) at nearly
// every sample pair: ~18 VALU + ~12 SALU instructions per sample (PMC, round
// 2).  Here a lane's samples are cut into intervals of three pairs (6 samples;
// four pairs where a half-chip lasts >= 8 samples, kIv4Kinc2).  When a
// half-chip lasts at least 6 samples (kinc2 <= 2^32 / 6, any fs >= 12.3 Msps)
// an interval holds at most one code carry, so every pair is split branch-free
// into the part before the carry ("pre", LO word masked by the carry position)
// and the whole pair ("tot"); at the end of each interval -- the same
// instruction for every lane -- the pre sums are flushed with the current
// E/P/L bits (correlator.c:213-241), the remainder carries over into the next
// segment and the bits are reloaded once (correlator.c:243-251).  The rare dump
// (epoch switch, correlator.c:251-281) is the only branch.
//
// Sample -> lane map: a channel's wave walks the call in pieces of 2048
// samples; lane l takes samples [2048 p + 32 l, +32) of piece p.  A piece is
// 64 lanes x 32 samples of CONTIGUOUS IF, so each wave load reads 1 KiB of
// consecutive bytes: int8 pieces (4 KiB) land by LDS-DMA in a wave-private,
// swizzled LDS slot (slot_entry; no workgroup barrier), packed pieces (16 B per
// lane) are loaded straight into registers and expanded through a 256-word LDS
// table.  No IF is shared between channels in LDS, so the receiver layout (12
// channels per stream) and one stream per channel run the same code with the
// same LDS footprint.
//
// Channels outside the fast form's conditions (kinc2 > 2^32/6, a half-chip
// range beyond the staged E/P/L row, no dump possible) run the per-sample
// reference recurrence (corr_sample_s) on the same words, wave-uniformly.
// ============================================================================
constexpr int kPieceLen = 32;                    // samples per lane per piece
constexpr int kPieceSpan = 64 * kPieceLen;       // samples per wave per piece
constexpr int kStage2Bytes = kPieceSpan * 2;     // int8 IQ bytes of one staged piece (4 KiB)
constexpr uint32_t kFastKinc2 = 0xFFFFFFFFu / 6u;   // >= 6 samples per half-chip

// hc_after without a 32-bit division (m < 2^24: fp32 reciprocal + one fix-up)
__device__ __forceinline__ void hc_after_fast(const Chan& c, uint64_t r, float invD, uint32_t& hc,
                                              uint32_t& ld, uint32_t& epoch) {
  hc_rule(c, r, hc, ld, epoch, [&](uint32_t m, uint32_t& e, uint32_t& qu) {
    e = (uint32_t)((float)m * invD);
    // e < 2^14 and D < 2^17 (r counts the half-chips of one call): a full-rate
    // 24-bit multiply, not v_mul_lo_u32
    int q = (int)(m - __umul24(e, c.D));
    if (q < 0) { q += (int)c.D; e--; }
    if (q >= (int)c.D) { q -= (int)c.D; e++; }
    qu = (uint32_t)q;
  });
}

// Lane state through its pieces.
struct Seg {
  uint32_t p0, kph, hc, ld;
  uint32_t cb, nb;             // kPF: row byte of the current bits / of index hc + 1
  int lb, pb, eb;
  int ti, tq, pi, pq;          // interval sums: whole pairs / part before the carry
  bool carried;               // a code carry in the current interval
};

// lane a | b << 3 writes the LO words of the sample pair (a, b) into the table
// lt: the ival word, and 64 entries on the qval word
__device__ __forceinline__ void lo_words(int lane, uint32_t* lt) {
  const int a = lane & 7, b = lane >> 3;
  const uint32_t ia = (uint32_t)__builtin_amdgcn_sbfe((int)kLutI, 4 * a, 4) & 0xFFu;
  const uint32_t qa = (uint32_t)__builtin_amdgcn_sbfe((int)kLutQ, 4 * a, 4) & 0xFFu;
  const uint32_t ib = (uint32_t)__builtin_amdgcn_sbfe((int)kLutI, 4 * b, 4) & 0xFFu;
  const uint32_t qb = (uint32_t)__builtin_amdgcn_sbfe((int)kLutQ, 4 * b, 4) & 0xFFu;
  lt[lane] = ia | qa << 8 | ib << 16 | qb << 24;
  lt[64 + lane] = qa | ((0u - ia) & 0xFFu) << 8 | qb << 16 | ((0u - ib) & 0xFFu) << 24;
}

// a pair's IF word x onto the interval sums: the whole word, and its part before
// the carry (mask m)
__device__ __forceinline__ void pair_dots(uint32_t x, uint32_t m, uint32_t lo_x, uint32_t lo_y,
                                          Seg& g) {
  const uint32_t xm = x & m;
  g.ti = dot4(x, lo_x, g.ti);
  g.tq = dot4(x, lo_y, g.tq);
  g.pi = dot4(xm, lo_x, g.pi);
  g.pq = dot4(xm, lo_y, g.pq);
}

// flush the part before the carry with the current bits and carry the rest into
// the next segment (correlator.c:213-241)
__device__ __forceinline__ void seg_carry(Seg& g, Acc& acc) {
  seg_flush(g.pi, g.pq, g.lb, g.pb, g.eb, acc);
  const int ri = g.ti - g.pi, rq = g.tq - g.pq;
  g.ti = g.pi = ri;
  g.tq = g.pq = rq;
}

// one pair of samples (IF word x, LO words lo_x / lo_y) in the branch-free
// interval form; ONE: the word holds a single (last) sample, so no carry after
// a second one.  (kPF: a piece's 16 LO word pairs are read from LDS before its
// first interval)
template <bool ONE>
__device__ __forceinline__ void pair2r(uint32_t x, uint32_t lo_x, uint32_t lo_y, const Chan& c,
                                       Seg& g) {
  const uint32_t k0 = g.kph + c.kinc2;
  const bool c0 = k0 < g.kph;
  uint32_t k1 = k0;
  bool c1 = false;
  if (!ONE) {
    k1 = k0 + c.kinc2;
    c1 = k1 < k0;
  }
  g.kph = k1;
  uint32_t m = c0 ? 0xFFFFu : 0xFFFFFFFFu;
  m = g.carried ? 0u : m;
  g.carried = g.carried | c0 | c1;
  pair_dots(x, m, lo_x, lo_y, g);
}

// the LO words of the pair at carrier phase g.p0, which moves on to the next
// pair.  The LO word pairs are two 256-byte tables (ival words, qval words): a
// ds_read_b32 of 64 lanes then touches each bank at most once per distinct entry
// (64 entries x 4 B = the 64 banks), where one 512-byte uint2 table would put
// entries e and e + 32 on the same banks.  (No __restrict__ of its own: what the
// compiler may assume of the tables stays what each caller says.)
__device__ __forceinline__ void pair_lo(const Chan& c, Seg& g, const uint32_t* lox,
                                        const uint32_t* loy, uint32_t& lo_x, uint32_t& lo_y) {
  const uint32_t p1 = g.p0 + c.cinc;
  const uint32_t idx = (g.p0 >> 29) | ((p1 >> 26) & 0x38u);
  lo_x = lox[idx];
  lo_y = loy[idx];
  g.p0 = p1 + c.cinc;
}

// pair2r with the pair's LO words looked up as it goes
template <bool ONE>
__device__ __forceinline__ void pair2s(uint32_t x, const Chan& c, Seg& g,
                                       const uint32_t* __restrict__ lox,
                                       const uint32_t* __restrict__ loy) {
  uint32_t lo_x, lo_y;
  pair_lo(c, g, lox, loy, lo_x, lo_y);
  pair2r<ONE>(x, lo_x, lo_y, c, g);
}

// ============================================================================
// osg_stream_kernel: ONE WAVEFRONT PER CHANNEL AND CALL (interleaved I,Q
// streams, int8 or 2-bit packed; round 4).
//
// The wave walks its channel's call in pieces of 2048 samples (lane l takes
// the contiguous samples [2048 p + 32 l, +32) of piece p), with the next
// piece already on its way while the current one is correlated:
//   * int8: LDS-DMA (global_load_lds_dwordx4, 4 wave-instructions of 1 KiB of
//     consecutive IF each) into the wave's 4 KiB slot; after the piece has
//     landed the lanes copy their 64 bytes to registers and the DMA of the
//     next piece is issued into the same slot;
//   * packed: the lane's 16 bytes straight into registers, one piece ahead.
// Each piece runs the branch-free interval form above (pair2s / pair2r,
// interval_end_s: at most one code carry per 6 samples) when a half-chip lasts
// >= 6 samples and the channel's E/P/L row fits the LDS stage, else the
// per-sample reference recurrence.  A lane carries ONE set of six running sums
// (its current epoch) across all its pieces; at an epoch change -- a dump
// inside its samples, or a later piece that starts in a later epoch -- it adds
// them into the wave's per-epoch LDS sums with LDS atomics (behind a
// wave-uniform branch: dumps are rare) and starts over.  No cross-lane
// reduction and no workgroup barrier: the epoch sums are complete when the
// wave is, and lane 0 runs the channel's epilogue (correlator.c:243-316).
//
// Against a per-call workgroup of 64-sample lanes (4 waves per channel,
// osg_track_kernel's shape, which served these streams until round 4): the
// per-wave fixed work (reduction, epilogue, state setup) is
// paid once per channel-call instead of four times, the IF of the next piece
// streams in while the current one computes, and a lane holds at most one
// dump per piece (32 samples << D >= 2046 half-chips) at every sample rate.
// Channels sharing a stream (receivers) read it through L2, which the
// XCD-aware channel order keeps on one XCD.
// ============================================================================
constexpr int kStreamCh = 4;   // channels (wavefronts) per workgroup (1 / 2 / 4 / 8 measured alike)
constexpr uint32_t kIv4Kinc2 = 0x20000000u;   // 8 kinc2 <= 2^32: 4-pair intervals

// The int8 piece slot (4 KiB: 256 chunks of 16 B = 8 IQ samples; lane l's 32
// samples are chunks 4 l .. 4 l + 3) is swizzled: chunk g sits at entry
// slot_entry(g) = 4 (g / 4) + ((g % 4) XOR (g / 16 % 4)).  A lane's ds_read_b128
// of its chunk j then hits 16-byte bank slot 4 (l % 4) + (j XOR (l / 4 % 4)), and
// each of the instruction's four 16-lane groups ({0-3,12-15,20-27}, ...,
// MI355X_MICROARCH.md LDS table) holds four lanes of every l % 4 with four
// different l / 4 % 4: 16 distinct slots, conflict-free.  Unswizzled, the lanes'
// 64-byte stride put four lanes on every slot (4-way, 12 extra LDS cycles per
// read).  The map is its own inverse: DMA entry e is
// filled from chunk slot_entry(e), which stays inside e's 4-chunk group, so a
// DMA instruction still reads whole 128-byte lines.
__device__ __forceinline__ int slot_entry(int g) { return g ^ ((g >> 4) & 3); }
__device__ __forceinline__ int slot_chunk(int e) { return slot_entry(e); }

// Orders LDS accesses between the lanes of ONE wave: every lane's earlier LDS
// writes (plain stores and atomics) are visible to every lane's later LDS reads
// and atomics.  The wave executes its LDS instructions in order, but without a
// fence the compiler may move one lane's read above another lane's write: the
// per-thread memory model knows nothing of the other lanes (the
// round-4 state broadcast bug).  Wavefront-scope fences emit no instruction; the
// wave barrier keeps the scheduler from moving memory operations across.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ void flush_epoch(Acc& acc, int e, int32_t* s_sum) {
#pragma unroll
  for (int k = 0; k < 6; k++) {
    atomicAdd(&s_sum[e * 6 + k], (int)acc.a[k]);
    acc.a[k] = 0;
  }
}

// Adds the six sums of every lane in `fl` (its epoch: e) into the wave's per-epoch
// LDS sums and, with CLEAR, zeroes them.  Per distinct epoch among those lanes
// (almost always one) a DPP scan inside each 16-lane row, then one LDS atomic per
// row from lanes 15/31/47/63.  Every lane of the wave must be active.  The piece
// starts after a dump and the call's end flush most lanes at once: 64 lanes each
// adding to the same six words serialise on one LDS address (63 extra LDS cycles
// per atomic, the bulk of the kernel's SQ_LDS_BANK_CONFLICT).
template <bool CLEAR>
__device__ __forceinline__ void flush_lanes(bool fl, Acc& acc, int e, int32_t* s_sum, int lane) {
  uint64_t m = __builtin_amdgcn_ballot_w64(fl);
  asm volatile("" : "+s"(m));
  while (m) {
    const int E = __builtin_amdgcn_readlane(e, (int)__builtin_ctzll(m));
    const bool mine = fl && e == E;
#pragma unroll
    for (int k = 0; k < 6; k++) {
      int v = mine ? (int)acc.a[k] : 0;
      v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);
      v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);
      v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);
      v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);
      if ((lane & 15) == 15) atomicAdd(&s_sum[E * 6 + k], v);
      if (CLEAR) acc.a[k] = mine ? 0u : acc.a[k];
    }
    uint64_t done = __builtin_amdgcn_ballot_w64(mine);
    asm volatile("" : "+s"(done));
    m &= ~done;
  }
}

// LDS per wavefront: [IF slot (int8)] [E/P/L row] [epoch sums] [64 LO word pairs]
__host__ __device__ constexpr int stream_sum_bytes(int nsamp) {
  return ((epoch_cap(nsamp) * 24 + 15) & ~15);
}
__host__ __device__ constexpr int stream_wave_lds(bool pk, int nsamp) {
  return (pk ? 0 : kStage2Bytes) + kPk8Stage + stream_sum_bytes(nsamp) + 512;
}

// Arguments of one osg_stream_kernel launch: n_calls consecutive calls of
// every channel (replay or closed loop) or one call.
struct StreamArgs {
  const int8_t* ifbuf;
  int64_t stream_stride;      // samples
  int64_t call_elems;         // int8 elements of one call within a stream (call k at + k*call_elems)
  int nsamp, n_channels, n_calls, cmd_step;   // call k's commands: cmds + k*cmd_step
  gnsscorr_nco_cmd* cmds;
  gnsscorr_chan_state* state;
  gnsscorr_track_result* res;  // call k: res + k*n_channels
  int32_t* all_dumps;          // single calls only
  int max_dumps;
  const uint32_t* pk;
  const uint8_t* pk8;
  int64_t tic, tic_ref;        // tic_explicit: call 0's TIC sample; else the TIC counter
  int tic_explicit;            // before call 0, stepped as gnsscorr_track_next_tic does
  int xcall_prefetch;          // prefetch the next call's first piece during this call's last
  gnsscorr_osg_loop_cfg lk;    // closed loop (loops != nullptr): gpsisr after every call
  gnsscorr_osg_loop* loops;
  gnsscorr_osg_loop* hist;     // call k: hist + k*n_channels (optional)
};

// end of an interval: flush the part before the carry with the current bits,
// carry the rest into the next segment, step the half-chip (correlator.c:243-283);
// a dump adds the epoch's sums to the LDS and starts the next epoch.  PF: the
// row bytes are read one interval ahead
template <bool PF, bool DUMPS = true>
__device__ __forceinline__ void interval_end_s(const Chan& c, Seg& g, Acc& acc, int& e,
                                               int32_t* s_sum, const uint8_t* __restrict__ row) {
  seg_carry(g, acc);
  const bool cy = g.carried;
  g.hc += cy ? 1u : 0u;
  if constexpr (!PF) g.ld = cy ? g.hc : g.ld;
  g.carried = false;
  if constexpr (DUMPS) {   // (!DUMPS: the caller showed that no lane dumps in this piece)
    const bool dump = cy && g.hc >= c.D;   // correlator.c:251-281
    uint64_t any = __builtin_amdgcn_ballot_w64(dump);
    asm volatile("" : "+s"(any));          // a uniform branch: the flush stays off the common path
    if (any) {
      if (dump) {
        flush_epoch(acc, e, s_sum);
        e++;
        g.hc = 0;        // the bits of half-chip 0 come from the pre-reset index ld
      }
    }
  }
  if constexpr (PF) {
    // a carry moves to index hc + 1 (the pre-reset index when it dumps): its row
    // byte was read one interval ahead; the next one is read now
    g.cb = cy ? g.nb : g.cb;
    unpack8(g.cb, g.lb, g.pb, g.eb);
    g.nb = row[g.hc + 1];
  } else {
    unpack8(row[g.ld], g.lb, g.pb, g.eb);
  }
}

// one sample of the reference recurrence (correlator.c:200-283) on the
// running sums; ROW: the E/P/L bits from the LDS row, else the global table
template <bool ROW>
__device__ __forceinline__ void corr_sample_s(int I, int Q, uint32_t& phase, uint32_t& kph,
                                              const Chan& c, uint32_t& hc, int& lb, int& pb,
                                              int& eb, Acc& acc, int& e, int32_t* s_sum,
                                              const uint8_t* row, const uint32_t* __restrict__ pk) {
  int il, ql;
  sample_lo(phase, il, ql);
  sample_acc(il * I + ql * Q,   // correlator.c:215
             ql * I - il * Q,   // correlator.c:214
             lb, pb, eb, acc);
  if (sample_nco(c, phase, kph)) {
    hc = (hc + 1u) & 0xFFFFu;
    const uint32_t ld = hc;
    if (hc >= c.D) {
      flush_epoch(acc, e, s_sum);
      e++;
      hc = 0;
    }
    if constexpr (ROW) {
      unpack8(row[ld], lb, pb, eb);
    } else {
      unpack_pk(pk[c.base + (int)ld], lb, pb, eb);
    }
  }
}

// Open loop: at least 4 waves per SIMD (<= 128 VGPRs; the build takes 117, no
// spills): 3072 channels put 3 waves on a SIMD, 12288 put 4; same-box A/B
// 3 % faster than the unbounded build at 3072 channels.  The closed loop (gpsisr
// inlined, ~150 VGPRs) keeps the default bound.
template <bool PK, bool CLOSED>
__global__ __launch_bounds__(64 * kStreamCh, CLOSED ? 1 : 4) void osg_stream_kernel(
    StreamArgs A) {
  // the LO words and row bytes read ahead in the open loop only: in the closed loop
  // their 32 registers pushed the kernel from 151 to 183 VGPRs (2 waves per SIMD:
  // 32.6 -> 42.7 us per 3072-channel call, same box)
  constexpr bool kPF = !CLOSED;
  extern __shared__ uint4 s_dyn[];
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = (int)threadIdx.x & 63;
  const int nsamp = A.nsamp;
  const int ep_cap = epoch_cap(nsamp);
  // the 64 (a, b) LO word pairs as two 256-byte tables at a fixed LDS address,
  // shared by the workgroup's waves: a pair's words are one ds_read2_b32 whose
  // address is the byte index 4 (a | b << 3) itself (kPF); without the read-ahead
  // each wave keeps its own copy beside its sums (s_lo)
  __shared__ uint32_t s_lot[128];
  // packed: byte b -> its four int8 levels (one LDS read instead of the spread
  // and v_perm of if2_expand_byte per output word)
  constexpr bool kX2 = PK;
  __shared__ uint32_t s_x2[kX2 ? 256 : 1];
  if constexpr (kX2) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) s_x2[i] = if2_expand_byte((uint32_t)i);
  }
  if (kPF && threadIdx.x < 64) {
    lo_words(lane, s_lot);
  }
  if (kPF || kX2) __syncthreads();   // the only workgroup barrier: before any wave leaves
  uint8_t* wb = reinterpret_cast<uint8_t*>(s_dyn) + wave * stream_wave_lds(PK, nsamp);
  uint4* const slot = reinterpret_cast<uint4*>(wb);                // int8 only: the piece slot
  uint8_t* s_row = wb + (PK ? 0 : kStage2Bytes);
  int32_t* s_sum = reinterpret_cast<int32_t*>(s_row + kPk8Stage);
  uint2* s_lo = reinterpret_cast<uint2*>(reinterpret_cast<uint8_t*>(s_sum) + stream_sum_bytes(nsamp));
  STREAM_PSTAMP(0);
  const int C = A.n_channels;
  const int chn = xcd_channel(blockIdx.x, gridDim.x) * kStreamCh + wave;
  if (chn >= C) return;   // wave-uniform; no workgroup barrier from here on
  if constexpr (!kPF) {
    lo_words(lane, reinterpret_cast<uint32_t*>(s_lo));
  }
  const uint32_t* lox = reinterpret_cast<const uint32_t*>(s_lo);
  const uint32_t* loy = lox + 64;
  (void)lox;
  (void)loy;
  constexpr bool closed = CLOSED;   // A.loops != nullptr: gpsisr after every call
  gnsscorr_chan_state st = A.state[chn];
  gnsscorr_nco_cmd cmd = A.cmds[chn];
  int64_t tic = A.tic;
  const int n_pieces = (nsamp + kPieceSpan - 1) / kPieceSpan;
  int row_base = -1, row_n32 = 0;   // the E/P/L row words staged in s_row (uniform)

  // ---- the piece in flight: LDS-DMA into the wave's slot (int8), or the lane's
  // 16 bytes in registers (packed).  iss / con: pieces issued / consumed; (q_k,
  // q_p): the last issued.
  int iss = 0, con = 0, q_k = -1, q_p = -1;
  uint2 pq0 = make_uint2(0u, 0u), pq1 = make_uint2(0u, 0u);
  auto issue = [&](int k, int p, int64_t e_call) {   // e_call: element offset of call k's stream
    const int n_piece = p * kPieceSpan;
    if constexpr (PK) {
      const int n0 = n_piece + lane * kPieceLen;
      const uint8_t* b = reinterpret_cast<const uint8_t*>(A.ifbuf) + ((e_call + 2 * (int64_t)n0) >> 2);
      if (n0 + kPieceLen <= nsamp) {
        pq0 = reinterpret_cast<const uint2*>(b)[0];
        pq1 = reinterpret_cast<const uint2*>(b)[1];
      } else {
        const int L = max(0, nsamp - n0);
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        for (int q = 0; 2 * q < L; q++) w[q >> 2] |= (uint32_t)b[q] << (8 * (q & 3));
        pq0 = make_uint2(w[0], w[1]);
        pq1 = make_uint2(w[2], w[3]);
      }
    } else {
      const int valid = min(kPieceSpan, nsamp - n_piece);
      const int full_chunks = valid / 8;
      const int8_t* g8 = A.ifbuf + e_call + 2 * (int64_t)n_piece;
      // DMA instruction r writes slot entries 64 r + lane; it reads the chunk the
      // entry holds in the swizzled slot layout (slot_chunk: the chunks of one
      // 128-byte line stay within one 8-lane group, so the loads stay coalesced)
      if (full_chunks == kPieceSpan / 8) {   // a whole piece: no per-lane guards
#pragma unroll
        for (int r = 0; r < 4; r++)
          __builtin_amdgcn_global_load_lds(
              (const void*)(g8 + 16 * slot_chunk(r * 64 + lane)),
              (__attribute__((address_space(3))) void*)(slot + r * 64), 16, 0, 0);
      } else {
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int i = slot_chunk(r * 64 + lane);
          if (i < full_chunks)
            __builtin_amdgcn_global_load_lds(
                (const void*)(g8 + 16 * i),
                (__attribute__((address_space(3))) void*)(slot + r * 64), 16, 0, 0);
        }
      }
    }
    iss = __builtin_amdgcn_readfirstlane(iss + 1);   // (uniform: scalar registers)
    q_k = __builtin_amdgcn_readfirstlane(k);
    q_p = __builtin_amdgcn_readfirstlane(p);
  };

  for (int k = 0; k < A.n_calls; k++) {
    // TIC of this call (gnsscorr_track_next_tic, correlator.c:155-165)
    int64_t tic_k;
    if (A.tic_explicit) {
      tic_k = tic;
    } else if (tic < nsamp) {
      tic_k = tic;
      tic += A.tic_ref - nsamp;
    } else {
      tic -= nsamp;
      tic_k = -1;
    }
    if (k > 0 && !closed) cmd = A.cmds[(int64_t)k * A.cmd_step + chn];
    Chan c;
    const bool active = chan_setup(cmd, st, c);
    const int64_t e_call = (int64_t)cmd.stream * A.stream_stride * 2 + (int64_t)k * A.call_elems;
    wave_lds_sync();   // lane 0 read the previous call's sums: they are zeroed only after
    for (int i = lane; i < ep_cap * 6; i += 64) s_sum[i] = 0;
    wave_lds_sync();   // ... and every lane's flushes add to zeroed sums
    const uint32_t pk_hi = max(max(c.D, c.hc0), (c.hc0 + 1u) & 0xFFFFu);
    const bool pk_lds = active && c.j1 != kNever && pk_hi < 3072u;
    if (active && q_k != k) issue(k, 0, e_call);
    if (pk_lds) {
      // the staged row serves later calls of the same PRN (replay, closed loop)
      // as far as it reaches
      const int n32 = (int)((pk_hi + (uint32_t)(c.base & 3)) >> 2) + 1;
      if (c.base != row_base || n32 > row_n32) {
        const uint32_t* g32 = reinterpret_cast<const uint32_t*>(A.pk8) + (c.base >> 2);
        uint32_t* l32 = reinterpret_cast<uint32_t*>(s_row);
        for (int i = lane; i < n32; i += 64) l32[i] = g32[i];
        row_base = c.base;
        row_n32 = n32;
      }
      wave_lds_sync();   // lanes read row words other lanes staged
    }
    STREAM_PSTAMP(1);
    const uint8_t* row = s_row + (c.base & 3);
    const bool fast = pk_lds && c.kinc2 <= kFastKinc2;
    const float invD = 1.0f / (float)c.D;
    // the next call's first piece (prefetched during this call's last piece)
    int64_t e_next = -1;
    if (k + 1 < A.n_calls && A.xcall_prefetch) {
      if (closed) {
        if (active) e_next = e_call + A.call_elems;   // gpsisr keeps prn and stream
      } else {
        const gnsscorr_nco_cmd& nc = A.cmds[(int64_t)(k + 1) * A.cmd_step + chn];
        if (nc.prn > 0 && nc.prn <= 32)
          e_next = (int64_t)nc.stream * A.stream_stride * 2 + (int64_t)(k + 1) * A.call_elems;
      }
    }
    // keep one piece in flight: the rest of this call, then the next call's
    auto top_up = [&]() {
      while (iss == con) {
        int nk = q_k, np = q_p + 1;
        if (np >= n_pieces) {
          nk++;
          np = 0;
        }
        if (nk == k) issue(k, np, e_call);
        else if (nk == k + 1 && e_next >= 0) issue(k + 1, np, e_next);
        else break;
      }
    };
    if (active) top_up();

    Acc acc;
#pragma unroll
    for (int q = 0; q < 6; q++) acc.a[q] = 0;
    int e = -1;   // epoch of acc (-1: nothing yet)
    Seg g;
    // the carrier and code NCO phases at the lane's first sample, advanced by one
    // piece (kPieceSpan samples: uniform steps) per piece with full-rate adds, not
    // a 32 x 32-bit and a 64-bit multiply per piece (quarter rate)
    // (the carrier phase steps in g.p0 itself where the pair loops do not advance
    // it, i.e. with the LO words read ahead)
    const uint32_t p0_step = (uint32_t)kPieceSpan * c.cinc;
    if constexpr (kPF) g.p0 = c.P0 + (uint32_t)(lane * kPieceLen) * c.cinc - p0_step;
    uint64_t x_cur = (uint64_t)c.K0 + (uint64_t)(uint32_t)(lane * kPieceLen) * c.kinc2;
    const uint64_t x_step = (uint64_t)kPieceSpan * c.kinc2;
    for (int p = 0; active && p < n_pieces; p++) {
      const int n0 = p * kPieceSpan + lane * kPieceLen;
      const int L = max(0, min(kPieceLen, nsamp - n0));
      if constexpr (kPF) g.p0 += p0_step;   // c.P0 + n0 cinc
      else g.p0 = c.P0 + (uint32_t)n0 * c.cinc;
      // the piece's 16 LO word pairs (pair q: carrier phases p0 + 2q cinc and
      // p0 + (2q + 1) cinc, correlator.c:203-204), read before the piece's IF
      // wait so that both LDS round trips overlap
      uint32_t lwx[kPieceLen / 2], lwy[kPieceLen / 2];
      if (kPF && fast) {
        uint32_t pa = g.p0;
#pragma unroll
        for (int q = 0; q < kPieceLen / 2; q++) {
          const uint32_t pb = pa + c.cinc;
          const uint32_t off = ((pa >> 27) & 0x1Cu) | ((pb >> 24) & 0xE0u);   // 4 (a | b << 3)
          const uint8_t* t = reinterpret_cast<const uint8_t*>(s_lot) + off;
          lwx[q] = *reinterpret_cast<const uint32_t*>(t);
          lwy[q] = *reinterpret_cast<const uint32_t*>(t + 256);
          pa = pb + c.cinc;
        }
      }
      // ---- this lane's 32 samples as 16 pair words (4 chunks of 4)
      uint4 ch4[4];
      if constexpr (PK) {
        auto x2 = [&](uint32_t w) {
          return make_uint4(s_x2[w & 0xFFu], s_x2[(w >> 8) & 0xFFu], s_x2[(w >> 16) & 0xFFu],
                            s_x2[w >> 24]);
        };
        ch4[0] = x2(pq0.x);
        ch4[1] = x2(pq0.y);
        ch4[2] = x2(pq1.x);
        ch4[3] = x2(pq1.y);
      } else {
        if (p * kPieceSpan + kPieceSpan > nsamp && (nsamp & 7)) {
          // the call's partial last chunk (nsamp not a multiple of 8; single
          // calls only): whole words and the odd sample by ordinary loads
          const int n_piece = p * kPieceSpan;
          const int valid = nsamp - n_piece;
          const int i = valid / 8;
          if (lane == (i & 63)) {
            const int rem = valid - i * 8;
            const uint32_t* g32 =
                reinterpret_cast<const uint32_t*>(A.ifbuf + e_call + 2 * (int64_t)n_piece) + 4 * i;
            uint32_t t[4] = {0u, 0u, 0u, 0u};
            for (int q = 0; q < rem / 2; q++) t[q] = g32[q];
            if (rem & 1) t[rem / 2] = (uint32_t)reinterpret_cast<const uint16_t*>(g32)[rem - 1];
            slot[slot_entry(i)] = make_uint4(t[0], t[1], t[2], t[3]);
          }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the piece has landed in the slot
        if (p == 0) STREAM_PSTAMP(2);
#pragma unroll
        for (int j = 0; j < 4; j++) ch4[j] = slot[slot_entry(4 * lane + j)];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // ... and is in registers
      }
      con = __builtin_amdgcn_readfirstlane(con + 1);
      top_up();   // the slot just read takes the next piece
      const uint64_t X = x_cur;   // c.K0 + n0 kinc2
      x_cur += x_step;
      const uint64_t r0 = X >> 32;
      g.kph = (uint32_t)X;
      uint32_t ep = (uint32_t)e;   // (lanes past the call's end keep their epoch)
      if (L > 0) {
        if (fast) hc_after_fast(c, r0, invD, g.hc, g.ld, ep);
        else hc_after(c, r0, g.hc, g.ld, ep);
      }
      {   // a piece that starts in a later epoch than the lane's sums (rare; every
          // lane still active: flush_lanes' DPP scans)
        uint64_t any = __builtin_amdgcn_ballot_w64((int)ep != e);
        asm volatile("" : "+s"(any));
        if (any) {
          flush_lanes<true>((int)ep != e && e >= 0, acc, e, s_sum, lane);
          e = (int)ep;
        }
      }
      if (L == 0) continue;
      if (fast) {
        if constexpr (kPF) {
          g.cb = row[g.ld];
          g.nb = row[g.hc + 1];
          unpack8(g.cb, g.lb, g.pb, g.eb);
        } else {
          unpack8(row[g.ld], g.lb, g.pb, g.eb);
        }
        g.ti = g.tq = g.pi = g.pq = 0;
        g.carried = false;
        // intervals of kIv pairs: 3 (6 samples) whenever a half-chip lasts >= 6
        // samples; 4 (8 samples, 4 interval ends per piece instead of 6) when it
        // lasts >= 8, i.e. 8 kinc2 <= 2^32 (at 16.368 Msps: code rates up to the
        // nominal 2.046 MHz of half-chips), still at most one carry per interval
        auto full_piece = [&](auto dumps_tag, auto iv_tag) {
          constexpr bool kD = decltype(dumps_tag)::value;
          constexpr int kIv = decltype(iv_tag)::value;
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const uint32_t words[4] = {ch4[j].x, ch4[j].y, ch4[j].z, ch4[j].w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
              const int q = 4 * j + i;
              if constexpr (kPF) pair2r<false>(words[i], lwx[q], lwy[q], c, g);
              else pair2s<false>(words[i], c, g, lox, loy);
              if (q % kIv == kIv - 1 || q == kPieceLen / 2 - 1)
                interval_end_s<kPF, kD>(c, g, acc, e, s_sum, row);
            }
          }
        };
        // a piece in which every lane's code carries fall at one offset j in each
        // of its four 8-sample intervals (chunk t = samples 8t .. 8t + 7, carry
        // between samples 8t + j - 1 and 8t + j): the part of a pair before the
        // carry has a mask fixed for the piece, so a pair is one AND and four dot4
        // (no NCO step or carry test per pair), and every interval ends on a carry
        auto aligned_piece = [&](const uint32_t (&mq)[4]) {
#pragma unroll
          for (int t = 0; t < 4; t++) {
            const uint32_t words[4] = {ch4[t].x, ch4[t].y, ch4[t].z, ch4[t].w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
              uint32_t lo_x, lo_y;
              if constexpr (kPF) {
                lo_x = lwx[4 * t + i];
                lo_y = lwy[4 * t + i];
              } else {
                pair_lo(c, g, lox, loy, lo_x, lo_y);
              }
              pair_dots(words[i], mq[i], lo_x, lo_y, g);
            }
            seg_carry(g, acc);
            g.hc += 1u;   // no dump in the piece (the caller's ballot)
            if constexpr (kPF) {
              g.cb = g.nb;
              unpack8(g.cb, g.lb, g.pb, g.eb);
              g.nb = row[g.hc + 1];
            } else {
              g.ld = g.hc;
              unpack8(row[g.ld], g.lb, g.pb, g.eb);
            }
          }
        };
        if (__all(L == kPieceLen)) {
          // whether any lane's 32 samples hold a dump: its half-chip count at the
          // window start plus the window's code carries, (kph + 32 kinc2) >> 32,
          // reaches D (one dump per ~16 k samples, so 7 of 8 pieces have none and
          // skip the dump test at every interval end)
          const bool dump_here =
              g.hc + (uint32_t)(((uint64_t)g.kph + (uint64_t)kPieceLen * c.kinc2) >> 32) >= c.D;
          uint64_t anyd = __builtin_amdgcn_ballot_w64(dump_here);
          asm volatile("" : "+s"(anyd));
          using I3 = std::integral_constant<int, 3>;
          using I4 = std::integral_constant<int, 4>;
          bool aligned = false;
          if (!anyd) {
            // j: samples before the lane's first carry (sample n has half-chip
            // hc + h(n), h(n) = (kph + n kinc2) >> 32), estimated in fp32 and
            // checked exactly.  h(j - 1) = 0, h(j) = 1, h(j + 23) = 3, h(j + 24) = 4
            // put the carries at j, j + 8, j + 16, j + 24: three spacings summing to
            // 24 from {floor P, ceil P} (P samples per half-chip) are all 8, and the
            // next carry (>= j + 31) is past the piece
            const float r = (4294967296.0f - (float)g.kph) * __builtin_amdgcn_rcpf((float)c.kinc2);
            const int j = min(8, max(1, (int)__builtin_ceilf(r)));
            // with Y = kph + j kinc2 and Z = Y + 24 kinc2: h(j) = 1 and h(j + 24) = 4 are
            // their high words; then h(j - 1) = 0 iff Y - kinc2 < 2^32, i.e. lo(Y) < kinc2,
            // and h(j + 23) = 3 iff lo(Z) < kinc2 (one 64-bit multiply, not four)
            const uint64_t Y = (uint64_t)g.kph + (uint64_t)(uint32_t)j * c.kinc2;
            const uint64_t Z = Y + 24ull * c.kinc2;
            const bool ok = (uint32_t)(Y >> 32) == 1u && (uint32_t)Y < c.kinc2 &&
                            (uint32_t)(Z >> 32) == 4u && (uint32_t)Z < c.kinc2;
            uint64_t bad = __builtin_amdgcn_ballot_w64(!ok);
            asm volatile("" : "+s"(bad));
            if (!bad) {
              uint32_t mq[4];
#pragma unroll
              for (int i = 0; i < 4; i++)
                mq[i] = j >= 2 * i + 2 ? 0xFFFFFFFFu : (j == 2 * i + 1 ? 0xFFFFu : 0u);
              aligned_piece(mq);
              aligned = true;
            }
          }
          if (aligned) {
          } else if (!anyd) {
            if (c.kinc2 <= kIv4Kinc2) full_piece(std::false_type{}, I4{});
            else full_piece(std::false_type{}, I3{});
          } else {
            full_piece(std::true_type{}, I3{});
          }
        } else {
          const int np = L >> 1;
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const uint32_t words[4] = {ch4[j].x, ch4[j].y, ch4[j].z, ch4[j].w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
              const int q = 4 * j + i;
              if constexpr (kPF) {
                if (q < np) pair2r<false>(words[i], lwx[q], lwy[q], c, g);
                else if (q == np && (L & 1)) pair2r<true>(words[i] & 0xFFFFu, lwx[q], lwy[q], c, g);
              } else {
                if (q < np) pair2s<false>(words[i], c, g, lox, loy);
                else if (q == np && (L & 1)) pair2s<true>(words[i] & 0xFFFFu, c, g, lox, loy);
              }
              if (q % 3 == 2 || q == kPieceLen / 2 - 1) interval_end_s<kPF>(c, g, acc, e, s_sum, row);
            }
          }
        }
        seg_flush(g.ti, g.tq, g.lb, g.pb, g.eb, acc);   // the open segment
      } else {
        uint32_t hc = g.hc;
        int lb, pb, eb;
        if (pk_lds) {
          unpack8(row[g.ld], lb, pb, eb);
        } else {
          unpack_pk(A.pk[c.base + (int)g.ld], lb, pb, eb);
        }
        uint32_t phase = g.p0, kph = g.kph;
        auto per_sample = [&](auto row_tag) {
          constexpr bool kRow = decltype(row_tag)::value;
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const uint32_t words[4] = {ch4[j].x, ch4[j].y, ch4[j].z, ch4[j].w};
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
              for (int hh = 0; hh < 2; hh++)
                if (2 * (4 * j + i) + hh < L)
                  corr_sample_s<kRow>(sbyte((int)words[i], 2 * hh),
                                      sbyte((int)words[i], 2 * hh + 1), phase, kph, c, hc, lb, pb,
                                      eb, acc, e, s_sum, row, A.pk);
          }
        };
        if (pk_lds) per_sample(std::true_type{});
        else per_sample(std::false_type{});
      }
    }
    flush_lanes<false>(e >= 0, acc, e, s_sum, lane);   // (the next call starts from zero)
    if (!active && iss != con) {
      // a prefetch for a call that turned out idle must land before the slot is reused
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      con = iss;
      q_k = q_p = -1;
    }
    wave_lds_sync();   // every lane's flushes land before lane 0 reads the sums
    STREAM_PSTAMP(3);
    // ---- the channel's epilogue (and closed loop: its gpsisr step) on lane 0; the
    // epoch sums are complete (the LDS operations of a wave execute in order)
    // lane 0's new state and command go to every lane by readfirstlane (an LDS
    // round trip would need a fence: without one the compiler may hoist the
    // other lanes' reads above lane 0's writes)
    uint32_t bw[20];
#pragma unroll
    for (int i = 0; i < 20; i++) bw[i] = 0u;
    if (lane == 0) {
      const uint64_t Rtot = ((uint64_t)c.K0 + (uint64_t)nsamp * c.kinc2) >> 32;
      gnsscorr_chan_state nst;
      const gnsscorr_track_result rr = channel_epilogue(
          c, cmd, st, chn, active, active ? n_dumps_after(c, Rtot) : 0u, Rtot, nsamp, tic_k,
          [&](int i) { return (uint32_t)s_sum[i]; }, A.res + (int64_t)k * C, A.state,
          A.n_calls == 1 ? A.all_dumps : nullptr, A.max_dumps, &nst);
      gnsscorr_nco_cmd r = cmd;
      if constexpr (CLOSED) {   // osgpsisr.c:360-768, osg_isr_kernel's body
        gnsscorr_osg_loop lc = A.loops[chn];
        osgisr::isr_step(A.lk, lc, r, rr);
        A.loops[chn] = lc;
        if (A.hist) A.hist[(int64_t)k * C + chn] = lc;
        if (k + 1 == A.n_calls) A.cmds[chn] = r;
      }
      memcpy(bw, &nst, sizeof nst);
      memcpy(bw + 14, &r, sizeof r);
    }
    {
      static_assert(sizeof(gnsscorr_chan_state) == 56 && sizeof(gnsscorr_nco_cmd) == 24, "bw");
      uint32_t* sv = reinterpret_cast<uint32_t*>(&st);
#pragma unroll
      for (int i = 0; i < 14; i++) sv[i] = (uint32_t)__builtin_amdgcn_readfirstlane((int)bw[i]);
      if (closed) {
        uint32_t* rv = reinterpret_cast<uint32_t*>(&cmd);
#pragma unroll
        for (int i = 0; i < 6; i++) rv[i] = (uint32_t)__builtin_amdgcn_readfirstlane((int)bw[14 + i]);
      }
    }
  }
  STREAM_PSTAMP(5);
}

}  // namespace

// (track_ctx.h)
int track_stream_launch(gnsscorr_track_ctx* c, const int8_t* d_if, int64_t stride, int64_t nsamp,
                        int n_calls, gnsscorr_nco_cmd* d_cmds, int cmd_step,
                        gnsscorr_track_result* d_res, int32_t* d_dumps, int64_t tic,
                        int tic_explicit, const gnsscorr_osg_loop_cfg* lcfg,
                        gnsscorr_osg_loop* d_loops, gnsscorr_osg_loop* d_hist) {
  const bool pk = packed(c), iq = bps_of(c) == 2;
  if (!iq) return GNSSCORR_TRACK_NOT_FUSED;
  if (int rc = gnsscorr_track_check_steps(c, d_if, stride, nsamp, 1)) return rc;
  // later calls start at + k * nsamp samples: the same alignment, and whole
  // 8-sample chunks (the partial-chunk path is for single calls)
  if (n_calls > 1 && ((nsamp * 2) & (pk ? 31 : 15))) return GNSSCORR_TRACK_NOT_FUSED;
  const int C = c->cfg.n_channels;
  size_t dyn = (size_t)stream_wave_lds(pk, (int)nsamp) * kStreamCh;
  constexpr size_t kStatic = 2048;   // s_lot, s_x2 (packed), with margin
  // every permitted nsamp fits the 64 KiB any workgroup may allocate
  static_assert(stream_wave_lds(false, kMaxNsamp) * kStreamCh + kStatic <= 64 * 1024, "stream LDS");
  if (dyn + kStatic > c->lds_max) {
    gnsscorr_set_error("gnsscorr_track: nsamp %lld needs %zu B of LDS per workgroup, the device "
                       "allows %zu", (long long)nsamp, dyn + kStatic, c->lds_max);
    return GNSSCORR_EINVAL;
  }
  // A launch takes as long as its busiest CU.  The dispatcher fills a CU with
  // as many workgroups as its resources allow, so at 768 workgroups on 256 CUs
  // some CUs got 4-5 while others got 2 (wave stamps: pieces p10 16.6 / p90
  // 27 us).  Asking for enough LDS that at most ceil(workgroups / CUs) fit on
  // a CU spreads them evenly.
  const int n_wg = (C + kStreamCh - 1) / kStreamCh;
  const int per_cu = (n_wg + c->n_cu - 1) / c->n_cu;
  // Only when the launch has more workgroups than CUs: with at most one per CU
  // the dispatcher spreads them already, and the padding would only lock other
  // streams' kernels out of those CUs' LDS (co-residency).
  if (c->balance && n_wg > c->n_cu) {
    const size_t cap = c->lds_max / (size_t)(per_cu + 1) + 16;   // per_cu + 1 no longer fit
    if (cap > dyn && (cap + kStatic) * per_cu <= c->lds_max) dyn = cap;
  }
  StreamArgs A;
  memset(&A, 0, sizeof A);
  A.ifbuf = d_if;
  A.stream_stride = stride;
  A.call_elems = nsamp * 2;
  A.nsamp = (int)nsamp;
  A.n_channels = C;
  A.n_calls = n_calls;
  A.cmd_step = cmd_step;
  A.cmds = d_cmds;
  A.state = c->d_state;
  A.res = d_res;
  A.all_dumps = d_dumps;
  A.max_dumps = c->max_dumps;
  A.pk = c->d_pk;
  A.pk8 = c->d_pk8;
  A.tic = tic;
  A.tic_ref = c->tic_ref;
  A.tic_explicit = tic_explicit;
  A.xcall_prefetch = c->xcall_prefetch;
  if (lcfg) A.lk = *lcfg;
  A.loops = d_loops;
  A.hist = d_hist;
  dim3 grid(n_wg), block(64 * kStreamCh);
  // the closed loop's gpsisr in its own instantiation: its registers stay out of
  // the open-loop kernel
  if (pk && d_loops) hipLaunchKernelGGL((osg_stream_kernel<true, true>), grid, block, dyn, c->stream, A);
  else if (pk) hipLaunchKernelGGL((osg_stream_kernel<true, false>), grid, block, dyn, c->stream, A);
  else if (d_loops) hipLaunchKernelGGL((osg_stream_kernel<false, true>), grid, block, dyn, c->stream, A);
  else hipLaunchKernelGGL((osg_stream_kernel<false, false>), grid, block, dyn, c->stream, A);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}
