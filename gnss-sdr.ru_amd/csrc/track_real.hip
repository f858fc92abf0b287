// track_real.hip -- the I-only engine of the OSG tracking correlator:
// osg_track_kernel, real-sample streams (int8 or 2-bit packed) as thread groups
// of 64-sample runs.  The closed form it starts every run from and the
// per-channel epilogue are osg_chan.h's; track.hip's head comment maps them onto
// Sim_GP2021_int (correlator.c:148-316).  Accumulation is int32
// two's-complement, so per-thread partial sums can be combined in any order:
// each thread keeps at most two epochs' sums (a run of 64 samples can straddle
// at most one dump, D >= 2046), the wavefront reduces them with cross-lane
// shuffles and one lane per wave adds into an LDS slot per epoch.
#include <hip/hip_runtime.h>
#include <limits.h>
#include "gnsscorr_internal.h"
#include "if2.h"
#include "osg_chan.h"
#include "track_ctx.h"

namespace {
using namespace osgchan;

constexpr int kRun = 64;              // samples per thread
constexpr int kMaxThreads = 1024;
static_assert(kRun * kMaxThreads == kMaxNsamp, "one thread per run of the longest call");
constexpr int kMaxCpw = 4;            // channels per workgroup (32 waves/CU: two 1024-thread WGs)

// Wave-wide reductions without the LDS crossbar (ds_bpermute): a DPP
// Hillis-Steele scan inside each 16-lane row (row_shr 1/2/4/8, identity
// shifted in), then the four row results (lanes 15/31/47/63) combined in
// scalar registers.  Every lane of the wave must be active.
template <typename Op>
__device__ __forceinline__ int wave_reduce(int v, int ident, Op op) {
  v = op(v, __builtin_amdgcn_update_dpp(ident, v, 0x111, 0xF, 0xF, false));
  v = op(v, __builtin_amdgcn_update_dpp(ident, v, 0x112, 0xF, 0xF, false));
  v = op(v, __builtin_amdgcn_update_dpp(ident, v, 0x114, 0xF, 0xF, false));
  v = op(v, __builtin_amdgcn_update_dpp(ident, v, 0x118, 0xF, 0xF, false));
  const int a = __builtin_amdgcn_readlane(v, 15), b = __builtin_amdgcn_readlane(v, 31);
  const int c = __builtin_amdgcn_readlane(v, 47), d = __builtin_amdgcn_readlane(v, 63);
  return op(op(a, b), op(c, d));
}
__device__ __forceinline__ int wave_sum(int v) {
  return wave_reduce(v, 0, [](int x, int y) { return (int)((uint32_t)x + (uint32_t)y); });
}
__device__ __forceinline__ int wave_max(int v) {
  return wave_reduce(v, INT_MIN, [](int x, int y) { return max(x, y); });
}
__device__ __forceinline__ int wave_min(int v) {
  return wave_reduce(v, INT_MAX, [](int x, int y) { return min(x, y); });
}

// one real sample of the reference recurrence (correlator.c:200-283) on a
// thread's (first, cur) epoch sums
__device__ __forceinline__ void corr_sample(int I, uint32_t& phase, uint32_t& kph, const Chan& c,
                                            uint32_t& hc, int& lb, int& pb, int& eb, Acc& cur,
                                            Acc& first, bool& switched,
                                            const uint32_t* __restrict__ pk) {
  int il, ql;
  sample_lo(phase, il, ql);
  sample_acc(I * il, I * ql, lb, pb, eb, cur);   // correlator.c:222-223
  if (sample_nco(c, phase, kph)) {
    hc = (hc + 1u) & 0xFFFFu;
    const uint32_t ld = hc;
    if (hc >= c.D) {  // dump (correlator.c:251-281)
#pragma unroll
      for (int k = 0; k < 6; k++) { first.a[k] = cur.a[k]; cur.a[k] = 0; }
      switched = true;
      hc = 0;
    }
    unpack_pk(pk[c.base + (int)ld], lb, pb, eb);
  }
}

// Epoch-segmented reduction of the per-thread sums and the per-channel epilogue
// (one thread per channel): dumps, ms/bit counters, TIC latch, carrier cycles and
// the new channel state (correlator.c:243-316).  Every thread of the workgroup
// calls it (it holds a barrier).
__device__ __forceinline__ void finish_call(const Chan& c, const gnsscorr_nco_cmd& cmd,
                                            gnsscorr_chan_state st, int chn, bool have,
                                            bool active, int tid, bool runs, int e0,
                                            bool switched, const Acc& first, const Acc& cur,
                                            int32_t* s_sum, uint32_t ndump, uint64_t Rtot,
                                            int nsamp, int64_t tic_count,
                                            gnsscorr_track_result* __restrict__ res,
                                            gnsscorr_chan_state* __restrict__ state,
                                            int32_t* __restrict__ all_dumps, int max_dumps) {
  // ---- epoch-segmented reduction ------------------------------------------
  // thread contributes (e0, switched ? first : cur) and (e0+1, cur) if switched
  // (a wave never spans two thread groups: T is a multiple of 64)
  const int e_hi_mine = e0 + (switched ? 1 : 0);
  const int e_lo = wave_min(runs ? e0 : 0x7fffffff);
  const int e_hi = wave_max(runs ? e_hi_mine : -1);
  const int lane = threadIdx.x & 63;
  for (int e = e_lo; e <= e_hi; e++) {
#pragma unroll
    for (int k = 0; k < 6; k++) {
      uint32_t v = 0;
      if (e == e0) v += switched ? first.a[k] : cur.a[k];
      if (switched && e == e0 + 1) v += cur.a[k];
      const int s = wave_sum((int)v);
      if (lane == 0) atomicAdd(&s_sum[e * 6 + k], s);
    }
  }
  __syncthreads();

  // ---- per-channel epilogue (one thread per channel) ------------------------
  if (tid != 0 || !have) return;
  channel_epilogue(c, cmd, st, chn, active, ndump, Rtot, nsamp, tic_count,
                   [&](int i) { return (uint32_t)s_sum[i]; }, res, state, all_dumps, max_dumps);
}

// ============================================================================
// osg_track_kernel: real-sample (I-only) streams, int8 or 2-bit packed (PK:
// GNSSCORR_IF_PACKED2, if2.h).  Interleaved I,Q streams run on
// osg_stream_kernel (track.hip).
//
// One workgroup = cpw channels (cpw = 1024 / threads-per-channel, at most
// kMaxCpw) x one call; thread group q = threadIdx.x / T runs channel
// grp * cpw + q.  Every thread walks its own run of kRun samples with the
// reference recurrence (corr_sample): 256 threads x 64 samples cover a 1-ms
// chunk at 16.368 Msps.  Full int8 runs are read as 16-byte vector loads, tail
// runs and packed runs element by element.
// ============================================================================
template <bool PK>
__global__ __launch_bounds__(kMaxThreads, 8) void osg_track_kernel(
    const int8_t* __restrict__ ifbuf, int64_t stream_stride, int nsamp, int n_channels, int cpw,
    const gnsscorr_nco_cmd* __restrict__ cmds, gnsscorr_chan_state* __restrict__ state,
    gnsscorr_track_result* __restrict__ res, int32_t* __restrict__ all_dumps, int max_dumps,
    const uint32_t* __restrict__ pk, int64_t tic_count) {
  // dynamic LDS: [cpw][ep_cap][6] epoch sums
  extern __shared__ uint4 s_dyn[];
  const int ep_cap = epoch_cap(nsamp);
  const int T = (int)blockDim.x / cpw;
  // wave-uniform (T is a multiple of 64): keeps the channel's command, state
  // and NCO constants in scalar registers
  const int q = __builtin_amdgcn_readfirstlane((int)threadIdx.x / T);
  const int tid = (int)threadIdx.x - q * T;
  int32_t* s_sum = reinterpret_cast<int32_t*>(s_dyn) + q * ep_cap * 6;
  const int chn = xcd_channel(blockIdx.x, gridDim.x) * cpw + q;
  const bool have = chn < n_channels;
  gnsscorr_nco_cmd cmd = {};
  gnsscorr_chan_state st = {};
  if (have) {
    cmd = cmds[chn];
    st = state[chn];
  }
  Chan c;
  const bool active = chan_setup(cmd, st, c) && have;
  const uint64_t Rtot = ((uint64_t)c.K0 + (uint64_t)nsamp * c.kinc2) >> 32;
  const uint32_t ndump = n_dumps_after(c, Rtot);
  const int n_epochs = (int)ndump + 1;
  if (active)
    for (int i = tid; i < n_epochs * 6; i += T) s_sum[i] = 0;
  __syncthreads();

  // ---- per-thread run of kRun samples --------------------------------------
  Acc cur, first;
#pragma unroll
  for (int k = 0; k < 6; k++) { cur.a[k] = 0; first.a[k] = 0; }
  bool switched = false;
  int e0 = 0;
  const int n0 = tid * kRun;
  const bool runs = active && n0 < nsamp;
  if (runs) {
    const uint64_t X = (uint64_t)c.K0 + (uint64_t)n0 * c.kinc2;
    uint32_t kph = (uint32_t)X;
    uint32_t phase = c.P0 + (uint32_t)n0 * c.cinc;
    uint32_t hc, ld, ep;
    hc_after(c, X >> 32, hc, ld, ep);
    e0 = (int)ep;
    int lb, pb, eb;
    unpack_pk(pk[c.base + (int)ld], lb, pb, eb);
    // element offset of the run (a multiple of 64: n0 and the stream base are);
    // src is its first byte in either format
    const int64_t e_run = (int64_t)cmd.stream * stream_stride + n0;
    const int8_t* src = PK ? ifbuf + (e_run >> 2) : ifbuf + e_run;
    if (!PK && n0 + kRun <= nsamp) {
      const int4* v = reinterpret_cast<const int4*>(src);
#pragma unroll
      for (int j = 0; j < kRun / 16; j++) {
        const int4 u = v[j];
        const int words[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int wd = 0; wd < 4; wd++)
#pragma unroll
          for (int b = 0; b < 4; b++)
            corr_sample(sbyte(words[wd], b), phase, kph, c, hc, lb, pb, eb, cur, first, switched, pk);
      }
    } else {   // per sample (tail runs; every packed run)
      const int L = min(kRun, nsamp - n0);
      for (int k = 0; k < L; k++)
        corr_sample(if_elem(src, k, PK), phase, kph, c, hc, lb, pb, eb, cur, first, switched, pk);
    }
  }
  finish_call(c, cmd, st, chn, have, active, tid, runs, e0, switched, first, cur, s_sum, ndump, Rtot,
              nsamp, tic_count, res, state, all_dumps, max_dumps);
}

}  // namespace

// one thread per 64-sample run, as many channels per workgroup as fit 1024 threads
int track_real_launch(gnsscorr_track_ctx* c, const int8_t* d_if, int64_t stride, int64_t nsamp,
                      const gnsscorr_nco_cmd* d_cmds, gnsscorr_track_result* d_res,
                      int32_t* d_dumps, int64_t tic) {
  const int C = c->cfg.n_channels;
  const int threads = ((int)((nsamp + kRun - 1) / kRun) + 63) & ~63;
  const int cpw = min(kMaxCpw, kMaxThreads / threads);
  // dynamic LDS: the channels' epoch sums (under 1 KiB at every permitted nsamp)
  const size_t dyn = (size_t)cpw * epoch_cap((int)nsamp) * 6 * sizeof(int32_t);
  dim3 grid((C + cpw - 1) / cpw), block(threads * cpw);
  if (packed(c))
    hipLaunchKernelGGL((osg_track_kernel<true>), grid, block, dyn, c->stream, d_if, stride, (int)nsamp,
                       C, cpw, d_cmds, c->d_state, d_res, d_dumps, c->max_dumps, c->d_pk, tic);
  else
    hipLaunchKernelGGL((osg_track_kernel<false>), grid, block, dyn, c->stream, d_if, stride, (int)nsamp,
                       C, cpw, d_cmds, c->d_state, d_res, d_dumps, c->max_dumps, c->d_pk, tic);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}
