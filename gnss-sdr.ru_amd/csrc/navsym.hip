// navsym.hip -- navigation symbols of Galileo E1B and GLONASS L3OC on the device
// ("nav"): synchronisation, deinterleaving and the K = 7 Viterbi decoder of the
// Scilab receiver's symbol chain, read from the trackers' epoch records in place.
//   GALILEO/E1/findPageStart.sci:39-63, GALILEO/E1/include/decode_gll_data.sci:16-39
//   GLONASS/L3/test_data_decode.sce:19-83
//   */convolution_decoding/convol_decoder.sci, convol_decoder_soft.sci,
//   convol_encoder.sci:50-57
// Everything here is integer or fp64-without-contraction arithmetic in the
// files' order: bits and positions are exact ("nav").
//
// nav_viterbi_kernel: one wave64 per stream, lane = state.  State s holds the
// last six inputs, newest in bit 5; new state l comes from p0 = 2 (l mod 32) or
// p0 + 1 with input l div 32.  A step is two lane permutes of the metric, two
// branch costs, one compare (the odd predecessor wins only when strictly
// smaller) and one ballot: the 64 decisions of a step are one 64-bit word.  The
// files' decision for bit c walks every state after step c + 41 back to step c
// and takes, of the states still alive, the smallest metric after step c (the
// lowest state on ties): the alive set is a 64-bit mask, and one step back is
//   X1 = A & D, X0 = A & ~D, A' = spread(fold(X0)) | spread(fold(X1)) << 1
// with fold = or of the two 32-bit halves and spread = bit k to bit 2k.  The
// walks of different bits do not depend on each other, so every 64 steps the
// wave's lanes run 64 of them side by side out of an LDS ring of the last
// kRing decision words and metric rows.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include "gnsscorr_internal.h"
#include "hostctx.h"
#include "nav_host.h"

namespace {

constexpr int kWin = 42;                  // f = 6 m steps in the decoding window
constexpr int kRing = 64 + kWin - 1;      // steps c0 .. c0 + 63 + 41 of one block of 64 bits
constexpr int kStartMetric = 10000;       // convol_decoder.sci:65
constexpr uint32_t kGen1 = 0x5B, kGen2 = 0x79;   // [1 0 1 1 0 1 1], [1 1 1 1 0 0 1], input first
// metrics are never normalised: 10000 + 2 T must fit an int32
constexpr int kMaxBits = (INT_MAX - kStartMetric) / 2 - kWin;
constexpr int kE1Page = 1000, kE1Syms = 240, kE1Bits = 120;
// entries that are -1, entry i in bit i
constexpr uint32_t kE1SyncNeg = 0x3E5;    // [-1 1 -1 1 1 -1 -1 -1 -1 -1]
constexpr uint32_t kNhNeg = 0x14F;        // [-1 -1 -1 -1 1 1 -1 1 -1 1]
constexpr uint32_t kBarkerNeg = 0x17;     // [-1 -1 -1 1 -1]
constexpr uint32_t kTimeMarkNeg = 0x8D6DF; // test_data_decode.sce:82
constexpr int kThreads = 256;

__device__ __forceinline__ uint64_t spread32(uint32_t v) {   // bit k -> bit 2k
  uint64_t x = v;
  x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
  x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
  x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | (x << 2)) & 0x3333333333333333ull;
  x = (x | (x << 1)) & 0x5555555555555555ull;
  return x;
}

// the states alive one step earlier: the predecessors the alive states chose
__device__ __forceinline__ uint64_t step_back(uint64_t alive, uint64_t dec) {
  const uint64_t x1 = alive & dec, x0 = alive & ~dec;
  return spread32((uint32_t)(x0 | (x0 >> 32))) | (spread32((uint32_t)(x1 | (x1 >> 32))) << 1);
}

// convol_decoder.sci:111, the Hamming distance of the pair to the branch output
__device__ __forceinline__ int branch_cost(int r1, int r2, int o1, int o2, int metric) {
  return ((r1 ^ o1) & 1) + ((r2 ^ o2) & 1) + metric;
}
// convol_decoder_soft.sci:120-122: sum(diffCode.^2) + Dist, in that order
__device__ __forceinline__ double branch_cost(double r1, double r2, int o1, int o2,
                                              double metric) {
#pragma clang fp contract(off)
  const double e1 = r1 - (double)o1, e2 = r2 - (double)o2;
  const double s = e1 * e1 + e2 * e2;
  return s + metric;
}

// code: uint8 0/1 pairs (hard) or fp64 pairs (soft), stream s at s * stride bytes.
// len: null, or the number of bits of each stream (0 .. l_max; bits past it are
// written as 0).  bits: stream s at s * l_max.
template <bool Soft>
__global__ __launch_bounds__(64) void nav_viterbi_kernel(const void* __restrict__ code,
                                                         int64_t stride, int l_max,
                                                         const int32_t* __restrict__ len,
                                                         uint8_t* __restrict__ bits) {
  using Rx = typename std::conditional<Soft, double, uint8_t>::type;
  using Metric = typename std::conditional<Soft, double, int>::type;
  __shared__ uint64_t dec[kRing];
  __shared__ Metric rows[kRing][64];
  __shared__ Rx rx[128];
  const int lane = threadIdx.x;
  const int64_t stream = blockIdx.x;
  const Rx* src = (const Rx*)((const char*)code + stream * stride);
  uint8_t* out = bits + stream * (int64_t)l_max;
  int L = l_max;
  if (len) {
    L = min(max(len[stream], 0), l_max);
    for (int c = L + lane; c < l_max; c += 64) out[c] = 0;
  }
  if (L < 1) return;

  const int p0 = 2 * (lane & 31), u = lane >> 5;
  const uint32_t reg0 = (uint32_t)(u << 6 | p0), reg1 = reg0 | 1u;
  const int a1 = __popc(reg0 & kGen1) & 1, a2 = __popc(reg0 & kGen2) & 1;
  const int b1 = __popc(reg1 & kGen1) & 1, b2 = __popc(reg1 & kGen2) & 1;
  Metric metric = lane == 0 ? (Metric)0 : (Metric)kStartMetric;
  const int T = L + kWin - 1;
  int slot = 0;                             // t mod kRing
  for (int t = 0; t < T; t++) {
    const int i = t & 63;
    if (i == 0) {                           // the next 64 received pairs, (0, 0) past L
      __syncthreads();
      const int tt = t + lane;
      rx[2 * lane] = tt < L ? src[2 * (int64_t)tt] : (Rx)0;
      rx[2 * lane + 1] = tt < L ? src[2 * (int64_t)tt + 1] : (Rx)0;
      __syncthreads();
    }
    const Metric m0 = __shfl(metric, p0), m1 = __shfl(metric, p0 + 1);
    Metric c0, c1;
    if constexpr (Soft) {
      c0 = branch_cost(rx[2 * i], rx[2 * i + 1], a1, a2, m0);
      c1 = branch_cost(rx[2 * i], rx[2 * i + 1], b1, b2, m1);
    } else {
      c0 = branch_cost((int)rx[2 * i], (int)rx[2 * i + 1], a1, a2, m0);
      c1 = branch_cost((int)rx[2 * i], (int)rx[2 * i + 1], b1, b2, m1);
    }
    const bool odd = c1 < c0;
    metric = odd ? c1 : c0;
    const uint64_t d = __ballot(odd);
    rows[slot][lane] = metric;
    if (lane == 0) dec[slot] = d;

    // bits 64 B .. 64 B + 63 are decided once step 64 B + 63 + 41 is done, the
    // last (partial) block at the last step
    const int c_last = t - (kWin - 1);
    if (c_last >= 0 && ((c_last & 63) == 63 || t == T - 1)) {
      __syncthreads();
      const int c = (c_last & ~63) + lane;
      if (c <= c_last) {
        uint64_t alive = ~0ull;
        int s = (c + kWin - 1) % kRing;
        for (int k = 0; k < kWin - 1; k++) {        // steps c + 41 .. c + 1
          alive = step_back(alive, dec[s]);
          s = s == 0 ? kRing - 1 : s - 1;
        }
        const Metric* row = rows[c % kRing];         // the metrics after step c
        int best = -1;
        Metric best_w = (Metric)0;
        while (alive) {
          const int st = __ffsll((long long)alive) - 1;
          alive &= alive - 1;
          const Metric w = row[st];
          if (best < 0 || w < best_w) {
            best = st;
            best_w = w;
          }
        }
        out[c] = (uint8_t)(best >> 5 & 1);
      }
      __syncthreads();
    }
    slot = slot + 1 == kRing ? 0 : slot + 1;
  }
}

// ---------------------------------------------------------------------------
// front ends: +-1 pattern correlations over sign(x), sign(0) = 0, samples past
// the end of a series count as 0
// ---------------------------------------------------------------------------
struct Series {            // an fp64 field inside an array of epoch records
  const char* base;
  int64_t stride;
  int n;
  __device__ int sign(int64_t k) const {
    if (k >= n) return 0;
    const double x = *(const double*)(base + k * stride);
    return (x > 0) - (x < 0);
  }
};

struct BitSeries {         // decoded bits as 2 b - 1
  const uint8_t* bits;
  int n;
  __device__ int sign(int64_t k) const { return k < n ? 2 * (int)bits[k] - 1 : 0; }
};

// sum_{i < len * rep} w[i / rep] * sign(x[k + i]); w[j] = -1 where bit j of neg is set
template <class S>
__device__ __forceinline__ int pattern_corr(const S& x, int64_t k, int len, int rep,
                                            uint32_t neg) {
  int acc = 0;
  for (int j = 0; j < len; j++) {
    int part = 0;
    for (int r = 0; r < rep; r++) part += x.sign(k + j * rep + r);
    acc += (neg >> j & 1) ? -part : part;
  }
  return acc;
}

// the smallest v any thread of the block offers (INT_MAX: none)
__device__ __forceinline__ int block_min(int v) {
  __shared__ int best;
  if (threadIdx.x == 0) best = INT_MAX;
  __syncthreads();
  if (v != INT_MAX) atomicMin(&best, v);
  __syncthreads();
  return best;
}

__device__ __forceinline__ bool e1_sync_hit(const Series& x, int64_t k) {
  return abs(pattern_corr(x, k, 10, 4, kE1SyncNeg)) > 38;     // findPageStart.sci:51
}

// findPageStart.sci:42-63: the first k with a hit at k and at k + 1000.  One
// block per channel.
__global__ __launch_bounds__(kThreads) void nav_e1_sync_kernel(
    const char* __restrict__ series, int64_t epoch_stride, int64_t chan_stride, int n_epochs,
    int max_pages, int32_t* __restrict__ first_page, int32_t* __restrict__ n_pages) {
  const int ch = blockIdx.x;
  const Series x{series + ch * chan_stride, epoch_stride, n_epochs};
  int mine = INT_MAX;
  for (int64_t k = threadIdx.x; k < (int64_t)n_epochs - kE1Page; k += kThreads)
    if (e1_sync_hit(x, k) && e1_sync_hit(x, k + kE1Page)) {
      mine = (int)k;
      break;
    }
  const int first = block_min(mine);
  if (threadIdx.x == 0) {
    first_page[ch] = first == INT_MAX ? -1 : first;
    n_pages[ch] = first == INT_MAX ? 0 : min((n_epochs - first) / kE1Page, max_pages);
  }
}

// decode_gll_data.sci:16-39 up to the decoder's input.  Block (page, channel).
__global__ __launch_bounds__(kThreads) void nav_e1_symbols_kernel(
    const char* __restrict__ series, int64_t epoch_stride, int64_t chan_stride, int n_epochs,
    int max_pages, const int32_t* __restrict__ first_page, const int32_t* __restrict__ n_pages,
    uint8_t* __restrict__ code, int32_t* __restrict__ len) {
  __shared__ int y[kE1Page / 4];
  __shared__ int flip;
  const int pg = blockIdx.x, ch = blockIdx.y, tid = threadIdx.x;
  const int64_t strm = (int64_t)ch * max_pages + pg;
  if (pg >= n_pages[ch]) {
    if (tid == 0) len[strm] = 0;
    return;
  }
  const Series x{series + ch * chan_stride, epoch_stride, n_epochs};
  const int64_t p = (int64_t)first_page[ch] + (int64_t)kE1Page * pg;
  if (tid < kE1Page / 4) {
    int s = 0;
    for (int j = 0; j < 4; j++) s += x.sign(p + 4 * tid + j);
    y[tid] = (s > 0) - (s < 0);
  }
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int i = 0; i < 10; i++) s += (kE1SyncNeg >> i & 1) ? -y[i] : y[i];
    flip = s < 0;                                   // :25-27
    len[strm] = kE1Bits;
  }
  __syncthreads();
  if (tid < kE1Syms) {                              // out[c + 8 r] = z[r + 30 c], :30-32
    const int c = tid & 7, r = tid >> 3;
    const int v = y[10 + r + 30 * c];
    code[strm * kE1Syms + tid] = (uint8_t)((flip ? -v : v) > 0);   // floor((out + 1) / 2)
  }
}

// test_data_decode.sce:19-22, 35-36: the first k whose ten pilot signs are the
// overlay or its negative, and the number of whole 10-ms bits from there.  One
// block per channel.
__global__ __launch_bounds__(kThreads) void nav_l3_start_kernel(
    const char* __restrict__ pilot, int64_t epoch_stride, int64_t chan_stride, int n_epochs,
    int32_t* __restrict__ start, int32_t* __restrict__ n_bits) {
  const int ch = blockIdx.x;
  const Series x{pilot + ch * chan_stride, epoch_stride, n_epochs};
  int mine = INT_MAX;
  for (int64_t k = threadIdx.x; k < n_epochs; k += kThreads)
    if (abs(pattern_corr(x, k, 10, 1, kNhNeg)) == 10) {
      mine = (int)k;
      break;
    }
  const int first = block_min(mine);
  if (threadIdx.x == 0) {
    start[ch] = first == INT_MAX ? -1 : first;
    n_bits[ch] = first == INT_MAX ? 0 : (n_epochs - first) / 10;
  }
}

// :39-44, 71-79: Barker wipe-off and the sum of five epochs per symbol (the
// sign test of :29 never fires: no inversion).  Grid (symbol blocks, channel).
__global__ __launch_bounds__(kThreads) void nav_l3_symbols_kernel(
    const char* __restrict__ data, int64_t epoch_stride, int64_t chan_stride, int n_epochs,
    int max_bits, const int32_t* __restrict__ start, const int32_t* __restrict__ n_bits,
    uint8_t* __restrict__ code) {
  const int ch = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= 2 * n_bits[ch]) return;
  const Series x{data + ch * chan_stride, epoch_stride, n_epochs};
  const int s = pattern_corr(x, (int64_t)start[ch] + 5 * (int64_t)i, 5, 1, kBarkerNeg);
  code[(int64_t)ch * 2 * max_bits + i] = (uint8_t)(s > 0);
}

// :82-83: every k whose twenty bits are the time mark or its complement, in
// ascending order.  One wave per channel.
__global__ __launch_bounds__(64) void nav_l3_marks_kernel(
    const uint8_t* __restrict__ bits, int max_bits, const int32_t* __restrict__ n_bits,
    int max_marks, int32_t* __restrict__ n_marks, int32_t* __restrict__ marks) {
  const int ch = blockIdx.x, lane = threadIdx.x;
  const BitSeries x{bits + (int64_t)ch * max_bits, n_bits[ch]};
  int32_t* out = marks + (int64_t)ch * max_marks;
  int count = 0;
  for (int base = 0; base < x.n; base += 64) {
    const int k = base + lane;
    const bool hit = k < x.n && abs(pattern_corr(x, k, 20, 1, kTimeMarkNeg)) == 20;
    const uint64_t m = __ballot(hit);
    const int at = count + __popcll(m & ((1ull << lane) - 1));
    if (hit && at < max_marks) out[at] = k;
    count += __popcll(m);
  }
  for (int j = count + lane; j < max_marks; j += 64) out[j] = -1;
  if (lane == 0) n_marks[ch] = count;
}

}  // namespace

// ============================================================================
// host side
// ============================================================================
using navhost::bad_arguments;
using navhost::check_series;
using navhost::series_bytes;

extern "C" int gnsscorr_nav_conv_encode(const uint8_t* msg, int n_bits, uint8_t* out) {
  if (!msg || !out || n_bits < 1) return bad_arguments(__func__, "msg, out, n_bits >= 1");
  uint32_t reg = 0;                            // input in bit 6, then the six before it
  for (int t = 0; t < n_bits + 6; t++) {
    const uint32_t in = t < n_bits ? (msg[t] & 1u) : 0u;
    reg = reg >> 1 | in << 6;
    out[2 * t] = (uint8_t)(__builtin_popcount(reg & kGen1) & 1);
    out[2 * t + 1] = (uint8_t)(__builtin_popcount(reg & kGen2) & 1);
  }
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_create(gnsscorr_nav_ctx** out, int device) {
  if (!out) return bad_arguments(__func__, "null out");
  *out = nullptr;
  int rc = hostctx::open_device(__func__, device);
  if (rc) return rc;
  auto* c = new gnsscorr_nav_ctx();
  c->cfg.device = device;
  const hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    gnsscorr_set_error("%s: hipStreamCreateWithFlags failed: %s", __func__, hipGetErrorString(e));
    delete c;
    return GNSSCORR_EDEVICE;
  }
  *out = c;
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_destroy(gnsscorr_nav_ctx* c) {
  return hostctx::destroy(c, [&] { hostctx::release(c->d_code, c->d_len, c->d_hitmap, c->d_rx_first); });
}

extern "C" int gnsscorr_nav_sync(gnsscorr_nav_ctx* c) { return hostctx::sync(c); }

extern "C" void* gnsscorr_nav_stream(gnsscorr_nav_ctx* c) { return hostctx::stream(c); }

static void launch_viterbi(gnsscorr_nav_ctx* c, const void* d_code, int64_t stride,
                           int64_t n_streams, int l_max, const int32_t* d_len, int soft,
                           uint8_t* d_bits) {
  const dim3 grid((unsigned)n_streams), block(64);
  if (soft)
    hipLaunchKernelGGL(nav_viterbi_kernel<true>, grid, block, 0, c->stream, d_code, stride, l_max,
                       d_len, d_bits);
  else
    hipLaunchKernelGGL(nav_viterbi_kernel<false>, grid, block, 0, c->stream, d_code, stride,
                       l_max, d_len, d_bits);
}

static int check_viterbi(const char* fn, const gnsscorr_nav_ctx* c, const void* code,
                         int64_t stride, int n_streams, int L, int soft, const void* bits) {
  if (!c || !code || !bits) return bad_arguments(fn, "null pointer");
  if (n_streams < 1 || L < 1) return bad_arguments(fn, "n_streams >= 1, L >= 1");
  if (L > kMaxBits) {
    gnsscorr_set_error("%s: L %d: the int32 path metrics could overflow past %d bits", fn, L,
                       kMaxBits);
    return GNSSCORR_EINVAL;
  }
  const int64_t pair = soft ? 16 : 2;
  if (n_streams > 1 && stride < pair * L)
    return bad_arguments(fn, "stream_stride_bytes smaller than one stream");
  if (soft && (((uintptr_t)code & 7) || (stride & 7)))
    return bad_arguments(fn, "soft input: 8-byte aligned d_code and stride");
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_viterbi_dev(gnsscorr_nav_ctx* c, const void* d_code,
                                        int64_t stream_stride_bytes, int n_streams, int L,
                                        int soft, uint8_t* d_bits) {
  int rc = check_viterbi(__func__, c, d_code, stream_stride_bytes, n_streams, L, soft, d_bits);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  launch_viterbi(c, d_code, stream_stride_bytes, n_streams, L, nullptr, soft, d_bits);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_viterbi(gnsscorr_nav_ctx* c, const void* h_code,
                                    int64_t stream_stride_bytes, int n_streams, int L, int soft,
                                    uint8_t* h_bits) {
  int rc = check_viterbi(__func__, c, h_code, stream_stride_bytes, n_streams, L, soft, h_bits);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  const size_t n_in = (size_t)(n_streams - 1) * stream_stride_bytes + (size_t)(soft ? 16 : 2) * L;
  hostctx::Staging st(c->stream);
  const char* d_code = st.in((const char*)h_code, n_in);
  uint8_t* d_bits = st.out(h_bits, (size_t)n_streams * L);
  if (st.status()) return st.status();
  rc = gnsscorr_nav_viterbi_dev(c, d_code, stream_stride_bytes, n_streams, L, soft, d_bits);
  return rc ? rc : st.finish();
}

static int check_e1(const char* fn, const gnsscorr_nav_ctx* c, const void* series,
                    int64_t epoch_stride, int64_t chan_stride, int n_epochs, int n_ch,
                    int max_pages, const void* first_page, const void* n_pages,
                    const void* bits) {
  int rc = check_series(fn, c, series, epoch_stride, chan_stride, n_epochs, n_ch);
  if (rc) return rc;
  if (!first_page || !n_pages || !bits) return bad_arguments(fn, "null pointer");
  if (max_pages < 1 || (int64_t)n_ch * max_pages > INT_MAX)
    return bad_arguments(fn, "max_pages >= 1, n_ch * max_pages < 2^31");
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_e1_pages_dev(gnsscorr_nav_ctx* c, const void* d_series,
                                         int64_t epoch_stride_bytes, int64_t chan_stride_bytes,
                                         int n_epochs, int n_ch, int max_pages,
                                         int32_t* d_first_page, int32_t* d_n_pages,
                                         uint8_t* d_bits) {
  int rc = check_e1(__func__, c, d_series, epoch_stride_bytes, chan_stride_bytes, n_epochs, n_ch,
                    max_pages, d_first_page, d_n_pages, d_bits);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  const int64_t n_streams = (int64_t)n_ch * max_pages;
  rc = hostctx::grow(c->d_code, (size_t)n_streams * kE1Syms);
  if (!rc) rc = hostctx::grow(c->d_len, (size_t)n_streams);
  if (rc) return rc;
  const char* s = (const char*)d_series;
  hipLaunchKernelGGL(nav_e1_sync_kernel, dim3(n_ch), dim3(kThreads), 0, c->stream, s,
                     epoch_stride_bytes, chan_stride_bytes, n_epochs, max_pages, d_first_page,
                     d_n_pages);
  hipLaunchKernelGGL(nav_e1_symbols_kernel, dim3(max_pages, n_ch), dim3(kThreads), 0, c->stream,
                     s, epoch_stride_bytes, chan_stride_bytes, n_epochs, max_pages, d_first_page,
                     d_n_pages, c->d_code.p, c->d_len.p);
  launch_viterbi(c, c->d_code.p, kE1Syms, n_streams, kE1Bits, c->d_len.p, 0, d_bits);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_e1_pages(gnsscorr_nav_ctx* c, const void* h_series,
                                     int64_t epoch_stride_bytes, int64_t chan_stride_bytes,
                                     int n_epochs, int n_ch, int max_pages, int32_t* h_first_page,
                                     int32_t* h_n_pages, uint8_t* h_bits) {
  int rc = check_e1(__func__, c, h_series, epoch_stride_bytes, chan_stride_bytes, n_epochs, n_ch,
                    max_pages, h_first_page, h_n_pages, h_bits);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  hostctx::Staging st(c->stream);
  const char* d_series = st.in(
      (const char*)h_series, series_bytes(epoch_stride_bytes, chan_stride_bytes, n_epochs, n_ch));
  int32_t* d_first_page = st.out(h_first_page, (size_t)n_ch);
  int32_t* d_n_pages = st.out(h_n_pages, (size_t)n_ch);
  uint8_t* d_bits = st.out(h_bits, (size_t)n_ch * max_pages * kE1Bits);
  if (st.status()) return st.status();
  rc = gnsscorr_nav_e1_pages_dev(c, d_series, epoch_stride_bytes, chan_stride_bytes, n_epochs,
                                 n_ch, max_pages, d_first_page, d_n_pages, d_bits);
  return rc ? rc : st.finish();
}

static int check_l3(const char* fn, const gnsscorr_nav_ctx* c, const void* pilot,
                    const void* data, int64_t epoch_stride, int64_t chan_stride, int n_epochs,
                    int n_ch, int max_marks, const void* start, const void* n_bits,
                    const void* bits, const void* n_marks, const void* marks) {
  int rc = check_series(fn, c, pilot, epoch_stride, chan_stride, n_epochs, n_ch);
  if (!rc) rc = check_series(fn, c, data, epoch_stride, chan_stride, n_epochs, n_ch);
  if (rc) return rc;
  if (!start || !n_bits || !bits || !n_marks || !marks) return bad_arguments(fn, "null pointer");
  if (max_marks < 1) return bad_arguments(fn, "max_marks >= 1");
  if (n_epochs / 10 > kMaxBits) {
    gnsscorr_set_error("%s: %d epochs: the int32 path metrics could overflow past %d bits", fn,
                       n_epochs, kMaxBits);
    return GNSSCORR_EINVAL;
  }
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_l3_decode_dev(gnsscorr_nav_ctx* c, const void* d_pilot,
                                          const void* d_data, int64_t epoch_stride_bytes,
                                          int64_t chan_stride_bytes, int n_epochs, int n_ch,
                                          int max_marks, int32_t* d_start, int32_t* d_n_bits,
                                          uint8_t* d_bits, int32_t* d_n_marks,
                                          int32_t* d_marks) {
  int rc = check_l3(__func__, c, d_pilot, d_data, epoch_stride_bytes, chan_stride_bytes, n_epochs,
                    n_ch, max_marks, d_start, d_n_bits, d_bits, d_n_marks, d_marks);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  const int max_bits = n_epochs / 10;
  rc = hostctx::grow(c->d_code, (size_t)n_ch * 2 * (size_t)(max_bits > 0 ? max_bits : 1));
  if (rc) return rc;
  hipLaunchKernelGGL(nav_l3_start_kernel, dim3(n_ch), dim3(kThreads), 0, c->stream,
                     (const char*)d_pilot, epoch_stride_bytes, chan_stride_bytes, n_epochs,
                     d_start, d_n_bits);
  if (max_bits > 0) {
    hipLaunchKernelGGL(nav_l3_symbols_kernel,
                       dim3((2 * (unsigned)max_bits + kThreads - 1) / kThreads, n_ch),
                       dim3(kThreads), 0, c->stream, (const char*)d_data, epoch_stride_bytes,
                       chan_stride_bytes, n_epochs, max_bits, d_start, d_n_bits, c->d_code.p);
    launch_viterbi(c, c->d_code.p, 2 * (int64_t)max_bits, n_ch, max_bits, d_n_bits, 0, d_bits);
  }
  hipLaunchKernelGGL(nav_l3_marks_kernel, dim3(n_ch), dim3(64), 0, c->stream, d_bits, max_bits,
                     d_n_bits, max_marks, d_n_marks, d_marks);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_l3_decode(gnsscorr_nav_ctx* c, const void* h_pilot,
                                      const void* h_data, int64_t epoch_stride_bytes,
                                      int64_t chan_stride_bytes, int n_epochs, int n_ch,
                                      int max_marks, int32_t* h_start, int32_t* h_n_bits,
                                      uint8_t* h_bits, int32_t* h_n_marks, int32_t* h_marks) {
  int rc = check_l3(__func__, c, h_pilot, h_data, epoch_stride_bytes, chan_stride_bytes, n_epochs,
                    n_ch, max_marks, h_start, h_n_bits, h_bits, h_n_marks, h_marks);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  const size_t n_in = series_bytes(epoch_stride_bytes, chan_stride_bytes, n_epochs, n_ch);
  const size_t n = (size_t)n_ch;
  hostctx::Staging st(c->stream);
  const char* d_pilot = st.in((const char*)h_pilot, n_in);
  const char* d_data = st.in((const char*)h_data, n_in);
  int32_t* d_start = st.out(h_start, n);
  int32_t* d_n_bits = st.out(h_n_bits, n);
  int32_t* d_n_marks = st.out(h_n_marks, n);
  int32_t* d_marks = st.out(h_marks, n * max_marks);
  uint8_t* d_bits = st.out(h_bits, n * (size_t)(n_epochs / 10));   // none below ten epochs
  if (st.status()) return st.status();
  rc = gnsscorr_nav_l3_decode_dev(c, d_pilot, d_data, epoch_stride_bytes, chan_stride_bytes,
                                  n_epochs, n_ch, max_marks, d_start, d_n_bits, d_bits, d_n_marks,
                                  d_marks);
  return rc ? rc : st.finish();
}
