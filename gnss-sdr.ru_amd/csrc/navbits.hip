// navbits.hip -- frame synchronisation and data bits of GPS L1 C/A, GLONASS L1OF
// and BeiDou B1I on the device ("nav"), read from the float tracker's epoch
// records (gnsscorr_sgt_epoch.i_p) in place.
//   GPS/L1/findPreambles.sci:49-153, GPS/L1/include/navPartyChk.sci:56-103,
//   GPS/L1/postNavigation.sci:91-106, GPS/L1/include/checkPhase.sci:45-52,
//   GPS/L1/include/ephemeris.sci:68-80
//   GLONASS/L1/findTimeMarks.sci:42-65, GLONASS/L1/postNavigation.sci:96-99,
//   GLONASS/L1/include/ephemeris.sci:30-36, GLONASS/L1/include/decode_gl_data.sci:17-34
//   COMPASS/B1/findSubframeStart.sci:39-62, COMPASS/B1/postNavigation.sci:88-92,
//   COMPASS/B1/include/ephemeris.sci:28-34, COMPASS/B1/include/decode_bd_data.sci:16-38
// Sign and integer work, and fp64 adds in the files' order: bits and positions
// are exact ("nav bits").
//
// nav_pattern_hits_kernel: the files' convol of a 160-, 300- or 220-tap +-1
// pattern with the signs of a 36-45 s series.  One workgroup per channel.  The
// strided fp64 field is loaded once and kept as two bit planes in LDS, P (x > 0)
// and N (x < 0), one wave ballot per 64 epochs; a tile is kTileW words, the
// kMaskW words a window reaches past it are carried over to the next tile.  A
// lane owns epoch k: its window is words k / 64 .. of each plane, funnel-shifted
// by k mod 64, and with the pattern as two masks Q+ and Q- in scalar registers
//   r[k] = popc(P & Q+ | N & Q-) - popc(P & Q- | N & Q+)
// over ceil(T / 64) words (P and N are disjoint, and so are Q+ and Q-: each of
// the two counts is the sum of two of the four popc(plane & mask) terms).  The
// 64 decisions of a wave are one ballot word; wave 0 turns a tile's words into
// the first hit, the count and the ascending list.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <string.h>
#include "gnsscorr_internal.h"
#include "hostctx.h"
#include "nav_host.h"

namespace {

constexpr int kHitThreads = 256, kHitWaves = kHitThreads / 64;
constexpr int kMaxTaps = 512, kMaskW = kMaxTaps / 64;
constexpr int kTileW = 128;                 // 64-epoch words of a tile: 8192 epochs
constexpr int kPlaneW = kTileW + kMaskW;    // the last group's window ends in word kTileW - 1 + kMaskW

constexpr int kGpsTaps = 160, kGpsThreshold = 153, kGpsSubframe = 6000;
constexpr int kGpsMaxSub = 5, kGpsBits = 300 * kGpsMaxSub;
constexpr int kGloTaps = 300, kGloThreshold = 290, kGloString = 2000, kGloSamples = 1700;
constexpr int kGloMaxStrings = 15, kGloBits = 85;
constexpr int kB1Taps = 220, kB1Threshold = 200, kB1Subframe = 6000;
constexpr int kB1MaxSub = 5, kB1Bits = 213;

// findPreambles.sci:56; findTimeMarks.sci:45; findSubframeStart.sci:42-43;
// decode_bd_data.sci:18-19 -- as the files write them
constexpr int8_t kGpsPreamble[8] = {1, 1, -1, 1, -1, -1, -1, 1};
constexpr int8_t kGloTimeMark[30] = {-1, 1, 1, -1, 1, -1, -1, 1, -1, -1, -1, -1, 1, -1, 1,
                                     -1, 1, 1, 1, -1, 1, 1, -1, -1, -1, 1, 1, 1, 1, 1};
constexpr int8_t kB1SearchPreamble[11] = {-1, 1, -1, -1, 1, -1, -1, -1, 1, 1, 1};
constexpr int8_t kB1SearchSecondary[20] = {-1, 1, 1, 1, -1, -1, 1, -1, 1, -1,
                                           1, 1, -1, -1, 1, -1, -1, -1, -1, -1};
constexpr int8_t kB1Preamble[11] = {1, 1, 1, -1, -1, -1, 1, -1, -1, 1, -1};
constexpr int8_t kB1Secondary[20] = {-1, -1, -1, -1, -1, 1, -1, -1, 1, 1,
                                     -1, 1, -1, 1, -1, -1, 1, 1, 1, -1};
template <int N>
constexpr uint32_t neg_mask(const int8_t (&v)[N]) {     // entries that are -1, entry i in bit i
  uint32_t m = 0;
  for (int i = 0; i < N; i++) m |= v[i] < 0 ? 1u << i : 0u;
  return m;
}
constexpr uint32_t kB1PreambleNeg = neg_mask(kB1Preamble);
constexpr uint32_t kB1SecondaryNeg = neg_mask(kB1Secondary);
static_assert(kB1PreambleNeg == 0x5B8 && kB1SecondaryNeg == 0x8D4DF, "decode_bd_data.sci:18-19");

// navPartyChk.sci:68-91, the files' 1-based indices; 0 ends a list
__constant__ int8_t kParityTerms[6][16] = {
    {1, 3, 4, 5, 7, 8, 12, 13, 14, 15, 16, 19, 20, 22, 25, 0},
    {2, 4, 5, 6, 8, 9, 13, 14, 15, 16, 17, 20, 21, 23, 26, 0},
    {1, 3, 5, 6, 7, 9, 10, 14, 15, 16, 17, 18, 21, 22, 24, 0},
    {2, 4, 6, 7, 8, 10, 11, 15, 16, 17, 18, 19, 22, 23, 25, 0},
    {2, 3, 5, 7, 8, 9, 11, 12, 16, 17, 18, 19, 20, 23, 24, 26},
    {1, 5, 7, 8, 10, 11, 12, 13, 15, 17, 21, 24, 25, 26, 0, 0}};

struct Series {            // an fp64 field inside an array of epoch records
  const char* base;
  int64_t stride;
  int n;
  __device__ double value(int64_t k) const {          // 0 outside the series
    return k >= 0 && k < n ? *(const double*)(base + k * stride) : 0.0;
  }
  __device__ int sign(int64_t k) const {
    const double x = value(k);
    return (x > 0) - (x < 0);
  }
  // sign of x[k] + x[k + 1] + ... + x[k + 19], fp64 adds one after another in
  // that order (sum(..., 'r') of a 20-row matrix)
  __device__ int sign_of_sum20(int64_t k) const {
    double acc = value(k);
    for (int t = 1; t < 20; t++) acc = acc + value(k + t);
    return (acc > 0) - (acc < 0);
  }
};

__device__ __forceinline__ uint8_t bit_of(int v) {     // (v + 1) / 2, 2 for 0.5
  return v > 0 ? 1 : v < 0 ? 0 : 2;
}

struct PatternMasks {      // tap i in bit i mod 64 of word i / 64
  uint64_t pos[kMaskW], neg[kMaskW];
};

// first, n_hits: null, or [n_ch]; hits: null, or [n_ch][max_hits].  hitmap: null, or
// [n_ch][map_words] words of 64 decisions, map_words = ceil(n_epochs / 64).
__global__ __launch_bounds__(kHitThreads) void nav_pattern_hits_kernel(
    const char* __restrict__ series, int64_t epoch_stride, int64_t chan_stride, int n_epochs,
    PatternMasks q, int n_mask_words, int threshold, int first_k, int max_hits,
    int32_t* __restrict__ first, int32_t* __restrict__ n_hits, int32_t* __restrict__ hits,
    uint64_t* __restrict__ hitmap, int map_words) {
  __shared__ uint64_t plane_p[kPlaneW], plane_n[kPlaneW], hit_words[kTileW];
  const int ch = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Series x{series + ch * chan_stride, epoch_stride, n_epochs};
  const int n_words = (n_epochs + 63) / 64;
  const int n_tiles = (n_words + kTileW - 1) / kTileW;
  int32_t* out = hits ? hits + (int64_t)ch * max_hits : nullptr;
  if (!out) max_hits = 0;
  int first_hit = -1, count = 0;                       // wave 0's

  for (int tile = 0; tile < n_tiles; tile++) {
    const int word0 = tile * kTileW;                   // the series word in plane word 0
    int lo = 0;
    if (tile > 0) {                                    // the words the last tile loaded past its end
      uint64_t cp = 0, cn = 0;
      if (tid < kMaskW) {
        cp = plane_p[kTileW + tid];
        cn = plane_n[kTileW + tid];
      }
      __syncthreads();
      if (tid < kMaskW) {
        plane_p[tid] = cp;
        plane_n[tid] = cn;
      }
      lo = kMaskW;
    }
    // four words per wave and pass: four loads of every lane in flight
    for (int w = lo + 4 * wave; w < kPlaneW; w += 4 * kHitWaves) {
      double v[4];
#pragma unroll
      for (int u = 0; u < 4; u++) v[u] = x.value(((int64_t)word0 + w + u) * 64 + lane);
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const uint64_t bp = __ballot(v[u] > 0), bn = __ballot(v[u] < 0);
        if (lane == 0 && w + u < kPlaneW) {
          plane_p[w + u] = bp;
          plane_n[w + u] = bn;
        }
      }
    }
    __syncthreads();

    for (int g = wave; g < kTileW; g += kHitWaves) {
      const int gw = word0 + g;
      uint64_t m = 0;
      if (gw < n_words && (int64_t)gw * 64 + 63 >= first_k) {
        const int64_t k = (int64_t)gw * 64 + lane;
        int r = 0;
        uint64_t lo_p = plane_p[g], lo_n = plane_n[g];
#pragma unroll
        for (int j = 0; j < kMaskW; j++) {
          if (j >= n_mask_words) break;
          const uint64_t hi_p = plane_p[g + j + 1], hi_n = plane_n[g + j + 1];
          // epochs k + 64 j .. k + 64 j + 63; the second shift is by 64 - lane in two steps
          const uint64_t wp = lo_p >> lane | hi_p << 1 << (63 - lane);
          const uint64_t wn = lo_n >> lane | hi_n << 1 << (63 - lane);
          r += __popcll((wp & q.pos[j]) | (wn & q.neg[j]));
          r -= __popcll((wp & q.neg[j]) | (wn & q.pos[j]));
          lo_p = hi_p;
          lo_n = hi_n;
        }
        m = __ballot(k >= first_k && k < n_epochs && abs(r) > threshold);
      }
      if (lane == 0) {
        hit_words[g] = m;
        if (hitmap && gw < n_words) hitmap[(int64_t)ch * map_words + gw] = m;
      }
    }
    __syncthreads();

    if (wave == 0 && first) {
      for (int h = 0; h < kTileW; h += 64) {
        uint64_t w = hit_words[h + lane];
        const uint64_t any = __ballot(w != 0);
        if (!any) continue;
        const int c = __popcll(w);
        int incl = c;                                  // hits in this and the lower lanes' words
        for (int d = 1; d < 64; d <<= 1) {
          const int t = __shfl_up(incl, d);
          if (lane >= d) incl += t;
        }
        if (first_hit < 0) {
          const int fl = __ffsll((long long)any) - 1;
          const uint64_t fw = __shfl(w, fl);
          first_hit = (word0 + h + fl) * 64 + __ffsll((long long)fw) - 1;
        }
        int64_t at = (int64_t)count + incl - c;
        while (w && at < max_hits) {
          out[at++] = (word0 + h + lane) * 64 + __ffsll((long long)w) - 1;
          w &= w - 1;
        }
        count += __shfl(incl, 63);
      }
    }
  }
  if (wave == 0 && first) {
    for (int64_t j = (int64_t)count + lane; j < max_hits; j += 64) out[j] = -1;
    if (lane == 0) {
      first[ch] = first_hit;
      n_hits[ch] = count;
    }
  }
}

// ---------------------------------------------------------------------------
// GPS L1 C/A.  One wave per channel.
// ---------------------------------------------------------------------------
// navPartyChk.sci:56-103 on b[0..31] in {-1, 0, 1} (ndat(i) = b[i - 1])
__device__ int nav_party_chk(const int* b) {
  const bool inv = b[1] != 1;                          // :56-58
  int same = 0;
  for (int p = 0; p < 6; p++) {
    int prod = 1;
    for (int t = 0; t < 16; t++) {
      const int i = kParityTerms[p][t];
      if (i == 0) break;
      const int v = b[i - 1];
      prod *= (inv && i >= 3 && i <= 26) ? -v : v;
    }
    same += prod == b[26 + p];                         // :94, ndat(27:32) is not inverted
  }
  return same == 6 ? -b[1] : 0;                        // :99
}

__global__ __launch_bounds__(64) void nav_gps_frames_kernel(
    const char* __restrict__ series, int64_t epoch_stride, int64_t chan_stride, int n_epochs,
    const uint64_t* __restrict__ hitmap, int map_words, int max_subframes,
    int32_t* __restrict__ first_subframe, int32_t* __restrict__ n_bits,
    uint8_t* __restrict__ bits) {
  __shared__ int b[62];
  __shared__ uint8_t raw[kGpsBits + 1];
  const int ch = blockIdx.x, lane = threadIdx.x;
  const Series x{series + ch * chan_stride, epoch_stride, n_epochs};
  const uint64_t* hit = hitmap + (int64_t)ch * map_words;
  uint8_t* out = bits + (int64_t)ch * kGpsBits;
  constexpr int kW = kGpsSubframe / 64, kS = kGpsSubframe % 64;   // 93 words and 48 bits

  // findPreambles.sci:109-153: the hits whose partner 6000 later is a hit, in
  // ascending order, until one passes both parity checks
  int found = -1;
  for (int base = 0; base < map_words && found < 0; base += 64) {
    const int w = base + lane;
    uint64_t cand = 0;
    if (w < map_words) {
      const uint64_t a = w + kW < map_words ? hit[w + kW] : 0;
      const uint64_t c = w + kW + 1 < map_words ? hit[w + kW + 1] : 0;
      cand = hit[w] & (a >> kS | c << (64 - kS));
    }
    uint64_t lanes = __ballot(cand != 0);
    while (lanes && found < 0) {
      const int l = __ffsll((long long)lanes) - 1;
      lanes &= lanes - 1;
      uint64_t cw = __shfl(cand, l);
      while (cw && found < 0) {
        const int p = (base + l) * 64 + __ffsll((long long)cw) - 1;
        cw &= cw - 1;
        __syncthreads();
        if (lane < 62) b[lane] = x.sign_of_sum20((int64_t)p - 40 + 20 * lane);   // :129-139
        __syncthreads();
        int ok = 0;
        if (lane < 2) ok = nav_party_chk(b + 30 * lane) != 0;                    // :142-143
        if ((__ballot(ok) & 3) == 3) found = p;
      }
    }
  }

  // postNavigation.sci:91-106 for the whole subframes that are there
  int n_sub = 0;
  if (found >= 0) n_sub = min(min(max_subframes, kGpsMaxSub), (n_epochs - found) / kGpsSubframe);
  const int nb = 300 * n_sub;
  __syncthreads();
  if (n_sub > 0)
    for (int j = lane; j <= nb; j += 64)
      raw[j] = bit_of(x.sign_of_sum20((int64_t)found - 20 + 20 * j));
  __syncthreads();
  // ephemeris.sci:74-80 with checkPhase.sci:45-52: bit i of the stream is
  // raw[1 + i]; checkPhase leaves bits 25-30 of a word alone, so the D30* of word
  // w is raw[30 w] as it stands
  for (int i = lane; i < kGpsBits; i += 64) {
    uint8_t v = 0;
    if (i < nb) {
      v = raw[1 + i];
      if (i % 30 < 24 && raw[i - i % 30] == 1 && v != 2) v = 1 - v;
    }
    out[i] = v;
  }
  if (lane == 0) {
    first_subframe[ch] = found;
    n_bits[ch] = nb;
  }
}

// ---------------------------------------------------------------------------
// GLONASS L1OF.  Block (channel, string).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(128) void nav_glo_strings_kernel(
    const char* __restrict__ series, int64_t epoch_stride, int64_t chan_stride, int n_epochs,
    int max_strings, const int32_t* __restrict__ first_mark, int32_t* __restrict__ n_strings,
    uint8_t* __restrict__ bits) {
  __shared__ int y[kGloBits];
  const int ch = blockIdx.x, i = blockIdx.y, tid = threadIdx.x;
  const Series x{series + ch * chan_stride, epoch_stride, n_epochs};
  uint8_t* out = bits + ((int64_t)ch * kGloMaxStrings + i) * kGloBits;
  const int first = first_mark[ch];
  // string j is there when its 1700 samples are: postNavigation.sci:96-97,
  // ephemeris.sci:31
  const int limit = min(max_strings, kGloMaxStrings);
  int present = 0;
  if (first >= 0) {
    const int64_t room = (int64_t)n_epochs - first - 300 - kGloSamples;
    present = room < 0 ? 0 : (int)min((int64_t)limit, room / kGloString + 1);
  }
  if (i == 0 && tid == 0) n_strings[ch] = present;
  if (i >= present) {
    if (tid < kGloBits) out[tid] = 0;
    return;
  }
  const int64_t s = (int64_t)first + 300 + (int64_t)kGloString * i;
  if (tid < kGloBits) {                                 // decode_gl_data.sci:19-29
    int acc = 0;
    for (int t = 0; t < 20; t++) acc += t < 10 ? -x.sign(s + 20 * tid + t) : x.sign(s + 20 * tid + t);
    y[tid] = (acc > 0) - (acc < 0);
  }
  __syncthreads();
  if (tid < kGloBits - 1) out[kGloBits - 2 - tid] = bit_of(-y[tid] * y[tid + 1]);   // :31-33
  if (tid == kGloBits - 1) out[tid] = 0;                                           // :34
}

// ---------------------------------------------------------------------------
// BeiDou B1I.  Block (channel, subframe).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(320) void nav_b1_subframes_kernel(
    const char* __restrict__ series, int64_t epoch_stride, int64_t chan_stride, int n_epochs,
    int max_subframes, const int32_t* __restrict__ first_sub, int32_t* __restrict__ n_subframes,
    uint8_t* __restrict__ bits) {
  __shared__ int y[300];
  __shared__ int negate;
  const int ch = blockIdx.x, i = blockIdx.y, tid = threadIdx.x;
  const Series x{series + ch * chan_stride, epoch_stride, n_epochs};
  uint8_t* out = bits + ((int64_t)ch * kB1MaxSub + i) * kB1Bits;
  const int first = first_sub[ch];
  const int limit = min(max_subframes, kB1MaxSub);
  const int present = first < 0 ? 0 : min(limit, (n_epochs - first) / kB1Subframe);
  if (i == 0 && tid == 0) n_subframes[ch] = present;
  if (i >= present) {
    if (tid < kB1Bits) out[tid] = 0;
    return;
  }
  const int64_t s = (int64_t)first + (int64_t)kB1Subframe * i;
  if (tid < 300) {                                      // decode_bd_data.sci:20-27
    int acc = 0;
    for (int t = 0; t < 20; t++) {
      const int v = x.sign(s + 20 * tid + t);
      acc += (kB1SecondaryNeg >> t & 1) ? -v : v;
    }
    y[tid] = (acc > 0) - (acc < 0);
  }
  __syncthreads();
  if (tid == 0) {                                       // :29-31
    int acc = 0;
    for (int j = 0; j < 11; j++) acc += (kB1PreambleNeg >> j & 1) ? -y[j] : y[j];
    negate = acc < 0;
  }
  __syncthreads();
  if (tid < kB1Bits) {                                  // :33-38
    int src;
    if (tid < 15) {
      src = 11 + tid;
    } else {
      const int w = 1 + (tid - 15) / 22, r = (tid - 15) % 22;
      src = 30 * w + (r < 11 ? 2 * r : 2 * (r - 11) + 1);
    }
    out[tid] = bit_of(negate ? -y[src] : y[src]);
  }
}

}  // namespace

// ============================================================================
// host side
// ============================================================================
using navhost::bad_arguments;
using navhost::check_series;
using navhost::series_bytes;

// pattern[i] in {-1, 0, 1} as the two masks; false for any other value
static bool make_masks(const int8_t* pattern, int T, PatternMasks* q) {
  memset(q, 0, sizeof *q);
  for (int i = 0; i < T; i++) {
    if (pattern[i] == 1) q->pos[i / 64] |= 1ull << (i % 64);
    else if (pattern[i] == -1) q->neg[i / 64] |= 1ull << (i % 64);
    else if (pattern[i] != 0) return false;
  }
  return true;
}

static void launch_hits(gnsscorr_nav_ctx* c, const void* d_series, int64_t epoch_stride,
                        int64_t chan_stride, int n_epochs, int n_ch, const PatternMasks& q, int T,
                        int threshold, int first_k, int max_hits, int32_t* d_first,
                        int32_t* d_n_hits, int32_t* d_hits, uint64_t* d_hitmap) {
  hipLaunchKernelGGL(nav_pattern_hits_kernel, dim3(n_ch), dim3(kHitThreads), 0, c->stream,
                     (const char*)d_series, epoch_stride, chan_stride, n_epochs, q, (T + 63) / 64,
                     threshold, first_k, max_hits, d_first, d_n_hits, d_hits, d_hitmap,
                     (n_epochs + 63) / 64);
}

// The reversed search patterns: convol(p, x)(T : $) at k is sum_i p[T - 1 - i] x[k + i].
static void gps_pattern(int8_t* p) {                    // findPreambles.sci:56-60
  for (int i = 0; i < kGpsTaps; i++) p[i] = kGpsPreamble[(kGpsTaps - 1 - i) / 20];
}
static void glo_pattern(int8_t* p) {                    // findTimeMarks.sci:45-46
  for (int i = 0; i < kGloTaps; i++) p[i] = (int8_t)-kGloTimeMark[(kGloTaps - 1 - i) / 10];
}
static void b1_pattern(int8_t* p) {                     // findSubframeStart.sci:42-44
  for (int i = 0; i < kB1Taps; i++) {
    const int r = kB1Taps - 1 - i;
    p[i] = (int8_t)(kB1SearchPreamble[r / 20] * -kB1SearchSecondary[r % 20]);
  }
}

static int check_hits(const char* fn, const gnsscorr_nav_ctx* c, const void* series,
                      int64_t epoch_stride, int64_t chan_stride, int n_epochs, int n_ch,
                      const int8_t* pattern, int T, int threshold, int first_k, int max_hits,
                      const void* first, const void* n_hits, const void* hits, PatternMasks* q) {
  int rc = check_series(fn, c, series, epoch_stride, chan_stride, n_epochs, n_ch);
  if (rc) return rc;
  if (!pattern || !first || !n_hits || !hits) return bad_arguments(fn, "null pointer");
  if (T < 1 || T > kMaxTaps) return bad_arguments(fn, "1 <= T <= 512");
  if (threshold < 0 || threshold >= T) return bad_arguments(fn, "0 <= threshold < T");
  if (first_k < 0) return bad_arguments(fn, "first_k >= 0");
  if (max_hits < 1) return bad_arguments(fn, "max_hits >= 1");
  if (!make_masks(pattern, T, q)) return bad_arguments(fn, "pattern values in {-1, 0, 1}");
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_pattern_hits_dev(gnsscorr_nav_ctx* c, const void* d_series,
                                             int64_t epoch_stride_bytes,
                                             int64_t chan_stride_bytes, int n_epochs, int n_ch,
                                             const int8_t* pattern, int T, int threshold,
                                             int first_k, int max_hits, int32_t* d_first,
                                             int32_t* d_n_hits, int32_t* d_hits) {
  PatternMasks q;
  int rc = check_hits(__func__, c, d_series, epoch_stride_bytes, chan_stride_bytes, n_epochs, n_ch,
                      pattern, T, threshold, first_k, max_hits, d_first, d_n_hits, d_hits, &q);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  launch_hits(c, d_series, epoch_stride_bytes, chan_stride_bytes, n_epochs, n_ch, q, T, threshold,
              first_k, max_hits, d_first, d_n_hits, d_hits, nullptr);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_pattern_hits(gnsscorr_nav_ctx* c, const void* h_series,
                                         int64_t epoch_stride_bytes, int64_t chan_stride_bytes,
                                         int n_epochs, int n_ch, const int8_t* pattern, int T,
                                         int threshold, int first_k, int max_hits,
                                         int32_t* h_first, int32_t* h_n_hits, int32_t* h_hits) {
  PatternMasks q;
  int rc = check_hits(__func__, c, h_series, epoch_stride_bytes, chan_stride_bytes, n_epochs, n_ch,
                      pattern, T, threshold, first_k, max_hits, h_first, h_n_hits, h_hits, &q);
  if (rc) return rc;
  if ((int64_t)n_ch * max_hits > INT_MAX) return bad_arguments(__func__, "n_ch * max_hits < 2^31");
  HIP_TRY(hipSetDevice(c->cfg.device));
  hostctx::Staging st(c->stream);
  const char* d_series = st.in(
      (const char*)h_series, series_bytes(epoch_stride_bytes, chan_stride_bytes, n_epochs, n_ch));
  int32_t* d_first = st.out(h_first, (size_t)n_ch);
  int32_t* d_n_hits = st.out(h_n_hits, (size_t)n_ch);
  int32_t* d_hits = st.out(h_hits, (size_t)n_ch * max_hits);
  if (st.status()) return st.status();
  rc = gnsscorr_nav_pattern_hits_dev(c, d_series, epoch_stride_bytes, chan_stride_bytes, n_epochs,
                                     n_ch, pattern, T, threshold, first_k, max_hits, d_first,
                                     d_n_hits, d_hits);
  return rc ? rc : st.finish();
}

// what the three chains check after the series
static int check_chain(const char* fn, int limit, const char* limit_text, const void* first,
                       const void* count, const void* bits) {
  if (!first || !count || !bits) return bad_arguments(fn, "null pointer");
  if (limit < 1) return bad_arguments(fn, limit_text);
  return GNSSCORR_OK;
}

// ---- GPS L1 C/A ------------------------------------------------------------
static int check_gps(const char* fn, const gnsscorr_nav_ctx* c, const void* series,
                     int64_t epoch_stride, int64_t chan_stride, int n_epochs, int n_ch,
                     int search_start, int max_subframes, const void* first, const void* n_bits,
                     const void* bits) {
  int rc = check_series(fn, c, series, epoch_stride, chan_stride, n_epochs, n_ch);
  if (!rc) rc = check_chain(fn, max_subframes, "max_subframes >= 1", first, n_bits, bits);
  if (rc) return rc;
  // the parity check reads 40 epochs before a hit
  if (search_start < 40) return bad_arguments(fn, "search_start >= 40");
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_gps_frames_dev(gnsscorr_nav_ctx* c, const void* d_series,
                                           int64_t epoch_stride_bytes, int64_t chan_stride_bytes,
                                           int n_epochs, int n_ch, int search_start,
                                           int max_subframes, int32_t* d_first_subframe,
                                           int32_t* d_n_bits, uint8_t* d_bits) {
  int rc = check_gps(__func__, c, d_series, epoch_stride_bytes, chan_stride_bytes, n_epochs, n_ch,
                     search_start, max_subframes, d_first_subframe, d_n_bits, d_bits);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  const int map_words = (n_epochs + 63) / 64;
  rc = hostctx::grow(c->d_hitmap, (size_t)n_ch * map_words);
  if (rc) return rc;
  int8_t pattern[kGpsTaps];
  PatternMasks q;
  gps_pattern(pattern);
  make_masks(pattern, kGpsTaps, &q);
  launch_hits(c, d_series, epoch_stride_bytes, chan_stride_bytes, n_epochs, n_ch, q, kGpsTaps,
              kGpsThreshold, search_start, 0, nullptr, nullptr, nullptr, c->d_hitmap.p);
  hipLaunchKernelGGL(nav_gps_frames_kernel, dim3(n_ch), dim3(64), 0, c->stream,
                     (const char*)d_series, epoch_stride_bytes, chan_stride_bytes, n_epochs,
                     c->d_hitmap.p, map_words, max_subframes, d_first_subframe, d_n_bits, d_bits);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_gps_frames(gnsscorr_nav_ctx* c, const void* h_series,
                                       int64_t epoch_stride_bytes, int64_t chan_stride_bytes,
                                       int n_epochs, int n_ch, int search_start,
                                       int max_subframes, int32_t* h_first_subframe,
                                       int32_t* h_n_bits, uint8_t* h_bits) {
  int rc = check_gps(__func__, c, h_series, epoch_stride_bytes, chan_stride_bytes, n_epochs, n_ch,
                     search_start, max_subframes, h_first_subframe, h_n_bits, h_bits);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  hostctx::Staging st(c->stream);
  const char* d_series = st.in(
      (const char*)h_series, series_bytes(epoch_stride_bytes, chan_stride_bytes, n_epochs, n_ch));
  int32_t* d_first_subframe = st.out(h_first_subframe, (size_t)n_ch);
  int32_t* d_n_bits = st.out(h_n_bits, (size_t)n_ch);
  uint8_t* d_bits = st.out(h_bits, (size_t)n_ch * kGpsBits);
  if (st.status()) return st.status();
  rc = gnsscorr_nav_gps_frames_dev(c, d_series, epoch_stride_bytes, chan_stride_bytes, n_epochs,
                                   n_ch, search_start, max_subframes, d_first_subframe, d_n_bits,
                                   d_bits);
  return rc ? rc : st.finish();
}

// ---- GLONASS L1OF and BeiDou B1I: the first hit, then one block per string
//      or subframe; d_count is the hit kernel's count until the second kernel
//      overwrites it with the number of strings or subframes
template <class Kernel>
static int first_hit_chain(const char* fn, gnsscorr_nav_ctx* c, const void* d_series,
                           int64_t epoch_stride, int64_t chan_stride, int n_epochs, int n_ch,
                           void (*make_pattern)(int8_t*), int T, int threshold, Kernel kernel,
                           int threads, int blocks, int limit, const char* limit_text,
                           int32_t* d_first, int32_t* d_count, uint8_t* d_bits) {
  int rc = check_series(fn, c, d_series, epoch_stride, chan_stride, n_epochs, n_ch);
  if (!rc) rc = check_chain(fn, limit, limit_text, d_first, d_count, d_bits);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  int8_t pattern[kMaxTaps];
  PatternMasks q;
  make_pattern(pattern);
  make_masks(pattern, T, &q);
  launch_hits(c, d_series, epoch_stride, chan_stride, n_epochs, n_ch, q, T, threshold, 0, 0,
              d_first, d_count, nullptr, nullptr);
  hipLaunchKernelGGL(kernel, dim3(n_ch, blocks), dim3(threads), 0, c->stream,
                     (const char*)d_series, epoch_stride, chan_stride, n_epochs, limit, d_first,
                     d_count, d_bits);
  HIP_TRY(hipGetLastError());
  return GNSSCORR_OK;
}

extern "C" int gnsscorr_nav_glo_strings_dev(gnsscorr_nav_ctx* c, const void* d_series,
                                            int64_t epoch_stride_bytes,
                                            int64_t chan_stride_bytes, int n_epochs, int n_ch,
                                            int max_strings, int32_t* d_first_mark,
                                            int32_t* d_n_strings, uint8_t* d_bits) {
  return first_hit_chain(__func__, c, d_series, epoch_stride_bytes, chan_stride_bytes, n_epochs,
                         n_ch, glo_pattern, kGloTaps, kGloThreshold, nav_glo_strings_kernel, 128,
                         kGloMaxStrings, max_strings, "max_strings >= 1", d_first_mark,
                         d_n_strings, d_bits);
}

extern "C" int gnsscorr_nav_glo_strings(gnsscorr_nav_ctx* c, const void* h_series,
                                        int64_t epoch_stride_bytes, int64_t chan_stride_bytes,
                                        int n_epochs, int n_ch, int max_strings,
                                        int32_t* h_first_mark, int32_t* h_n_strings,
                                        uint8_t* h_bits) {
  int rc = check_series(__func__, c, h_series, epoch_stride_bytes, chan_stride_bytes, n_epochs,
                        n_ch);
  if (!rc)
    rc = check_chain(__func__, max_strings, "max_strings >= 1", h_first_mark, h_n_strings, h_bits);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  hostctx::Staging st(c->stream);
  const char* d_series = st.in(
      (const char*)h_series, series_bytes(epoch_stride_bytes, chan_stride_bytes, n_epochs, n_ch));
  int32_t* d_first_mark = st.out(h_first_mark, (size_t)n_ch);
  int32_t* d_n_strings = st.out(h_n_strings, (size_t)n_ch);
  uint8_t* d_bits = st.out(h_bits, (size_t)n_ch * kGloMaxStrings * kGloBits);
  if (st.status()) return st.status();
  rc = gnsscorr_nav_glo_strings_dev(c, d_series, epoch_stride_bytes, chan_stride_bytes, n_epochs,
                                    n_ch, max_strings, d_first_mark, d_n_strings, d_bits);
  return rc ? rc : st.finish();
}

extern "C" int gnsscorr_nav_b1_subframes_dev(gnsscorr_nav_ctx* c, const void* d_series,
                                             int64_t epoch_stride_bytes,
                                             int64_t chan_stride_bytes, int n_epochs, int n_ch,
                                             int max_subframes, int32_t* d_first,
                                             int32_t* d_n_subframes, uint8_t* d_bits) {
  return first_hit_chain(__func__, c, d_series, epoch_stride_bytes, chan_stride_bytes, n_epochs,
                         n_ch, b1_pattern, kB1Taps, kB1Threshold, nav_b1_subframes_kernel, 320,
                         kB1MaxSub, max_subframes, "max_subframes >= 1", d_first, d_n_subframes,
                         d_bits);
}

extern "C" int gnsscorr_nav_b1_subframes(gnsscorr_nav_ctx* c, const void* h_series,
                                         int64_t epoch_stride_bytes, int64_t chan_stride_bytes,
                                         int n_epochs, int n_ch, int max_subframes,
                                         int32_t* h_first, int32_t* h_n_subframes,
                                         uint8_t* h_bits) {
  int rc = check_series(__func__, c, h_series, epoch_stride_bytes, chan_stride_bytes, n_epochs,
                        n_ch);
  if (!rc)
    rc = check_chain(__func__, max_subframes, "max_subframes >= 1", h_first, h_n_subframes, h_bits);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->cfg.device));
  hostctx::Staging st(c->stream);
  const char* d_series = st.in(
      (const char*)h_series, series_bytes(epoch_stride_bytes, chan_stride_bytes, n_epochs, n_ch));
  int32_t* d_first = st.out(h_first, (size_t)n_ch);
  int32_t* d_n_subframes = st.out(h_n_subframes, (size_t)n_ch);
  uint8_t* d_bits = st.out(h_bits, (size_t)n_ch * kB1MaxSub * kB1Bits);
  if (st.status()) return st.status();
  rc = gnsscorr_nav_b1_subframes_dev(c, d_series, epoch_stride_bytes, chan_stride_bytes, n_epochs,
                                     n_ch, max_subframes, d_first, d_n_subframes, d_bits);
  return rc ? rc : st.finish();
}
