// acq_peak.h -- the row statistics of every acquisition engine, defined once.
//
// Every engine (acq32.hip: fp32; acq64.hip: the compiled fp64 plans; acq64_gen.hip: the
// generic passes, the four-step plans, chirp-z) reports per correlation row
//   peak    the row maximum,
//   argmax  its index,
//   second  the maximum outside the open circular window (argmax - spc, argmax + spc)
// (acquisition.sci:141-166).  The kernels differ in how they hold a row (registers,
// LDS, global memory) and reduce over it; the rule itself is this file's.
//
// Tie rules (tests/test_acq_window_gpu.py pins them):
//  * argmax is the first natural index among equal maxima: better();
//  * the fp32 kernels alone keep, among one thread's own exactly equal outputs, the
//    slot visited first rather than the first natural index (push_slot_order; across
//    threads better() decides);
//  * best-of-blocks keeps a later block unless the kept maximum is strictly larger
//    (acquisition.sci:126-132), so identical blocks report the last one;
//  * a group naming one frequency twice reports the first of the identical bins.
#pragma once
#include <limits.h>
#include <math.h>
#include <hip/hip_runtime.h>
#include "gnsscorr.h"

// (v1, k1) beats (v0, k0): larger value, first natural index among equals
template <class T>
__host__ __device__ __forceinline__ bool better(T v1, int k1, T v0, int k0) {
  return v1 > v0 || (v1 == v0 && k1 < k0);
}

// k is outside the open circular window (argmax - spc, argmax + spc) of a row of N
// samples: a sample at distance exactly spc counts as outside, on both sides.
// k in [0, N) or INT_MAX (an empty Top2, whose values are both -1), argmax in [0, N).
__host__ __device__ __forceinline__ bool outside_window(int k, int argmax, int spc, int N) {
  int d = k - argmax;
  d += d < 0 ? N : 0;
  return d >= spc && d <= N - spc;
}

// The second-peak candidates of GLONASS/L3/acquisition.sci:134-153 (set_peak_period): the
// range is written on a period S = samplesPerCode while the row holds several periods
// (5 S there), so it is not a window circular in the row.  0-based, a = argmax in
// [0, row length), s = spc, 2 s < S:
//   a <= s            a + s <= k <= S + a - s      (index S itself is reachable: a = s)
//   else a >= S - s   a + s - S <= k <= a - s      (linear, not wrapped, for every such a)
//   else              k <= a - s  or  a + s <= k <= S - 1
// The caller scans k over the row only, so an index at or past the row's end (S + a - s
// with S = row length, on which Scilab would abort) is no candidate.  One thread's
// top-2 does not answer this set: rows with a period take the exact pass.
__host__ __device__ __forceinline__ bool in_period_range(int k, int a, int s, int S) {
  if (a <= s) return k >= a + s && k <= S + a - s;
  if (a >= S - s) return k >= a + s - S && k <= a - s;
  return k <= a - s || (k >= a + s && k <= S - 1);
}

// Bounds of that set: every k in_period_range(k, a, s, S) admits lies in [lo, hi], and
// hi - lo <= S, so a scan of lo .. hi under the predicate visits at most S + 1 indices
// whatever the row's length (the concatenated rows of COMPASS/B1/acquisition_7x3ms.sci:
// 21 periods).  Not the rule: the predicate above still decides every index.
struct PeriodSpan {
  int lo, hi;
};
__host__ __device__ __forceinline__ PeriodSpan period_span(int a, int s, int S) {
  if (a <= s) return PeriodSpan{a + s, S + a - s};
  if (a >= S - s) return PeriodSpan{a + s - S, a - s};
  return PeriodSpan{0, S - 1};
}

// A set of samples at least `stride` apart (circularly) has at most one member among
// the window's 2 spc - 1 samples when this holds; then the set's {maximum, its index,
// runner-up} answer `second` in one pass: the maximum if it is outside the window,
// else the runner-up, which is.  Each caller states the stride of its own sets.
__host__ __device__ constexpr bool top2_exact(int stride, int spc) {
  return 2 * spc - 1 <= stride;
}

// {maximum, runner-up, first natural index of the maximum} of a set of samples >= 0
template <class T>
struct Top2 {
  T a1 = -1, a2 = -1;
  int ak = INT_MAX;
  // one more sample (a2 = max(a2, min(v, a1)) holds whether or not v takes the lead)
  __host__ __device__ __forceinline__ void push(T v, int k) {
    const bool take = better(v, k, a1, ak);
    a2 = fmax(a2, fmin(v, a1));
    ak = take ? k : ak;
    a1 = fmax(a1, v);
  }
  // the top-2 of a disjoint set
  __host__ __device__ __forceinline__ void merge(const Top2& b) {
    const bool take = better(b.a1, b.ak, a1, ak);
    a2 = take ? fmax(a1, b.a2) : fmax(a2, b.a1);
    ak = take ? b.ak : ak;
    a1 = take ? b.a1 : a1;
  }
  // this set's candidate for `second`, exact where top2_exact holds for the set
  __host__ __device__ __forceinline__ T second(int argmax, int spc, int N) const {
    return outside_window(ak, argmax, spc, N) ? a1 : a2;
  }
};

// The fp32 kernels' push: d is the thread's slot, not a natural index, and an exact
// tie keeps the slot pushed first (3 VALU operations; Top2::push's index compare
// would need the natural index of every output).
__device__ __forceinline__ void push_slot_order(float v, int d, float& m1, float& m2, int& d1) {
  d1 = v > m1 ? d : d1;
  m2 = __builtin_amdgcn_fmed3f(m2, m1, v);
  m1 = fmaxf(m1, v);
}

// work unit -> (row, block): a non-coherent unit is a whole row, a best-of-blocks
// unit one block of it
struct UnitRow {
  int rowid, blk0;
};
__host__ __device__ __forceinline__ UnitRow unit_row(int unit, int n_blocks, bool nc) {
  return nc ? UnitRow{unit, 0} : UnitRow{unit / n_blocks, unit % n_blocks};
}

// the row record of (rowid, blk0); a non-coherent row carries no block choice
template <class T>
__device__ __forceinline__ void store_row(gnsscorr_acq_row* stats, int rowid, int blk0,
                                          int n_blocks, bool nc, T peak, int argmax,
                                          T second) {
  gnsscorr_acq_row r;
  r.peak = peak;
  r.second = second;
  r.argmax = argmax;
  r.block = nc ? -1 : blk0;
  stats[(long)rowid * n_blocks + blk0] = r;
}

// canonical residue of f on a grid of spacing delta, in [0, delta)
__host__ __device__ __forceinline__ double grid_residue(double f, double delta) {
  const double r = fmod(f, delta);
  return r < 0 ? r + delta : r;
}
