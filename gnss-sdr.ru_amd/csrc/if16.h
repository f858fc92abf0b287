// if16.h -- device helpers for int16 IF records (GNSSCORR_IF_INT16 of the fp64
// acquisition, record format 2 of the float trackers sgt, e1t, l3t).
//
// Elements are native little-endian int16_t: settings.dataType 'sl' of the Scilab
// receivers (dataTypeSizeInBytes = 2) and the CPX packets GPS_Source::Read writes
// (objects/gps_source.cpp:167-176).  FT is settings.fileType: 2 = sample s is
// elements 2s, 2s+1 (one dword), 1 = element s.  Every value is carried to fp64 from
// its full 16 bits: nothing is narrowed.
//
// The chunked tracker paths keep the chunk grid of an int8 record on a
// 16-byte-aligned base (ChunkGrid's constructor from a sample position), so a lane
// holds the samples it holds on int8 and the sums of int8-range levels are the int8
// path's to the bit.  A chunk is then twice the bytes: a 16-sample I,Q chunk is 64
// bytes, four dwordx4 loads from a 32-byte boundary of the stream.
#ifndef GNSSCORR_IF16_H
#define GNSSCORR_IF16_H
#include <hip/hip_runtime.h>
#include <stdint.h>

// bytes of one sample
template <int FT>
__host__ __device__ constexpr int if16_sample_bytes() { return FT == 2 ? 4 : 2; }

// sample s of a record as the per-sample passes take it: FT 2 the pair as a dword
// (first element in the low half), FT 1 the sign-extended value
template <int FT>
__device__ __forceinline__ int if16_sample(const uint8_t* __restrict__ base, int64_t s) {
  if (FT == 2) return (int)reinterpret_cast<const uint32_t*>(base)[s];
  return reinterpret_cast<const int16_t*>(base)[s];
}

// the halves of a pair dword: sh = 0 the first element, 16 the second
__device__ __forceinline__ int if16_half(uint32_t w, int sh) {
  return (int)__builtin_amdgcn_sbfe(w, sh, 16);
}

// sample n of a chunk held as dwords from its first sample on: FT 2 dword n (re at
// bit sh_re, im at 16 - sh_re), FT 1 half n & 1 of dword n >> 1
template <int FT>
__device__ __forceinline__ int if16_re(const uint32_t* w, int n, int sh_re) {
  if (FT == 2) return if16_half(w[n], sh_re);
  return if16_half(w[n >> 1], (n & 1) * 16);
}
template <int FT>
__device__ __forceinline__ int if16_im(const uint32_t* w, int n, int sh_re) {
  if (FT == 2) return if16_half(w[n], 16 - sh_re);
  return 0;
}

// W_n * raw of sample n of such a chunk (W = exp(i*A*n/fs) as (cos, sin)): the int8
// chunk loops' forms on the full 16 bits
template <int FT>
__device__ __forceinline__ void if16_wraw(const uint32_t* w, int n, int sh_re, double2 W,
                                          double& ur, double& ui) {
#pragma clang fp contract(off)
  const double re = (double)if16_re<FT>(w, n, sh_re);
  if (FT == 2) {
    const double im = (double)if16_im<FT>(w, n, sh_re);
    ur = fma(W.x, re, -(W.y * im));
    ui = fma(W.x, im, W.y * re);
  } else {
    ur = W.x * re;
    ui = W.y * re;
  }
}

// the dword at byte offset o (a multiple of 2) of a record that ends at byte `end`
// (a multiple of 2): a dword the end cuts gives its first element alone, nothing at
// or past the end is loaded
__device__ __forceinline__ uint32_t if16_load_dword(const uint8_t* __restrict__ base, int64_t o,
                                                    int64_t end) {
  if (o + 4 <= end) return *reinterpret_cast<const uint32_t*>(base + o);
  if (o + 2 <= end) return *reinterpret_cast<const uint16_t*>(base + o);
  return 0u;
}

// the 16-byte word at byte offset o (a multiple of 16) of such a record: one dwordx4
// load when it lies inside, else element by element up to the end
__device__ __forceinline__ uint4 if16_load_word(const uint8_t* __restrict__ base, int64_t o,
                                                int64_t end) {
  if (o + 16 <= end) return *reinterpret_cast<const uint4*>(base + o);
  return make_uint4(if16_load_dword(base, o, end), if16_load_dword(base, o + 4, end),
                    if16_load_dword(base, o + 8, end), if16_load_dword(base, o + 12, end));
}
#endif
