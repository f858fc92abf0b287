// if2.h -- device helpers for the IF sample formats of the batched API.
//
// GNSSCORR_IF_PACKED2 (gnsscorr.h): four 2-bit codes per byte, element e of a
// stream in bits 2*(e&3)..2*(e&3)+1 of byte e>>2 (elements are I,Q,I,Q,... for
// complex streams), code c -> level 2c-3, i.e. the GN3S LUT {-3,-1,1,3} of
// GPS_Source::Read_GN3S (REALTIME_RECEIVERS/GPS/GPS_SDR_REAL_TIME_GPS_RECEIVER/
// objects/gps_source.cpp:692).  A packed stream holds exactly the int8 stream
// of those levels in a quarter of the bytes, so every kernel result is
// identical to the int8 path on the unpacked samples.
#ifndef GNSSCORR_IF2_H
#define GNSSCORR_IF2_H
#include <hip/hip_runtime.h>
#include <stdint.h>

// one packed byte (4 elements) -> 4 int8 levels, element j in byte j
__device__ __forceinline__ uint32_t if2_expand_byte(uint32_t b) {
  uint32_t t = b | (b << 6);    // codes 0, 1 -> bytes 0, 1 (bits 0-1, 8-9)
  t |= t << 12;                 // codes 2, 3 -> bytes 2, 3 (bits 16-17, 24-25)
  t &= 0x03030303u;
  // v_perm_b32 byte select from {0, table}: selector c picks table byte c
  return __builtin_amdgcn_perm(0u, 0x0301FFFDu, t);   // {-3, -1, 1, 3} as int8
}

// one packed 32-bit word (16 elements) -> four int8 words
__device__ __forceinline__ uint4 if2_expand_word(uint32_t p) {
  return make_uint4(if2_expand_byte(p & 0xFFu), if2_expand_byte((p >> 8) & 0xFFu),
                    if2_expand_byte((p >> 16) & 0xFFu), if2_expand_byte(p >> 24));
}

// element e of a stream (int8 or packed)
__device__ __forceinline__ int if_elem(const int8_t* __restrict__ base, int64_t e, bool packed) {
  if (packed) {
    const uint32_t b = reinterpret_cast<const uint8_t*>(base)[e >> 2];
    return 2 * (int)((b >> (2 * (e & 3))) & 3u) - 3;
  }
  return base[e];
}

// bytes holding n elements
__host__ __device__ __forceinline__ int64_t if_bytes(int64_t n_elems, bool packed) {
  return packed ? (n_elems + 3) >> 2 : n_elems;
}

// ---- packed records of the float trackers (sgt, e1t, l3t; gnsscorr_*_set_packed).
// A record is the element stream above from a 16-byte-aligned stream base; FT is
// settings.fileType: 2 = sample s is elements 2s, 2s+1 (the int8 pair), 1 = element s.

// sample s of a record as the int8 path's per-sample load returns it: FT 2 the pair
// as a 16-bit word (first element in the low byte), FT 1 the level
template <int FT>
__device__ __forceinline__ int if2_sample(const uint8_t* __restrict__ base, int64_t s) {
  if (FT == 2) {
    // both elements of a pair sit in one nibble
    const uint32_t b = (uint32_t)base[s >> 1] >> (4 * (int)(s & 1));
    const uint32_t t = (b & 3u) | ((b & 0xCu) << 6) | 0x0C0C0000u;   // selector 0x0C: byte 0x00
    return (int)__builtin_amdgcn_perm(0u, 0x0301FFFDu, t);
  }
  return 2 * (int)(((uint32_t)base[s >> 2] >> (2 * (int)(s & 3))) & 3u) - 3;
}

// dword d of a record that ends at byte `end` (if_bytes of its elements): a dword
// the end cuts is read byte by byte, nothing at or past the end is loaded
__device__ __forceinline__ uint32_t if2_load_dword(const uint8_t* __restrict__ base, int64_t d,
                                                   int64_t end) {
  const uint8_t* p = base + 4 * d;
  if (4 * d + 4 <= end) return *reinterpret_cast<const uint32_t*>(p);
  uint32_t v = 0;
#pragma unroll
  for (int i = 0; i < 3; i++)
    if (4 * d + i < end) v |= (uint32_t)p[i] << (8 * i);
  return v;
}

// kW consecutive dwords from a dword boundary in one dword / dwordx2 / dwordx4 load
typedef uint32_t if2_u32x2a4 __attribute__((ext_vector_type(2), aligned(4)));
typedef uint32_t if2_u32x4a4 __attribute__((ext_vector_type(4), aligned(4)));
template <int kW>
__device__ __forceinline__ void if2_load_words(const uint32_t* __restrict__ p, uint32_t (&x)[kW]) {
  static_assert(kW == 1 || kW == 2 || kW == 4, "a chunk is 4, 8 or 16 packed bytes");
  if constexpr (kW == 1) {
    x[0] = p[0];
  } else if constexpr (kW == 2) {
    const if2_u32x2a4 v = *reinterpret_cast<const if2_u32x2a4*>(p);
    x[0] = v.x; x[1] = v.y;
  } else {
    const if2_u32x4a4 v = *reinterpret_cast<const if2_u32x4a4*>(p);
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
  }
}
#endif
