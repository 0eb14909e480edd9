// The hi/lo operand split behind every fast route (fused FC kernels, tiled
// GEMM, convolution), stated once.
//
// A float32 operand x becomes two 16-bit parts,
//   hi = cvt(x),  lo = cvt(x - float(hi))      (round to nearest even)
// and a product is formed on the matrix cores as hi*hi + hi*lo + lo*hi with
// v_mfma_f32_32x32x16_{bf16,f16} (mfma16) or v_mfma_f32_16x16x32_{bf16,f16}
// (mfma_k32: same rate per clock, a higher clock under load), f32 accumulate:
// 3 MFMA per algorithmic product, 5.3x the peak of the exact-f32 MFMA of
// gemm_f32.h.  Two part types
// behind one template flag, same MFMA rate and same bytes:
//   F16 = false ("bf16x3"): bf16 parts, 8 + 8 significand bits, ~2^-16
//     relative per product: 1.6e-5 from the reference after 200 iterations,
//     the reference's own f32 noise.  bf16 has the exponent range of f32, so
//     operands enter as they are.
//   F16 = true ("f16x3"): f16 parts, 11 + 11 bits, ~2^-21 per product, the
//     float32 noise floor (2.5e-6).  f16 has 5 exponent bits, so an operand is
//     first multiplied by a power of two (exact, and undone exactly on the f32
//     accumulators) that puts its maximum well inside the f16 range; an entry
//     2^12 below the maximum still has all 22 bits, below that the lo part
//     goes subnormal and the absolute error stays at 2^-29 of the maximum.
//     Where the scales come from is the business of the caller: fc_fused.hip
//     (per patch), x3_scale.h (per launch / per image, from max |x|).
#pragma once

#include "common.h"

namespace vtc {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// the part type of a split, and W parts as packed words / as a vector
template <bool F16> struct split_part_type { typedef __bf16 type; };
template <> struct split_part_type<true> { typedef _Float16 type; };
template <int W> struct split_words;
template <> struct split_words<4> { typedef uint2 type; typedef bf16x4 bf16; };
template <> struct split_words<8> { typedef uint4 type; typedef bf16x8 bf16; };

// (component by component: the form the kernels' register allocation was
// tuned with)
__device__ __forceinline__ uint2 pack_words(const unsigned (&w)[2]) {
  return make_uint2(w[0], w[1]);
}
__device__ __forceinline__ uint4 pack_words(const unsigned (&w)[4]) {
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// one 32x32x16 product of two fragments of 8 parts per lane
template <bool F16>
__device__ __forceinline__ f32x16 mfma16(const uint4& a, const uint4& b,
                                         const f32x16& c) {
  if (F16)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(
        __builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(
      __builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// one 16x16x32 product of two fragments of 8 parts per lane: lane l holds
// A[row l&15][k = 8(l>>4) + j] and B[k = 8(l>>4) + j][col l&15], and element e
// of the result is C[row 4(l>>4) + e][col l&15].  Same cycles per FLOP as the
// 32x32x16 form, but the chip holds a higher clock on it under load
// (profiles/fused_mfma_shape.txt).
template <bool F16>
__device__ __forceinline__ f32x4 mfma_k32(const uint4& a, const uint4& b,
                                          const f32x4& c) {
  if (F16)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(
        __builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(
      __builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// one value -> its hi and lo parts (bit patterns)
template <bool F16>
__device__ __forceinline__ void split1(float x, uint16_t& hi, uint16_t& lo) {
  typedef typename split_part_type<F16>::type part;
  const part h = (part)x;
  hi = __builtin_bit_cast(uint16_t, h);
  lo = __builtin_bit_cast(uint16_t, (part)(x - (float)h));
}
// the same, one part per call (lo = 0: hi part, 1: lo part)
template <bool F16>
__device__ __forceinline__ unsigned short split_part(float x, int lo) {
  uint16_t h, l;
  split1<F16>(x, h, l);
  return lo ? l : h;
}

// W = 4 or 8 values -> packed hi parts and (LO) lo parts.  SCALED: the values
// times a power of two first, F16 only -- the bf16 split takes its operands as
// they are (callers pass 1).
template <bool F16, int W, bool LO, bool SCALED>
__device__ __forceinline__ void split_packed_as(
    const float (&v)[W], float scale, typename split_words<W>::type& hi_out,
    typename split_words<W>::type& lo_out) {
  typedef typename split_words<W>::type words;
  if (F16) {
    // two values per instruction (v_pk_mul_f32 when scaled, v_cvt_pk_f16_f32,
    // round to nearest even as the scalar conversion; v_pk_add_f32): the same
    // arithmetic in 3 VALU instructions per element instead of 5
    typedef float pair_f32 __attribute__((ext_vector_type(2)));
    typedef _Float16 pair_f16 __attribute__((ext_vector_type(2)));
    unsigned hw[W / 2], lw[W / 2];
#pragma unroll
    for (int k = 0; k < W / 2; ++k) {
      const pair_f32 x = {SCALED ? v[2 * k] * scale : v[2 * k],
                          SCALED ? v[2 * k + 1] * scale : v[2 * k + 1]};
      const pair_f16 h = __builtin_convertvector(x, pair_f16);
      hw[k] = __builtin_bit_cast(unsigned, h);
      if (LO)
        lw[k] = __builtin_bit_cast(
            unsigned, __builtin_convertvector(
                          x - __builtin_convertvector(h, pair_f32), pair_f16));
    }
    hi_out = pack_words(hw);
    if (LO) lo_out = pack_words(lw);
  } else {
    typename split_words<W>::bf16 hi, lo;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      hi[k] = (__bf16)v[k];
      if (LO) lo[k] = (__bf16)(v[k] - (float)hi[k]);
    }
    hi_out = __builtin_bit_cast(words, hi);
    if (LO) lo_out = __builtin_bit_cast(words, lo);
  }
}
// Un-scaled: no multiply at all (the fused FC kernels are VALU-bound beside
// their MFMAs).
template <bool F16, int W, bool LO = true>
__device__ __forceinline__ void split_packed(
    const float (&v)[W], typename split_words<W>::type& hi,
    typename split_words<W>::type& lo) {
  split_packed_as<F16, W, LO, false>(v, 1.f, hi, lo);
}
template <bool F16, int W, bool LO = true>
__device__ __forceinline__ void split_packed(
    const float (&v)[W], float scale, typename split_words<W>::type& hi,
    typename split_words<W>::type& lo) {
  split_packed_as<F16, W, LO, true>(v, scale, hi, lo);
}

// The exact three-part bf16 split (gemm_b3.h):
//   h = bf16(x),  m = bf16(x - h),  l = bf16(x - h - m)   (nearest even)
// 8 + 8 + 8 significand bits cover the 24 of a float32, both subtractions are
// exact, so h + m + l == x; bf16 has the exponent range of f32, so operands
// enter as they are.  Every part product is exact in f32.  A product keeps
// hh, hm, mh, hl, lh and mm (6 MFMA); the dropped ml, lm and ll are below
// 2^-24 of the product each.  W = 4 values -> packed parts.
__device__ __forceinline__ void split3_packed(const float (&v)[4], uint2& h_out,
                                              uint2& m_out, uint2& l_out) {
  bf16x4 h, m, l;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    h[k] = (__bf16)v[k];
    const float r1 = v[k] - (float)h[k];
    m[k] = (__bf16)r1;
    l[k] = (__bf16)(r1 - (float)m[k]);
  }
  h_out = __builtin_bit_cast(uint2, h);
  m_out = __builtin_bit_cast(uint2, m);
  l_out = __builtin_bit_cast(uint2, l);
}

}  // namespace vtc
