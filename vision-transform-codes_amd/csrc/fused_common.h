// Device helpers shared by the fused persistent kernels (fc_fused.hip: state on
// chip; fused_stream.hip: state streamed): dictionary packing into MFMA
// fragment order (32x32x16 operands, or 16x16x32 ones for fc_fused.hip's
// second tile), the f16 dictionary scale, buffer loads, stamps.  The hi/lo
// operand split and the MFMA wrapper are split_operand.h's.
#pragma once
#include "common.h"
#include "split_operand.h"

namespace vtc {

constexpr int kFP = 32;    // patches per workgroup
constexpr int kFN = 256;   // pixels per patch
constexpr int kPhaseAtoms = 128;

// ---------------------------------------------------------------- packing
// packA fragment (tile t of 32 atoms, k-step ks over pixels), lane l:
//   D[32t + (l&31)][16ks + 8(l>>5) + j],  j = 0..7
// packT fragment (phase p, pixel block nb of 32, k-step ks over the phase's
// atoms), lane l:
//   D[128p + 16ks + 8(l>>5) + j][32nb + (l&31)]
// TILE16, the same tiles as 16x16x32 operands (fc_fused.hip): still 16 one-KiB
// fragments per wave and segment, the same bytes in the same workspace.
// packA fragment (tile t, 16-atom half m, k-step ks over 32 pixels; fragment
// t*16 + 2ks + m), lane l:
//   D[32t + 16m + (l&15)][32ks + 8(l>>4) + j]
// packT fragment (phase p, pixel block nb of 16, k-step ks over 32 of the
// phase's atoms; fragment (16p + nb)*4 + ks), lane l:
//   D[128p + 32ks + 8(l>>4) + j][16nb + (l&15)]

// F16: sigma_D = 2^(8 - floor(log2 max|D|)), so that max |sigma_D D| lies in
// [256, 512): far from the f16 overflow (65504) and with the lo parts of all
// but vanishing entries in the normal range.  One block; scale[0] = sigma_D,
// scale[1] = 1 / sigma_D.  (Not cx_array_scale_kernel of x3_scale.h: that one
// aims at [16, 32) and works on bit patterns; this range is the fused kernels'.)
static __global__ __launch_bounds__(1024) void dictionary_scale_kernel(
    const float* __restrict__ D, int64_t count, float* __restrict__ scale) {
  __shared__ float part[16];
  float m = 0.f;
  // count = s * 256: 16-byte loads, four independent maxima in flight
  const float4* D4 = reinterpret_cast<const float4*>(D);
  float m1 = 0.f, m2 = 0.f, m3 = 0.f;
  for (int64_t i = threadIdx.x; i < count / 4; i += 1024) {
    const float4 v = D4[i];
    m = fmaxf(m, fabsf(v.x));
    m1 = fmaxf(m1, fabsf(v.y));
    m2 = fmaxf(m2, fabsf(v.z));
    m3 = fmaxf(m3, fabsf(v.w));
  }
  m = fmaxf(fmaxf(m, m1), fmaxf(m2, m3));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 16; ++k) m = fmaxf(m, part[k]);
    int e = 0;
    if (m > 0.f && m < __builtin_inff()) e = ilogbf(m);
    e = e < -100 ? -100 : (e > 100 ? 100 : e);
    scale[0] = ldexpf(1.f, 8 - e);
    scale[1] = ldexpf(1.f, e - 8);
  }
}

// Both parts in one pass (loA / loT null: hi part only).
template <bool F16, bool TILE16 = false>
__global__ void pack_dictionary_kernel(const float* __restrict__ D, int s,
                                       unsigned short* __restrict__ packA,
                                       unsigned short* __restrict__ packT,
                                       unsigned short* __restrict__ loA,
                                       unsigned short* __restrict__ loT,
                                       const float* __restrict__ scale) {
  const float sg = F16 ? scale[0] : 1.f;
  const int64_t frags = (int64_t)s * kFN / 8;  // 16-byte units per packing
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < frags;
       u += (int64_t)gridDim.x * blockDim.x) {
    const int l = (int)(u & 63);
    const int r = TILE16 ? (l & 15) : (l & 31), h = TILE16 ? (l >> 4) : (l >> 5);
    {
      const int64_t f = u >> 6;  // = t*16 + ks, TILE16: t*16 + 2ks + m
      const int t = (int)(f >> 4), ks = (int)(f & 15);
      const float* src =
          TILE16 ? D + (int64_t)(32 * t + 16 * (ks & 1) + r) * kFN +
                       32 * (ks >> 1) + 8 * h
                 : D + (int64_t)(32 * t + r) * kFN + 16 * ks + 8 * h;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = src[j] * sg;
        packA[u * 8 + j] = split_part<F16>(v, 0);
        if (loA) loA[u * 8 + j] = split_part<F16>(v, 1);
      }
    }
    {
      const int64_t f = u >> 6;  // = (p*8 + nb)*8 + ks, TILE16: (p*16 + nb)*4 + ks
      const int ks = (int)(f & (TILE16 ? 3 : 7)), p = (int)(f >> 6);
      const int nb = TILE16 ? (int)((f >> 2) & 15) : (int)((f >> 3) & 7);
      const float* src =
          TILE16 ? D + (int64_t)(128 * p + 32 * ks + 8 * h) * kFN + 16 * nb + r
                 : D + (int64_t)(128 * p + 16 * ks + 8 * h) * kFN + 32 * nb + r;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = src[(int64_t)j * kFN] * sg;
        packT[u * 8 + j] = split_part<F16>(v, 0);
        if (loT) loT[u * 8 + j] = split_part<F16>(v, 1);
      }
    }
  }
}

template <int MODE>
__device__ __forceinline__ float shrink_fast(float c, float cutoff) {
  if (MODE == VTC_SOFT) {
    // sign(c) * max(|c| - t, 0) == c - clamp(c, -t, t) bit for bit (up to the
    // sign of a zero result): one v_med3 + one v_sub.
    return sub_rn(c, __builtin_amdgcn_fmed3f(c, -cutoff, cutoff));
  }
  return shrink(c, cutoff, MODE);
}

__device__ __forceinline__ uint4 buffer_load16(__amdgpu_buffer_rsrc_t rsrc,
                                               unsigned voff, unsigned soff) {
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 0);
  return make_uint4(v[0], v[1], v[2], v[3]);
}

// In-kernel stamps (diagnostic instantiation only, STAMP = true): where a
// phase spends its cycles.  s_memtime + its wait in one statement, fenced.
__device__ __forceinline__ unsigned long long stamp_now() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}

}  // namespace vtc
