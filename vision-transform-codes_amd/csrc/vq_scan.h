// The scan of the vector quantiser, shared by vq.hip (include/vtc_vq.h) and
// vq_large.hip (include/vtc_vq_large.h): vq_assign_kernel, its launcher and
// the small helpers both translation units need.  The kernel has no limit on
// the number of codewords: the codebook streams through LDS in tiles.  Each
// translation unit instantiates its own copy (internal linkage).
#pragma once

#include "../../include/vtc_vq.h"
#include "common.h"

namespace vtc {
namespace {

constexpr int kThreads = VTC_VQ_ASSIGN_ROWS;
constexpr int kMaxDim = VTC_VQ_MAX_DIM;
constexpr int kTileDoubles = VTC_VQ_TILE_DOUBLES;
constexpr int64_t kMaxGrid = ((int64_t)1 << 31) - 1;

static_assert(kThreads == 256, "one row per lane of a 256-thread workgroup");
static_assert(kTileDoubles >= kMaxDim, "a tile holds at least one codeword");

__device__ __forceinline__ double inf_f64() {
  return __longlong_as_double(0x7ff0000000000000ll);
}
__device__ __forceinline__ double nan_f64() {
  return __longlong_as_double(0x7ff8000000000000ll);
}
__device__ __forceinline__ int clamp_k(int k, int kmax) {
  return k < 1 ? 1 : (k > kmax ? kmax : k);
}

__global__ void zero_status_kernel(int64_t* __restrict__ status) {
  status[0] = 0;
}

// `active` null: a plain assignment.  `rowdist` null: not wanted.
template <int DP, bool kLengths>
__global__ void __launch_bounds__(kThreads)
vq_assign_kernel(const float* __restrict__ vectors, int64_t b, int d,
                 const double* __restrict__ codebook,
                 const double* __restrict__ lengths,
                 const int* __restrict__ k, int kmax, double lambda,
                 const int* __restrict__ active, int* __restrict__ indices,
                 float* __restrict__ dequantized,
                 double* __restrict__ rowdist, int64_t* __restrict__ status) {
  constexpr int kTile = kTileDoubles / DP;   // whole codewords of one tile
  __shared__ double sh_cb[kTile * DP];
  __shared__ double sh_len[kLengths ? kTile : 1];
  if (active && active[0] == 0) return;      // the same for every thread
  const int kk = clamp_k(k[0], kmax);
  const int64_t row = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool have = row < b;

  double x[DP];
  bool nan = false;
#pragma unroll
  for (int t = 0; t < DP; ++t) {
    float v = 0.0f;
    if (have && t < d) v = vectors[row * d + t];
    nan = nan || v != v;
    x[t] = (double)v;
  }

  int best_i = 0;
  double best = inf_f64(), best_d = 0.0;
  for (int base = 0; base < kk; base += kTile) {
    const int cells = kk - base < kTile ? kk - base : kTile;
    __syncthreads();                         // the previous tile has been read
    for (int e = threadIdx.x; e < cells * DP; e += kThreads) {
      const int i = e / DP, t = e - i * DP;
      sh_cb[e] = t < d ? codebook[(base + i) * d + t] : 0.0;   // base + i < kk
    }
    if (kLengths)
      for (int e = threadIdx.x; e < cells; e += kThreads)
        sh_len[e] = lengths[base + e];
    __syncthreads();
    for (int i = 0; i < cells; ++i) {
      const double* c = sh_cb + i * DP;
      double e = __dsub_rn(x[0], c[0]);
      double dist = __dmul_rn(e, e);         // 0.0 + e * e, bit for bit
#pragma unroll
      for (int t = 1; t < DP; ++t) {
        e = __dsub_rn(x[t], c[t]);
        dist = __dadd_rn(dist, __dmul_rn(e, e));
      }
      const double cost =
          kLengths ? __dadd_rn(dist, __dmul_rn(lambda, sh_len[i])) : dist;
      if (cost < best || base + i == 0) {   // cell 0 starts the scan
        best = cost;
        best_d = dist;
        best_i = base + i;
      }
    }
  }
  if (!have) return;
  const int cell = nan ? -1 : best_i;
  indices[row] = cell;
  if (rowdist) rowdist[row] = nan ? 0.0 : best_d;
  if (dequantized) {
    for (int t = 0; t < d; ++t)
      dequantized[row * d + t] = nan ? __int_as_float(0x7fc00000)
                                     : (float)codebook[best_i * d + t];
  }
  if (nan)
    atomicAdd(reinterpret_cast<unsigned long long*>(status), 1ull);
}

// d rounded up to a register count the kernels are built for
#define VTC_VQ_DISPATCH(d, CALL) \
  do {                           \
    if ((d) <= 4) {              \
      CALL(4);                   \
    } else if ((d) <= 8) {       \
      CALL(8);                   \
    } else if ((d) <= 16) {      \
      CALL(16);                  \
    } else if ((d) <= 24) {      \
      CALL(24);                  \
    } else {                     \
      CALL(32);                  \
    }                            \
  } while (0)

void launch_assign(const float* vectors, int64_t b, int d,
                   const double* codebook, const double* lengths,
                   const int* k, int kmax, double lambda, const int* active,
                   int* indices, float* dequantized, double* rowdist,
                   int64_t* status, hipStream_t st) {
  const unsigned grid = (unsigned)ceil_div(b, kThreads);
#define VTC_VQ_ASSIGN(DP)                                                    \
  if (lambda != 0.0)                                                         \
    vq_assign_kernel<DP, true><<<grid, kThreads, 0, st>>>(                   \
        vectors, b, d, codebook, lengths, k, kmax, lambda, active, indices,  \
        dequantized, rowdist, status);                                       \
  else                                                                       \
    vq_assign_kernel<DP, false><<<grid, kThreads, 0, st>>>(                  \
        vectors, b, d, codebook, lengths, k, kmax, lambda, active, indices,  \
        dequantized, rowdist, status)
  VTC_VQ_DISPATCH(d, VTC_VQ_ASSIGN);
#undef VTC_VQ_ASSIGN
}

}  // namespace
}  // namespace vtc
