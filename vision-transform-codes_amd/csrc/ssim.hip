// Structural similarity of image stacks (include/vtc_quality.h): the
// reference's compute_ssim, utils/plotting.py:42-64, i.e. scikit-image's
// compare_ssim with an 11-tap Gaussian window.  DESIGN.md 4.13 states the
// rules and the LDS budget.
//
// Two launches per call, both on the caller's stream:
//   1. ssim_tile_kernel, one workgroup per kTileH x kTileW output tile of one
//      image: both inputs with a 5-sample halo go to LDS as float64, the
//      reflection folded at load time (sep_filter.h: every index is folded
//      into the image, so a tile that hangs over the edge, or a window that
//      reflects on both sides at once, reads no sample outside it); the
//      vertical pass writes the five moment planes of X, Y, X*X, Y*Y, X*Y to
//      LDS; the horizontal pass runs per output sample and ends in the SSIM
//      formula.  The map is stored when asked for, the cropped samples are
//      summed per block into one partial in the workspace.
//   2. ssim_mean_kernel, one wave per image: adds the image's partials
//      (lane-strided, then the butterfly) and divides by (h - 10)(w - 10).
//
// Every sum has a fixed order and there is no floating-point atomic, so a
// call gives the same bits every time and an image's result does not depend
// on its neighbours in the stack.  The formula is written with __dmul_rn /
// __dadd_rn: never contracted, whatever the compiler's default.
#include "../../include/vtc_quality.h"
#include "common.h"
#include "sep_filter.h"

#include <cmath>

namespace vtc {
namespace {

constexpr int kRadius = VTC_SSIM_RADIUS;
constexpr int kTaps = 2 * kRadius + 1;
constexpr int kTileH = 16, kTileW = 32;       // output tile of one workgroup
constexpr int kInH = kTileH + 2 * kRadius;    // 26
constexpr int kInW = kTileW + 2 * kRadius;    // 42
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPlanes = 5;                    // X, Y, X*X, Y*Y, X*Y
constexpr double kSigma = 1.5, kK1 = 0.01, kK2 = 0.03;

struct SsimTaps {
  double g[kTaps];
};

// scipy.ndimage's _gaussian_kernel1d(sigma, 0, radius)
SsimTaps make_taps() {
  SsimTaps t;
  double sum = 0.0;
  for (int k = 0; k < kTaps; ++k) {
    const double v = (double)(k - kRadius);
    t.g[k] = std::exp(-0.5 / (kSigma * kSigma) * (v * v));
    sum += t.g[k];
  }
  for (int k = 0; k < kTaps; ++k) t.g[k] /= sum;
  return t;
}

struct SsimLayout {
  double* partial;   // [count][tiles_y * tiles_x]
  SsimLayout(Carver& ws, int64_t count, int32_t h, int32_t w) {
    partial = ws.take<double>((size_t)count * (size_t)ceil_div(h, kTileH) *
                              (size_t)ceil_div(w, kTileW));
  }
};

// S of one sample from its five windowed moments; C1, C2 of the image.
__device__ __forceinline__ double ssim_of(double ux, double uy, double uxx,
                                          double uyy, double uxy, double c1,
                                          double c2) {
  const double vx = __dsub_rn(uxx, __dmul_rn(ux, ux));
  const double vy = __dsub_rn(uyy, __dmul_rn(uy, uy));
  const double vxy = __dsub_rn(uxy, __dmul_rn(ux, uy));
  const double a1 = __dadd_rn(__dmul_rn(__dmul_rn(2.0, ux), uy), c1);
  const double a2 = __dadd_rn(__dmul_rn(2.0, vxy), c2);
  const double b1 =
      __dadd_rn(__dadd_rn(__dmul_rn(ux, ux), __dmul_rn(uy, uy)), c1);
  const double b2 = __dadd_rn(__dadd_rn(vx, vy), c2);
  return __ddiv_rn(__dmul_rn(a1, a2), __dmul_rn(b1, b2));
}

template <class T>
__global__ void __launch_bounds__(kThreads)
ssim_tile_kernel(const T* __restrict__ x, const T* __restrict__ y,
                 const double* __restrict__ data_range,
                 double* __restrict__ map_out, double* __restrict__ partial,
                 int h, int w, int tiles_y, int tiles_x, SsimTaps taps) {
  __shared__ double in_x[kInH * kInW], in_y[kInH * kInW];
  __shared__ double mom[kPlanes][kTileH * kInW];
  __shared__ double red[kWaves];

  int64_t t = blockIdx.x;
  const int tx = (int)(t % tiles_x);
  t /= tiles_x;
  const int ty = (int)(t % tiles_y);
  const int64_t img = t / tiles_y;
  const int y0 = ty * kTileH, x0 = tx * kTileW;
  const int64_t plane = img * (int64_t)h * w;

  for (int i = threadIdx.x; i < kInH * kInW; i += kThreads) {
    const int yy = i / kInW, xx = i - yy * kInW;
    const int gy = fold(y0 + yy - kRadius, h), gx = fold(x0 + xx - kRadius, w);
    const int64_t e = plane + (int64_t)gy * w + gx;   // 0 <= gy < h, gx < w
    in_x[i] = (double)x[e];
    in_y[i] = (double)y[e];
  }
  __syncthreads();

  // vertical pass: rows y0 .. y0 + kTileH - 1 of every column of the tile and
  // its halo, taps in ascending order
  for (int i = threadIdx.x; i < kTileH * kInW; i += kThreads) {
    const int r = i / kInW, c = i - r * kInW;
    double acc[kPlanes] = {};
    for (int k = 0; k < kTaps; ++k) {
      const double a = in_x[(r + k) * kInW + c], b = in_y[(r + k) * kInW + c];
      const double g = taps.g[k];
      acc[0] = __dadd_rn(acc[0], __dmul_rn(a, g));
      acc[1] = __dadd_rn(acc[1], __dmul_rn(b, g));
      acc[2] = __dadd_rn(acc[2], __dmul_rn(__dmul_rn(a, a), g));
      acc[3] = __dadd_rn(acc[3], __dmul_rn(__dmul_rn(b, b), g));
      acc[4] = __dadd_rn(acc[4], __dmul_rn(__dmul_rn(a, b), g));
    }
#pragma unroll
    for (int p = 0; p < kPlanes; ++p) mom[p][i] = acc[p];
  }
  __syncthreads();

  const double range = data_range[img];
  const double k1r = __dmul_rn(kK1, range), k2r = __dmul_rn(kK2, range);
  const double c1 = __dmul_rn(k1r, k1r), c2 = __dmul_rn(k2r, k2r);

  // horizontal pass and the formula: kTileH * kTileW / kThreads samples per
  // thread, summed in ascending sample order
  double local = 0.0;
  for (int o = threadIdx.x; o < kTileH * kTileW; o += kThreads) {
    const int r = o / kTileW, c = o - r * kTileW;
    const int oy = y0 + r, ox = x0 + c;
    if (oy >= h || ox >= w) continue;
    double acc[kPlanes] = {};
    for (int k = 0; k < kTaps; ++k) {
      const double g = taps.g[k];
#pragma unroll
      for (int p = 0; p < kPlanes; ++p)
        acc[p] = __dadd_rn(acc[p], __dmul_rn(mom[p][r * kInW + c + k], g));
    }
    const double s = ssim_of(acc[0], acc[1], acc[2], acc[3], acc[4], c1, c2);
    if (map_out) map_out[plane + (int64_t)oy * w + ox] = s;
    if (oy >= kRadius && oy < h - kRadius && ox >= kRadius && ox < w - kRadius)
      local = __dadd_rn(local, s);
  }
  local = wave_sum(local);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    double sum = red[0];
    for (int v = 1; v < kWaves; ++v) sum = __dadd_rn(sum, red[v]);
    partial[blockIdx.x] = sum;
  }
}

__global__ void __launch_bounds__(64)
ssim_mean_kernel(const double* __restrict__ partial, int64_t tiles,
                 double cropped, double* __restrict__ mean_out) {
  const int64_t img = blockIdx.x;
  const double* p = partial + img * tiles;
  double sum = 0.0;
  for (int64_t i = threadIdx.x; i < tiles; i += 64)
    sum = __dadd_rn(sum, p[i]);
  sum = wave_sum(sum);
  if (threadIdx.x == 0) mean_out[img] = __ddiv_rn(sum, cropped);
}

bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a);
  const uintptr_t pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + b_bytes && pb < pa + a_bytes;
}

}  // namespace
}  // namespace vtc

using namespace vtc;

extern "C" int vtc_quality_abi_version(void) { return VTC_QUALITY_ABI_VERSION; }

extern "C" size_t vtc_ssim_workspace_bytes(int64_t count, int32_t h,
                                           int32_t w) {
  if (count < 1 || h < kTaps || w < kTaps) return 0;
  return measured_bytes<SsimLayout>(count, h, w);
}

extern "C" int vtc_ssim(const void* x, const void* y, int dtype,
                        const double* data_range, double* mean_out,
                        double* map_out, int64_t count, int32_t h, int32_t w,
                        void* workspace, size_t workspace_bytes,
                        void* stream) {
  const char* who = "vtc_ssim";
  VTC_REQUIRE(x && y && data_range && mean_out, "%s: null pointer", who);
  VTC_REQUIRE(count >= 1, "%s: bad size count = %lld", who, (long long)count);
  VTC_REQUIRE(h >= 1 && w >= 1, "%s: bad size h = %d, w = %d", who, h, w);
  VTC_REQUIRE(dtype == VTC_DTYPE_F32 || dtype == VTC_DTYPE_F64,
              "%s: unknown dtype %d", who, dtype);
  if (h < kTaps || w < kTaps) {
    set_error("%s: h = %d, w = %d: the %d-tap window exceeds the image extent",
              who, h, w, kTaps);
    return VTC_ERR_UNSUPPORTED;
  }
  const int64_t tiles_y = ceil_div(h, kTileH), tiles_x = ceil_div(w, kTileW);
  const int64_t tiles = tiles_y * tiles_x;
  VTC_REQUIRE(count < ((int64_t)1 << 31) / tiles, "%s: stack too large", who);
  const size_t need = vtc_ssim_workspace_bytes(count, h, w);
  if (!workspace || workspace_bytes < need) {
    set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
              need);
    return VTC_ERR_WORKSPACE;
  }
  const size_t samples = (size_t)count * (size_t)h * (size_t)w;
  const size_t in_bytes =
      samples * (dtype == VTC_DTYPE_F32 ? sizeof(float) : sizeof(double));
  VTC_REQUIRE(!map_out ||
                  (!overlap(map_out, samples * sizeof(double), x, in_bytes) &&
                   !overlap(map_out, samples * sizeof(double), y, in_bytes)),
              "%s: map_out must not alias the images", who);
  Carver carve(workspace);
  double* partial = SsimLayout(carve, count, h, w).partial;
  const SsimTaps taps = make_taps();
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)(count * tiles));
  if (dtype == VTC_DTYPE_F32)
    ssim_tile_kernel<float><<<grid, kThreads, 0, st>>>(
        static_cast<const float*>(x), static_cast<const float*>(y), data_range,
        map_out, partial, h, w, (int)tiles_y, (int)tiles_x, taps);
  else
    ssim_tile_kernel<double><<<grid, kThreads, 0, st>>>(
        static_cast<const double*>(x), static_cast<const double*>(y),
        data_range, map_out, partial, h, w, (int)tiles_y, (int)tiles_x, taps);
  VTC_LAUNCH_CHECK();
  const double cropped =
      (double)(h - 2 * kRadius) * (double)(w - 2 * kRadius);
  ssim_mean_kernel<<<(unsigned)count, 64, 0, st>>>(partial, tiles, cropped,
                                                   mean_out);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}
