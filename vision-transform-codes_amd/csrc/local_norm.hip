// Gaussian local normalisation of whole images and the component / sample
// statistics of a patch matrix: the preprocessing operations of
// create_patch_training_set that are not whitening or patching.
//
// Restates
//   utils/image_processing.py:18-60    filter_sd (convolve2d, 'same', 'symm')
//   utils/image_processing.py:136-170  get_gaussian_filter_2d
//   utils/image_processing.py:463-493  local_contrast_normalization
//   utils/image_processing.py:496-523  local_luminance_subtraction
//   utils/image_processing.py:527-594  center_each_component,
//                                      center_each_sample,
//                                      normalize_component_variance
//
// The Gaussian window of the reference is the normalised outer product of one
// 1D factor, so the 2D convolution is applied as two 1D passes, both
// accumulated in float64 (the reference convolves in float64 and rounds the
// result to float32).  scipy's 'symm' boundary is numpy's 'symmetric' padding:
// index i folds with period 2n, i mod 2n in [n, 2n) mirroring to 2n - 1 - i,
// which stays right for windows wider than the image.
#include "common.h"
#include "sep_filter.h"

#include <cmath>

namespace vtc {

namespace {

constexpr int kMaxRadius = 128;       // taps travel as a kernel argument
constexpr int kTileRadius = 16;       // LDS route up to r = 16 (sigma 4 -> 8)
constexpr int kTileH = 32;            // output tile of one workgroup
constexpr int kTileW = 64;
constexpr int kThreads = 256;

struct Taps {
  int radius;
  double g[2 * kMaxRadius + 1];
};

// float32 value the filter reads: the pixel (LLS) or its float32 square (LCN,
// `image**2`).
__device__ __forceinline__ float filter_input(float v, int mode) {
  return mode == VTC_LOCAL_CONTRAST ? mul_rn(v, v) : v;
}

// The reference's epilogues, in its operation order, all in float32.
__device__ __forceinline__ void epilogue(double filtered, float x, int mode,
                                         float* out, float* aux) {
  float f = (float)filtered;
  if (mode == VTC_LOCAL_CONTRAST) {
    if (f == 0.f) f = 1.f;            // local_variance[local_variance == 0] = 1
    const float s = __fsqrt_rn(f);
    *aux = s;
    *out = __fdiv_rn(x, s);
  } else {
    *aux = f;
    *out = sub_rn(x, f);
  }
}

// One workgroup: a kTileH x kTileW output tile of one (image, channel) plane.
// The input tile plus halo is staged in LDS with the reflection folded at
// load time, the horizontal pass goes to LDS in float64, the vertical pass
// runs in registers.
__global__ void __launch_bounds__(kThreads)
local_norm_tile_kernel(const float* __restrict__ x, float* __restrict__ out,
                       float* __restrict__ aux, int h, int w, int c,
                       int tiles_y, int tiles_x, int mode, Taps taps) {
  extern __shared__ double lds_d[];
  const int r = taps.radius;
  const int k_taps = 2 * r + 1;
  const int in_h = kTileH + 2 * r;
  const int in_w = kTileW + 2 * r;
  double* hsum = lds_d;                                        // in_h x kTileW
  float* tile = reinterpret_cast<float*>(lds_d + in_h * kTileW);  // in_h x in_w

  int64_t t = blockIdx.x;
  const int tx = (int)(t % tiles_x);
  t /= tiles_x;
  const int ty = (int)(t % tiles_y);
  t /= tiles_y;
  const int ch = (int)(t % c);
  const int64_t img = t / c;
  const int y0 = ty * kTileH, x0 = tx * kTileW;
  const int64_t plane = img * (int64_t)h * w;

  for (int i = threadIdx.x; i < in_h * in_w; i += kThreads) {
    const int yy = i / in_w, xx = i - yy * in_w;
    const int gy = fold(y0 + yy - r, h), gx = fold(x0 + xx - r, w);
    tile[i] = filter_input(x[(plane + (int64_t)gy * w + gx) * c + ch], mode);
  }
  __syncthreads();
  // Each thread keeps several independent sums (k outer), so the float64
  // FMA chains overlap; every sum still runs over k in ascending order.
  constexpr int kColsPerThread = 4;
  constexpr int kColStride = kTileW / kColsPerThread;
  for (int i = threadIdx.x; i < in_h * kColStride; i += kThreads) {
    const int yy = i / kColStride, xx = i - yy * kColStride;
    const float* row = tile + yy * in_w + xx;
    double acc[kColsPerThread] = {};
    for (int k = 0; k < k_taps; ++k) {
      const double g = taps.g[k];
#pragma unroll
      for (int q = 0; q < kColsPerThread; ++q)
        acc[q] += (double)row[q * kColStride + k] * g;
    }
#pragma unroll
    for (int q = 0; q < kColsPerThread; ++q)
      hsum[yy * kTileW + q * kColStride + xx] = acc[q];
  }
  __syncthreads();
  const int xx = threadIdx.x % kTileW;
  const int ox = x0 + xx;
  if (ox >= w) return;
  constexpr int kRowsPerThread = kTileH / (kThreads / kTileW);
  const int row0 = (threadIdx.x / kTileW) * kRowsPerThread;
  const double* col = hsum + row0 * kTileW + xx;
  double acc[kRowsPerThread] = {};
  for (int k = 0; k < k_taps; ++k) {
    const double g = taps.g[k];
#pragma unroll
    for (int j = 0; j < kRowsPerThread; ++j)
      acc[j] += col[(j + k) * kTileW] * g;
  }
#pragma unroll
  for (int j = 0; j < kRowsPerThread; ++j) {
    const int oy = y0 + row0 + j;
    if (oy >= h) break;
    const int64_t e = (plane + (int64_t)oy * w + ox) * c + ch;
    epilogue(acc[j], x[e], mode, out + e, aux + e);
  }
}

// Wide windows: the horizontal pass into a float64 workspace plane (same
// channel-last layout as the images), then the vertical pass and epilogue.
__global__ void local_norm_rows_kernel(const float* __restrict__ x,
                                       double* __restrict__ ws, int64_t total,
                                       int w, int c, int mode, Taps taps) {
  const int r = taps.radius;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int ch = (int)(e % c);
    const int64_t pix = e / c;
    const int px = (int)(pix % w);
    const int64_t row = pix - px;
    ws[e] = tap_sum(
        [&](int k) { return taps.g[k]; }, 2 * r + 1, r, px, w, [&](int gx) {
          return (double)filter_input(x[(row + gx) * c + ch], mode);
        });
  }
}

__global__ void local_norm_cols_kernel(const float* __restrict__ x,
                                       const double* __restrict__ ws,
                                       float* __restrict__ out,
                                       float* __restrict__ aux, int64_t total,
                                       int h, int w, int c, int mode,
                                       Taps taps) {
  const int r = taps.radius;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int ch = (int)(e % c);
    const int64_t pix = e / c;
    const int px = (int)(pix % w);
    const int64_t prow = pix / w;
    const int py = (int)(prow % h);
    const int64_t plane = prow - py;
    const double acc = tap_sum(
        [&](int k) { return taps.g[k]; }, 2 * r + 1, r, py, h,
        [&](int gy) { return ws[((plane + gy) * w + px) * c + ch]; });
    epilogue(acc, x[e], mode, out + e, aux + e);
  }
}

// get_gaussian_filter_2d(sigma, (4 sigma + 1, 4 sigma + 1)): coordinates
// -floor(ws / 2) .. upper - 1 with upper = floor(ws / 2) + 1 for a window
// that is not an even number, floor(ws / 2) otherwise.  Returns the tap count
// (0 when sigma is not a positive number below 1e7).
int gaussian_tap_count(double sigma, int* lower) {
  if (!(sigma > 0.0) || !(sigma < 1e7)) return 0;
  const double ws = 4.0 * sigma + 1.0;
  const double half = std::floor(ws / 2.0);
  *lower = -(int)half;
  const int upper = std::fmod(ws, 2.0) != 0.0 ? (int)half + 1 : (int)half;
  return upper - *lower;
}

int make_taps(double sigma, Taps* taps, const char* who) {
  int lower = 0;
  const int n = gaussian_tap_count(sigma, &lower);
  VTC_REQUIRE(n > 0, "%s: filter_sigma must be a positive number below 1e7",
              who);
  VTC_REQUIRE(n % 2 == 1,
              "%s: filter_sigma %g gives an even window of %d taps (4 sigma + "
              "1 must not be an even number)", who, sigma, n);
  if (-lower > kMaxRadius) {
    set_error("%s: filter radius %d exceeds %d (filter_sigma %g)", who,
              -lower, kMaxRadius, sigma);
    return VTC_ERR_UNSUPPORTED;
  }
  taps->radius = -lower;
  double sum = 0.0;
  for (int k = 0; k < n; ++k) {
    const double v = (double)(lower + k);
    taps->g[k] = std::exp(-0.5 * (v * v) / (sigma * sigma));
    sum += taps->g[k];
  }
  for (int k = 0; k < n; ++k) taps->g[k] /= sum;
  return VTC_OK;
}

size_t tile_lds_bytes(int r) {
  return (size_t)(kTileH + 2 * r) * kTileW * sizeof(double) +
         (size_t)(kTileH + 2 * r) * (kTileW + 2 * r) * sizeof(float);
}

unsigned grid_for(int64_t total) {
  int64_t blocks = ceil_div(total, 256);
  if (blocks > 65536) blocks = 65536;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

// ---- column moments / apply ------------------------------------------------
constexpr int kMomCols = 64;          // columns per workgroup
constexpr int kMomLanes = kThreads / kMomCols;
constexpr int64_t kMaxSlabs = 1024;

template <class T>
__device__ __forceinline__ float as_f32(T v) { return (float)v; }

int64_t moment_slabs(int64_t rows, int64_t cols) {
  const int64_t col_blocks = ceil_div(cols, kMomCols);
  int64_t slabs = ceil_div(rows, 256);
  const int64_t want = ceil_div(2048, col_blocks);
  if (slabs > want) slabs = want;
  if (slabs > kMaxSlabs) slabs = kMaxSlabs;
  return slabs < 1 ? 1 : slabs;
}

// Partial sums of (x - x[0, j]) and its square per (slab, column), float64.
// The shift by the column's first value keeps the one-pass variance free of
// cancellation when the mean is large against the spread.
template <class T>
__global__ void __launch_bounds__(kThreads)
column_partials_kernel(const T* __restrict__ x, int64_t rows, int64_t cols,
                       int64_t slab_rows, double* __restrict__ partial) {
  __shared__ double red[2][kMomLanes][kMomCols];
  const int lc = threadIdx.x % kMomCols, lane = threadIdx.x / kMomCols;
  const int64_t j = blockIdx.x * (int64_t)kMomCols + lc;
  const int64_t slab = blockIdx.y;
  const int64_t r0 = slab * slab_rows;
  int64_t r1 = r0 + slab_rows;
  if (r1 > rows) r1 = rows;
  double s1 = 0.0, s2 = 0.0;
  if (j < cols) {
    const double shift = (double)as_f32(x[j]);
    for (int64_t i = r0 + lane; i < r1; i += kMomLanes) {
      const double d = (double)as_f32(x[i * cols + j]) - shift;
      s1 += d;
      s2 += d * d;
    }
  }
  red[0][lane][lc] = s1;
  red[1][lane][lc] = s2;
  __syncthreads();
  if (lane == 0 && j < cols) {
    for (int l = 1; l < kMomLanes; ++l) {
      s1 += red[0][l][lc];
      s2 += red[1][l][lc];
    }
    partial[(slab * cols + j) * 2] = s1;
    partial[(slab * cols + j) * 2 + 1] = s2;
  }
}

template <class T>
__global__ void column_finish_kernel(const T* __restrict__ x, int64_t rows,
                                     int64_t cols, int64_t slabs,
                                     const double* __restrict__ partial,
                                     float* __restrict__ mean,
                                     float* __restrict__ var) {
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (j >= cols) return;
  double s1 = 0.0, s2 = 0.0;
  for (int64_t s = 0; s < slabs; ++s) {
    s1 += partial[(s * cols + j) * 2];
    s2 += partial[(s * cols + j) * 2 + 1];
  }
  const double n = (double)rows;
  const double shift = (double)as_f32(x[j]);
  if (mean) mean[j] = (float)(shift + s1 / n);
  if (var) {
    double v = (s2 - s1 * s1 / n) / n;
    var[j] = (float)(v < 0.0 ? 0.0 : v);
  }
}

template <class T>
__global__ void column_apply_kernel(const T* __restrict__ x, int64_t total,
                                    int64_t cols, int op,
                                    const float* __restrict__ v,
                                    float* __restrict__ out) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const float a = as_f32(x[e]);
    const float b = v[e % cols];
    out[e] = op == VTC_COLUMN_SUBTRACT ? sub_rn(a, b)
                                       : __fdiv_rn(a, __fsqrt_rn(b));
  }
}

// One wave per row: float64 sum in a fixed order (lane-strided, then the
// butterfly), the float32 mean, then x - mean in float32.
template <class T>
__global__ void __launch_bounds__(kThreads)
row_center_kernel(const T* __restrict__ x, int64_t rows, int64_t cols,
                  float* __restrict__ out, float* __restrict__ row_means) {
  const int64_t i = blockIdx.x * (int64_t)(kThreads / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  if (i >= rows) return;
  const T* xr = x + i * cols;
  double s = 0.0;
  for (int64_t j = lane; j < cols; j += 64) s += (double)as_f32(xr[j]);
  s = wave_sum(s);
  const float m = (float)(s / (double)cols);
  if (lane == 0 && row_means) row_means[i] = m;
  float* orow = out + i * cols;
  for (int64_t j = lane; j < cols; j += 64) orow[j] = sub_rn(as_f32(xr[j]), m);
}

// Scratch of the separable route of vtc_local_normalize: one float64 plane
// per image channel (the row pass), size published without padding
struct LocalNormLayout {
  double* rows_pass;
  LocalNormLayout(Carver& ws, int64_t count, int32_t h, int32_t w, int32_t c) {
    rows_pass = ws.take_unpadded<double>((size_t)count * h * w * c);
  }
};

// Scratch of vtc_column_moments: per slab and column the partial sum and sum
// of squares, size published without padding
struct MomentsLayout {
  double* partial;
  MomentsLayout(Carver& ws, int64_t rows, int64_t cols) {
    partial = ws.take_unpadded<double>((size_t)moment_slabs(rows, cols) *
                                       cols * 2);
  }
};

}  // namespace

}  // namespace vtc

using namespace vtc;

extern "C" size_t vtc_local_normalize_workspace_bytes(int64_t count,
                                                      int32_t h, int32_t w,
                                                      int32_t c,
                                                      double filter_sigma) {
  int lower = 0;
  const int n = gaussian_tap_count(filter_sigma, &lower);
  if (n <= 0 || count <= 0 || h <= 0 || w <= 0 || c <= 0) return 0;
  if (-lower <= kTileRadius) return 0;
  return measured_bytes<LocalNormLayout>(count, h, w, c);
}

extern "C" int vtc_local_normalize(const float* images, float* out, float* aux,
                                   int64_t count, int32_t h, int32_t w,
                                   int32_t c, double filter_sigma, int mode,
                                   void* workspace, size_t workspace_bytes,
                                   void* stream) {
  const char* who = "vtc_local_normalize";
  VTC_REQUIRE(images && out && aux, "%s: null pointer", who);
  VTC_REQUIRE(count > 0 && h > 0 && w > 0 && c > 0, "%s: bad shape", who);
  VTC_REQUIRE(mode == VTC_LOCAL_LUMINANCE || mode == VTC_LOCAL_CONTRAST,
              "%s: unknown mode %d", who, mode);
  VTC_REQUIRE(out != aux && images != aux,
              "%s: aux must not alias the images or the output", who);
  Taps taps;
  int rc = make_taps(filter_sigma, &taps, who);
  if (rc != VTC_OK) return rc;
  const int64_t total = count * (int64_t)h * w * c;
  const size_t need = vtc_local_normalize_workspace_bytes(count, h, w, c,
                                                          filter_sigma);
  if (need > 0 && (!workspace || workspace_bytes < need)) {
    set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
              need);
    return VTC_ERR_WORKSPACE;
  }
  VTC_REQUIRE(images != out, "%s: out must not alias the images", who);
  if (need == 0) {
    const int64_t tiles_y = ceil_div(h, kTileH), tiles_x = ceil_div(w, kTileW);
    const int64_t blocks = count * c * tiles_y * tiles_x;
    VTC_REQUIRE(blocks < (int64_t)1 << 31, "%s: stack too large", who);
    hipLaunchKernelGGL(local_norm_tile_kernel, dim3((unsigned)blocks),
                       dim3(kThreads), tile_lds_bytes(taps.radius),
                       as_stream(stream), images, out, aux, h, w, c,
                       (int)tiles_y, (int)tiles_x, mode, taps);
    VTC_LAUNCH_CHECK();
    return VTC_OK;
  }
  Carver carve(workspace);
  double* ws = LocalNormLayout(carve, count, h, w, c).rows_pass;
  hipLaunchKernelGGL(local_norm_rows_kernel, dim3(grid_for(total)), dim3(256),
                     0, as_stream(stream), images, ws, total, w, c, mode,
                     taps);
  VTC_LAUNCH_CHECK();
  hipLaunchKernelGGL(local_norm_cols_kernel, dim3(grid_for(total)), dim3(256),
                     0, as_stream(stream), images, ws, out, aux, total, h, w,
                     c, mode, taps);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" size_t vtc_column_moments_workspace_bytes(int64_t rows,
                                                     int64_t cols) {
  if (rows <= 0 || cols <= 0) return 0;
  return measured_bytes<MomentsLayout>(rows, cols);
}

extern "C" int vtc_column_moments(const void* x, int dtype, int64_t rows,
                                  int64_t cols, float* mean, float* var,
                                  void* workspace, size_t workspace_bytes,
                                  void* stream) {
  const char* who = "vtc_column_moments";
  VTC_REQUIRE(x && (mean || var) && workspace, "%s: null pointer", who);
  VTC_REQUIRE(rows > 0 && cols > 0, "%s: bad shape", who);
  VTC_REQUIRE(dtype == VTC_DTYPE_F32 || dtype == VTC_DTYPE_U8,
              "%s: unknown dtype %d", who, dtype);
  const size_t need = vtc_column_moments_workspace_bytes(rows, cols);
  if (workspace_bytes < need) {
    set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
              need);
    return VTC_ERR_WORKSPACE;
  }
  const int64_t slabs = moment_slabs(rows, cols);
  const int64_t slab_rows = ceil_div(rows, slabs);
  const dim3 grid((unsigned)ceil_div(cols, kMomCols), (unsigned)slabs);
  Carver carve(workspace);
  double* partial = MomentsLayout(carve, rows, cols).partial;
  const unsigned fin = (unsigned)ceil_div(cols, 256);
  if (dtype == VTC_DTYPE_F32) {
    const float* p = static_cast<const float*>(x);
    hipLaunchKernelGGL(column_partials_kernel<float>, grid, dim3(kThreads), 0,
                       as_stream(stream), p, rows, cols, slab_rows, partial);
    VTC_LAUNCH_CHECK();
    hipLaunchKernelGGL(column_finish_kernel<float>, dim3(fin), dim3(256), 0,
                       as_stream(stream), p, rows, cols, slabs, partial, mean,
                       var);
  } else {
    const uint8_t* p = static_cast<const uint8_t*>(x);
    hipLaunchKernelGGL(column_partials_kernel<uint8_t>, grid, dim3(kThreads),
                       0, as_stream(stream), p, rows, cols, slab_rows,
                       partial);
    VTC_LAUNCH_CHECK();
    hipLaunchKernelGGL(column_finish_kernel<uint8_t>, dim3(fin), dim3(256), 0,
                       as_stream(stream), p, rows, cols, slabs, partial, mean,
                       var);
  }
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" int vtc_column_apply(const void* x, int dtype, int64_t rows,
                                int64_t cols, int op, const float* v,
                                float* out, void* stream) {
  const char* who = "vtc_column_apply";
  VTC_REQUIRE(x && v && out, "%s: null pointer", who);
  VTC_REQUIRE(rows > 0 && cols > 0, "%s: bad shape", who);
  VTC_REQUIRE(dtype == VTC_DTYPE_F32 || dtype == VTC_DTYPE_U8,
              "%s: unknown dtype %d", who, dtype);
  VTC_REQUIRE(op == VTC_COLUMN_SUBTRACT || op == VTC_COLUMN_DIVIDE_SQRT,
              "%s: unknown op %d", who, op);
  const int64_t total = rows * cols;
  if (dtype == VTC_DTYPE_F32)
    hipLaunchKernelGGL(column_apply_kernel<float>, dim3(grid_for(total)),
                       dim3(256), 0, as_stream(stream),
                       static_cast<const float*>(x), total, cols, op, v, out);
  else
    hipLaunchKernelGGL(column_apply_kernel<uint8_t>, dim3(grid_for(total)),
                       dim3(256), 0, as_stream(stream),
                       static_cast<const uint8_t*>(x), total, cols, op, v,
                       out);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" int vtc_row_center(const void* x, int dtype, int64_t rows,
                              int64_t cols, float* out, float* row_means,
                              void* stream) {
  const char* who = "vtc_row_center";
  VTC_REQUIRE(x && out, "%s: null pointer", who);
  VTC_REQUIRE(rows > 0 && cols > 0, "%s: bad shape", who);
  VTC_REQUIRE(dtype == VTC_DTYPE_F32 || dtype == VTC_DTYPE_U8,
              "%s: unknown dtype %d", who, dtype);
  const int64_t blocks = ceil_div(rows, kThreads / 64);
  VTC_REQUIRE(blocks < (int64_t)1 << 31, "%s: too many rows", who);
  if (dtype == VTC_DTYPE_F32)
    hipLaunchKernelGGL(row_center_kernel<float>, dim3((unsigned)blocks),
                       dim3(kThreads), 0, as_stream(stream),
                       static_cast<const float*>(x), rows, cols, out,
                       row_means);
  else
    hipLaunchKernelGGL(row_center_kernel<uint8_t>, dim3((unsigned)blocks),
                       dim3(kThreads), 0, as_stream(stream),
                       static_cast<const uint8_t*>(x), rows, cols, out,
                       row_means);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}
