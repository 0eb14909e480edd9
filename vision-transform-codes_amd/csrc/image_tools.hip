// The image-level half of utils/image_processing.py (include/vtc_image.h):
// a caller's own filter in the frequency or the spatial domain, tiling an
// image into patches and back, and downsampling.
//
// Restates
//   utils/image_processing.py:18-60    filter_sd
//   utils/image_processing.py:63-92    filter_fd
//   utils/image_processing.py:95-114   downsample
//   utils/image_processing.py:597-648  patches_from_single_image
//   utils/image_processing.py:651-699  assemble_image_from_patches
//
// Both filters accumulate in float64 and round once to float32, as the
// reference does through numpy and scipy.
#include "common.h"
#include "fft_plans.h"
#include "sep_filter.h"

#include "../../include/vtc_image.h"

namespace vtc {

namespace {

constexpr int kMaxTaps = 63;          // per axis, both routes of filter_sd
constexpr int kSdTileH = 16;          // output tile of one workgroup
constexpr int kSdTileW = 64;
constexpr int kThreads = 256;
constexpr int kSdRows = kSdTileH / (kThreads / kSdTileW);   // per thread

unsigned grid_for(int64_t total) {
  int64_t blocks = ceil_div(total, kThreads);
  if (blocks > 65536) blocks = 65536;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

// ---- filter_fd -------------------------------------------------------------
// (count, h, w, c) channel-last -> (count*c, fh, fw) float64 planes, zeros
// beyond (h, w)
template <class T>
__global__ void fd_planes_kernel(const T* __restrict__ in,
                                 double* __restrict__ planes, int64_t count,
                                 int h, int w, int c, int fh, int fw) {
  const int64_t total = count * c * fh * fw;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % fw);
    const int y = (int)((i / fw) % fh);
    const int ch = (int)((i / ((int64_t)fw * fh)) % c);
    const int64_t img = i / ((int64_t)fw * fh * c);
    planes[i] = (y < h && x < w)
                    ? (double)in[((img * h + y) * w + x) * c + ch]
                    : 0.0;
  }
}

// spec (planes, fh, fw/2+1) *= Fh / (fh fw), Fh[k] = (F[k] + conj(F[-k])) / 2:
// the part of the filter that survives taking the real part of the inverse
// transform of a real image's spectrum.  1 / (fh fw) is the scale of the
// unnormalised inverse transform.
__global__ void fd_multiply_kernel(hipfftDoubleComplex* __restrict__ spec,
                                   const double* __restrict__ filter,
                                   int64_t planes, int fh, int fw) {
  const int wh = fw / 2 + 1;
  const int64_t total = planes * fh * wh;
  const double norm = 0.5 / ((double)fh * (double)fw);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int kx = (int)(i % wh);
    const int ky = (int)((i / wh) % fh);
    const int my = ky == 0 ? 0 : fh - ky, mx = kx == 0 ? 0 : fw - kx;
    const double* f = filter + 2 * ((int64_t)ky * fw + kx);
    const double* m = filter + 2 * ((int64_t)my * fw + mx);
    const double re = (f[0] + m[0]) * norm, im = (f[1] - m[1]) * norm;
    const double sx = spec[i].x, sy = spec[i].y;
    spec[i].x = sx * re - sy * im;
    spec[i].y = sx * im + sy * re;
  }
}

// (count*c, fh, fw) float64 planes -> the leading (h, w) of each, float32
// channel-last
__global__ void fd_crop_kernel(const double* __restrict__ planes,
                               float* __restrict__ out, int64_t count, int h,
                               int w, int c, int fh, int fw) {
  const int64_t total = count * h * w * c;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int ch = (int)(e % c);
    const int x = (int)((e / c) % w);
    const int y = (int)((e / ((int64_t)c * w)) % h);
    const int64_t img = e / ((int64_t)c * w * h);
    out[e] = (float)planes[((img * c + ch) * fh + y) * (int64_t)fw + x];
  }
}

// Scratch of vtc_img_filter_fd: the padded float64 planes and their half
// spectra.
struct FilterFdLayout {
  double* real;
  hipfftDoubleComplex* spec;
  FilterFdLayout(Carver& ws, int64_t planes, int32_t fh, int32_t fw) {
    real = ws.take<double>((size_t)planes * fh * fw);
    spec = ws.take<hipfftDoubleComplex>((size_t)planes * fh * (fw / 2 + 1));
  }
};

// ---- filter_sd, general 2D filter ----------------------------------------------
// One workgroup: a kSdTileH x kSdTileW output tile of one (image, channel)
// plane.  LDS holds the filter, reversed in both axes (a convolution is a
// correlation with the reversed filter), and the input tile with its halo,
// the reflection folded at load time.  Each thread owns kSdRows consecutive
// rows of one column; every sum runs over the reversed filter in row-major
// order.
template <class T>
__global__ void __launch_bounds__(kThreads)
filter_sd_tile_kernel(const T* __restrict__ x,
                      const double* __restrict__ filter,
                      float* __restrict__ out, int h, int w, int c, int fh,
                      int fw, int tiles_y, int tiles_x) {
  extern __shared__ double sd_lds[];
  double* filt = sd_lds;                                   // fh x fw
  float* tile = reinterpret_cast<float*>(sd_lds + fh * fw);  // in_h x in_w
  const int in_h = kSdTileH + fh - 1, in_w = kSdTileW + fw - 1;
  const int lead_y = fh / 2, lead_x = fw / 2;   // = f - 1 - (f - 1) / 2

  int64_t t = blockIdx.x;
  const int tx = (int)(t % tiles_x);
  t /= tiles_x;
  const int ty = (int)(t % tiles_y);
  t /= tiles_y;
  const int ch = (int)(t % c);
  const int64_t img = t / c;
  const int y0 = ty * kSdTileH, x0 = tx * kSdTileW;
  const int64_t plane = img * (int64_t)h * w;

  for (int i = threadIdx.x; i < fh * fw; i += kThreads)
    filt[i] = filter[fh * fw - 1 - i];
  for (int i = threadIdx.x; i < in_h * in_w; i += kThreads) {
    const int yy = i / in_w, xx = i - yy * in_w;
    const int gy = fold(y0 + yy - lead_y, h), gx = fold(x0 + xx - lead_x, w);
    tile[i] = (float)x[(plane + (int64_t)gy * w + gx) * c + ch];
  }
  __syncthreads();
  const int xx = threadIdx.x % kSdTileW;
  const int row0 = (threadIdx.x / kSdTileW) * kSdRows;
  const int ox = x0 + xx;
  if (ox >= w) return;
  double acc[kSdRows] = {};
  for (int a = 0; a < fh; ++a) {
    const float* in = tile + (row0 + a) * in_w + xx;
    const double* g = filt + a * fw;
    for (int b = 0; b < fw; ++b) {
      const double gv = g[b];
#pragma unroll
      for (int j = 0; j < kSdRows; ++j)
        acc[j] += (double)in[j * in_w + b] * gv;
    }
  }
#pragma unroll
  for (int j = 0; j < kSdRows; ++j) {
    const int oy = y0 + row0 + j;
    if (oy >= h) break;
    out[(plane + (int64_t)oy * w + ox) * c + ch] = (float)acc[j];
  }
}

size_t sd_tile_lds_bytes(int fh, int fw) {
  return (size_t)fh * fw * sizeof(double) +
         (size_t)(kSdTileH + fh - 1) * (kSdTileW + fw - 1) * sizeof(float);
}

// ---- filter_sd, separable route ------------------------------------------------
// scipy.ndimage.convolve1d stores its result in the input's element type:
// float32 rounded to nearest, uint8 by C conversion (toward zero, modulo 256).
template <class T>
__device__ __forceinline__ float stored_as(double v);
template <>
__device__ __forceinline__ float stored_as<float>(double v) {
  return (float)v;
}
template <>
__device__ __forceinline__ float stored_as<uint8_t>(double v) {
  return (float)(uint8_t)(long long)v;
}

// horizontal pass: mid = convolve1d(x, horz) along w, in x's element type
template <class T>
__global__ void sd_rows_kernel(const T* __restrict__ x,
                               const double* __restrict__ horz,
                               float* __restrict__ mid, int64_t total, int w,
                               int c, int fw) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int ch = (int)(e % c);
    const int64_t pix = e / c;
    const int px = (int)(pix % w);
    const int64_t row = pix - px;
    mid[e] = stored_as<T>(tap_sum(
        [&](int k) { return horz[fw - 1 - k]; }, fw, (fw - 1) / 2, px, w,
        [&](int gx) { return (double)x[(row + gx) * c + ch]; }));
  }
}

// vertical pass on the stored intermediate
__global__ void sd_cols_kernel(const float* __restrict__ mid,
                               const double* __restrict__ vert,
                               float* __restrict__ out, int64_t total, int h,
                               int w, int c, int fh) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int ch = (int)(e % c);
    const int64_t pix = e / c;
    const int px = (int)(pix % w);
    const int64_t prow = pix / w;
    const int py = (int)(prow % h);
    const int64_t plane = prow - py;
    out[e] = (float)tap_sum(
        [&](int k) { return vert[fh - 1 - k]; }, fh, (fh - 1) / 2, py, h,
        [&](int gy) {
          return (double)mid[((plane + gy) * w + px) * c + ch];
        });
  }
}

// Scratch of the separable route of vtc_img_filter_sd: the horizontal pass,
// size published without padding
struct FilterSdLayout {
  float* mid;
  FilterSdLayout(Carver& ws, int64_t count, int32_t h, int32_t w, int32_t c) {
    mid = ws.take_unpadded<float>((size_t)count * h * w * c);
  }
};

// ---- moves ---------------------------------------------------------------------
// patches[n, p, dy, dx, ch] = images[n, (p / nx) ph + dy, (p % nx) pw + dx, ch]
template <class T>
__global__ void tile_patches_kernel(const T* __restrict__ images,
                                    T* __restrict__ patches, int64_t total,
                                    int h, int w, int c, int ph, int pw,
                                    int ny, int nx) {
  const int row_len = pw * c;
  const int n = ph * row_len;
  const int64_t per_image = (int64_t)ny * nx * n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t img = i / per_image;
    const int64_t r = i - img * per_image;
    const int p = (int)(r / n), e = (int)(r % n);
    const int dy = e / row_len, rest = e % row_len;
    const int y = (p / nx) * ph + dy;
    const int64_t x_c = (int64_t)(p % nx) * row_len + rest;
    patches[i] = images[(img * h + y) * (int64_t)w * c + x_c];
  }
}

__device__ __forceinline__ bool patch_inside(int vert, int horz, int ph,
                                             int pw, int out_h, int out_w) {
  return vert >= 0 && horz >= 0 && vert <= out_h - ph && horz <= out_w - pw;
}

// disjoint positions: every patch element has a destination of its own
template <class T>
__global__ void assemble_scatter_kernel(const T* __restrict__ patches,
                                        const int32_t* __restrict__ positions,
                                        T* __restrict__ image, int64_t total,
                                        int ph, int pw, int c, int out_h,
                                        int out_w) {
  const int row_len = pw * c;
  const int n = ph * row_len;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = i / n;
    const int e = (int)(i % n);
    const int vert = positions[2 * p], horz = positions[2 * p + 1];
    if (!patch_inside(vert, horz, ph, pw, out_h, out_w)) continue;
    const int dy = e / row_len, rest = e % row_len;
    image[((int64_t)(vert + dy) * out_w + horz) * c + rest] = patches[i];
  }
}

// any positions: each image element takes the last patch that covers it
template <class T>
__global__ void assemble_ordered_kernel(const T* __restrict__ patches,
                                        const int32_t* __restrict__ positions,
                                        T* __restrict__ image, int64_t k,
                                        int ph, int pw, int c, int out_h,
                                        int out_w) {
  const int64_t total = (int64_t)out_h * out_w * c;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int ch = (int)(e % c);
    const int x = (int)((e / c) % out_w);
    const int y = (int)(e / ((int64_t)c * out_w));
    T v = 0;
    for (int64_t p = k - 1; p >= 0; --p) {
      const int vert = positions[2 * p], horz = positions[2 * p + 1];
      if (y < vert || y >= vert + ph || x < horz || x >= horz + pw ||
          !patch_inside(vert, horz, ph, pw, out_h, out_w))
        continue;
      v = patches[((p * ph + (y - vert)) * pw + (x - horz)) * c + ch];
      break;
    }
    image[e] = v;
  }
}

// out[n, y, x, ch] = images[n, y f, x f, ch]
template <class T>
__global__ void downsample_kernel(const T* __restrict__ images,
                                  T* __restrict__ out, int64_t total, int h,
                                  int w, int c, int oh, int ow, int f) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int ch = (int)(e % c);
    const int x = (int)((e / c) % ow);
    const int y = (int)((e / ((int64_t)c * ow)) % oh);
    const int64_t img = e / ((int64_t)c * ow * oh);
    out[e] = images[((img * h + (int64_t)y * f) * w + (int64_t)x * f) * c + ch];
  }
}

bool known_dtype(int dtype) {
  return dtype == VTC_DTYPE_F32 || dtype == VTC_DTYPE_U8;
}

// the size rule of both routes of vtc_img_filter_sd, after the shape checks
int filter_sd_supported(const char* who, int32_t h, int32_t w, int32_t fh,
                        int32_t fw) {
  if (fh > kMaxTaps || fw > kMaxTaps || fh > h || fw > w) {
    set_error("%s: a %d x %d filter on a %d x %d image (at most %d taps per "
              "axis and no larger than the image)", who, fh, fw, h, w,
              kMaxTaps);
    return VTC_ERR_UNSUPPORTED;
  }
  return VTC_OK;
}

template <class T>
int launch_filter_sd_tile(const T* x, const double* filter, float* out,
                          int64_t count, int h, int w, int c, int fh, int fw,
                          hipStream_t st) {
  const int64_t tiles_y = ceil_div(h, kSdTileH), tiles_x = ceil_div(w, kSdTileW);
  const int64_t blocks = count * c * tiles_y * tiles_x;
  VTC_REQUIRE(blocks < (int64_t)1 << 31, "vtc_img_filter_sd: stack too large");
  auto kernel = filter_sd_tile_kernel<T>;
  const size_t lds = sd_tile_lds_bytes(fh, fw);
  static unsigned long long configured = 0;
  if (lds > 64 * 1024 && first_use_on_this_device(&configured)) {
    VTC_HIP_CHECK(hipFuncSetAttribute(
        reinterpret_cast<const void*>(kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize,
        (int)sd_tile_lds_bytes(kMaxTaps, kMaxTaps)));
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kThreads), lds, st,
                     x, filter, out, h, w, c, fh, fw, (int)tiles_y,
                     (int)tiles_x);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

template <class T>
int launch_filter_sd_separable(const T* x, const double* vert,
                               const double* horz, float* mid, float* out,
                               int64_t total, int h, int w, int c, int fh,
                               int fw, hipStream_t st) {
  hipLaunchKernelGGL(sd_rows_kernel<T>, dim3(grid_for(total)), dim3(kThreads),
                     0, st, x, horz, mid, total, w, c, fw);
  VTC_LAUNCH_CHECK();
  hipLaunchKernelGGL(sd_cols_kernel, dim3(grid_for(total)), dim3(kThreads), 0,
                     st, mid, vert, out, total, h, w, c, fh);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

template <class T>
int launch_assemble(const T* patches, const int32_t* positions, T* image,
                    int64_t k, int ph, int pw, int c, int out_h, int out_w,
                    bool disjoint, hipStream_t st) {
  const int64_t image_elems = (int64_t)out_h * out_w * c;
  if (disjoint) {
    VTC_HIP_CHECK(hipMemsetAsync(image, 0, (size_t)image_elems * sizeof(T),
                                 st));
    const int64_t total = k * ph * pw * c;
    hipLaunchKernelGGL(assemble_scatter_kernel<T>, dim3(grid_for(total)),
                       dim3(kThreads), 0, st, patches, positions, image, total,
                       ph, pw, c, out_h, out_w);
  } else {
    hipLaunchKernelGGL(assemble_ordered_kernel<T>,
                       dim3(grid_for(image_elems)), dim3(kThreads), 0, st,
                       patches, positions, image, k, ph, pw, c, out_h, out_w);
  }
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

}  // namespace

}  // namespace vtc

using namespace vtc;

extern "C" int vtc_image_abi_version(void) { return VTC_IMAGE_ABI_VERSION; }

extern "C" size_t vtc_img_filter_fd_workspace_bytes(int64_t count, int32_t h,
                                                    int32_t w, int32_t c,
                                                    int32_t fh, int32_t fw) {
  if (count <= 0 || h <= 0 || w <= 0 || c <= 0 || fh < h || fw < w) return 0;
  return measured_bytes<FilterFdLayout>(count * c, fh, fw);
}

extern "C" int vtc_img_filter_fd(const void* images, int dtype,
                                 const double* filter_dft, float* out,
                                 int64_t count, int32_t h, int32_t w,
                                 int32_t c, int32_t fh, int32_t fw,
                                 void* workspace, size_t workspace_bytes,
                                 void* stream) {
  const char* who = "vtc_img_filter_fd";
  VTC_REQUIRE(images && filter_dft && out, "%s: null pointer", who);
  VTC_REQUIRE(count > 0 && h > 0 && w > 0 && c > 0, "%s: bad shape", who);
  VTC_REQUIRE(known_dtype(dtype), "%s: unknown dtype %d", who, dtype);
  VTC_REQUIRE(fh >= h && fw >= w,
              "%s: a %d x %d filter undersamples the DFT of a %d x %d image",
              who, fh, fw, h, w);
  VTC_REQUIRE(images != (const void*)out, "%s: out must not alias the images",
              who);
  VTC_REQUIRE(count * c <= 0x7fffffffLL, "%s: too many planes", who);
  const size_t need = vtc_img_filter_fd_workspace_bytes(count, h, w, c, fh,
                                                        fw);
  if (!workspace || workspace_bytes < need) {
    set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
              need);
    return VTC_ERR_WORKSPACE;
  }
  const int64_t planes = count * c;
  hipStream_t st = as_stream(stream);
  FftPlans plans;
  int rc = get_plans(st, fh, fw, (int)planes, &plans);
  if (rc != VTC_OK) return rc;
  const FftApi& api = fft_api();
  Carver ws(workspace);
  const FilterFdLayout L(ws, planes, fh, fw);
  const unsigned grid = grid_for(planes * fh * fw);
  if (dtype == VTC_DTYPE_F32)
    hipLaunchKernelGGL(fd_planes_kernel<float>, dim3(grid), dim3(kThreads), 0,
                       st, static_cast<const float*>(images), L.real, count, h,
                       w, c, fh, fw);
  else
    hipLaunchKernelGGL(fd_planes_kernel<uint8_t>, dim3(grid), dim3(kThreads),
                       0, st, static_cast<const uint8_t*>(images), L.real,
                       count, h, w, c, fh, fw);
  VTC_LAUNCH_CHECK();
  if (api.exec_d2z(plans.forward, L.real, L.spec) != HIPFFT_SUCCESS) {
    set_error("%s: forward transform failed", who);
    return VTC_ERR_HIP;
  }
  hipLaunchKernelGGL(fd_multiply_kernel,
                     dim3(grid_for(planes * fh * (fw / 2 + 1))),
                     dim3(kThreads), 0, st, L.spec, filter_dft, planes, fh,
                     fw);
  VTC_LAUNCH_CHECK();
  if (api.exec_z2d(plans.inverse, L.spec, L.real) != HIPFFT_SUCCESS) {
    set_error("%s: inverse transform failed", who);
    return VTC_ERR_HIP;
  }
  hipLaunchKernelGGL(fd_crop_kernel, dim3(grid_for(count * h * w * c)),
                     dim3(kThreads), 0, st, L.real, out, count, h, w, c, fh,
                     fw);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" size_t vtc_img_filter_sd_workspace_bytes(int64_t count, int32_t h,
                                                    int32_t w, int32_t c,
                                                    int32_t fh, int32_t fw,
                                                    int separable) {
  if (!separable || count <= 0 || h <= 0 || w <= 0 || c <= 0 || fh <= 0 ||
      fw <= 0 || fh > kMaxTaps || fw > kMaxTaps || fh > h || fw > w)
    return 0;
  return measured_bytes<FilterSdLayout>(count, h, w, c);
}

extern "C" int vtc_img_filter_sd(const void* images, int dtype,
                                 const double* filter,
                                 const double* separable_vert,
                                 const double* separable_horz, float* out,
                                 int64_t count, int32_t h, int32_t w,
                                 int32_t c, int32_t fh, int32_t fw,
                                 void* workspace, size_t workspace_bytes,
                                 void* stream) {
  const char* who = "vtc_img_filter_sd";
  const bool separable = separable_vert || separable_horz;
  VTC_REQUIRE(images && out && (separable ? separable_vert && separable_horz
                                          : filter != nullptr),
              "%s: null pointer", who);
  VTC_REQUIRE(count > 0 && h > 0 && w > 0 && c > 0 && fh > 0 && fw > 0,
              "%s: bad shape", who);
  VTC_REQUIRE(known_dtype(dtype), "%s: unknown dtype %d", who, dtype);
  VTC_REQUIRE(images != (const void*)out, "%s: out must not alias the images",
              who);
  int rc = filter_sd_supported(who, h, w, fh, fw);
  if (rc != VTC_OK) return rc;
  hipStream_t st = as_stream(stream);
  if (!separable) {
    if (dtype == VTC_DTYPE_F32)
      return launch_filter_sd_tile(static_cast<const float*>(images), filter,
                                   out, count, h, w, c, fh, fw, st);
    return launch_filter_sd_tile(static_cast<const uint8_t*>(images), filter,
                                 out, count, h, w, c, fh, fw, st);
  }
  const size_t need = vtc_img_filter_sd_workspace_bytes(count, h, w, c, fh, fw,
                                                        1);
  if (!workspace || workspace_bytes < need) {
    set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
              need);
    return VTC_ERR_WORKSPACE;
  }
  Carver carve(workspace);
  float* mid = FilterSdLayout(carve, count, h, w, c).mid;
  const int64_t total = count * (int64_t)h * w * c;
  if (dtype == VTC_DTYPE_F32)
    return launch_filter_sd_separable(static_cast<const float*>(images),
                                      separable_vert, separable_horz, mid, out,
                                      total, h, w, c, fh, fw, st);
  return launch_filter_sd_separable(static_cast<const uint8_t*>(images),
                                    separable_vert, separable_horz, mid, out,
                                    total, h, w, c, fh, fw, st);
}

extern "C" int vtc_img_tile_patches(const void* images, int dtype,
                                    void* patches, int64_t count, int32_t h,
                                    int32_t w, int32_t c, int32_t ph,
                                    int32_t pw, void* stream) {
  const char* who = "vtc_img_tile_patches";
  VTC_REQUIRE(images && patches, "%s: null pointer", who);
  VTC_REQUIRE(count > 0 && h > 0 && w > 0 && c > 0 && ph > 0 && pw > 0 &&
                  ph <= h && pw <= w, "%s: bad sizes", who);
  VTC_REQUIRE(known_dtype(dtype), "%s: unknown dtype %d", who, dtype);
  const int ny = h / ph, nx = w / pw;
  const int64_t total = count * ny * nx * ph * pw * c;
  hipStream_t st = as_stream(stream);
  if (dtype == VTC_DTYPE_F32)
    hipLaunchKernelGGL(tile_patches_kernel<float>, dim3(grid_for(total)),
                       dim3(kThreads), 0, st,
                       static_cast<const float*>(images),
                       static_cast<float*>(patches), total, h, w, c, ph, pw,
                       ny, nx);
  else
    hipLaunchKernelGGL(tile_patches_kernel<uint8_t>, dim3(grid_for(total)),
                       dim3(kThreads), 0, st,
                       static_cast<const uint8_t*>(images),
                       static_cast<uint8_t*>(patches), total, h, w, c, ph, pw,
                       ny, nx);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" int vtc_img_assemble_patches(const void* patches, int dtype,
                                        const int32_t* positions, void* image,
                                        int64_t k, int32_t ph, int32_t pw,
                                        int32_t c, int32_t out_h,
                                        int32_t out_w, int positions_disjoint,
                                        void* stream) {
  const char* who = "vtc_img_assemble_patches";
  VTC_REQUIRE(patches && positions && image, "%s: null pointer", who);
  VTC_REQUIRE(k > 0 && ph > 0 && pw > 0 && c > 0 && out_h >= ph &&
                  out_w >= pw, "%s: bad sizes", who);
  VTC_REQUIRE(known_dtype(dtype), "%s: unknown dtype %d", who, dtype);
  hipStream_t st = as_stream(stream);
  if (dtype == VTC_DTYPE_F32)
    return launch_assemble(static_cast<const float*>(patches), positions,
                           static_cast<float*>(image), k, ph, pw, c, out_h,
                           out_w, positions_disjoint != 0, st);
  return launch_assemble(static_cast<const uint8_t*>(patches), positions,
                         static_cast<uint8_t*>(image), k, ph, pw, c, out_h,
                         out_w, positions_disjoint != 0, st);
}

extern "C" int vtc_img_downsample(const void* images, int dtype, void* out,
                                  int64_t count, int32_t h, int32_t w,
                                  int32_t c, int32_t factor, void* stream) {
  const char* who = "vtc_img_downsample";
  VTC_REQUIRE(images && out, "%s: null pointer", who);
  VTC_REQUIRE(count > 0 && h > 0 && w > 0 && c > 0 && factor > 0,
              "%s: bad sizes", who);
  VTC_REQUIRE(known_dtype(dtype), "%s: unknown dtype %d", who, dtype);
  const int oh = (int)ceil_div(h, factor), ow = (int)ceil_div(w, factor);
  const int64_t total = count * oh * ow * c;
  hipStream_t st = as_stream(stream);
  if (dtype == VTC_DTYPE_F32)
    hipLaunchKernelGGL(downsample_kernel<float>, dim3(grid_for(total)),
                       dim3(kThreads), 0, st,
                       static_cast<const float*>(images),
                       static_cast<float*>(out), total, h, w, c, oh, ow,
                       factor);
  else
    hipLaunchKernelGGL(downsample_kernel<uint8_t>, dim3(grid_for(total)),
                       dim3(kThreads), 0, st,
                       static_cast<const uint8_t*>(images),
                       static_cast<uint8_t*>(out), total, h, w, c, oh, ow,
                       factor);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}
