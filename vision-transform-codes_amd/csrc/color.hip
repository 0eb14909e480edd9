// The colour step of an image-level rate-distortion point
// (include/ext/vtc_color.h): a 3 x 3 affine map per pixel between channel-last
// and planar stacks, the box mean that takes a chroma plane to reduced
// resolution and the replicate / triangle filters that bring it back.
//
// The reference has no colour path to restate.  The header fixes the order of
// every operation instead: float64 operations rounded one by one (the
// Makefile's -ffp-contract=off keeps hipcc from fusing them), one rounding to
// float32 at the store, every output element computed by one thread from the
// inputs alone.  tests/color_data.py restates the same order in numpy and the
// GPU tests compare bit patterns.
//
// All three kernels are pure streaming: no LDS, no atomics, no workspace.
// Index arithmetic is int64, the loops are grid-stride under a capped grid.
#include <stdlib.h>

#include "common.h"

#include "../../include/ext/vtc_color.h"

namespace vtc {

namespace {

constexpr int kThreads = 256;
// a memory-bound grid: 8 blocks per compute unit, the rest by grid stride
constexpr int64_t kMaxBlocks = 2048;
constexpr int64_t kMaxPlane = 0x7fffffffLL;   // h * w

// VTC_COLOR_MAX_BLOCKS=<n> lowers the cap (1 .. 2048) so that a small array
// already turns the grid-stride loops over; read at every call, tests only.
unsigned grid_for(int64_t items) {
  int64_t cap = kMaxBlocks;
  if (const char* v = getenv("VTC_COLOR_MAX_BLOCKS")) {
    const long forced = atol(v);
    if (forced >= 1 && forced < cap) cap = forced;
  }
  int64_t blocks = ceil_div(items, kThreads);
  if (blocks > cap) blocks = cap;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

// The map of one call, a kernel argument: 17 doubles and a flag.
struct ColorMap {
  double m[9];
  double pre[3];
  double post[3];
  double lo, hi;
  int clamp;
};

// e = q * d + r, 0 <= r < d, d <= 2^31 - 1: a 32-bit division where e allows
__device__ __forceinline__ void div_mod(int64_t e, int64_t d, int64_t* q,
                                        int64_t* r) {
  if (e <= 0xffffffffLL) {
    const uint32_t quotient = (uint32_t)e / (uint32_t)d;
    *q = quotient;
    *r = (uint32_t)e - quotient * (uint32_t)d;
  } else {
    *q = e / d;
    *r = e - *q * d;
  }
}

// element index of channel 0 of pixel p and the stride between its channels
template <bool CHW>
__device__ __forceinline__ int64_t pixel_base(int64_t p, int64_t plane) {
  if (!CHW) return 3 * p;
  int64_t image, rest;
  div_mod(p, plane, &image, &rest);
  return image * 3 * plane + rest;
}

__device__ __forceinline__ void map_pixel(const ColorMap& k, const float* in,
                                          float* out) {
  const double t0 = (double)in[0] - k.pre[0];
  const double t1 = (double)in[1] - k.pre[1];
  const double t2 = (double)in[2] - k.pre[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double v = ((k.m[3 * i] * t0 + k.m[3 * i + 1] * t1) + k.m[3 * i + 2] * t2) +
               k.post[i];
    if (k.clamp) v = v < k.lo ? k.lo : (v > k.hi ? k.hi : v);   // NaN stays
    out[i] = (float)v;
  }
}

template <bool IN_CHW, bool OUT_CHW>
__device__ __forceinline__ void one_pixel(const ColorMap& k,
                                          const float* __restrict__ in,
                                          float* __restrict__ out, int64_t p,
                                          int64_t plane) {
  const int64_t from = pixel_base<IN_CHW>(p, plane);
  const int64_t to = pixel_base<OUT_CHW>(p, plane);
  const int64_t in_step = IN_CHW ? plane : 1, out_step = OUT_CHW ? plane : 1;
  const float x[3] = {in[from], in[from + in_step], in[from + 2 * in_step]};
  float y[3];
  map_pixel(k, x, y);
  out[to] = y[0];
  out[to + out_step] = y[1];
  out[to + 2 * out_step] = y[2];
}

// One pixel per lane, element by element: any element-aligned pointers.
template <bool IN_CHW, bool OUT_CHW>
__global__ void __launch_bounds__(kThreads)
color_pixel_kernel(const float* __restrict__ in, float* __restrict__ out,
                   int64_t pixels, int64_t plane, ColorMap k) {
  for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < pixels;
       p += (int64_t)gridDim.x * kThreads)
    one_pixel<IN_CHW, OUT_CHW>(k, in, out, p, plane);
}

// Four pixels per lane as three 16-byte loads and three 16-byte stores.  A
// channel-last group is 48 contiguous bytes; a planar group is 16 bytes of
// each plane (plane % 4 == 0, so a group never leaves its image).  Both bases
// are 16-byte aligned.  The pixels % 4 pixels behind the last group (only a
// channel-last pair can have them) go one per lane through one_pixel.
template <bool IN_CHW, bool OUT_CHW>
__global__ void __launch_bounds__(kThreads)
color_quad_kernel(const float* __restrict__ in, float* __restrict__ out,
                  int64_t pixels, int64_t plane, ColorMap k) {
  const int64_t groups = pixels >> 2;
  const int64_t items = groups + (pixels & 3);
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < items;
       e += (int64_t)gridDim.x * kThreads) {
    if (e >= groups) {
      one_pixel<IN_CHW, OUT_CHW>(k, in, out, 4 * groups + (e - groups), plane);
      continue;
    }
    const int64_t p = 4 * e;
    const int64_t from = pixel_base<IN_CHW>(p, plane);
    const int64_t to = pixel_base<OUT_CHW>(p, plane);
    const int64_t in_step = IN_CHW ? plane : 4, out_step = OUT_CHW ? plane : 4;
    float4 v[3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
      v[j] = *reinterpret_cast<const float4*>(in + from + j * in_step);
    const float f[12] = {v[0].x, v[0].y, v[0].z, v[0].w, v[1].x, v[1].y,
                         v[1].z, v[1].w, v[2].x, v[2].y, v[2].z, v[2].w};
    float g[12];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      // planar: f[4 j + q]; channel-last: f[3 q + j]
      const float x[3] = {IN_CHW ? f[q] : f[3 * q],
                          IN_CHW ? f[4 + q] : f[3 * q + 1],
                          IN_CHW ? f[8 + q] : f[3 * q + 2]};
      float y[3];
      map_pixel(k, x, y);
#pragma unroll
      for (int i = 0; i < 3; ++i) g[OUT_CHW ? 4 * i + q : 3 * q + i] = y[i];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
      *reinterpret_cast<float4*>(out + to + j * out_step) =
          make_float4(g[4 * j], g[4 * j + 1], g[4 * j + 2], g[4 * j + 3]);
  }
}

// out[n, Y, X] = mean of the pixels of box (Y, X) that exist
__global__ void __launch_bounds__(kThreads)
plane_downsample_kernel(const float* __restrict__ in, float* __restrict__ out,
                        int64_t total, int h, int w, int oh, int ow, int fv,
                        int fh) {
  const int64_t out_plane = (int64_t)oh * ow;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * kThreads) {
    int64_t image, rest;
    div_mod(e, out_plane, &image, &rest);
    const int Y = (int)((uint32_t)rest / (uint32_t)ow);
    const int X = (int)((uint32_t)rest - (uint32_t)Y * (uint32_t)ow);
    const int y0 = Y * fv, x0 = X * fh;
    const int y1 = min(h, y0 + fv), x1 = min(w, x0 + fh);
    const float* plane = in + image * h * w;
    double sum = 0.0;
    for (int y = y0; y < y1; ++y)
      for (int x = x0; x < x1; ++x) sum += (double)plane[(int64_t)y * w + x];
    out[e] = (float)(sum / (double)((y1 - y0) * (x1 - x0)));
  }
}

// the two taps of output index i and the weight of the second
struct Taps {
  int a, b;
  double t;
};
// 1 / f for f = 1, 2, 4: the product with it is the quotient by f, exactly
__device__ __forceinline__ double inverse_factor(int f) {
  return f == 1 ? 1.0 : (f == 2 ? 0.5 : 0.25);
}
__device__ __forceinline__ Taps triangle_taps(int i, double inverse_f, int n) {
  const double u = ((double)i + 0.5) * inverse_f - 0.5;
  const double lower = floor(u);
  const int i0 = (int)lower;
  Taps taps;
  taps.t = u - lower;
  taps.a = min(max(i0, 0), n - 1);
  taps.b = min(max(i0 + 1, 0), n - 1);
  return taps;
}

template <bool TRIANGLE>
__global__ void __launch_bounds__(kThreads)
plane_upsample_kernel(const float* __restrict__ in, float* __restrict__ out,
                      int64_t total, int h_in, int w_in, int h_out, int w_out,
                      int fv, int fh) {
  const int64_t out_plane = (int64_t)h_out * w_out;
  const int shift_v = fv >> 1, shift_h = fh >> 1;   // log2 of 1, 2, 4
  const double inverse_v = inverse_factor(fv), inverse_h = inverse_factor(fh);
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * kThreads) {
    int64_t image, rest;
    div_mod(e, out_plane, &image, &rest);
    const int y = (int)((uint32_t)rest / (uint32_t)w_out);
    const int x = (int)((uint32_t)rest - (uint32_t)y * (uint32_t)w_out);
    const float* plane = in + image * h_in * w_in;
    if (!TRIANGLE) {
      out[e] = plane[(int64_t)(y >> shift_v) * w_in + (x >> shift_h)];
      continue;
    }
    const Taps v = triangle_taps(y, inverse_v, h_in);
    const Taps u = triangle_taps(x, inverse_h, w_in);
    const float* top = plane + (int64_t)v.a * w_in;
    const float* bottom = plane + (int64_t)v.b * w_in;
    const double keep_h = 1.0 - u.t, keep_v = 1.0 - v.t;
    const double upper = keep_h * (double)top[u.a] + u.t * (double)top[u.b];
    const double lower =
        keep_h * (double)bottom[u.a] + u.t * (double)bottom[u.b];
    out[e] = (float)(keep_v * upper + v.t * lower);
  }
}

// ---- host side -----------------------------------------------------------
bool overlap(const void* a, const void* b, int64_t bytes_a, int64_t bytes_b) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a);
  const uintptr_t pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + (uintptr_t)bytes_b && pb < pa + (uintptr_t)bytes_a;
}

bool aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

// count, h, w >= 1, h * w <= 2^31 - 1, count * h * w * channels floats
// addressable; `hn` and `wn` are the arguments' names
int check_stack(const char* who, int64_t count, int32_t h, int32_t w,
                const char* hn, const char* wn, int channels) {
  VTC_REQUIRE(count >= 1, "%s: bad size count = %lld", who, (long long)count);
  VTC_REQUIRE(h >= 1, "%s: bad size %s = %d", who, hn, h);
  VTC_REQUIRE(w >= 1, "%s: bad size %s = %d", who, wn, w);
  const int64_t plane = (int64_t)h * w;
  if (plane > kMaxPlane) {
    set_error("%s: %s * %s = %lld, at most 2^31 - 1", who, hn, wn,
              (long long)plane);
    return VTC_ERR_UNSUPPORTED;
  }
  if (count > (INT64_MAX >> 3) / (plane * channels)) {
    set_error("%s: count = %lld planes of %lld pixels, too many elements",
              who, (long long)count, (long long)plane);
    return VTC_ERR_UNSUPPORTED;
  }
  return VTC_OK;
}

int check_factor(const char* who, const char* name, int32_t f) {
  if (f != 1 && f != 2 && f != 4) {
    set_error("%s: %s = %d, the factors are 1, 2 and 4", who, name, f);
    return VTC_ERR_UNSUPPORTED;
  }
  return VTC_OK;
}

int check_layout(const char* who, const char* name, int layout) {
  if (layout != VTC_COLOR_HWC && layout != VTC_COLOR_CHW) {
    set_error("%s: unknown %s = %d", who, name, layout);
    return VTC_ERR_UNSUPPORTED;
  }
  return VTC_OK;
}

template <bool IN_CHW, bool OUT_CHW>
void launch_color(const float* in, float* out, int64_t pixels, int64_t plane,
                  const ColorMap& k, hipStream_t st) {
  const bool wide = aligned16(in) && aligned16(out) &&
                    (!(IN_CHW || OUT_CHW) || plane % 4 == 0);
  if (wide) {
    const int64_t items = (pixels >> 2) + (pixels & 3);
    hipLaunchKernelGGL((color_quad_kernel<IN_CHW, OUT_CHW>),
                       dim3(grid_for(items)), dim3(kThreads), 0, st, in, out,
                       pixels, plane, k);
  } else {
    hipLaunchKernelGGL((color_pixel_kernel<IN_CHW, OUT_CHW>),
                       dim3(grid_for(pixels)), dim3(kThreads), 0, st, in, out,
                       pixels, plane, k);
  }
}

}  // namespace
}  // namespace vtc

using namespace vtc;

extern "C" int vtc_color_abi_version(void) { return VTC_COLOR_ABI_VERSION; }

extern "C" int vtc_color_transform(const float* in, int in_layout, float* out,
                                   int out_layout, int64_t count, int32_t h,
                                   int32_t w, const double* matrix,
                                   const double* pre, const double* post,
                                   int clamp, double lo, double hi,
                                   void* stream) {
  const char* who = "vtc_color_transform";
  VTC_REQUIRE(in, "%s: null pointer in", who);
  VTC_REQUIRE(out, "%s: null pointer out", who);
  VTC_REQUIRE(matrix, "%s: null pointer matrix", who);
  VTC_REQUIRE(pre, "%s: null pointer pre", who);
  VTC_REQUIRE(post, "%s: null pointer post", who);
  int rc = check_stack(who, count, h, w, "h", "w", 3);
  if (rc != VTC_OK) return rc;
  rc = check_layout(who, "in_layout", in_layout);
  if (rc != VTC_OK) return rc;
  rc = check_layout(who, "out_layout", out_layout);
  if (rc != VTC_OK) return rc;
  VTC_REQUIRE(!clamp || lo <= hi, "%s: clamp with lo = %g, hi = %g", who, lo,
              hi);
  const int64_t plane = (int64_t)h * w;
  const int64_t pixels = count * plane;
  VTC_REQUIRE(!overlap(in, out, 12 * pixels, 12 * pixels),
              "%s: out overlaps in", who);
  ColorMap k;
  for (int i = 0; i < 9; ++i) k.m[i] = matrix[i];
  for (int i = 0; i < 3; ++i) {
    k.pre[i] = pre[i];
    k.post[i] = post[i];
  }
  k.clamp = clamp != 0;
  k.lo = clamp ? lo : 0.0;
  k.hi = clamp ? hi : 0.0;
  hipStream_t st = as_stream(stream);
  const bool in_chw = in_layout == VTC_COLOR_CHW;
  const bool out_chw = out_layout == VTC_COLOR_CHW;
  if (in_chw && out_chw)
    launch_color<true, true>(in, out, pixels, plane, k, st);
  else if (in_chw)
    launch_color<true, false>(in, out, pixels, plane, k, st);
  else if (out_chw)
    launch_color<false, true>(in, out, pixels, plane, k, st);
  else
    launch_color<false, false>(in, out, pixels, plane, k, st);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" int vtc_plane_downsample(const float* in, float* out, int64_t count,
                                    int32_t h, int32_t w, int32_t fv,
                                    int32_t fh, void* stream) {
  const char* who = "vtc_plane_downsample";
  VTC_REQUIRE(in, "%s: null pointer in", who);
  VTC_REQUIRE(out, "%s: null pointer out", who);
  int rc = check_stack(who, count, h, w, "h", "w", 1);
  if (rc != VTC_OK) return rc;
  rc = check_factor(who, "fv", fv);
  if (rc != VTC_OK) return rc;
  rc = check_factor(who, "fh", fh);
  if (rc != VTC_OK) return rc;
  const int oh = (int)ceil_div(h, fv), ow = (int)ceil_div(w, fh);
  const int64_t total = count * oh * ow;
  VTC_REQUIRE(!overlap(in, out, 4 * count * h * w, 4 * total),
              "%s: out overlaps in", who);
  hipLaunchKernelGGL(plane_downsample_kernel, dim3(grid_for(total)),
                     dim3(kThreads), 0, as_stream(stream), in, out, total, h,
                     w, oh, ow, fv, fh);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" int vtc_plane_upsample(const float* in, float* out, int64_t count,
                                  int32_t h_in, int32_t w_in, int32_t h_out,
                                  int32_t w_out, int32_t fv, int32_t fh,
                                  int mode, void* stream) {
  const char* who = "vtc_plane_upsample";
  VTC_REQUIRE(in, "%s: null pointer in", who);
  VTC_REQUIRE(out, "%s: null pointer out", who);
  VTC_REQUIRE(h_in >= 1, "%s: bad size h_in = %d", who, h_in);
  VTC_REQUIRE(w_in >= 1, "%s: bad size w_in = %d", who, w_in);
  int rc = check_stack(who, count, h_out, w_out, "h_out", "w_out", 1);
  if (rc != VTC_OK) return rc;
  rc = check_factor(who, "fv", fv);
  if (rc != VTC_OK) return rc;
  rc = check_factor(who, "fh", fh);
  if (rc != VTC_OK) return rc;
  if (mode != VTC_UPSAMPLE_REPLICATE && mode != VTC_UPSAMPLE_TRIANGLE) {
    set_error("%s: unknown mode = %d", who, mode);
    return VTC_ERR_UNSUPPORTED;
  }
  VTC_REQUIRE(ceil_div(h_out, fv) == h_in,
              "%s: h_out = %d with fv = %d needs h_in = %lld, got %d", who,
              h_out, fv, (long long)ceil_div(h_out, fv), h_in);
  VTC_REQUIRE(ceil_div(w_out, fh) == w_in,
              "%s: w_out = %d with fh = %d needs w_in = %lld, got %d", who,
              w_out, fh, (long long)ceil_div(w_out, fh), w_in);
  const int64_t total = count * h_out * w_out;
  VTC_REQUIRE(!overlap(in, out, 4 * count * h_in * w_in, 4 * total),
              "%s: out overlaps in", who);
  hipStream_t st = as_stream(stream);
  if (mode == VTC_UPSAMPLE_TRIANGLE)
    hipLaunchKernelGGL(plane_upsample_kernel<true>, dim3(grid_for(total)),
                       dim3(kThreads), 0, st, in, out, total, h_in, w_in,
                       h_out, w_out, fv, fh);
  else
    hipLaunchKernelGGL(plane_upsample_kernel<false>, dim3(grid_for(total)),
                       dim3(kThreads), 0, st, in, out, total, h_in, w_in,
                       h_out, w_out, fv, fh);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}
