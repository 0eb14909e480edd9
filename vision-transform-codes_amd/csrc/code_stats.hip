// Code statistics (include/vtc_stats.h): per-column summaries, marginal and
// joint histograms with numpy's bin rules, and the segmented mean behind
// rotational_average.  DESIGN.md 4.14 states the rules, the tiles and the LDS
// bound.
//
//   vtc_code_summary          summary_partial_kernel<false>, summary_mean_kernel,
//                             summary_partial_kernel<true>, summary_var_kernel
//   vtc_code_histogram        hist_prepare_kernel, hist_kernel
//   vtc_code_joint_histogram  zero_counts_kernel, joint_range_kernel,
//                             joint_range_final_kernel, joint_count_kernel
//   vtc_binned_mean           binned_partial_kernel, binned_final_kernel
//
// Loads along a row of `codes` are coalesced: a wave reads adjacent columns of
// one row.  Floating-point sums have a fixed order given by the constants of
// the header (512 rows, 4096 samples), never by the grid; counts go through
// uint32 LDS counters and integer atomics on the int64 output.
#include "../../include/vtc_stats.h"
#include "common.h"

#include <cmath>

namespace vtc {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxIgnore = VTC_STATS_MAX_IGNORE;
constexpr int kSumRows = VTC_STATS_SUMMARY_ROWS;
constexpr int kSumCols = 64;                  // one lane per column
constexpr int kHistRows = 1024;               // rows of one histogram block
constexpr int kHistMaxCols = 64;
constexpr int kHistMinCols = 4;
constexpr int kLdsCounters = 16384;           // 64 KiB of uint32
constexpr int kJointRows = VTC_STATS_JOINT_ROWS;
constexpr int kJointLdsBins = 128;            // 128 * 128 = kLdsCounters
constexpr int kBinnedSamples = VTC_STATS_BINNED_SAMPLES;
constexpr int64_t kMaxGrid = ((int64_t)1 << 31) - 1;

// ---- the filter -----------------------------------------------------------
struct Filter {
  float v[kMaxIgnore];
  int n;
  __device__ __forceinline__ void load(const float* ignore, int n_ignore) {
    n = n_ignore;
#pragma unroll
    for (int i = 0; i < kMaxIgnore; ++i) v[i] = i < n_ignore ? ignore[i] : 0.f;
  }
  __device__ __forceinline__ bool keeps(float x) const {
    bool keep = true;
#pragma unroll
    for (int i = 0; i < kMaxIgnore; ++i)
      if (i < n && x == v[i]) keep = false;
    return keep;
  }
};

__device__ __forceinline__ bool finite_f32(float x) {
  return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
}

__device__ __forceinline__ double nan_f64() {
  return __longlong_as_double(0x7ff8000000000000ll);
}

// ---- numpy's bins -----------------------------------------------------------
// step = (hi - lo) / bins, scale = bins / (hi - lo); e_k = lo + k * step with
// the product and the sum rounded separately, e_bins = hi.  -1: not counted.
__device__ __forceinline__ double edge_of(int k, double lo, double step) {
  return __dadd_rn(lo, __dmul_rn((double)k, step));
}

__device__ __forceinline__ int bin_of_value(double x, double lo, double hi,
                                            double step, double scale,
                                            int bins) {
  if (!(x >= lo && x <= hi)) return -1;
  if (lo == hi) return bins - 1;
  const double g = __dmul_rn(__dsub_rn(x, lo), scale);
  int k = !(g >= 0.0) ? 0 : (g >= (double)bins ? bins - 1 : (int)g);
  // 0 <= k <= bins - 1 from here on; e_{k+1} below is never e_bins
  while (k > 0 && x < edge_of(k, lo, step)) --k;
  while (k < bins - 1 && x >= edge_of(k + 1, lo, step)) ++k;
  return k;
}

// ---- vtc_code_summary -----------------------------------------------------
struct SummaryLayout {
  double* sum;       // [chunks][s]
  int* kept;
  int* nonfinite;
  float* lo;
  float* hi;
  SummaryLayout(Carver& ws, int64_t b, int64_t s) {
    const size_t n = (size_t)ceil_div(b, kSumRows) * (size_t)s;
    sum = ws.take<double>(n);
    kept = ws.take<int>(n);
    nonfinite = ws.take<int>(n);
    lo = ws.take<float>(n);
    hi = ws.take<float>(n);
  }
};

// One workgroup per 64 adjacent columns x 512 rows: lane = column, wave w
// takes rows w, w + 4, ... of the block.  kSecond: the sum of (x - mean)^2.
template <bool kSecond>
__global__ void __launch_bounds__(kThreads)
summary_partial_kernel(const float* __restrict__ codes, int64_t b, int64_t s,
                       const float* __restrict__ ignore, int n_ignore,
                       int64_t col_tiles, const double* __restrict__ mean,
                       SummaryLayout part) {
  __shared__ double sh_sum[kWaves][kSumCols];
  __shared__ int sh_kept[kWaves][kSumCols], sh_nonf[kWaves][kSumCols];
  __shared__ float sh_lo[kWaves][kSumCols], sh_hi[kWaves][kSumCols];

  const int64_t chunk = blockIdx.x / col_tiles;
  const int64_t tile = blockIdx.x - chunk * col_tiles;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t col = tile * kSumCols + lane;
  const int64_t r0 = chunk * kSumRows;
  const int64_t r1 = r0 + kSumRows < b ? r0 + kSumRows : b;

  Filter f;
  f.load(ignore, n_ignore);
  double sum = 0.0;
  int kept = 0, nonf = 0;
  float lo = INFINITY, hi = -INFINITY;
  if (col < s) {
    const double m = kSecond ? mean[col] : 0.0;
    for (int64_t r = r0 + wave; r < r1; r += kWaves) {
      const float x = codes[r * s + col];   // r < b, col < s
      if (!f.keeps(x)) continue;
      ++kept;
      if (!finite_f32(x)) {
        ++nonf;
        continue;
      }
      if (kSecond) {
        const double d = __dsub_rn((double)x, m);
        sum = __dadd_rn(sum, __dmul_rn(d, d));
      } else {
        sum = __dadd_rn(sum, (double)x);
        lo = x < lo ? x : lo;
        hi = x > hi ? x : hi;
      }
    }
  }
  sh_sum[wave][lane] = sum;
  sh_kept[wave][lane] = kept;
  sh_nonf[wave][lane] = nonf;
  sh_lo[wave][lane] = lo;
  sh_hi[wave][lane] = hi;
  __syncthreads();
  if (wave == 0 && col < s) {
    for (int v = 1; v < kWaves; ++v) {
      sum = __dadd_rn(sum, sh_sum[v][lane]);
      kept += sh_kept[v][lane];
      nonf += sh_nonf[v][lane];
      lo = sh_lo[v][lane] < lo ? sh_lo[v][lane] : lo;
      hi = sh_hi[v][lane] > hi ? sh_hi[v][lane] : hi;
    }
    const int64_t at = chunk * s + col;
    part.sum[at] = sum;
    if (!kSecond) {
      part.kept[at] = kept;
      part.nonfinite[at] = nonf;
      part.lo[at] = lo;
      part.hi[at] = hi;
    }
  }
}

__global__ void __launch_bounds__(kThreads)
summary_mean_kernel(SummaryLayout part, int64_t chunks, int64_t s,
                    int64_t* __restrict__ kept_out, double* __restrict__ lo_out,
                    double* __restrict__ hi_out, double* __restrict__ mean_out,
                    int64_t* __restrict__ nonfinite_out) {
  const int64_t col = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (col >= s) return;
  double sum = 0.0;
  int64_t kept = 0, nonf = 0;
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t c = 0; c < chunks; ++c) {
    const int64_t at = c * s + col;
    sum = __dadd_rn(sum, part.sum[at]);
    kept += part.kept[at];
    nonf += part.nonfinite[at];
    lo = part.lo[at] < lo ? part.lo[at] : lo;
    hi = part.hi[at] > hi ? part.hi[at] : hi;
  }
  const int64_t n = kept - nonf;
  kept_out[col] = kept;
  nonfinite_out[col] = nonf;
  lo_out[col] = n > 0 ? (double)lo : nan_f64();
  hi_out[col] = n > 0 ? (double)hi : nan_f64();
  mean_out[col] = n > 0 ? __ddiv_rn(sum, (double)n) : nan_f64();
}

__global__ void __launch_bounds__(kThreads)
summary_var_kernel(SummaryLayout part, int64_t chunks, int64_t s,
                   const int64_t* __restrict__ kept,
                   const int64_t* __restrict__ nonfinite,
                   double* __restrict__ var_out) {
  const int64_t col = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (col >= s) return;
  double sum = 0.0;
  for (int64_t c = 0; c < chunks; ++c)
    sum = __dadd_rn(sum, part.sum[c * s + col]);
  const int64_t n = kept[col] - nonfinite[col];
  var_out[col] = n > 0 ? __ddiv_rn(sum, (double)n) : nan_f64();
}

// ---- vtc_code_histogram -----------------------------------------------------
struct HistLayout {
  double* step;    // [s]
  double* scale;   // [s]
  HistLayout(Carver& ws, int64_t s) {
    step = ws.take<double>((size_t)s);
    scale = ws.take<double>((size_t)s);
  }
};

// Columns of one workgroup, 64 halved down to 4 until the counters fit, and
// the counters per column: bins | 1 where that fits (always but at bins =
// 4096), an odd stride so that the columns of one row, which mostly fall near
// the same bin, spread over the LDS banks.
struct HistTile {
  int cols, stride;
  explicit HistTile(int bins) {
    cols = kHistMaxCols;
    while (cols > kHistMinCols && cols * (bins | 1) > kLdsCounters) cols >>= 1;
    stride = cols * (bins | 1) <= kLdsCounters ? (bins | 1) : bins;
  }
  int counters() const { return cols * stride; }   // <= kLdsCounters
};

__global__ void __launch_bounds__(kThreads)
zero_counts_kernel(int64_t* __restrict__ counts, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * kThreads)
    counts[i] = 0;
}

__global__ void __launch_bounds__(kThreads)
hist_prepare_kernel(const double* __restrict__ lo, const double* __restrict__ hi,
                    int64_t s, int bins, HistLayout par,
                    int64_t* __restrict__ counts) {
  const int64_t first = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = first; i < s * bins; i += stride) counts[i] = 0;
  for (int64_t c = first; c < s; c += stride) {
    const double width = __dsub_rn(hi[c], lo[c]);
    par.step[c] = __ddiv_rn(width, (double)bins);
    par.scale[c] = __ddiv_rn((double)bins, width);
  }
}

// One workgroup per tile.cols adjacent columns x kHistRows rows.  Counter of
// (column c of the tile, bin k): cnt[c * tile.stride + k], in
// tile.counters() words of dynamic LDS.
__global__ void __launch_bounds__(kThreads)
hist_kernel(const float* __restrict__ codes, int64_t b, int64_t s,
            const float* __restrict__ ignore, int n_ignore,
            const double* __restrict__ lo, const double* __restrict__ hi,
            HistLayout par, int bins, HistTile shape, int64_t col_tiles,
            int64_t* __restrict__ counts) {
  extern __shared__ unsigned cnt[];
  const int tile_cols = shape.cols, stride = shape.stride;
  const int used = tile_cols * stride;
  for (int i = threadIdx.x; i < used; i += kThreads) cnt[i] = 0u;
  __syncthreads();

  const int64_t chunk = blockIdx.x / col_tiles;
  const int64_t tile = blockIdx.x - chunk * col_tiles;
  const int c = threadIdx.x % tile_cols, phase = threadIdx.x / tile_cols;
  const int phases = kThreads / tile_cols;
  const int64_t col = tile * tile_cols + c;
  const int64_t r0 = chunk * kHistRows;
  const int64_t r1 = r0 + kHistRows < b ? r0 + kHistRows : b;

  Filter f;
  f.load(ignore, n_ignore);
  if (col < s) {
    const double l = lo[col], h = hi[col];
    const double step = par.step[col], scale = par.scale[col];
    if (l <= h) {   // false for a NaN range
      for (int64_t r = r0 + phase; r < r1; r += phases) {
        const float x = codes[r * s + col];   // r < b, col < s
        if (!f.keeps(x) || !finite_f32(x)) continue;
        const int k = bin_of_value((double)x, l, h, step, scale, bins);
        if (k >= 0) atomicAdd(&cnt[c * stride + k], 1u);   // k < bins
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < used; i += kThreads) {
    const unsigned v = cnt[i];
    if (!v) continue;
    const int cc = i / stride, k = i - cc * stride;
    const int64_t out_col = tile * tile_cols + cc;   // v != 0: out_col < s
    atomicAdd(reinterpret_cast<unsigned long long*>(counts) +
                  (out_col * bins + k),
              (unsigned long long)v);
  }
}

// ---- vtc_code_joint_histogram -----------------------------------------------
struct JointLayout {
  float* lo0;   // [n_pairs][chunks]
  float* hi0;
  float* lo1;
  float* hi1;
  int* kept;
  JointLayout(Carver& ws, int64_t b, int64_t n_pairs) {
    const size_t n = (size_t)n_pairs * (size_t)ceil_div(b, kJointRows);
    lo0 = ws.take<float>(n);
    hi0 = ws.take<float>(n);
    lo1 = ws.take<float>(n);
    hi1 = ws.take<float>(n);
    kept = ws.take<int>(n);
  }
};

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ float wave_maxf(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

__device__ __forceinline__ bool pair_in_range(int i, int j, int max_column) {
  return i >= 0 && i < max_column && j >= 0 && j < max_column;
}

// One workgroup per pair x kJointRows rows: the range of both axes over the
// kept rows with two finite values, and the number of kept rows.
__global__ void __launch_bounds__(kThreads)
joint_range_kernel(const float* __restrict__ codes, int64_t b, int64_t s,
                   const int* __restrict__ pairs, int max_column,
                   const float* __restrict__ ignore, int n_ignore,
                   int64_t chunks, JointLayout part) {
  __shared__ float sh[4][kWaves];
  __shared__ int sh_kept[kWaves];
  const int64_t pair = blockIdx.x / chunks;
  const int64_t chunk = blockIdx.x - pair * chunks;
  const int i = pairs[2 * pair], j = pairs[2 * pair + 1];
  if (!pair_in_range(i, j, max_column)) return;   // max_column <= s
  const int64_t r0 = chunk * kJointRows;
  const int64_t r1 = r0 + kJointRows < b ? r0 + kJointRows : b;
  Filter f;
  f.load(ignore, n_ignore);
  float lo0 = INFINITY, hi0 = -INFINITY, lo1 = INFINITY, hi1 = -INFINITY;
  int kept = 0;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += kThreads) {
    const float x = codes[r * s + i], y = codes[r * s + j];
    if (!f.keeps(x) || !f.keeps(y)) continue;
    ++kept;
    if (!finite_f32(x) || !finite_f32(y)) continue;
    lo0 = x < lo0 ? x : lo0;
    hi0 = x > hi0 ? x : hi0;
    lo1 = y < lo1 ? y : lo1;
    hi1 = y > hi1 ? y : hi1;
  }
  lo0 = wave_min(lo0);
  hi0 = wave_maxf(hi0);
  lo1 = wave_min(lo1);
  hi1 = wave_maxf(hi1);
  kept = wave_sum_int(kept);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sh[0][wave] = lo0;
    sh[1][wave] = hi0;
    sh[2][wave] = lo1;
    sh[3][wave] = hi1;
    sh_kept[wave] = kept;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int v = 1; v < kWaves; ++v) {
      lo0 = sh[0][v] < lo0 ? sh[0][v] : lo0;
      hi0 = sh[1][v] > hi0 ? sh[1][v] : hi0;
      lo1 = sh[2][v] < lo1 ? sh[2][v] : lo1;
      hi1 = sh[3][v] > hi1 ? sh[3][v] : hi1;
      kept += sh_kept[v];
    }
    const int64_t at = pair * chunks + chunk;
    part.lo0[at] = lo0;
    part.hi0[at] = hi0;
    part.lo1[at] = lo1;
    part.hi1[at] = hi1;
    part.kept[at] = kept;
  }
}

// One wave per pair: the partial ranges of its blocks of rows.
__global__ void __launch_bounds__(64)
joint_range_final_kernel(JointLayout part, int64_t chunks,
                         const int* __restrict__ pairs, int max_column,
                         int64_t* __restrict__ kept_out,
                         double* __restrict__ lo_out,
                         double* __restrict__ hi_out) {
  const int64_t pair = blockIdx.x;
  const int i = pairs[2 * pair], j = pairs[2 * pair + 1];
  if (!pair_in_range(i, j, max_column)) {
    if (threadIdx.x == 0) {
      kept_out[pair] = -1;
      lo_out[2 * pair] = lo_out[2 * pair + 1] = nan_f64();
      hi_out[2 * pair] = hi_out[2 * pair + 1] = nan_f64();
    }
    return;
  }
  float lo0 = INFINITY, hi0 = -INFINITY, lo1 = INFINITY, hi1 = -INFINITY;
  int64_t kept = 0;
  for (int64_t c = threadIdx.x; c < chunks; c += 64) {
    const int64_t at = pair * chunks + c;
    lo0 = part.lo0[at] < lo0 ? part.lo0[at] : lo0;
    hi0 = part.hi0[at] > hi0 ? part.hi0[at] : hi0;
    lo1 = part.lo1[at] < lo1 ? part.lo1[at] : lo1;
    hi1 = part.hi1[at] > hi1 ? part.hi1[at] : hi1;
    kept += part.kept[at];
  }
  lo0 = wave_min(lo0);
  hi0 = wave_maxf(hi0);
  lo1 = wave_min(lo1);
  hi1 = wave_maxf(hi1);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) kept += __shfl_xor(kept, off, 64);
  if (threadIdx.x == 0) {
    kept_out[pair] = kept;
    const bool any = lo0 <= hi0;   // a row with two finite values was seen
    lo_out[2 * pair] = any ? (double)lo0 : nan_f64();
    hi_out[2 * pair] = any ? (double)hi0 : nan_f64();
    lo_out[2 * pair + 1] = any ? (double)lo1 : nan_f64();
    hi_out[2 * pair + 1] = any ? (double)hi1 : nan_f64();
  }
}

// One workgroup per pair x kJointRows rows.  kLds: bins <= 128, the bins^2
// counters of the block live in LDS and are flushed once; above that every
// counted row is one atomic on the output.
template <bool kLds>
__global__ void __launch_bounds__(kThreads)
joint_count_kernel(const float* __restrict__ codes, int64_t b, int64_t s,
                   const int* __restrict__ pairs, int max_column,
                   const float* __restrict__ ignore, int n_ignore,
                   int64_t chunks, const double* __restrict__ lo,
                   const double* __restrict__ hi, int bins,
                   int64_t* __restrict__ counts) {
  extern __shared__ unsigned cnt[];   // kLds: bins * bins words
  const int64_t pair = blockIdx.x / chunks;
  const int64_t chunk = blockIdx.x - pair * chunks;
  const int i = pairs[2 * pair], j = pairs[2 * pair + 1];
  if (!pair_in_range(i, j, max_column)) return;
  const double l0 = lo[2 * pair], h0 = hi[2 * pair];
  const double l1 = lo[2 * pair + 1], h1 = hi[2 * pair + 1];
  if (!(l0 <= h0 && l1 <= h1)) return;   // nothing to count: NaN range
  const int cells = bins * bins;
  if (kLds) {
    for (int k = threadIdx.x; k < cells; k += kThreads) cnt[k] = 0u;
    __syncthreads();
  }
  const double w0 = __dsub_rn(h0, l0), w1 = __dsub_rn(h1, l1);
  const double step0 = __ddiv_rn(w0, (double)bins);
  const double step1 = __ddiv_rn(w1, (double)bins);
  const double scale0 = __ddiv_rn((double)bins, w0);
  const double scale1 = __ddiv_rn((double)bins, w1);
  unsigned long long* out =
      reinterpret_cast<unsigned long long*>(counts) + pair * (int64_t)cells;
  const int64_t r0 = chunk * kJointRows;
  const int64_t r1 = r0 + kJointRows < b ? r0 + kJointRows : b;
  Filter f;
  f.load(ignore, n_ignore);
  for (int64_t r = r0 + threadIdx.x; r < r1; r += kThreads) {
    const float x = codes[r * s + i], y = codes[r * s + j];
    if (!f.keeps(x) || !f.keeps(y)) continue;
    if (!finite_f32(x) || !finite_f32(y)) continue;
    const int k0 = bin_of_value((double)x, l0, h0, step0, scale0, bins);
    const int k1 = bin_of_value((double)y, l1, h1, step1, scale1, bins);
    if (k0 < 0 || k1 < 0) continue;
    if (kLds)
      atomicAdd(&cnt[k0 * bins + k1], 1u);
    else
      atomicAdd(out + (k0 * bins + k1), 1ull);
  }
  if (kLds) {
    __syncthreads();
    for (int k = threadIdx.x; k < cells; k += kThreads)
      if (cnt[k]) atomicAdd(out + k, (unsigned long long)cnt[k]);
  }
}

// ---- vtc_binned_mean ----------------------------------------------------------
struct BinnedLayout {
  double* sum;     // [count][chunks][nbins]
  int* members;    // [chunks][nbins]
  BinnedLayout(Carver& ws, int64_t count, int32_t h, int32_t w, int32_t nbins) {
    const size_t chunks = (size_t)ceil_div((int64_t)h * w, kBinnedSamples);
    sum = ws.take<double>((size_t)count * chunks * (size_t)nbins);
    members = ws.take<int>(chunks * (size_t)nbins);
  }
};

// One workgroup per image x block of 4096 samples x group of 256 bins: thread
// t owns bin 256 * group + t.  The samples pass through LDS 256 at a time and
// every thread walks them in row-major order, adding those of its bin.
template <class T>
__global__ void __launch_bounds__(kThreads)
binned_partial_kernel(const T* __restrict__ images,
                      const int* __restrict__ bin_of, int64_t hw, int nbins,
                      int64_t chunks, int groups, BinnedLayout part) {
  __shared__ double xs[kThreads];
  __shared__ int bs[kThreads];
  int64_t t = blockIdx.x;
  const int group = (int)(t % groups);
  t /= groups;
  const int64_t chunk = t % chunks;
  const int64_t img = t / chunks;
  const int mine = group * kThreads + threadIdx.x;
  const int64_t p0 = chunk * kBinnedSamples;
  const int64_t p1 = p0 + kBinnedSamples < hw ? p0 + kBinnedSamples : hw;
  double sum = 0.0;
  int members = 0;
  for (int64_t base = p0; base < p1; base += kThreads) {
    const int64_t p = base + threadIdx.x;
    __syncthreads();
    if (p < p1) {
      xs[threadIdx.x] = (double)images[img * hw + p];   // p < hw
      bs[threadIdx.x] = bin_of[p];
    }
    __syncthreads();
    const int n = p1 - base < kThreads ? (int)(p1 - base) : kThreads;
    for (int q = 0; q < n; ++q) {
      if (bs[q] == mine) {
        sum = __dadd_rn(sum, xs[q]);
        ++members;
      }
    }
  }
  if (mine < nbins) {
    part.sum[(img * chunks + chunk) * nbins + mine] = sum;
    if (img == 0) part.members[chunk * nbins + mine] = members;
  }
}

__global__ void __launch_bounds__(kThreads)
binned_final_kernel(BinnedLayout part, int64_t count, int64_t chunks, int nbins,
                    double* __restrict__ means, int64_t* __restrict__ members) {
  const int64_t at = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (at >= count * nbins) return;
  const int64_t img = at / nbins;
  const int bin = (int)(at - img * nbins);
  double sum = 0.0;
  int64_t n = 0;
  for (int64_t c = 0; c < chunks; ++c) {
    sum = __dadd_rn(sum, part.sum[(img * chunks + c) * nbins + bin]);
    n += part.members[c * nbins + bin];
  }
  means[at] = n > 0 ? __ddiv_rn(sum, (double)n) : nan_f64();
  if (img == 0) members[bin] = n;
}

// ---- argument checks shared by the code entry points -----------------------
int check_codes(const char* who, const void* codes, int64_t b, int64_t s,
                const void* ignore, int32_t n_ignore) {
  VTC_REQUIRE(codes, "%s: null pointer", who);
  VTC_REQUIRE(b >= 1 && s >= 1, "%s: bad size b = %lld, s = %lld", who,
              (long long)b, (long long)s);
  VTC_REQUIRE(n_ignore >= 0 && n_ignore <= kMaxIgnore,
              "%s: bad size n_ignore = %d (0 .. %d)", who, n_ignore,
              kMaxIgnore);
  VTC_REQUIRE(ignore || n_ignore == 0, "%s: null pointer (ignore)", who);
  return VTC_OK;
}

int check_workspace(const char* who, const void* workspace, size_t have,
                    size_t need) {
  if (!workspace || have < need) {
    set_error("%s: workspace of %zu bytes, %zu needed", who, have, need);
    return VTC_ERR_WORKSPACE;
  }
  return VTC_OK;
}

unsigned zero_grid(int64_t total) {
  const int64_t blocks = ceil_div(total, kThreads);
  return (unsigned)(blocks < 4096 ? blocks : 4096);
}

}  // namespace
}  // namespace vtc

using namespace vtc;

extern "C" int vtc_stats_abi_version(void) { return VTC_STATS_ABI_VERSION; }

// ------------------------------------------------------------------ summary
extern "C" size_t vtc_code_summary_workspace_bytes(int64_t b, int64_t s) {
  if (b < 1 || s < 1) return 0;
  return measured_bytes<SummaryLayout>(b, s);
}

extern "C" int vtc_code_summary(const float* codes, int64_t b, int64_t s,
                                const float* ignore, int32_t n_ignore,
                                int64_t* kept, double* lo, double* hi,
                                double* mean, double* var, int64_t* nonfinite,
                                void* workspace, size_t workspace_bytes,
                                void* stream) {
  const char* who = "vtc_code_summary";
  if (int rc = check_codes(who, codes, b, s, ignore, n_ignore)) return rc;
  VTC_REQUIRE(kept && lo && hi && mean && var && nonfinite,
              "%s: null pointer", who);
  const int64_t chunks = ceil_div(b, kSumRows);
  const int64_t col_tiles = ceil_div(s, kSumCols);
  VTC_REQUIRE(chunks <= kMaxGrid / col_tiles, "%s: codes too large", who);
  if (int rc = check_workspace(who, workspace, workspace_bytes,
                               vtc_code_summary_workspace_bytes(b, s)))
    return rc;
  Carver carve(workspace);
  const SummaryLayout part(carve, b, s);
  hipStream_t st = as_stream(stream);
  const unsigned grid = (unsigned)(chunks * col_tiles);
  const unsigned col_grid = (unsigned)ceil_div(s, kThreads);
  summary_partial_kernel<false><<<grid, kThreads, 0, st>>>(
      codes, b, s, ignore, n_ignore, col_tiles, nullptr, part);
  VTC_LAUNCH_CHECK();
  summary_mean_kernel<<<col_grid, kThreads, 0, st>>>(part, chunks, s, kept, lo,
                                                     hi, mean, nonfinite);
  VTC_LAUNCH_CHECK();
  summary_partial_kernel<true><<<grid, kThreads, 0, st>>>(
      codes, b, s, ignore, n_ignore, col_tiles, mean, part);
  VTC_LAUNCH_CHECK();
  summary_var_kernel<<<col_grid, kThreads, 0, st>>>(part, chunks, s, kept,
                                                    nonfinite, var);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

// ---------------------------------------------------------------- histogram
extern "C" size_t vtc_code_histogram_workspace_bytes(int64_t b, int64_t s,
                                                     int32_t bins) {
  if (b < 1 || s < 1 || bins < 1 || bins > VTC_STATS_MAX_BINS) return 0;
  return measured_bytes<HistLayout>(s);
}

extern "C" int vtc_code_histogram(const float* codes, int64_t b, int64_t s,
                                  const float* ignore, int32_t n_ignore,
                                  const double* lo, const double* hi,
                                  int32_t bins, int64_t* counts,
                                  void* workspace, size_t workspace_bytes,
                                  void* stream) {
  const char* who = "vtc_code_histogram";
  if (int rc = check_codes(who, codes, b, s, ignore, n_ignore)) return rc;
  VTC_REQUIRE(lo && hi && counts, "%s: null pointer", who);
  VTC_REQUIRE(bins >= 1, "%s: bad size bins = %d", who, bins);
  if (bins > VTC_STATS_MAX_BINS) {
    set_error("%s: bins = %d, at most %d", who, bins, VTC_STATS_MAX_BINS);
    return VTC_ERR_UNSUPPORTED;
  }
  const HistTile tile(bins);
  const int64_t col_tiles = ceil_div(s, tile.cols);
  const int64_t chunks = ceil_div(b, kHistRows);
  VTC_REQUIRE(chunks <= kMaxGrid / col_tiles, "%s: codes too large", who);
  if (int rc = check_workspace(who, workspace, workspace_bytes,
                               vtc_code_histogram_workspace_bytes(b, s, bins)))
    return rc;
  Carver carve(workspace);
  const HistLayout par(carve, s);
  hipStream_t st = as_stream(stream);
  hist_prepare_kernel<<<zero_grid(s * bins), kThreads, 0, st>>>(lo, hi, s, bins,
                                                                par, counts);
  VTC_LAUNCH_CHECK();
  hist_kernel<<<(unsigned)(chunks * col_tiles), kThreads,
                tile.counters() * sizeof(unsigned), st>>>(
      codes, b, s, ignore, n_ignore, lo, hi, par, bins, tile, col_tiles,
      counts);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

// -------------------------------------------------------------------- joint
extern "C" size_t vtc_code_joint_histogram_workspace_bytes(int64_t b,
                                                           int64_t n_pairs) {
  if (b < 1 || n_pairs < 1) return 0;
  return measured_bytes<JointLayout>(b, n_pairs);
}

extern "C" int vtc_code_joint_histogram(
    const float* codes, int64_t b, int64_t s, const int32_t* pairs,
    int64_t n_pairs, int32_t max_column, const float* ignore, int32_t n_ignore,
    int32_t bins, int64_t* kept, double* lo, double* hi, int64_t* counts,
    void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "vtc_code_joint_histogram";
  if (int rc = check_codes(who, codes, b, s, ignore, n_ignore)) return rc;
  VTC_REQUIRE(pairs && kept && lo && hi && counts, "%s: null pointer", who);
  VTC_REQUIRE(n_pairs >= 1, "%s: bad size n_pairs = %lld", who,
              (long long)n_pairs);
  VTC_REQUIRE(max_column >= 1 && (int64_t)max_column <= s,
              "%s: bad size max_column = %d (1 .. s = %lld)", who, max_column,
              (long long)s);
  VTC_REQUIRE(bins >= 1, "%s: bad size bins = %d", who, bins);
  if (bins > VTC_STATS_MAX_JOINT_BINS) {
    set_error("%s: bins = %d, at most %d per axis", who, bins,
              VTC_STATS_MAX_JOINT_BINS);
    return VTC_ERR_UNSUPPORTED;
  }
  const int64_t chunks = ceil_div(b, kJointRows);
  VTC_REQUIRE(n_pairs <= kMaxGrid / chunks, "%s: codes too large", who);
  if (int rc = check_workspace(
          who, workspace, workspace_bytes,
          vtc_code_joint_histogram_workspace_bytes(b, n_pairs)))
    return rc;
  Carver carve(workspace);
  const JointLayout part(carve, b, n_pairs);
  hipStream_t st = as_stream(stream);
  const int64_t cells = n_pairs * bins * bins;
  const unsigned grid = (unsigned)(n_pairs * chunks);
  zero_counts_kernel<<<zero_grid(cells), kThreads, 0, st>>>(counts, cells);
  VTC_LAUNCH_CHECK();
  joint_range_kernel<<<grid, kThreads, 0, st>>>(
      codes, b, s, pairs, max_column, ignore, n_ignore, chunks, part);
  VTC_LAUNCH_CHECK();
  joint_range_final_kernel<<<(unsigned)n_pairs, 64, 0, st>>>(
      part, chunks, pairs, max_column, kept, lo, hi);
  VTC_LAUNCH_CHECK();
  if (bins <= kJointLdsBins)
    joint_count_kernel<true><<<grid, kThreads,
                               (size_t)bins * bins * sizeof(unsigned), st>>>(
        codes, b, s, pairs, max_column, ignore, n_ignore, chunks, lo, hi, bins,
        counts);
  else
    joint_count_kernel<false><<<grid, kThreads, 0, st>>>(
        codes, b, s, pairs, max_column, ignore, n_ignore, chunks, lo, hi, bins,
        counts);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

// -------------------------------------------------------------- binned mean
extern "C" size_t vtc_binned_mean_workspace_bytes(int64_t count, int32_t h,
                                                  int32_t w, int32_t nbins) {
  if (count < 1 || h < 1 || w < 1 || nbins < 1 || nbins > VTC_STATS_MAX_BINS)
    return 0;
  return measured_bytes<BinnedLayout>(count, h, w, nbins);
}

extern "C" int vtc_binned_mean(const void* images, int dtype,
                               const int32_t* bin_of, int64_t count, int32_t h,
                               int32_t w, int32_t nbins, double* means,
                               int64_t* members, void* workspace,
                               size_t workspace_bytes, void* stream) {
  const char* who = "vtc_binned_mean";
  VTC_REQUIRE(images && bin_of && means && members, "%s: null pointer", who);
  VTC_REQUIRE(count >= 1, "%s: bad size count = %lld", who, (long long)count);
  VTC_REQUIRE(h >= 1 && w >= 1, "%s: bad size h = %d, w = %d", who, h, w);
  VTC_REQUIRE(dtype == VTC_DTYPE_F32 || dtype == VTC_DTYPE_F64,
              "%s: unknown dtype %d", who, dtype);
  VTC_REQUIRE(nbins >= 1, "%s: bad size nbins = %d", who, nbins);
  if (nbins > VTC_STATS_MAX_BINS) {
    set_error("%s: nbins = %d, at most %d", who, nbins, VTC_STATS_MAX_BINS);
    return VTC_ERR_UNSUPPORTED;
  }
  const int64_t hw = (int64_t)h * w;
  const int64_t chunks = ceil_div(hw, kBinnedSamples);
  const int groups = (int)ceil_div(nbins, kThreads);
  VTC_REQUIRE(count <= kMaxGrid / (chunks * groups), "%s: stack too large",
              who);
  if (int rc = check_workspace(
          who, workspace, workspace_bytes,
          vtc_binned_mean_workspace_bytes(count, h, w, nbins)))
    return rc;
  Carver carve(workspace);
  const BinnedLayout part(carve, count, h, w, nbins);
  hipStream_t st = as_stream(stream);
  const unsigned grid = (unsigned)(count * chunks * groups);
  if (dtype == VTC_DTYPE_F32)
    binned_partial_kernel<float><<<grid, kThreads, 0, st>>>(
        static_cast<const float*>(images), bin_of, hw, nbins, chunks, groups,
        part);
  else
    binned_partial_kernel<double><<<grid, kThreads, 0, st>>>(
        static_cast<const double*>(images), bin_of, hw, nbins, chunks, groups,
        part);
  VTC_LAUNCH_CHECK();
  binned_final_kernel<<<(unsigned)ceil_div(count * nbins, kThreads), kThreads,
                        0, st>>>(part, count, chunks, nbins, means, members);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}
