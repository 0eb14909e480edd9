// Scalar quantisers (include/vtc_quant.h): entropy-constrained assignment of
// codes to per-column codebooks, one Lloyd step with its convergence test on
// the device, and the counts of an index tensor.  DESIGN.md 4.15 states the
// contract, the order of the sums and the LDS budget.
//
//   vtc_quant_assign        zero_status_kernel, assign_kernel<false>
//   vtc_quant_lloyd_step    zero_status_kernel, assign_kernel<true>,
//                           update_kernel
//   vtc_quant_index_counts  zero_counts_kernel, index_counts_kernel
//
// One workgroup of assign_kernel takes a tile of adjacent columns x 512 rows.
// The codebooks (and, when lambda != 0, the lengths) of the tile's columns are
// staged in LDS once; thread t then owns column t % cols of the tile and walks
// the rows t / cols, t / cols + 256 / cols, ...: the lanes of a wave read
// adjacent columns of a few rows, and every lane scans its own column's cells
// in index order with float64 VALU arithmetic.  The scan is linear on purpose:
// the cells need not be sorted (a Lloyd update under lambda > 0 does not keep
// them apart in any order), k is small where the time goes (tens of cells at
// the experiment's size), and a linear scan is the only one whose tie rule is
// the contract's by construction.
//
// In a Lloyd step the indices of the block stay in LDS (int16) and a second
// phase gives every (column, cell) pair to 8 adjacent lanes: lane g walks the
// rows g, g + 8, ... of the block in ascending order and adds its members, and
// the 8 partial sums are added in ascending g through wave shuffles: a fixed
// order without floating-point atomics, and the many members of the zero cell
// are shared by 8 lanes whose LDS reads fall into different banks.  The
// per-block partials go to the workspace and update_kernel, one workgroup per
// column, adds them in ascending block order.
#include "../../include/vtc_quant.h"
#include "common.h"

#include <cmath>

namespace vtc {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxCodewords = VTC_QUANT_MAX_CODEWORDS;
constexpr int kRows = VTC_QUANT_ROWS;
constexpr int kMaxCols = 32;                  // columns of one tile, at most
constexpr int kLanes = VTC_QUANT_LANES;       // lanes that share one cell's sums
constexpr int kWave = 64;
constexpr int kLdsBytes = 64 * 1024;
constexpr size_t kStaticLds = kMaxCols * sizeof(int);   // sh_k of assign_kernel
constexpr int kCountRows = 1024;              // rows of one index_counts block
constexpr int kLdsCounters = 16384;           // 64 KiB of uint32
constexpr int64_t kMaxGrid = ((int64_t)1 << 31) - 1;

static_assert(kRows <= 32767 && kMaxCodewords <= 32767, "indices are int16");
static_assert(kWave % kLanes == 0 && kThreads % kWave == 0,
              "the lanes of one cell sit in one wave");

__device__ __forceinline__ double inf_f64() {
  return __longlong_as_double(0x7ff0000000000000ll);
}
__device__ __forceinline__ double nan_f64() {
  return __longlong_as_double(0x7ff8000000000000ll);
}

// Columns of one workgroup, 32 halved down to 1 until the workgroup's LDS fits
// 64 KiB: one float64 array of `stride` cells per column for the codebooks, a
// second for the lengths when lambda != 0, the block's int16 indices in a
// Lloyd step only, and the static sh_k of assign_kernel.  stride = kmax | 1 is
// odd, so the same cell of adjacent columns falls into different LDS banks.
// kmax = 1024 with lengths: 2 columns, 32 KiB (+ 2 KiB of indices in a step);
// without lengths 4 columns.
struct QuantTile {
  int cols, stride, planes;
  bool step;
  QuantTile(int kmax, bool step_, bool with_lengths) {
    stride = kmax | 1;
    planes = with_lengths ? 2 : 1;
    step = step_;
    cols = kMaxCols;
    while (cols > 1 && bytes() + kStaticLds > (size_t)kLdsBytes) cols >>= 1;
  }
  size_t bytes() const {   // the dynamic part
    return (size_t)planes * cols * stride * sizeof(double) +
           (step ? (size_t)kRows * cols * sizeof(short) : 0);
  }
};

struct StepLayout {
  double* sum;    // [chunks][s][kmax]
  double* dist;   // [chunks][s][kmax]
  int* count;     // [chunks][s][kmax]
  StepLayout(Carver& ws, int64_t b, int64_t s, int32_t kmax) {
    const size_t n = (size_t)ceil_div(b, kRows) * (size_t)s * (size_t)kmax;
    sum = ws.take<double>(n);
    dist = ws.take<double>(n);
    count = ws.take<int>(n);
  }
};

__device__ __forceinline__ int clamp_k(int k, int kmax) {
  return k < 1 ? 1 : (k > kmax ? kmax : k);
}

__global__ void zero_status_kernel(int64_t* __restrict__ status) {
  status[0] = 0;
}

__global__ void __launch_bounds__(kThreads)
zero_counts_kernel(int64_t* __restrict__ counts, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * kThreads)
    counts[i] = 0;
}

// The rule of the header on the `kk` staged cells of one column.  x is not NaN.
__device__ __forceinline__ int nearest_cell(double x, const double* cb,
                                            const double* ln, int kk,
                                            double lambda, bool with_lengths) {
  int best_i = 0;
  double d = __dsub_rn(x, cb[0]);
  double best = __dmul_rn(d, d);
  if (with_lengths) {
    best = __dadd_rn(best, __dmul_rn(lambda, ln[0]));
    for (int i = 1; i < kk; ++i) {
      d = __dsub_rn(x, cb[i]);
      const double cost = __dadd_rn(__dmul_rn(d, d), __dmul_rn(lambda, ln[i]));
      if (cost < best) {
        best = cost;
        best_i = i;
      }
    }
  } else {
    for (int i = 1; i < kk; ++i) {
      d = __dsub_rn(x, cb[i]);
      const double cost = __dmul_rn(d, d);
      if (cost < best) {
        best = cost;
        best_i = i;
      }
    }
  }
  return best_i;
}

// kStep false: indices and dequantised codes of every element.
// kStep true: the partial sums of the block for the active columns.
template <bool kStep>
__global__ void __launch_bounds__(kThreads)
assign_kernel(const float* __restrict__ codes, int64_t b, int64_t s,
              const double* __restrict__ codebooks,
              const double* __restrict__ lengths, const int* __restrict__ k,
              int kmax, double lambda, QuantTile shape, int64_t col_tiles,
              const int* __restrict__ active, int* __restrict__ indices,
              float* __restrict__ dequantized, int64_t* __restrict__ status,
              StepLayout part) {
  extern __shared__ double lds[];
  __shared__ int sh_k[kMaxCols];
  const int cols = shape.cols, stride = shape.stride;
  double* cb = lds;                          // [cols][stride]
  double* ln = lds + cols * stride;          // [cols][stride], lambda != 0
  short* idx =                               // [kRows][cols], a step only
      reinterpret_cast<short*>(lds + shape.planes * cols * stride);

  const int64_t chunk = blockIdx.x / col_tiles;
  const int64_t tile = blockIdx.x - chunk * col_tiles;
  const int64_t col0 = tile * cols;
  const int64_t r0 = chunk * kRows;
  const int rows = (int)(r0 + kRows < b ? kRows : b - r0);
  const bool with_lengths = shape.planes == 2;   // lambda != 0

  // cells in use of every column of the tile; 0: nothing to do for it
  if (threadIdx.x < cols) {
    const int64_t col = col0 + threadIdx.x;
    int kk = 0;
    if (col < s && (!kStep || active[col] != 0)) kk = clamp_k(k[col], kmax);
    sh_k[threadIdx.x] = kk;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < cols * kmax; e += kThreads) {
    const int cc = e / kmax, i = e - cc * kmax;
    if (i >= sh_k[cc]) continue;             // sh_k > 0: col0 + cc < s
    const int64_t at = (col0 + cc) * kmax + i;
    cb[cc * stride + i] = codebooks[at];
    if (with_lengths) ln[cc * stride + i] = lengths[at];
  }
  __syncthreads();

  {
    const int c = threadIdx.x % cols, phase = threadIdx.x / cols;
    const int phases = kThreads / cols;
    const int64_t col = col0 + c;
    const int kk = sh_k[c];
    const double* my_cb = cb + c * stride;
    const double* my_ln = ln + c * stride;
    int nans = 0;
    if (kk > 0) {
      for (int q = phase; q < rows; q += phases) {
        const int64_t at = (r0 + q) * s + col;   // r0 + q < b, col < s
        const float x = codes[at];
        int cell = -1;
        if (x == x)
          cell = nearest_cell((double)x, my_cb, my_ln, kk, lambda,
                              with_lengths);
        else
          ++nans;
        if (kStep) {
          idx[q * cols + c] = (short)cell;       // q < kRows, c < cols
        } else {
          indices[at] = cell;
          if (dequantized)
            dequantized[at] = cell >= 0 ? (float)my_cb[cell]
                                        : __int_as_float(0x7fc00000);
        }
      }
    }
    if (nans)
      atomicAdd(reinterpret_cast<unsigned long long*>(status),
                (unsigned long long)nans);
  }
  if (!kStep) return;
  __syncthreads();

  // kLanes adjacent lanes per (column, cell): lane g adds the members among
  // the rows g, g + kLanes, ... in ascending order, then the kLanes partials
  // are added in ascending g.  Every lane of the workgroup makes every pass:
  // the shuffles need the whole wave.
  const int items = cols * kmax * kLanes;
  for (int e0 = 0; e0 < items; e0 += kThreads) {
    const int e = e0 + threadIdx.x;
    const int pair = e / kLanes, g = e - pair * kLanes;
    const int cc = pair / kmax, i = pair - cc * kmax;
    const bool live = e < items && i < sh_k[cc];   // cc < cols when e < items
    const int64_t col = col0 + cc;
    double sum = 0.0, dist = 0.0;
    int members = 0;
    if (live) {
      const double centre = cb[cc * stride + i];
      for (int q = g; q < rows; q += kLanes) {
        if (idx[q * cols + cc] != (short)i) continue;
        const double x = (double)codes[(r0 + q) * s + col];
        const double d = __dsub_rn(x, centre);
        sum = __dadd_rn(sum, x);
        dist = __dadd_rn(dist, __dmul_rn(d, d));
        ++members;
      }
    }
    const int first = (threadIdx.x & (kWave - 1)) - g;   // lane of g = 0
    double sum_all = __shfl(sum, first), dist_all = __shfl(dist, first);
    int members_all = __shfl(members, first);
    for (int h = 1; h < kLanes; ++h) {
      sum_all = __dadd_rn(sum_all, __shfl(sum, first + h));
      dist_all = __dadd_rn(dist_all, __shfl(dist, first + h));
      members_all += __shfl(members, first + h);
    }
    if (live && g == 0) {
      const int64_t at = (chunk * s + col) * kmax + i;
      part.sum[at] = sum_all;
      part.dist[at] = dist_all;
      part.count[at] = members_all;
    }
  }
}

// One workgroup per column: the block partials in ascending order, then the
// cells in ascending order, the update and the convergence test.
__global__ void __launch_bounds__(kThreads)
update_kernel(vtc_quant_state in, vtc_quant_state out, StepLayout part,
              int64_t chunks, int64_t s, int kmax, double lambda,
              double epsilon, int pin_zero) {
  __shared__ double sh_sum[kMaxCodewords], sh_dist[kMaxCodewords];
  __shared__ long long sh_n[kMaxCodewords];
  __shared__ short sh_pos[kMaxCodewords];    // new slot, -1: removed
  __shared__ double sh_cost[3];
  __shared__ long long sh_total;
  __shared__ int sh_knew, sh_znew;

  const int64_t j = blockIdx.x;
  const int64_t row = j * kmax;
  const int t = threadIdx.x;
  if (in.active[j] == 0) {   // the same for the whole workgroup
    for (int i = t; i < kmax; i += kThreads) {
      out.codebooks[row + i] = in.codebooks[row + i];
      out.lengths[row + i] = in.lengths[row + i];
      out.counts[row + i] = in.counts[row + i];
    }
    if (t < 3) out.cost[3 * j + t] = in.cost[3 * j + t];
    if (t == 0) {
      out.k[j] = in.k[j];
      out.zero_index[j] = in.zero_index[j];
      out.active[j] = 0;
      out.iterations[j] = in.iterations[j];
    }
    return;
  }
  const int k0 = clamp_k(in.k[j], kmax);
  const int z = in.zero_index[j];
  const bool pinned = pin_zero != 0 && z >= 0 && z < k0;
  for (int i = t; i < k0; i += kThreads) {
    double sum = 0.0, dist = 0.0;
    long long n = 0;
    for (int64_t c = 0; c < chunks; ++c) {
      const int64_t at = (c * s + j) * kmax + i;
      sum = __dadd_rn(sum, part.sum[at]);
      dist = __dadd_rn(dist, part.dist[at]);
      n += part.count[at];
    }
    sh_sum[i] = sum;
    sh_dist[i] = dist;
    sh_n[i] = n;
  }
  __syncthreads();
  if (t == 0) {
    long long total = 0;
    double D = 0.0, R = 0.0;
    int knew = 0;
    for (int i = 0; i < k0; ++i) {
      const long long n = sh_n[i];
      total += n;
      D = __dadd_rn(D, sh_dist[i]);
      if (n > 0) R = __dadd_rn(R, __dmul_rn((double)n, in.lengths[row + i]));
      const bool keep = n > 0 || (pinned && i == z);
      sh_pos[i] = keep ? (short)knew++ : (short)-1;
    }
    sh_total = total;
    sh_knew = knew;
    sh_znew = -1;   // until the thread that moves cell z says otherwise
    sh_cost[0] = lambda == 0.0 ? D : __dadd_rn(D, __dmul_rn(lambda, R));
    sh_cost[1] = D;
    sh_cost[2] = R;
  }
  __syncthreads();   // in.lengths has been read: a step in place may write now
  const long long total = sh_total;
  if (total == 0) {   // every code NaN: nothing to fit
    for (int i = t; i < kmax; i += kThreads) {
      out.codebooks[row + i] = in.codebooks[row + i];
      out.lengths[row + i] = in.lengths[row + i];
      out.counts[row + i] = in.counts[row + i];
    }
    if (t < 3) out.cost[3 * j + t] = nan_f64();
    if (t == 0) {
      out.k[j] = in.k[j];
      out.zero_index[j] = z;
      out.active[j] = 0;
      out.iterations[j] = in.iterations[j] + 1;
    }
    return;
  }
  const int knew = sh_knew;
  for (int i = t; i < k0; i += kThreads) {
    const int p = sh_pos[i];
    if (p < 0) continue;
    const long long n = sh_n[i];
    const double c = (pinned && i == z) ? 0.0
                                        : __ddiv_rn(sh_sum[i], (double)n);
    const double len =
        n > 0 ? -log2(__ddiv_rn((double)n, (double)total)) : inf_f64();
    out.codebooks[row + p] = c;   // p <= i < kmax
    out.lengths[row + p] = len;
    out.counts[row + p] = n;
    if (i == z && c == 0.0) sh_znew = p;   // still the zero codeword
  }
  for (int i = knew + t; i < kmax; i += kThreads) {
    out.codebooks[row + i] = 0.0;   // never read: finite, for a caller's checks
    out.lengths[row + i] = 0.0;
    out.counts[row + i] = 0;
  }
  __syncthreads();
  if (t == 0) {
    const int it = in.iterations[j];
    const double J = sh_cost[0], J_prev = in.cost[3 * j];
    const bool done = it > 0 &&
                      __dsub_rn(J_prev, J) <= __dmul_rn(epsilon, J_prev);
    out.cost[3 * j] = J;
    out.cost[3 * j + 1] = sh_cost[1];
    out.cost[3 * j + 2] = sh_cost[2];
    out.k[j] = knew;
    out.zero_index[j] = sh_znew;
    out.active[j] = done ? 0 : 1;
    out.iterations[j] = it + 1;
  }
}

// Columns of one index_counts workgroup: 32 halved until cols * kmax uint32
// counters fit 64 KiB (kmax = 1024: 16 columns).
struct CountTile {
  int cols;
  explicit CountTile(int kmax) {
    cols = kMaxCols;
    while (cols > 1 && cols * kmax > kLdsCounters) cols >>= 1;
  }
};

__global__ void __launch_bounds__(kThreads)
index_counts_kernel(const int* __restrict__ indices, int64_t b, int64_t s,
                    int kmax, int cols, int64_t col_tiles,
                    int64_t* __restrict__ counts) {
  extern __shared__ unsigned cnt[];   // [cols][kmax]
  const int used = cols * kmax;
  for (int i = threadIdx.x; i < used; i += kThreads) cnt[i] = 0u;
  __syncthreads();
  const int64_t chunk = blockIdx.x / col_tiles;
  const int64_t tile = blockIdx.x - chunk * col_tiles;
  const int c = threadIdx.x % cols, phase = threadIdx.x / cols;
  const int phases = kThreads / cols;
  const int64_t col = tile * cols + c;
  const int64_t r0 = chunk * kCountRows;
  const int64_t r1 = r0 + kCountRows < b ? r0 + kCountRows : b;
  if (col < s) {
    for (int64_t r = r0 + phase; r < r1; r += phases) {
      const int i = indices[r * s + col];   // r < b, col < s
      if (i >= 0 && i < kmax) atomicAdd(&cnt[c * kmax + i], 1u);
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < used; e += kThreads) {
    const unsigned v = cnt[e];
    if (!v) continue;
    const int cc = e / kmax, i = e - cc * kmax;
    const int64_t out_col = tile * cols + cc;   // v != 0: out_col < s
    atomicAdd(reinterpret_cast<unsigned long long*>(counts) +
                  (out_col * kmax + i),
              (unsigned long long)v);
  }
}

// ---- argument checks --------------------------------------------------------
int check_shape(const char* who, int64_t b, int64_t s, int32_t kmax) {
  VTC_REQUIRE(b >= 1 && s >= 1, "%s: bad size b = %lld, s = %lld", who,
              (long long)b, (long long)s);
  VTC_REQUIRE(kmax >= 1, "%s: bad size kmax = %d", who, kmax);
  if (kmax > kMaxCodewords) {
    set_error("%s: kmax = %d, at most %d", who, kmax, kMaxCodewords);
    return VTC_ERR_UNSUPPORTED;
  }
  return VTC_OK;
}

// blocks of an assign_kernel launch, 0 when they pass the grid limit
int64_t assign_grid(int64_t b, int64_t s, const QuantTile& tile) {
  const int64_t chunks = ceil_div(b, kRows);
  const int64_t col_tiles = ceil_div(s, tile.cols);
  return chunks <= kMaxGrid / col_tiles ? chunks * col_tiles : 0;
}

bool state_complete(const vtc_quant_state* st) {
  return st && st->codebooks && st->lengths && st->counts && st->cost &&
         st->k && st->zero_index && st->active && st->iterations;
}

unsigned zero_grid(int64_t total) {
  const int64_t blocks = ceil_div(total, kThreads);
  return (unsigned)(blocks < 4096 ? blocks : 4096);
}

}  // namespace
}  // namespace vtc

using namespace vtc;

extern "C" int vtc_quant_abi_version(void) { return VTC_QUANT_ABI_VERSION; }

// ------------------------------------------------------------------- assign
extern "C" int vtc_quant_assign(const float* codes, int64_t b, int64_t s,
                                const double* codebooks, const double* lengths,
                                const int32_t* k, int32_t kmax, double lambda,
                                int32_t* indices, float* dequantized,
                                int64_t* status, void* stream) {
  const char* who = "vtc_quant_assign";
  VTC_REQUIRE(codes && codebooks && k && indices && status,
              "%s: null pointer", who);
  if (int rc = check_shape(who, b, s, kmax)) return rc;
  VTC_REQUIRE(lambda >= 0.0, "%s: bad lambda = %g", who, lambda);
  VTC_REQUIRE(lengths || lambda == 0.0, "%s: null pointer (lengths)", who);
  const QuantTile tile(kmax, false, lambda != 0.0);
  const int64_t grid = assign_grid(b, s, tile);
  VTC_REQUIRE(grid > 0, "%s: codes too large", who);
  hipStream_t st = as_stream(stream);
  Carver none(nullptr);
  const StepLayout no_partials(none, b, s, kmax);
  zero_status_kernel<<<1, 1, 0, st>>>(status);
  VTC_LAUNCH_CHECK();
  assign_kernel<false><<<(unsigned)grid, kThreads, tile.bytes(), st>>>(
      codes, b, s, codebooks, lengths, k, kmax, lambda, tile,
      ceil_div(s, tile.cols), nullptr, indices, dequantized, status,
      no_partials);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

// --------------------------------------------------------------- Lloyd step
extern "C" size_t vtc_quant_lloyd_step_workspace_bytes(int64_t b, int64_t s,
                                                       int32_t kmax) {
  if (b < 1 || s < 1 || kmax < 1 || kmax > kMaxCodewords) return 0;
  // the narrowest tile of a step, so the answer does not depend on lambda
  if (s > kMaxGrid || assign_grid(b, s, QuantTile(kmax, true, true)) == 0)
    return 0;
  return measured_bytes<StepLayout>(b, s, kmax);
}

extern "C" int vtc_quant_lloyd_step(const float* codes, int64_t b, int64_t s,
                                    int32_t kmax, double lambda,
                                    double epsilon, int32_t pin_zero,
                                    const vtc_quant_state* in,
                                    const vtc_quant_state* out,
                                    int64_t* status, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  const char* who = "vtc_quant_lloyd_step";
  VTC_REQUIRE(codes && status, "%s: null pointer", who);
  VTC_REQUIRE(state_complete(in), "%s: null pointer (in)", who);
  VTC_REQUIRE(state_complete(out), "%s: null pointer (out)", who);
  if (int rc = check_shape(who, b, s, kmax)) return rc;
  VTC_REQUIRE(lambda >= 0.0, "%s: bad lambda = %g", who, lambda);
  const size_t need = vtc_quant_lloyd_step_workspace_bytes(b, s, kmax);
  VTC_REQUIRE(need > 0, "%s: codes too large", who);
  const QuantTile tile(kmax, true, lambda != 0.0);
  const int64_t grid = assign_grid(b, s, tile);   // <= that of the query's tile
  if (!workspace || workspace_bytes < need) {
    set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
              need);
    return VTC_ERR_WORKSPACE;
  }
  Carver carve(workspace);
  const StepLayout part(carve, b, s, kmax);
  hipStream_t st = as_stream(stream);
  zero_status_kernel<<<1, 1, 0, st>>>(status);
  VTC_LAUNCH_CHECK();
  assign_kernel<true><<<(unsigned)grid, kThreads, tile.bytes(), st>>>(
      codes, b, s, in->codebooks, in->lengths, in->k, kmax, lambda, tile,
      ceil_div(s, tile.cols), in->active, nullptr, nullptr, status, part);
  VTC_LAUNCH_CHECK();
  update_kernel<<<(unsigned)s, kThreads, 0, st>>>(
      *in, *out, part, ceil_div(b, kRows), s, kmax, lambda, epsilon, pin_zero);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

// ------------------------------------------------------------- index counts
extern "C" int vtc_quant_index_counts(const int32_t* indices, int64_t b,
                                      int64_t s, int32_t kmax, int64_t* counts,
                                      void* stream) {
  const char* who = "vtc_quant_index_counts";
  VTC_REQUIRE(indices && counts, "%s: null pointer", who);
  if (int rc = check_shape(who, b, s, kmax)) return rc;
  const CountTile tile(kmax);
  const int64_t chunks = ceil_div(b, kCountRows);
  const int64_t col_tiles = ceil_div(s, tile.cols);
  VTC_REQUIRE(chunks <= kMaxGrid / col_tiles, "%s: indices too large", who);
  hipStream_t st = as_stream(stream);
  zero_counts_kernel<<<zero_grid(s * kmax), kThreads, 0, st>>>(counts,
                                                               s * kmax);
  VTC_LAUNCH_CHECK();
  index_counts_kernel<<<(unsigned)(chunks * col_tiles), kThreads,
                        (size_t)tile.cols * kmax * sizeof(unsigned), st>>>(
      indices, b, s, kmax, tile.cols, col_tiles, counts);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}
