// Vector quantiser for up to 131 072 codewords (include/vtc_vq_large.h): the
// contract, the order of the sums and the bits of vq.hip, without its three
// kmax-sized LDS arrays and without per-block partials of every cell.
// DESIGN.md 4.20.
//
//   vtc_vq_large_assign      zero_status_kernel, vq_assign_kernel (vq_scan.h)
//   vtc_vq_large_lloyd_step  zero_status_kernel, vq_assign_kernel,
//                            vql_accumulate_kernel, vql_totals_kernel,
//                            vql_reduce_kernel, vql_update_kernel
//   vtc_vq_large_index_counts  vql_zero_counts_kernel, vql_index_counts_kernel
//
// vql_accumulate_kernel, one workgroup per block of 2048 rows, stages the
// block's indices in LDS (int32) and sorts a copy of them there (bitonic, 2048
// keys): the heads of the runs are the block's distinct cells, in ascending
// order, and the distance between two heads is a cell's members.  A block
// holds at most 2048 distinct cells whatever kmax is.  The list goes to the
// workspace, and beside it the sums, distances and counts of the listed cells:
// 16 adjacent lanes per listed cell walk the staged indices exactly as
// vq_accumulate_kernel does.
//
// vql_totals_kernel, one thread per cell, looks its cell up in every block's
// sorted list (a binary search of at most 12 probes) in ascending block order
// and adds the counts and distances it finds.  vql_reduce_kernel, one
// workgroup of 1024 threads, forms D and R in the 1024-lane order, the
// convergence test, and the new slot of every kept cell by a prefix scan over
// 1024 contiguous ranges of cells.  vql_update_kernel, one thread per element
// of the new codebook, adds the block partials of the sums the same way and
// writes the state.  Only vql_update_kernel writes `out`, and it reads `in`
// only where it copies a slot onto itself, so a step in place is safe.  The
// kernels are separate launches: no workgroup waits for another.
#include "../../include/vtc_vq_large.h"
#include "vq_scan.h"

#include <cmath>

namespace vtc {
namespace {

constexpr int kLargeMaxCodewords = VTC_VQ_LARGE_MAX_CODEWORDS;
constexpr int kRows = VTC_VQ_ROWS;
constexpr int kLanes = VTC_VQ_LANES;
constexpr int kCostLanes = VTC_VQ_COST_LANES;
constexpr int kWave = 64;
constexpr int kCountRows = 4096;     // rows of one index_counts block
constexpr int kCountWindow = 4096;   // cells of one index_counts block
constexpr int kNoCell = 0x7fffffff;  // sorts behind every cell
constexpr int kProbes = 12;          // a binary search among <= 2048 entries

static_assert(kRows == 2048 && kThreads == 256 && kRows % kThreads == 0,
              "the bitonic sort and the scan of the heads are written for it");
static_assert((1 << (kProbes - 1)) == kRows, "");
static_assert(kWave % kLanes == 0 && kThreads % kWave == 0,
              "the lanes of one cell sit in one wave");
static_assert(kCostLanes == 1024, "vql_reduce_kernel scans 1024 ranges");
static_assert((int64_t)kLargeMaxCodewords * kMaxDim < ((int64_t)1 << 31),
              "an element of the codebook is numbered in an int");

// the records of a step that vql_reduce_kernel leaves for vql_update_kernel
enum { kModeFrozen = 0, kModeNothing = 1, kModeStep = 2 };
enum { kMetaMode, kMetaKnew, kMetaTotal, kMetaPinned, kMetaK, kMetaZero,
       kMetaActive, kMetaIterations, kMetaInts };

struct VqLargeLayout {
  int* index;            // [b]
  double* rowdist;       // [b]
  int* cell;             // [chunks][2048], ascending, `listed` of them
  int* listed;           // [chunks]
  double* sum;           // [chunks][2048][d], by place in the list
  double* dist;          // [chunks][2048]
  int* count;            // [chunks][2048]
  long long* cell_n;     // [kmax], members of every cell
  double* cell_dist;     // [kmax], summed distances of every cell
  long long* members;    // [kmax], by new slot
  int* source;           // [kmax], the cell a new slot comes from
  double* cost;          // [3] (256 bytes)
  long long* meta;       // [kMetaInts] (256 bytes)
  VqLargeLayout(Carver& ws, int64_t b, int32_t d, int32_t kmax) {
    const size_t chunks = (size_t)ceil_div(b, kRows);
    const size_t places = chunks * (size_t)kRows;
    index = ws.take<int>((size_t)b);
    rowdist = ws.take<double>((size_t)b);
    cell = ws.take<int>(places);
    listed = ws.take<int>(chunks);
    sum = ws.take<double>(places * (size_t)d);
    dist = ws.take<double>(places);
    count = ws.take<int>(places);
    cell_n = ws.take<long long>((size_t)kmax);
    cell_dist = ws.take<double>((size_t)kmax);
    members = ws.take<long long>((size_t)kmax);
    source = ws.take<int>((size_t)kmax);
    cost = ws.take<double>(32);
    meta = ws.take<long long>(32);
  }
};

// The place of cell i in the ascending list `cells` of n <= 2048 entries, or
// -1.  At most kProbes probes.
__device__ __forceinline__ int place_of(const int* __restrict__ cells, int n,
                                        int i) {
  int lo = 0, hi = n;
  for (int s = 0; s < kProbes && lo < hi; ++s) {
    const int mid = (lo + hi) >> 1;
    if (cells[mid] < i)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < n && cells[lo] == i ? lo : -1;
}

// The per-block sums of a step, for the cells that occur in the block.  Every
// lane of the workgroup makes every pass: the shuffles need the whole wave.
template <int DP>
__global__ void __launch_bounds__(kThreads)
vql_accumulate_kernel(const float* __restrict__ vectors, int64_t b, int d,
                      const int* __restrict__ k, int kmax,
                      const int* __restrict__ active, VqLargeLayout part) {
  constexpr int kPer = kRows / kThreads;     // sorted keys of one thread
  __shared__ int idx[kRows];                 // the cell of every row
  __shared__ int key[kRows];                 // the same, sorted
  __shared__ int list[kRows];                // the distinct cells, ascending
  __shared__ int start[kRows + 1];           // where their runs begin in `key`
  __shared__ int scan[kThreads];
  if (active[0] == 0) return;
  const int kk = clamp_k(k[0], kmax);
  const int64_t chunk = blockIdx.x;
  const int64_t r0 = chunk * kRows;
  const int rows = (int)(r0 + kRows < b ? kRows : b - r0);
  for (int q = threadIdx.x; q < kRows; q += kThreads) {
    const int cell = q < rows ? part.index[r0 + q] : -1;   // -1 or < kk
    idx[q] = cell;
    key[q] = cell >= 0 && cell < kk ? cell : kNoCell;
  }
  __syncthreads();
  // bitonic sort of the 2048 keys, ascending
  for (int size = 2; size <= kRows; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int e = threadIdx.x; e < kRows / 2; e += kThreads) {
        const int lo = 2 * e - (e & (stride - 1));   // bit `stride` clear
        const int hi = lo + stride;
        const bool up = (lo & size) == 0;
        const int a = key[lo], c = key[hi];
        if ((a > c) == up) {
          key[lo] = c;
          key[hi] = a;
        }
      }
      __syncthreads();
    }
  }
  // the heads of the runs; the run of kNoCell, if any, is the last head
  const int first = threadIdx.x * kPer;
  int heads = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int q = first + j;
    heads += q == 0 || key[q] != key[q - 1];
  }
  scan[threadIdx.x] = heads;
  __syncthreads();
  for (int off = 1; off < kThreads; off <<= 1) {
    const int below = threadIdx.x >= off ? scan[threadIdx.x - off] : 0;
    __syncthreads();
    scan[threadIdx.x] += below;
    __syncthreads();
  }
  int at = scan[threadIdx.x] - heads;
  const int all_heads = scan[kThreads - 1];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int q = first + j;
    if (q == 0 || key[q] != key[q - 1]) {
      list[at] = key[q];
      start[at] = q;
      ++at;
    }
  }
  if (threadIdx.x == 0) start[all_heads] = kRows;
  __syncthreads();
  const int listed = all_heads - (key[kRows - 1] == kNoCell ? 1 : 0);
  const int64_t place0 = chunk * kRows;
  if (threadIdx.x == 0) part.listed[chunk] = listed;
  for (int p = threadIdx.x; p < listed; p += kThreads) {
    part.cell[place0 + p] = list[p];
    part.count[place0 + p] = start[p + 1] - start[p];
  }

  // kLanes adjacent lanes per listed cell: lane g adds the members among the
  // rows g, g + kLanes, ... in ascending order, then the kLanes partials are
  // added in ascending g.
  const int items = listed * kLanes;
  for (int e0 = 0; e0 < items; e0 += kThreads) {
    const int e = e0 + threadIdx.x;
    const int g = e % kLanes;
    const bool live = e < items;
    const int p = e / kLanes;
    const int i = live ? list[p] : -2;       // -2 matches no row
    double acc[DP];
#pragma unroll
    for (int t = 0; t < DP; ++t) acc[t] = 0.0;
    double dist = 0.0;
    if (live) {
      for (int q = g; q < rows; q += kLanes) {
        if (idx[q] != i) continue;
        const int64_t row = r0 + q;
#pragma unroll
        for (int t = 0; t < DP; ++t)
          if (t < d) acc[t] = __dadd_rn(acc[t], (double)vectors[row * d + t]);
        dist = __dadd_rn(dist, part.rowdist[row]);
      }
    }
    const int lane0 = (threadIdx.x & (kWave - 1)) - g;   // lane of g = 0
    const int64_t place = place0 + p;
    double dist_all = __shfl(dist, lane0);
#pragma unroll
    for (int h = 1; h < kLanes; ++h)
      dist_all = __dadd_rn(dist_all, __shfl(dist, lane0 + h));
#pragma unroll
    for (int t = 0; t < DP; ++t) {
      if (t < d) {                           // d is the same for every lane
        double all = __shfl(acc[t], lane0);
#pragma unroll
        for (int h = 1; h < kLanes; ++h)
          all = __dadd_rn(all, __shfl(acc[t], lane0 + h));
        if (live && g == 0) part.sum[place * d + t] = all;
      }
    }
    if (live && g == 0) part.dist[place] = dist_all;
  }
}

// One thread per cell: its members and its summed distances over the blocks,
// in ascending block order.  A block that does not list the cell is skipped
// (include/vtc_vq_large.h says why that changes no bit).
__global__ void __launch_bounds__(kThreads)
vql_totals_kernel(vtc_vq_state in, VqLargeLayout part, int64_t chunks,
                  int kmax) {
  if (in.active[0] == 0) return;
  const int k0 = clamp_k(in.k[0], kmax);
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= k0) return;
  double dist = 0.0;
  long long n = 0;
  for (int64_t c = 0; c < chunks; ++c) {
    const int p = place_of(part.cell + c * kRows, part.listed[c], i);
    if (p < 0) continue;
    dist = __dadd_rn(dist, part.dist[c * kRows + p]);
    n += part.count[c * kRows + p];
  }
  part.cell_n[i] = n;
  part.cell_dist[i] = dist;
}

// One workgroup of kCostLanes threads: D, R, J, the convergence test, the new
// slot of every kept cell.  Writes the workspace only.
__global__ void __launch_bounds__(kCostLanes)
vql_reduce_kernel(vtc_vq_state in, VqLargeLayout part, int64_t chunks, int d,
                  int kmax, double lambda, double epsilon, int pin_zero) {
  __shared__ double sh_d[kCostLanes], sh_r[kCostLanes];
  __shared__ int sh_scan[kCostLanes];
  __shared__ unsigned long long sh_total;
  __shared__ int sh_zero_moved;              // cell z: a new component != 0.0
  __shared__ int sh_znew;
  const int t = threadIdx.x;
  long long* meta = part.meta;
  if (in.active[0] == 0) {
    if (t == 0) {
      meta[kMetaMode] = kModeFrozen;
      meta[kMetaK] = in.k[0];
      meta[kMetaZero] = in.zero_index[0];
      meta[kMetaActive] = 0;
      meta[kMetaIterations] = in.iterations[0];
      for (int c = 0; c < 3; ++c) part.cost[c] = in.cost[c];
    }
    return;
  }
  const int k0 = clamp_k(in.k[0], kmax);
  const int z = in.zero_index[0];
  const bool pinned = pin_zero != 0 && z >= 0 && z < k0;
  if (t == 0) {
    sh_total = 0ull;
    sh_zero_moved = 0;
    sh_znew = -1;
  }
  __syncthreads();
  double d_part = 0.0, r_part = 0.0;
  long long n_part = 0;
  for (int i = t; i < k0; i += kCostLanes) {
    const long long n = part.cell_n[i];
    n_part += n;
    d_part = __dadd_rn(d_part, part.cell_dist[i]);
    if (n > 0)
      r_part = __dadd_rn(r_part, __dmul_rn((double)n, in.lengths[i]));
  }
  sh_d[t] = d_part;
  sh_r[t] = r_part;
  if (n_part) atomicAdd(&sh_total, (unsigned long long)n_part);
  // does the codeword of cell z stay the zero vector?  (unpinned: the mean)
  if (!pinned && z >= 0 && z < k0 && t < d && part.cell_n[z] > 0) {
    double sum = 0.0;
    for (int64_t c = 0; c < chunks; ++c) {
      const int p = place_of(part.cell + c * kRows, part.listed[c], z);
      if (p >= 0) sum = __dadd_rn(sum, part.sum[(c * kRows + p) * d + t]);
    }
    if (__ddiv_rn(sum, (double)part.cell_n[z]) != 0.0)
      atomicOr(&sh_zero_moved, 1);
  }
  // the kept cells of the range [lo, hi) of this thread, then their slots
  const int per = (k0 + kCostLanes - 1) / kCostLanes;
  const int lo = t * per < k0 ? t * per : k0;
  const int hi = lo + per < k0 ? lo + per : k0;
  int kept = 0;
  for (int i = lo; i < hi; ++i)
    kept += part.cell_n[i] > 0 || (pinned && i == z);
  sh_scan[t] = kept;
  __syncthreads();
  for (int off = 1; off < kCostLanes; off <<= 1) {
    const int below = t >= off ? sh_scan[t - off] : 0;
    __syncthreads();
    sh_scan[t] += below;
    __syncthreads();
  }
  int slot = sh_scan[t] - kept;
  for (int i = lo; i < hi; ++i) {
    const long long n = part.cell_n[i];
    if (n > 0 || (pinned && i == z)) {
      if (i == z && !sh_zero_moved) sh_znew = slot;
      part.members[slot] = n;                // slot <= i < kmax
      part.source[slot] = i;
      ++slot;
    }
  }
  __syncthreads();
  if (t != 0) return;
  const long long total = (long long)sh_total;
  const int knew = sh_scan[kCostLanes - 1], znew = sh_znew;
  double D = 0.0, R = 0.0;
  for (int p = 0; p < kCostLanes; ++p) {
    D = __dadd_rn(D, sh_d[p]);
    R = __dadd_rn(R, sh_r[p]);
  }
  const int it = in.iterations[0];
  meta[kMetaIterations] = it + 1;
  meta[kMetaTotal] = total;
  meta[kMetaPinned] = pinned ? z : -1;
  if (total == 0) {                          // every row NaN: nothing to fit
    meta[kMetaMode] = kModeNothing;
    meta[kMetaK] = in.k[0];
    meta[kMetaZero] = z;
    meta[kMetaActive] = 0;
    for (int c = 0; c < 3; ++c) part.cost[c] = nan_f64();
    return;
  }
  const double J = lambda == 0.0 ? D : __dadd_rn(D, __dmul_rn(lambda, R));
  const double J_prev = in.cost[0];
  const bool done =
      it > 0 && __dsub_rn(J_prev, J) <= __dmul_rn(epsilon, J_prev);
  meta[kMetaMode] = kModeStep;
  meta[kMetaKnew] = knew;
  meta[kMetaK] = knew;
  meta[kMetaZero] = znew;
  meta[kMetaActive] = done ? 0 : 1;
  part.cost[0] = J;
  part.cost[1] = D;
  part.cost[2] = R;
}

// One thread per element of the (kmax, d) codebook; the threads of component 0
// also write the slot's length and count, the first thread the scalars.
__global__ void __launch_bounds__(kThreads)
vql_update_kernel(vtc_vq_state in, vtc_vq_state out, VqLargeLayout part,
                  int64_t chunks, int d, int kmax) {
  const long long* meta = part.meta;
  const int mode = (int)meta[kMetaMode];
  const int e = blockIdx.x * kThreads + threadIdx.x;   // kmax * d < 2^31
  if (e == 0) {
    out.k[0] = (int)meta[kMetaK];
    out.zero_index[0] = (int)meta[kMetaZero];
    out.active[0] = (int)meta[kMetaActive];
    out.iterations[0] = (int)meta[kMetaIterations];
    for (int c = 0; c < 3; ++c) out.cost[c] = part.cost[c];
  }
  if (e >= kmax * d) return;
  const int p = e / d, t = e - p * d;
  if (mode != kModeStep) {                   // every slot onto itself
    out.codebook[e] = in.codebook[e];
    if (t == 0) {
      out.lengths[p] = in.lengths[p];
      out.counts[p] = in.counts[p];
    }
    return;
  }
  const int knew = (int)meta[kMetaKnew];
  if (p >= knew) {
    out.codebook[e] = 0.0;   // never read: finite, for a caller's checks
    if (t == 0) {
      out.lengths[p] = 0.0;
      out.counts[p] = 0;
    }
    return;
  }
  const int i = part.source[p];
  const long long n = part.members[p];
  double value = 0.0;
  if (i != (int)meta[kMetaPinned]) {
    double sum = 0.0;
    for (int64_t c = 0; c < chunks; ++c) {
      const int at = place_of(part.cell + c * kRows, part.listed[c], i);
      if (at >= 0) sum = __dadd_rn(sum, part.sum[(c * kRows + at) * d + t]);
    }
    value = __ddiv_rn(sum, (double)n);
  }
  out.codebook[e] = value;
  if (t == 0) {
    const double total = (double)meta[kMetaTotal];
    out.lengths[p] = n > 0 ? -log2(__ddiv_rn((double)n, total)) : inf_f64();
    out.counts[p] = n;
  }
}

__global__ void __launch_bounds__(kThreads)
vql_zero_counts_kernel(int64_t* __restrict__ counts, int kmax) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < kmax) counts[i] = 0;
}

// Integer counts: blockIdx.x a block of rows, blockIdx.y a window of 4096
// cells; an LDS histogram of the window, then integer atomics.
__global__ void __launch_bounds__(kThreads)
vql_index_counts_kernel(const int* __restrict__ indices, int64_t b, int kmax,
                        int64_t* __restrict__ counts) {
  __shared__ unsigned cnt[kCountWindow];
  const int w0 = blockIdx.y * kCountWindow;
  const int cells = kmax - w0 < kCountWindow ? kmax - w0 : kCountWindow;
  for (int i = threadIdx.x; i < cells; i += kThreads) cnt[i] = 0u;
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * kCountRows;
  const int64_t r1 = r0 + kCountRows < b ? r0 + kCountRows : b;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += kThreads) {
    const int i = indices[r] - w0;
    if (i >= 0 && i < cells) atomicAdd(&cnt[i], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cells; i += kThreads) {
    const unsigned v = cnt[i];
    if (v)
      atomicAdd(reinterpret_cast<unsigned long long*>(counts) + w0 + i,
                (unsigned long long)v);
  }
}

// ---- argument checks --------------------------------------------------------
int check_shape(const char* who, int64_t b, int32_t d, int32_t kmax) {
  VTC_REQUIRE(b >= 1, "%s: bad size b = %lld", who, (long long)b);
  VTC_REQUIRE(d >= 1, "%s: bad size d = %d", who, d);
  VTC_REQUIRE(kmax >= 1, "%s: bad size kmax = %d", who, kmax);
  if (d > kMaxDim) {
    set_error("%s: d = %d, at most %d", who, d, kMaxDim);
    return VTC_ERR_UNSUPPORTED;
  }
  if (kmax > kLargeMaxCodewords) {
    set_error("%s: kmax = %d, at most %d", who, kmax, kLargeMaxCodewords);
    return VTC_ERR_UNSUPPORTED;
  }
  VTC_REQUIRE(ceil_div(b, kThreads) <= kMaxGrid, "%s: vectors too large", who);
  return VTC_OK;
}

bool state_complete(const vtc_vq_state* st) {
  return st && st->codebook && st->lengths && st->counts && st->cost &&
         st->k && st->zero_index && st->active && st->iterations;
}

}  // namespace
}  // namespace vtc

using namespace vtc;

extern "C" int vtc_vq_large_abi_version(void) {
  return VTC_VQ_LARGE_ABI_VERSION;
}

// ------------------------------------------------------------------- assign
extern "C" int vtc_vq_large_assign(const float* vectors, int64_t b, int32_t d,
                                   const double* codebook,
                                   const double* lengths, const int32_t* k,
                                   int32_t kmax, double lambda,
                                   int32_t* indices, float* dequantized,
                                   int64_t* status, void* stream) {
  const char* who = "vtc_vq_large_assign";
  VTC_REQUIRE(vectors && codebook && k && indices && status,
              "%s: null pointer", who);
  if (int rc = check_shape(who, b, d, kmax)) return rc;
  VTC_REQUIRE(lambda >= 0.0, "%s: bad lambda = %g", who, lambda);
  VTC_REQUIRE(lengths || lambda == 0.0, "%s: null pointer (lengths)", who);
  hipStream_t st = as_stream(stream);
  zero_status_kernel<<<1, 1, 0, st>>>(status);
  VTC_LAUNCH_CHECK();
  launch_assign(vectors, b, d, codebook, lengths, k, kmax, lambda, nullptr,
                indices, dequantized, nullptr, status, st);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

// --------------------------------------------------------------- Lloyd step
extern "C" size_t vtc_vq_large_lloyd_step_workspace_bytes(int64_t b, int32_t d,
                                                          int32_t kmax) {
  if (b < 1 || d < 1 || d > kMaxDim || kmax < 1 || kmax > kLargeMaxCodewords)
    return 0;
  if (ceil_div(b, kThreads) > kMaxGrid) return 0;
  return measured_bytes<VqLargeLayout>(b, d, kmax);
}

extern "C" int vtc_vq_large_lloyd_step(const float* vectors, int64_t b,
                                       int32_t d, int32_t kmax, double lambda,
                                       double epsilon, int32_t pin_zero,
                                       const vtc_vq_state* in,
                                       const vtc_vq_state* out,
                                       int64_t* status, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  const char* who = "vtc_vq_large_lloyd_step";
  VTC_REQUIRE(vectors && status, "%s: null pointer", who);
  VTC_REQUIRE(state_complete(in), "%s: null pointer (in)", who);
  VTC_REQUIRE(state_complete(out), "%s: null pointer (out)", who);
  if (int rc = check_shape(who, b, d, kmax)) return rc;
  VTC_REQUIRE(lambda >= 0.0, "%s: bad lambda = %g", who, lambda);
  const size_t need = vtc_vq_large_lloyd_step_workspace_bytes(b, d, kmax);
  if (!workspace || workspace_bytes < need) {
    set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
              need);
    return VTC_ERR_WORKSPACE;
  }
  Carver carve(workspace);
  const VqLargeLayout part(carve, b, d, kmax);
  const int64_t chunks = ceil_div(b, kRows);
  hipStream_t st = as_stream(stream);
  zero_status_kernel<<<1, 1, 0, st>>>(status);
  VTC_LAUNCH_CHECK();
  launch_assign(vectors, b, d, in->codebook, in->lengths, in->k, kmax, lambda,
                in->active, part.index, nullptr, part.rowdist, status, st);
  VTC_LAUNCH_CHECK();
#define VTC_VQ_ACCUMULATE(DP)                                        \
  vql_accumulate_kernel<DP><<<(unsigned)chunks, kThreads, 0, st>>>(  \
      vectors, b, d, in->k, kmax, in->active, part)
  VTC_VQ_DISPATCH(d, VTC_VQ_ACCUMULATE);
#undef VTC_VQ_ACCUMULATE
  VTC_LAUNCH_CHECK();
  vql_totals_kernel<<<(unsigned)ceil_div(kmax, kThreads), kThreads, 0, st>>>(
      *in, part, chunks, kmax);
  VTC_LAUNCH_CHECK();
  vql_reduce_kernel<<<1, kCostLanes, 0, st>>>(*in, part, chunks, d, kmax,
                                              lambda, epsilon, pin_zero);
  VTC_LAUNCH_CHECK();
  vql_update_kernel<<<(unsigned)ceil_div((int64_t)kmax * d, kThreads),
                      kThreads, 0, st>>>(*in, *out, part, chunks, d, kmax);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

// ------------------------------------------------------------- index counts
extern "C" int vtc_vq_large_index_counts(const int32_t* indices, int64_t b,
                                         int32_t kmax, int64_t* counts,
                                         void* stream) {
  const char* who = "vtc_vq_large_index_counts";
  VTC_REQUIRE(indices && counts, "%s: null pointer", who);
  if (int rc = check_shape(who, b, 1, kmax)) return rc;
  hipStream_t st = as_stream(stream);
  vql_zero_counts_kernel<<<(unsigned)ceil_div(kmax, kThreads), kThreads, 0,
                           st>>>(counts, kmax);
  VTC_LAUNCH_CHECK();
  const dim3 grid((unsigned)ceil_div(b, kCountRows),
                  (unsigned)ceil_div(kmax, kCountWindow));
  vql_index_counts_kernel<<<grid, kThreads, 0, st>>>(indices, b, kmax, counts);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}
