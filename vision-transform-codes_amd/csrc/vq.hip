// Vector quantiser (include/vtc_vq.h): entropy-constrained assignment of
// d-vectors to one codebook, and one Lloyd step with its convergence test on
// the device.  DESIGN.md 4.16 states the contract, the order of the sums and
// the LDS and register budgets.
//
//   vtc_vq_assign      zero_status_kernel, vq_assign_kernel
//   vtc_vq_lloyd_step  zero_status_kernel, vq_assign_kernel,
//                      vq_accumulate_kernel, vq_reduce_kernel, vq_update_kernel
//   vtc_vq_index_counts  vq_zero_counts_kernel, vq_index_counts_kernel
//
// vq_assign_kernel (vq_scan.h, shared with vq_large.hip): one row per lane,
// its components converted once to
// float64 and held in registers (DP of them, d rounded up to 4, 8, 16, 24 or
// 32 and padded with 0.0; a padded component adds e * e = 0.0 to a distance,
// which changes no bit of it).  The codebook streams through LDS in tiles of
// 4096 / DP whole codewords, in index order, padded the same way; every lane
// of a wave reads the same codeword element at the same time, an LDS
// broadcast.  The scan is linear: three float64 VALU operations per component
// and cell, and the tie rule is the contract's by construction.
//
// A Lloyd step keeps the index and the squared distance of every row in the
// workspace.  vq_accumulate_kernel, one workgroup per block of 2048 rows,
// stages the block's indices in LDS (int16), counts the members of every cell
// there, and gives every cell that has members in the block to 16 adjacent
// lanes: lane g walks the rows g, g + 16, ... of the block in
// ascending order and adds its members, and the 16 partial sums are added in
// ascending g through wave shuffles, so the many members of the zero cell are
// shared by 16 lanes.  vq_reduce_kernel (one workgroup) adds the block
// partials of the counts and distances, forms the cost, the convergence test
// and the new slot of every kept cell; vq_update_kernel, one thread per
// element of the new codebook, adds the block partials of the sums in
// ascending block order and writes the state.  Only vq_update_kernel writes
// `out`, and it reads `in` only where it copies a slot onto itself, so a step
// in place is safe.
#include "vq_scan.h"

#include <cmath>

namespace vtc {
namespace {

constexpr int kMaxCodewords = VTC_VQ_MAX_CODEWORDS;
constexpr int kRows = VTC_VQ_ROWS;
constexpr int kLanes = VTC_VQ_LANES;
constexpr int kCostLanes = VTC_VQ_COST_LANES;
constexpr int kWave = 64;
constexpr int kCountRows = 4096;              // rows of one index_counts block

static_assert(kMaxCodewords <= 32767, "the staged indices are int16");
static_assert(kWave % kLanes == 0 && kThreads % kWave == 0,
              "the lanes of one cell sit in one wave");
static_assert(kTileDoubles / 4 <= kMaxCodewords, "a tile holds whole codewords");
static_assert(kMaxCodewords % kCostLanes == 0 && kCostLanes <= 1024, "");

// the records of a step that vq_reduce_kernel leaves for vq_update_kernel
enum { kModeFrozen = 0, kModeNothing = 1, kModeStep = 2 };
enum { kMetaMode, kMetaKnew, kMetaTotal, kMetaPinned, kMetaK, kMetaZero,
       kMetaActive, kMetaIterations, kMetaInts };

struct VqLayout {
  int* index;            // [b]
  double* rowdist;       // [b]
  double* sum;           // [chunks][kmax][d]
  double* dist;          // [chunks][kmax]
  int* count;            // [chunks][kmax]
  long long* members;    // [kmax], by new slot
  int* source;           // [kmax], the cell a new slot comes from
  double* cost;          // [3] (256 bytes)
  long long* meta;       // [kMetaInts] (256 bytes)
  VqLayout(Carver& ws, int64_t b, int32_t d, int32_t kmax) {
    const size_t cells = (size_t)ceil_div(b, kRows) * (size_t)kmax;
    index = ws.take<int>((size_t)b);
    rowdist = ws.take<double>((size_t)b);
    sum = ws.take<double>(cells * (size_t)d);
    dist = ws.take<double>(cells);
    count = ws.take<int>(cells);
    members = ws.take<long long>((size_t)kmax);
    source = ws.take<int>((size_t)kmax);
    cost = ws.take<double>(32);
    meta = ws.take<long long>(32);
  }
};

// The per-block sums of a step.  The cells without a member in the block (most
// of them: a block of 2048 rows, nine tenths of them in the zero cell, cannot
// fill thousands of cells) get their zeros at once; only the others are walked.
// The order in which the cells are taken does not matter: every cell's sums are
// its own.  Every lane of the workgroup makes every pass: the shuffles need the
// whole wave.
template <int DP>
__global__ void __launch_bounds__(kThreads)
vq_accumulate_kernel(const float* __restrict__ vectors, int64_t b, int d,
                     const int* __restrict__ k, int kmax,
                     const int* __restrict__ active, VqLayout part) {
  __shared__ short idx[kRows];
  __shared__ int cnt[kMaxCodewords];         // members of every cell in the block
  __shared__ short list[kMaxCodewords];      // the cells with members
  __shared__ int sh_listed;
  if (active[0] == 0) return;
  const int kk = clamp_k(k[0], kmax);
  const int64_t chunk = blockIdx.x;
  const int64_t r0 = chunk * kRows;
  const int rows = (int)(r0 + kRows < b ? kRows : b - r0);
  for (int i = threadIdx.x; i < kk; i += kThreads) cnt[i] = 0;
  if (threadIdx.x == 0) sh_listed = 0;
  __syncthreads();
  for (int q = threadIdx.x; q < rows; q += kThreads) {
    const int cell = part.index[r0 + q];     // r0 + q < b; -1 or < kk
    idx[q] = (short)cell;
    if (cell >= 0 && cell < kk) atomicAdd(&cnt[cell], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kk; i += kThreads) {
    const int64_t at = chunk * kmax + i;
    part.count[at] = cnt[i];
    if (cnt[i] > 0)
      list[atomicAdd(&sh_listed, 1)] = (short)i;   // fewer than kk entries
    else
      part.dist[at] = 0.0;
  }
  for (int e = threadIdx.x; e < kk * d; e += kThreads)
    if (cnt[e / d] == 0) part.sum[chunk * kmax * d + e] = 0.0;
  __syncthreads();

  // kLanes adjacent lanes per listed cell: lane g adds the members among the
  // rows g, g + kLanes, ... in ascending order, then the kLanes partials are
  // added in ascending g.
  const int items = sh_listed * kLanes;
  for (int e0 = 0; e0 < items; e0 += kThreads) {
    const int e = e0 + threadIdx.x;
    const int g = e % kLanes;
    const bool live = e < items;
    const int i = live ? list[e / kLanes] : -2;    // -2 matches no row
    double acc[DP];
#pragma unroll
    for (int t = 0; t < DP; ++t) acc[t] = 0.0;
    double dist = 0.0;
    if (live) {
      for (int q = g; q < rows; q += kLanes) {
        if (idx[q] != (short)i) continue;
        const int64_t row = r0 + q;
#pragma unroll
        for (int t = 0; t < DP; ++t)
          if (t < d) acc[t] = __dadd_rn(acc[t], (double)vectors[row * d + t]);
        dist = __dadd_rn(dist, part.rowdist[row]);
      }
    }
    const int first = (threadIdx.x & (kWave - 1)) - g;   // lane of g = 0
    const int64_t at = chunk * kmax + i;
    double dist_all = __shfl(dist, first);
#pragma unroll
    for (int h = 1; h < kLanes; ++h)
      dist_all = __dadd_rn(dist_all, __shfl(dist, first + h));
#pragma unroll
    for (int t = 0; t < DP; ++t) {
      if (t < d) {                           // d is the same for every lane
        double all = __shfl(acc[t], first);
#pragma unroll
        for (int h = 1; h < kLanes; ++h)
          all = __dadd_rn(all, __shfl(acc[t], first + h));
        if (live && g == 0) part.sum[at * d + t] = all;
      }
    }
    if (live && g == 0) part.dist[at] = dist_all;
  }
}

// One workgroup of kCostLanes threads: counts and distances of every cell over
// the blocks, D, R, J, the convergence test, the new slot of every kept cell.
// Writes the workspace only.
__global__ void __launch_bounds__(kCostLanes)
vq_reduce_kernel(vtc_vq_state in, VqLayout part, int64_t chunks, int d,
                 int kmax, double lambda, double epsilon, int pin_zero) {
  __shared__ long long sh_n[kMaxCodewords];
  __shared__ double sh_d[kCostLanes], sh_r[kCostLanes];
  __shared__ int sh_zero_moved;              // cell z: a new component != 0.0
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
  if (t == 0) sh_zero_moved = 0;
  double d_part = 0.0, r_part = 0.0;
  for (int i = t; i < k0; i += kCostLanes) {
    double dist = 0.0;
    long long n = 0;
    for (int64_t c = 0; c < chunks; ++c) {
      dist = __dadd_rn(dist, part.dist[c * kmax + i]);
      n += part.count[c * kmax + i];
    }
    sh_n[i] = n;
    d_part = __dadd_rn(d_part, dist);
    if (n > 0)
      r_part = __dadd_rn(r_part, __dmul_rn((double)n, in.lengths[i]));
  }
  sh_d[t] = d_part;
  sh_r[t] = r_part;
  __syncthreads();
  // does the codeword of cell z stay the zero vector?  (unpinned: the mean)
  if (!pinned && z >= 0 && z < k0 && t < d && sh_n[z] > 0) {
    double sum = 0.0;
    for (int64_t c = 0; c < chunks; ++c)
      sum = __dadd_rn(sum, part.sum[(c * kmax + z) * d + t]);
    if (__ddiv_rn(sum, (double)sh_n[z]) != 0.0) atomicOr(&sh_zero_moved, 1);
  }
  __syncthreads();
  if (t != 0) return;
  long long total = 0;
  int knew = 0, znew = -1;
  for (int i = 0; i < k0; ++i) {
    const long long n = sh_n[i];
    total += n;
    if (n > 0 || (pinned && i == z)) {
      if (i == z && !sh_zero_moved) znew = knew;
      part.members[knew] = n;                // knew <= i < kmax
      part.source[knew] = i;
      ++knew;
    }
  }
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
vq_update_kernel(vtc_vq_state in, vtc_vq_state out, VqLayout part,
                 int64_t chunks, int d, int kmax) {
  const long long* meta = part.meta;
  const int mode = (int)meta[kMetaMode];
  const int e = blockIdx.x * kThreads + threadIdx.x;   // kmax * d <= 2^17
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
    for (int64_t c = 0; c < chunks; ++c)
      sum = __dadd_rn(sum, part.sum[(c * kmax + i) * d + t]);
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
vq_zero_counts_kernel(int64_t* __restrict__ counts, int kmax) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < kmax) counts[i] = 0;
}

// Integer counts: an LDS histogram per block of rows, then integer atomics.
__global__ void __launch_bounds__(kThreads)
vq_index_counts_kernel(const int* __restrict__ indices, int64_t b, int kmax,
                       int64_t* __restrict__ counts) {
  __shared__ unsigned cnt[kMaxCodewords];
  for (int i = threadIdx.x; i < kmax; i += kThreads) cnt[i] = 0u;
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * kCountRows;
  const int64_t r1 = r0 + kCountRows < b ? r0 + kCountRows : b;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += kThreads) {
    const int i = indices[r];
    if (i >= 0 && i < kmax) atomicAdd(&cnt[i], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kmax; i += kThreads) {
    const unsigned v = cnt[i];
    if (v)
      atomicAdd(reinterpret_cast<unsigned long long*>(counts) + i,
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
  if (kmax > kMaxCodewords) {
    set_error("%s: kmax = %d, at most %d", who, kmax, kMaxCodewords);
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

extern "C" int vtc_vq_abi_version(void) { return VTC_VQ_ABI_VERSION; }

// ------------------------------------------------------------------- assign
extern "C" int vtc_vq_assign(const float* vectors, int64_t b, int32_t d,
                             const double* codebook, const double* lengths,
                             const int32_t* k, int32_t kmax, double lambda,
                             int32_t* indices, float* dequantized,
                             int64_t* status, void* stream) {
  const char* who = "vtc_vq_assign";
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
extern "C" size_t vtc_vq_lloyd_step_workspace_bytes(int64_t b, int32_t d,
                                                    int32_t kmax) {
  if (b < 1 || d < 1 || d > kMaxDim || kmax < 1 || kmax > kMaxCodewords)
    return 0;
  if (ceil_div(b, kThreads) > kMaxGrid) return 0;
  return measured_bytes<VqLayout>(b, d, kmax);
}

extern "C" int vtc_vq_lloyd_step(const float* vectors, int64_t b, int32_t d,
                                 int32_t kmax, double lambda, double epsilon,
                                 int32_t pin_zero, const vtc_vq_state* in,
                                 const vtc_vq_state* out, int64_t* status,
                                 void* workspace, size_t workspace_bytes,
                                 void* stream) {
  const char* who = "vtc_vq_lloyd_step";
  VTC_REQUIRE(vectors && status, "%s: null pointer", who);
  VTC_REQUIRE(state_complete(in), "%s: null pointer (in)", who);
  VTC_REQUIRE(state_complete(out), "%s: null pointer (out)", who);
  if (int rc = check_shape(who, b, d, kmax)) return rc;
  VTC_REQUIRE(lambda >= 0.0, "%s: bad lambda = %g", who, lambda);
  const size_t need = vtc_vq_lloyd_step_workspace_bytes(b, d, kmax);
  if (!workspace || workspace_bytes < need) {
    set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
              need);
    return VTC_ERR_WORKSPACE;
  }
  Carver carve(workspace);
  const VqLayout part(carve, b, d, kmax);
  const int64_t chunks = ceil_div(b, kRows);
  hipStream_t st = as_stream(stream);
  zero_status_kernel<<<1, 1, 0, st>>>(status);
  VTC_LAUNCH_CHECK();
  launch_assign(vectors, b, d, in->codebook, in->lengths, in->k, kmax, lambda,
                in->active, part.index, nullptr, part.rowdist, status, st);
  VTC_LAUNCH_CHECK();
#define VTC_VQ_ACCUMULATE(DP)                                       \
  vq_accumulate_kernel<DP><<<(unsigned)chunks, kThreads, 0, st>>>(  \
      vectors, b, d, in->k, kmax, in->active, part)
  VTC_VQ_DISPATCH(d, VTC_VQ_ACCUMULATE);
#undef VTC_VQ_ACCUMULATE
  VTC_LAUNCH_CHECK();
  vq_reduce_kernel<<<1, kCostLanes, 0, st>>>(*in, part, chunks, d, kmax,
                                             lambda, epsilon, pin_zero);
  VTC_LAUNCH_CHECK();
  vq_update_kernel<<<(unsigned)ceil_div((int64_t)kmax * d, kThreads),
                     kThreads, 0, st>>>(*in, *out, part, chunks, d, kmax);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

// ------------------------------------------------------------- index counts
extern "C" int vtc_vq_index_counts(const int32_t* indices, int64_t b,
                                   int32_t kmax, int64_t* counts,
                                   void* stream) {
  const char* who = "vtc_vq_index_counts";
  VTC_REQUIRE(indices && counts, "%s: null pointer", who);
  if (int rc = check_shape(who, b, 1, kmax)) return rc;
  hipStream_t st = as_stream(stream);
  vq_zero_counts_kernel<<<(unsigned)ceil_div(kmax, kThreads), kThreads, 0,
                          st>>>(counts, kmax);
  VTC_LAUNCH_CHECK();
  vq_index_counts_kernel<<<(unsigned)ceil_div(b, kCountRows), kThreads, 0,
                           st>>>(indices, b, kmax, counts);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}
