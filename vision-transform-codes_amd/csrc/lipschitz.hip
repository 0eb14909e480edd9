// Largest eigenvalue of a small symmetric matrix on the device.
//
// The reference takes the ISTA/FISTA step size from
//   torch.symeig(D^T D)[0][-1]        (ista_fista.py:72-80, and the subspace /
//                                      convolutional variants)
// once per plugin call, i.e. once per training step.  A full rocSOLVER
// eigen-decomposition of a 256 x 256 matrix costs ~4 ms on MI355X (measured:
// 5 % of a whole training step).  Only the top eigenvalue is needed, so this is
// a single-workgroup Lanczos iteration followed by sectioning on the
// tridiagonal matrix with Sturm counts in double precision.  n <= 256: the
// matrix lives in registers and the recurrence runs without
// re-orthogonalisation (lanczos_lambda_max_kernel); 256 < n <= 1024: matrix
// streamed from L2, Krylov basis in a global workspace, full
// re-orthogonalisation (lanczos_large_kernel).  128 steps converge to f32
// resolution on the spectra of interest (extreme eigenvalue, Kaniel-Paige).
#include "common.h"

#include <stdlib.h>

namespace vtc {

constexpr int kLanczosMaxN = 256;
constexpr int kLanczosMaxK = 128;

constexpr int kLanczosThreads = 1024;   // 16 waves: 4 per SIMD

// sum over the first 256 threads (the vector components); every thread of the
// block calls this and receives the result
__device__ __forceinline__ double block_sum_vec(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();
  if (threadIdx.x < 256 && (threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// Largest eigenvalue of the symmetric tridiagonal matrix (alpha, beta) of
// order m from Sturm counts, double precision, by ONE WAVE (all 64 lanes call
// it with the same arguments and get the same result): every round each lane
// takes the Sturm count at one of 64 interior points of the bracket, which
// shrinks 65x per round (a one-lane bisection, 50 rounds of an m-long chain of
// divisions at every convergence check, was 1 ms of the 1.1 ms this kernel took).
__device__ double tridiagonal_lambda_max(const double* alpha,
                                         const double* beta, int m) {
  const int lane = threadIdx.x & 63;
  double lo = alpha[0], hi = alpha[0];
  for (int i = 0; i < m; ++i) {
    const double off = (i > 0 ? fabs(beta[i - 1]) : 0.0) +
                       (i + 1 < m ? fabs(beta[i]) : 0.0);
    lo = fmin(lo, alpha[i] - off);
    hi = fmax(hi, alpha[i] + off);
  }
  if (!(hi == hi) || !(lo == lo)) return hi + lo;  // NaN propagates
  // invariant: count(lo) < m <= count(hi), count(x) = #eigenvalues < x
  for (int it = 0; it < 40 && hi - lo > 1e-14 * fmax(fabs(hi), fabs(lo));
       ++it) {
    const double step = (hi - lo) / 65.0;
    const double x = lo + step * (double)(lane + 1);
    int below = 0;
    double d = 1.0;
    for (int i = 0; i < m; ++i) {
      const double off2 = (i > 0) ? beta[i - 1] * beta[i - 1] : 0.0;
      d = (alpha[i] - x) - (i > 0 ? off2 / d : 0.0);
      if (d == 0.0) d = -1e-300;
      if (d < 0.0) ++below;
    }
    // the lanes whose point is above the top eigenvalue form a suffix
    const unsigned long long above = __ballot(below == m);
    if (above == 0ull) {
      lo = lo + step * 64.0;
    } else {
      const int first = __ffsll((long long)above) - 1;
      const double new_hi = lo + step * (double)(first + 1);
      if (first > 0) lo = lo + step * (double)first;
      hi = new_hi;
    }
  }
  return 0.5 * (lo + hi);
}

// Sectioning for the n <= 256 kernel: the first four waves (one per SIMD) take
// 256 points per round, the bracket shrinks 257x per round.  The Sturm count
// comes from the three-term recurrence of the characteristic polynomials
//   p_i = (alpha_i - x) p_{i-1} - beta_{i-1}^2 p_{i-2},
// count(x) = number of sign changes along p_0..p_m, which has no division in
// its dependency chain (an f64 divide is ~40 instructions; here a row costs
// three f64 operations and an integer sign test).  Rows go in chunks of 8 --
// their coefficients are fetched from LDS together, ahead of the chain -- and
// the pair (p, p_prev) is rescaled by a power of two after every chunk so that
// neither overflows.  alpha / beta2 are padded to a multiple of 8 rows with
// (alpha = x-independent huge, beta2 = 0), which adds no sign change.  Every
// thread of the block calls it and gets the same result.
__device__ double tridiagonal_lambda_max_block(const double* alpha,
                                               const double* beta2, int m,
                                               double lo, double hi,
                                               int rounds, int* scratch) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (!(hi == hi) || !(lo == lo)) return hi + lo;  // NaN propagates
  // invariant: count(lo) < m <= count(hi), count(x) = #eigenvalues < x
  for (int it = 0; it < rounds; ++it) {
    const double step = (hi - lo) / 257.0;
    if (wave < 4) {
      const double x = lo + step * (double)(tid + 1);
      double p_prev = 0.0, p = 1.0;     // p_{-1}, p_0
      int below = 0;
      for (int i0 = 0; i0 < m; i0 += 8) {
        double al[8], b2[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          al[q] = alpha[i0 + q];
          b2[q] = (i0 + q > 0) ? beta2[i0 + q - 1] : 0.0;
        }
        // rows past m are padded by the caller with alpha = 1e30, beta2 = 0:
        // p keeps its sign there, so they add no sign change
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const double pn = fma(al[q] - x, p, -b2[q] * p_prev);
          below += ((__double2hiint(pn) ^ __double2hiint(p)) >> 31) & 1;
          p_prev = p;
          p = pn;
        }
        const int e = ilogb(p);
        p = ldexp(p, -e);
        p_prev = ldexp(p_prev, -e);
      }
      // the threads whose point is above the top eigenvalue form a suffix
      const unsigned long long above = __ballot(below == m);
      if (lane == 0)
        scratch[wave] =
            above ? 64 * wave + (__ffsll((long long)above) - 1) : 256;
    }
    __syncthreads();
    int first = 256;
    for (int w = 0; w < 4; ++w) first = scratch[w] < first ? scratch[w] : first;
    __syncthreads();
    if (first == 256) {
      lo = lo + step * 256.0;
    } else {
      const double new_hi = lo + step * (double)(first + 1);
      if (first > 0) lo = lo + step * (double)first;
      hi = new_hi;
    }
  }
  return 0.5 * (lo + hi);
}

// True when every eigenvalue of the leading m x m block of the tridiagonal
// matrix lies below x (Sturm count == m), by the division-free polynomial
// recurrence above; every thread evaluates the same point.  Used once per
// solve for the convergence test, so it is a plain loop.
__device__ bool tridiagonal_all_below(const double* alpha, const double* beta2,
                                      int m, double x) {
  double p_prev = 0.0, p = 1.0;
  int below = 0;
  for (int i = 0; i < m; ++i) {
    const double b2 = i > 0 ? beta2[i - 1] : 0.0;
    const double pn = fma(alpha[i] - x, p, -b2 * p_prev);
    below += ((__double2hiint(pn) ^ __double2hiint(p)) >> 31) & 1;
    p_prev = p;
    p = pn;
    if ((i & 7) == 7) {
      const int e = ilogb(p);
      p = ldexp(p, -e);
      p_prev = ldexp(p_prev, -e);
    }
  }
  return below == m;
}

// Wave-wide sums on the DPP network (row shifts, then the two row broadcasts):
// a handful of VALU instructions, where __shfl_xor goes through ds_bpermute at
// an LDS round trip per stage -- this kernel is one workgroup running a chain
// of dependent phases, so every such latency is exposed.  The total is
// returned to all lanes.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_shift(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, true);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_shift(double v) {
  const int lo = dpp_shift<CTRL, ROW_MASK>(__double2loint(v));
  const int hi = dpp_shift<CTRL, ROW_MASK>(__double2hiint(v));
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double dpp_wave_sum(double v) {
  v += dpp_shift<0x111, 0xf>(v);   // row_shr:1
  v += dpp_shift<0x112, 0xf>(v);   // row_shr:2
  v += dpp_shift<0x114, 0xf>(v);   // row_shr:4
  v += dpp_shift<0x118, 0xf>(v);   // row_shr:8   lane 15 of a row = row sum
  v += dpp_shift<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
  v += dpp_shift<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), 63);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), 63);
  return __hiloint2double(hi, lo);
}

// 1 / sqrt(x) in f64 from the f32 hardware estimate and two Newton steps (an
// IEEE f64 sqrt or divide is a ~40-instruction dependent chain, and this
// kernel would run three of them per Lanczos step on its critical path).
__device__ __forceinline__ double fast_rsqrt(double x) {
  double r = (double)__frsqrt_rn((float)x);
  r = r * (1.5 - 0.5 * x * r * r);
  r = r * (1.5 - 0.5 * x * r * r);
  return r;
}

// n <= 256: the plain Lanczos three-term recurrence, 512 threads.
//
// Thread (q, cp) keeps rows [64 q, 64 q + 64) of the column pair (2 cp,
// 2 cp + 1) of the symmetric matrix in REGISTERS for the whole iteration: the
// matrix is read from memory once (a single workgroup re-streaming 256 KiB from
// L2 per step was 2 us of every step).  One step = mat-vec (64 packed FMAs per
// thread against 16 broadcast LDS reads of v_j), alpha_j = <w, v_j>,
// w -= alpha_j v_j + beta_{j-1} v_{j-1}, beta_j = ||w||: two barriers.  No re-orthogonalisation: only the TOP
// eigenvalue is wanted, and the extreme Ritz value of the three-term
// recurrence converges to it regardless of the loss of orthogonality among the
// Lanczos vectors (which only breeds copies of already converged Ritz values);
// what full re-orthogonalisation cost was five more block-wide phases per
// step, each an LDS round trip plus a 16-wave barrier (measured: 6300 cycles
// per step against 2600 here).  min(96, 2n) steps; measured against LAPACK on
// dictionary Grams of every shape in tests/test_lipschitz_gpu.py: <= 4e-7.
constexpr int kLzThreads = 512;
constexpr int kLzMaxSteps = 256;   // upper end of the step count (arrays)
constexpr int kLzExtend = 16;      // steps added when the test below fails
constexpr int kLzLookBack = 8;
// Agreement asked of the two Ritz values.  The Lanczos vectors are f32 (and
// normalised with an f32 reciprocal), so the tridiagonal entries -- and with
// them every Ritz value -- carry noise of a few 2^-24 relative (measured
// against LAPACK: <= 4e-7; a 1e-7 test called converged 8 x 8 runs
// unconverged).
constexpr double kLzAgree = 1e-6;

template <bool STAMP>
__global__ __launch_bounds__(kLzThreads) void lanczos_lambda_max_kernel(
    const float* __restrict__ G, int n, int k, int k_cap,
    float* __restrict__ out, float* __restrict__ mirror) {
  __shared__ __attribute__((aligned(16))) float vcur[256];  // b_{j-1} v_j
  __shared__ __attribute__((aligned(16))) float partial[4][256];
  __shared__ double red_a[8], red_b[4];
  __shared__ double alpha[kLzMaxSteps + 8];
  __shared__ double beta[kLzMaxSteps + 8];
  __shared__ double beta2[kLzMaxSteps + 8];
  __shared__ int scratch[4];
  unsigned long long st_t0 = 0, st_acc[4] = {0, 0, 0, 0};
#define LZ_STAMP(slot)                                                   \
  if (STAMP) {                                                           \
    unsigned long long now_;                                             \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now_)::"memory"); \
    st_acc[slot] += now_ - st_t0;                                        \
    st_t0 = now_;                                                        \
  }
  const int tid = threadIdx.x;
  const int t = tid & 255, half = tid >> 8;
  const int lane = tid & 63, wave = tid >> 6;   // 8 waves
  const bool on = t < n;
  const bool owner = (half == 0);

  // mat-vec layout: thread (q, cp) holds rows [64 q, 64 q + 64) of the column
  // pair (2 cp, 2 cp + 1): 64 broadcast reads of v per thread instead of 128,
  // and the products as packed f32 FMAs (v_pk_fma_f32: two columns per
  // instruction)
  const int q = tid >> 7, cp = tid & 127;
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  f32x2 g[64];
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    const int row = 64 * q + i;
    const int r_ok = row < n ? row : 0;
    const float x0 = G[(size_t)r_ok * n + (2 * cp < n ? 2 * cp : 0)];
    const float x1 = G[(size_t)r_ok * n + (2 * cp + 1 < n ? 2 * cp + 1 : 0)];
    g[i][0] = (row < n && 2 * cp < n) ? x0 : 0.f;
    g[i][1] = (row < n && 2 * cp + 1 < n) ? x1 : 0.f;
  }

  // deterministic, generic start vector (components past n are zero)
  {
    float v = 0.f;
    if (on) {
      unsigned x = (unsigned)t * 2654435761u + 12345u;
      x ^= x >> 13; x *= 0x5bd1e995u; x ^= x >> 15;
      v = 0.5f + (float)(x & 0xffff) / 65536.f;
    }
    const double ps = dpp_wave_sum(owner ? (double)v * v : 0.0);
    if (owner && lane == 0) red_b[wave] = ps;
    if (owner) vcur[t] = v;
  }
  // padding rows of the tridiagonal matrix (see the solver): every row is a
  // padding row until the recurrence overwrites it
  for (int i = tid; i < kLzMaxSteps + 8; i += kLzThreads) {
    alpha[i] = 1e30;
    beta2[i] = 0.0;
  }
  __syncthreads();
  double b2 = (red_b[0] + red_b[1]) + (red_b[2] + red_b[3]);
  double rb = fast_rsqrt(b2);
  double b = b2 * rb;
  double tscale = 0.0, beta_prev = 0.0;
  float v_prev = 0.f;
  int steps = 0;
  if (STAMP)
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_t0)::"memory");

  // A Ritz value approaches lambda_max from below, so a fixed step count
  // could hand back eta > 1 / L without a sign of it.  After the first
  // `k` steps -- and after every kLzExtend more -- the top Ritz value of all
  // steps is compared with that of the steps up to kLzLookBack earlier; the
  // recurrence goes on (to at most k_cap steps) while they differ by more
  // than kLzAgree relative, and the verdict is written next to the eigenvalue.
  int target = k, j = 0;
  bool exhausted = false, converged = false;
  double lambda = 0.0;
  for (;;) {
  for (; j < target; ++j) {
    const float inv_b = (float)rb;
    const float vt = vcur[t] * inv_b;        // component t of v_j
    // ---- [A] w = G v_j: this thread's 64 rows of its two columns, and this
    // wave's share of <w, v_j>
    {
      const float4* v4 = reinterpret_cast<const float4*>(vcur + 64 * q);
      f32x2 acc0 = {0.f, 0.f}, acc1 = {0.f, 0.f}, acc2 = {0.f, 0.f},
            acc3 = {0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float4 x = v4[i];
        acc0 = __builtin_elementwise_fma(g[4 * i + 0], (f32x2){x.x, x.x}, acc0);
        acc1 = __builtin_elementwise_fma(g[4 * i + 1], (f32x2){x.y, x.y}, acc1);
        acc2 = __builtin_elementwise_fma(g[4 * i + 2], (f32x2){x.z, x.z}, acc2);
        acc3 = __builtin_elementwise_fma(g[4 * i + 3], (f32x2){x.w, x.w}, acc3);
      }
      const f32x2 pw = ((acc0 + acc1) + (acc2 + acc3)) * inv_b;
      *reinterpret_cast<f32x2*>(&partial[q][2 * cp]) = pw;
      const f32x2 vv = *reinterpret_cast<const f32x2*>(vcur + 2 * cp);
      const double pa = dpp_wave_sum((double)pw[0] * (double)(vv[0] * inv_b) +
                                     (double)pw[1] * (double)(vv[1] * inv_b));
      if (lane == 0) red_a[wave] = pa;
    }
    __syncthreads();
    LZ_STAMP(0)
    // ---- [B] w -= alpha_j v_j + beta_{j-1} v_{j-1};  ||w||^2
    float w = (partial[0][t] + partial[1][t]) + (partial[2][t] + partial[3][t]);
    double a = 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u) a += red_a[u];
    w = w - (float)a * vt - (float)beta_prev * v_prev;
    {
      const double pb = dpp_wave_sum(owner ? (double)w * w : 0.0);
      if (owner && lane == 0) red_b[wave] = pb;
      if (owner) vcur[t] = w;      // every mat-vec read of v_j is behind us
    }
    v_prev = vt;
    __syncthreads();
    LZ_STAMP(1)
    b2 = (red_b[0] + red_b[1]) + (red_b[2] + red_b[3]);
    rb = fast_rsqrt(b2);
    b = b2 * rb;                      // 0 * inf = NaN for b2 == 0: stops below
    if (tid == 0) {
      alpha[j] = a;
      beta[j] = b2 > 0.0 ? b : 0.0;
      beta2[j] = b2;
    }
    steps = j + 1;
    tscale = fmax(tscale, fmax(fabs(a), b));
    // Krylov space exhausted (rank-deficient Gram, invariant subspace) or a
    // NaN: what is left of w is rounding noise -- normalising it would feed
    // amplified garbage into the recurrence.  The tridiagonal matrix so far
    // already holds the spectrum of the reachable space.
    if (!(b > 1e-5 * tscale)) {
      exhausted = true;
      break;
    }
    beta_prev = b;
  }
  __syncthreads();
  double lo = alpha[0], hi = alpha[0];
  for (int i = 0; i < steps; ++i) {
    const double off = (i > 0 ? beta[i - 1] : 0.0) +
                       (i + 1 < steps ? beta[i] : 0.0);
    lo = fmin(lo, alpha[i] - off);
    hi = fmax(hi, alpha[i] + off);
  }
  LZ_STAMP(2)
  // 257^4 = 4.4e9 sections of a bracket a few lambda wide: below f32 resolution
  const double coupling = beta2[steps - 1];
  __syncthreads();
  if (tid == 0) beta2[steps - 1] = 0.0;   // no coupling into the padding rows
  __syncthreads();
  lambda = tridiagonal_lambda_max_block(alpha, beta2, steps, lo, hi, 4, scratch);
  // converged: the Krylov space is exhausted (the tridiagonal matrix holds the
  // whole reachable spectrum), or the steps up to kLzLookBack ago already had
  // a Ritz value within kLzAgree of this one
  converged = exhausted ||
              (steps > kLzLookBack &&
               !tridiagonal_all_below(alpha, beta2, steps - kLzLookBack,
                                      lambda - kLzAgree * fabs(lambda)));
  if (converged || !(lambda == lambda) || steps >= k_cap) break;
  __syncthreads();
  if (tid == 0) beta2[steps - 1] = coupling;
  {
    const int more = steps / 2 > kLzExtend ? steps / 2 : kLzExtend;
    target = steps + more < k_cap ? steps + more : k_cap;
  }
  __syncthreads();
  }
  const float lf = (float)lambda;
  LZ_STAMP(3)
  if (tid == 0) {
    const float flag = converged ? 1.f : 0.f;
    out[0] = lf;
    out[1] = 1.f / lf;  // the reference's `1. / lipschitz_constant` in f32
    out[2] = flag;
    if (mirror) {       // host-visible copy for the caller's error channel
      mirror[0] = lf;
      mirror[1] = 1.f / lf;
      mirror[2] = flag;
    }
    if (STAMP)
      for (int q = 0; q < 4; ++q) out[3 + q] = (float)st_acc[q];
  }
#undef LZ_STAMP
}

// ---------------------------------------------------------------- n > 256
// Same iteration for 256 < n <= 1024 (e.g. 20x20 or 32x32 patches): one
// thread per vector component, the Krylov basis (k x n floats, up to 512 KiB)
// in a global workspace instead of LDS.  ~2 ms at n = 1024, once per call.
constexpr int kLanczosLargeN = 1024;

__device__ __forceinline__ double block_sum_all(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double total = 0.0;
  for (int w = 0; w < kLanczosThreads / 64; ++w) total += red[w];
  return total;
}

__global__ __launch_bounds__(kLanczosThreads) void lanczos_large_kernel(
    const float* __restrict__ G, int n, int k, float* __restrict__ V,
    float* __restrict__ out, float* __restrict__ mirror) {
  __shared__ float vcur[kLanczosLargeN];
  __shared__ float wl[kLanczosLargeN];
  __shared__ float coef[kLanczosMaxK];
  __shared__ double red[kLanczosThreads / 64];
  __shared__ double alpha[kLanczosMaxK];
  __shared__ double beta[kLanczosMaxK];
  __shared__ int steps_done;
  __shared__ int stop_flag, loose_flag;
  __shared__ double last_ritz;
  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const bool on = t < n;

  float v = 0.f;
  if (on) {
    unsigned x = (unsigned)t * 2654435761u + 12345u;
    x ^= x >> 13; x *= 0x5bd1e995u; x ^= x >> 15;
    v = 0.5f + (float)(x & 0xffff) / 65536.f;
  }
  const double nrm = sqrt(block_sum_all((double)v * v, red));
  v = (float)(v / nrm);
  float v_prev = 0.f;
  double beta_prev = 0.0;
  if (t == 0) {
    steps_done = k;
    stop_flag = 0;
    loose_flag = 0;
    last_ritz = -1.0;
  }
  double tscale = 0.0;
  __syncthreads();

  for (int j = 0; j < k; ++j) {
    if (on) {
      V[(size_t)j * n + t] = v;
      vcur[t] = v;
    }
    __syncthreads();
    // w = G v: G symmetric, so "column" t is read along rows, coalesced
    float w = 0.f;
    if (on) {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      int i = 0;
      for (; i + 3 < n; i += 4) {
        a0 = fmaf(G[(size_t)(i + 0) * n + t], vcur[i + 0], a0);
        a1 = fmaf(G[(size_t)(i + 1) * n + t], vcur[i + 1], a1);
        a2 = fmaf(G[(size_t)(i + 2) * n + t], vcur[i + 2], a2);
        a3 = fmaf(G[(size_t)(i + 3) * n + t], vcur[i + 3], a3);
      }
      for (; i < n; ++i) a0 = fmaf(G[(size_t)i * n + t], vcur[i], a0);
      w = (a0 + a1) + (a2 + a3);
    }
    const double a = block_sum_all(on ? (double)w * v : 0.0, red);
    if (on) {
      w = w - (float)a * v - (float)beta_prev * v_prev;
      wl[t] = w;
    }
    __threadfence_block();
    __syncthreads();
    // full re-orthogonalisation against V[0..j] (this block wrote them)
    for (int i = wave; i <= j; i += kLanczosThreads / 64) {
      float p = 0.f;
      for (int c = lane; c < n; c += 64) p = fmaf(V[(size_t)i * n + c], wl[c], p);
      p = wave_sum(p);
      if (lane == 0) coef[i] = p;
    }
    __syncthreads();
    if (on) {
      float corr = 0.f;
      for (int i = 0; i <= j; ++i) corr = fmaf(coef[i], V[(size_t)i * n + t], corr);
      w -= corr;
    }
    const double b = sqrt(block_sum_all(on ? (double)w * w : 0.0, red));
    if (t == 0) {
      alpha[j] = a;
      beta[j] = b;
    }
    tscale = fmax(tscale, fmax(fabs(a), b));
    if (!(b > 1e-5 * tscale)) {
      if (t == 0) steps_done = j + 1;
      break;
    }
    if ((j & 7) == 7) {
      __syncthreads();
      if (wave == 0) {
        const double ritz = tridiagonal_lambda_max(alpha, beta, j + 1);
        if (t == 0) {
          stop_flag = (last_ritz > 0.0 &&
                       fabs(ritz - last_ritz) <= 2e-8 * fabs(ritz)) ? 1 : 0;
          loose_flag = (last_ritz > 0.0 &&
                        fabs(ritz - last_ritz) <= kLzAgree * fabs(ritz)) ? 1 : 0;
          last_ritz = ritz;
        }
      }
      __syncthreads();
      if (stop_flag) {
        if (t == 0) steps_done = j + 1;
        break;
      }
    }
    v_prev = v;
    v = (float)(w / b);
    beta_prev = b;
  }
  __syncthreads();
  if (wave == 0) {
    const double lambda = tridiagonal_lambda_max(alpha, beta, steps_done);
    const float lf = (float)lambda;
    if (t == 0) {
      // converged: stopped by the test above, Krylov space exhausted (the
      // last coupling vanished), or the latest of the 8-step comparisons
      // within kLzAgree
      const bool ok = stop_flag || steps_done < k || loose_flag;
      const float flag = ok ? 1.f : 0.f;
      out[0] = lf;
      out[1] = 1.f / lf;
      out[2] = flag;
      if (mirror) {
        mirror[0] = lf;
        mirror[1] = 1.f / lf;
        mirror[2] = flag;
      }
    }
  }
}

// Scratch of the large-matrix Lanczos kernel: its basis vectors
struct LanczosLayout {
  float* basis;
  LanczosLayout(Carver& ws, int64_t n) {
    basis = ws.take<float>((size_t)kLanczosMaxK * n);
  }
};

}  // namespace vtc

using namespace vtc;

extern "C" size_t vtc_lambda_max_workspace_bytes(int64_t n) {
  if (n <= kLanczosMaxN || n > kLanczosLargeN) return 256;
  return measured_bytes<LanczosLayout>(n);
}

// out: 3 floats on the device: [lambda_max, 1/lambda_max, converged (1 / 0)]
static int lambda_max_impl(const float* symmetric, int64_t n, float* out,
                           float* mirror, void* workspace,
                           size_t workspace_bytes, void* stream) {
  VTC_REQUIRE(symmetric && out, "vtc_lambda_max: null pointer");
  VTC_REQUIRE(n > 0, "vtc_lambda_max: bad size");
  if (n > kLanczosLargeN) {
    set_error("vtc_lambda_max: n = %lld exceeds the single-workgroup Lanczos "
              "limit of %d", (long long)n, kLanczosLargeN);
    return VTC_ERR_UNSUPPORTED;
  }
  const int k = (int)(n < kLanczosMaxK ? n : kLanczosMaxK);
  if (n > kLanczosMaxN) {
    if (!workspace || workspace_bytes < vtc_lambda_max_workspace_bytes(n)) {
      set_error("vtc_lambda_max: workspace too small");
      return VTC_ERR_WORKSPACE;
    }
    Carver ws(workspace);
    hipLaunchKernelGGL(lanczos_large_kernel, dim3(1), dim3(kLanczosThreads), 0,
                       as_stream(stream), symmetric, (int)n, k,
                       LanczosLayout(ws, n).basis, out, mirror);
    VTC_LAUNCH_CHECK();
    return VTC_OK;
  }
  // diagnostic: VTC_LANCZOS_STAMPS=1 and an `out` of 7 floats -> cycles per
  // phase in out[3..6] (A mat-vec, B update, bounds, tridiagonal solve)
  static const bool stamps = getenv("VTC_LANCZOS_STAMPS") != nullptr;
  // 96 steps: on every spectrum tried (dictionary Grams of all shapes in the
  // tests, clustered tops) the top Ritz value is within 2e-7 of LAPACK's
  // eigenvalue from step ~80 on; beyond convergence more steps only add
  // rounding noise from the copies of converged Ritz values
  // (the kernel checks that itself and goes on, kLzExtend steps at a time up
  // to k_cap = min(2n, kLzMaxSteps), while the value still moves)
  // Small matrices get n + 16 steps (steps past n only breed copies of
  // converged Ritz values), so that the look-back comparison has a converged
  // prefix to look at.
  // Round 3: the kernel reports convergence itself, so the first look comes at
  // 32 steps (random-dictionary Gram matrices of 256 to 1024 atoms have
  // converged by 24 to 48: 7e-9 from the float64 value) and later ones after
  // half as many steps again, at least 16 -- 32, 48, 72, 108, 162, 243 --,
  // each costing one sectioning pass (18 us).
  constexpr int kSteps = 32;
  const int64_t want = 2 * n > n + 16 ? 2 * n : n + 16;
  const int64_t most = 2 * n > n + 48 ? 2 * n : n + 48;
  int k_small = (int)(want < kSteps ? want : kSteps);
  int k_cap = (int)(most < kLzMaxSteps ? most : kLzMaxSteps);
  // test hook: VTC_LANCZOS_MAX_STEPS caps both (an unconverged solve on demand)
  static const int forced_cap = getenv("VTC_LANCZOS_MAX_STEPS")
                                    ? atoi(getenv("VTC_LANCZOS_MAX_STEPS")) : 0;
  if (forced_cap > 0) {
    k_cap = forced_cap < k_cap ? forced_cap : k_cap;
    k_small = k_small < k_cap ? k_small : k_cap;
  }
  if (stamps)
    hipLaunchKernelGGL(lanczos_lambda_max_kernel<true>, dim3(1),
                       dim3(kLzThreads), 0, as_stream(stream), symmetric,
                       (int)n, k_small, k_cap, out, mirror);
  else
    hipLaunchKernelGGL(lanczos_lambda_max_kernel<false>, dim3(1),
                       dim3(kLzThreads), 0, as_stream(stream), symmetric,
                       (int)n, k_small, k_cap, out, mirror);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" int vtc_lambda_max(const float* symmetric, int64_t n, float* out,
                              void* workspace, size_t workspace_bytes,
                              void* stream) {
  return lambda_max_impl(symmetric, n, out, nullptr, workspace,
                         workspace_bytes, stream);
}

extern "C" int vtc_lambda_max_mirrored(const float* symmetric, int64_t n,
                                       float* out, float* host_mirror,
                                       void* workspace,
                                       size_t workspace_bytes, void* stream) {
  return lambda_max_impl(symmetric, n, out, host_mirror, workspace,
                         workspace_bytes, stream);
}
