// Matrix inverse on the device for the invertible-linear analysis transform
// (analysis_transforms/fully_connected/invertible_linear.py of the reference:
// codes = images @ torch.inverse(dictionary)).
//
// Float64 throughout, rounded once to float32 at the end.  The matrix is
// padded to m = n rounded up to 32 with an identity block, so every panel and
// every trailing block is a whole number of 32-wide (4-wide) tiles; padded
// rows hold zeros in the real columns and are never chosen as pivots.
//
//   phase 1  one workgroup of 1024 threads: right-looking blocked LU with
//            partial pivoting, P A = L U, on a float64 copy in the workspace
//            (L2-resident, 512 KiB at n = 256).  Each 32-column panel is
//            factorised in LDS (pivot: the largest |value|, ties to the lower
//            row), its row interchanges are applied to the other columns,
//            U12 = L11^-1 A12 is solved into LDS and A22 -= L21 U12 is a
//            register-tiled product out of LDS.  ~n^3/3 FMAs.
//   phase 2  A^-1 = U^-1 L^-1 P, kInvCols columns of P per workgroup:
//            forward then backward substitution with one thread per row and
//            the workgroup's right-hand sides in registers; each finished row
//            is broadcast through LDS.  Rows of L and U are read from L2 in
//            32-wide blocks.  No synchronisation between workgroups.
//
// Every sum runs in a fixed order, so two calls give identical bits.
#include "common.h"

namespace vtc {

constexpr int kInvMaxN = 256;
constexpr int kInvPanel = 32;
constexpr int kInvPitch = kInvPanel + 1;  // panel row pitch (doubles)
constexpr int kInvThreads = 1024;
constexpr int kInvCols = 8;               // right-hand sides per workgroup

__host__ __device__ static inline int inv_padded(int64_t n) {
  return (int)((n + kInvPanel - 1) / kInvPanel * kInvPanel);
}

// LDS of the factorisation: panel [m][kInvPitch], U12 [32][m - 32],
// then int piv[32], perm[m], flags[2]
static inline size_t inv_factor_lds_bytes(int m) {
  return ((size_t)m * kInvPitch + (size_t)kInvPanel * (m - kInvPanel)) *
             sizeof(double) +
         (size_t)(kInvPanel + m + 2) * sizeof(int);
}

__global__ __launch_bounds__(kInvThreads) void lu_factor_kernel(
    const float* __restrict__ a, int n, int m, double* __restrict__ A,
    int* __restrict__ perm_out, int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double inv_lds[];
  double* P = inv_lds;
  double* Ub = P + m * kInvPitch;
  int* piv = reinterpret_cast<int*>(Ub + kInvPanel * (m - kInvPanel));
  int* perm = piv + kInvPanel;
  int* flags = perm + m;  // [first bad pivot or -1, non-finite input seen]
  const int t = threadIdx.x;

  if (t == 0) {
    flags[0] = -1;
    flags[1] = 0;
  }
  for (int i = t; i < m; i += kInvThreads) perm[i] = i;
  __syncthreads();
  int nonfinite = 0;
  for (int e = t; e < m * m; e += kInvThreads) {
    const int i = e / m, j = e % m;
    double v = (i == j) ? 1.0 : 0.0;
    if (i < n && j < n) {
      v = (double)a[(int64_t)i * n + j];
      if (!isfinite(v)) nonfinite = 1;
    }
    A[e] = v;
  }
  if (nonfinite) atomicOr(&flags[1], 1);
  __syncthreads();

  for (int k0 = 0; k0 < m; k0 += kInvPanel) {
    const int rows = m - k0, w = m - k0 - kInvPanel;
    for (int e = t; e < rows * kInvPanel; e += kInvThreads) {
      const int r = e / kInvPanel, c = e % kInvPanel;
      P[r * kInvPitch + c] = A[(int64_t)(k0 + r) * m + k0 + c];
    }
    __syncthreads();

    // ---- panel factorisation in LDS
    for (int j = 0; j < kInvPanel; ++j) {
      if (t < 64) {
        double best = -1.0;  // NaN never wins: an all-NaN column pivots on j
        int at = j;
        for (int r = j + t; r < rows; r += 64) {
          const double v = fabs(P[r * kInvPitch + j]);
          if (v > best) {  // r increases: ties keep the lower row
            best = v;
            at = r;
          }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const double ob = __shfl_xor(best, off, 64);
          const int oa = __shfl_xor(at, off, 64);
          if (ob > best || (ob == best && oa < at)) {
            best = ob;
            at = oa;
          }
        }
        const double d = P[at * kInvPitch + j];
        if (at != j && t < kInvPanel) {
          const double x = P[j * kInvPitch + t];
          P[j * kInvPitch + t] = P[at * kInvPitch + t];
          P[at * kInvPitch + t] = x;
        }
        if (t == 0) {
          piv[j] = at;
          if (k0 + j < n && flags[0] < 0 && (d == 0.0 || !isfinite(d)))
            flags[0] = k0 + j;
          const int x = perm[k0 + j];
          perm[k0 + j] = perm[k0 + at];
          perm[k0 + at] = x;
        }
      }
      __syncthreads();
      if (t > j && t < rows)  // multipliers
        P[t * kInvPitch + j] = P[t * kInvPitch + j] / P[j * kInvPitch + j];
      __syncthreads();
      // rank-1 update of the panel's remaining columns, one element per
      // thread and pass (independent, so their LDS latencies overlap)
      const int cols = kInvPanel - 1 - j;
      for (int e = t; e < (rows - 1 - j) * cols; e += kInvThreads) {
        const int r = j + 1 + e / cols, c = j + 1 + e % cols;
        P[r * kInvPitch + c] = fma(-P[r * kInvPitch + j],
                                   P[j * kInvPitch + c], P[r * kInvPitch + c]);
      }
      __syncthreads();
    }
    for (int e = t; e < rows * kInvPanel; e += kInvThreads) {
      const int r = e / kInvPanel, c = e % kInvPanel;
      A[(int64_t)(k0 + r) * m + k0 + c] = P[r * kInvPitch + c];
    }
    // ---- the panel's row interchanges on every other column (L and A12/A22)
    for (int ci = t; ci < m - kInvPanel; ci += kInvThreads) {
      const int c = ci < k0 ? ci : ci + kInvPanel;
      for (int j = 0; j < kInvPanel; ++j) {
        const int p = piv[j];
        if (p != j) {
          const double x = A[(int64_t)(k0 + j) * m + c];
          A[(int64_t)(k0 + j) * m + c] = A[(int64_t)(k0 + p) * m + c];
          A[(int64_t)(k0 + p) * m + c] = x;
        }
      }
    }
    __syncthreads();
    if (w == 0) break;

    // ---- U12 = L11^-1 A12 (unit lower), one column per thread, in LDS
    for (int ci = t; ci < w; ci += kInvThreads) {
      const int64_t c = k0 + kInvPanel + ci;
      for (int i = 0; i < kInvPanel; ++i) {
        double x = A[(int64_t)(k0 + i) * m + c];
        for (int q = 0; q < i; ++q)
          x = fma(-P[i * kInvPitch + q], Ub[q * w + ci], x);
        Ub[i * w + ci] = x;
        A[(int64_t)(k0 + i) * m + c] = x;
      }
    }
    __syncthreads();

    // ---- A22 -= L21 U12, 4 x 4 tiles; consecutive threads share a tile row
    const int tw = w / 4;
    for (int e = t; e < tw * tw; e += kInvThreads) {
      const int r0 = (e / tw) * 4, c0 = (e % tw) * 4;
      double* base = A + (int64_t)(k0 + kInvPanel + r0) * m + k0 + kInvPanel +
                     c0;
      double acc[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc[i][jj] = base[(int64_t)i * m + jj];
#pragma unroll 4
      for (int q = 0; q < kInvPanel; ++q) {
        double av[4], bv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          av[i] = P[(kInvPanel + r0 + i) * kInvPitch + q];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) bv[jj] = Ub[q * w + c0 + jj];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj)
            acc[i][jj] = fma(-av[i], bv[jj], acc[i][jj]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) base[(int64_t)i * m + jj] = acc[i][jj];
    }
    __syncthreads();
  }

  for (int i = t; i < m; i += kInvThreads) perm_out[i] = perm[i];
  if (t == 0) {
    status[0] = (flags[0] < 0 && flags[1] == 0) ? 1 : 0;
    status[1] = flags[0];
  }
}

// X = U^-1 L^-1 P for columns c0 .. c0 + kInvCols - 1.  Thread i owns row i;
// column c of P has its one in the row i with perm[i] == c.
__global__ __launch_bounds__(kInvMaxN) void lu_solve_kernel(
    const double* __restrict__ A, const int* __restrict__ perm, int n, int m,
    float* __restrict__ a_inv) {
  __shared__ double y[kInvMaxN][kInvCols];
  __shared__ double x[kInvMaxN][kInvCols];
  const int i = threadIdx.x;
  const int c0 = blockIdx.x * kInvCols;
  const bool live = i < m;
  const int pi = live ? perm[i] : -1;
  const double* row = A + (int64_t)(live ? i : 0) * m;
  double b[kInvCols];
#pragma unroll
  for (int cc = 0; cc < kInvCols; ++cc) b[cc] = (pi == c0 + cc) ? 1.0 : 0.0;

  // forward: L y = P e_c, L unit lower
  for (int jb = 0; jb < m; jb += kInvPanel) {
    double l[kInvPanel];
#pragma unroll
    for (int q = 0; q < kInvPanel; ++q) l[q] = row[jb + q];
#pragma unroll
    for (int q = 0; q < kInvPanel; ++q) {
      const int j = jb + q;
      if (i == j) {
#pragma unroll
        for (int cc = 0; cc < kInvCols; ++cc) y[j][cc] = b[cc];
      }
      __syncthreads();
      if (live && i > j) {
#pragma unroll
        for (int cc = 0; cc < kInvCols; ++cc)
          b[cc] = fma(-l[q], y[j][cc], b[cc]);
      }
    }
  }
  // backward: U x = y
  for (int jb = m - kInvPanel; jb >= 0; jb -= kInvPanel) {
    double u[kInvPanel];
#pragma unroll
    for (int q = 0; q < kInvPanel; ++q) u[q] = row[jb + q];
#pragma unroll
    for (int q = kInvPanel - 1; q >= 0; --q) {
      const int j = jb + q;
      if (i == j) {
#pragma unroll
        for (int cc = 0; cc < kInvCols; ++cc) {
          b[cc] = b[cc] / u[q];
          x[j][cc] = b[cc];
        }
      }
      __syncthreads();
      if (i < j) {
#pragma unroll
        for (int cc = 0; cc < kInvCols; ++cc)
          b[cc] = fma(-u[q], x[j][cc], b[cc]);
      }
    }
  }
  if (i < n) {
#pragma unroll
    for (int cc = 0; cc < kInvCols; ++cc)
      if (c0 + cc < n) a_inv[(int64_t)i * n + c0 + cc] = (float)b[cc];
  }
}

// Scratch of vtc_mat_inverse: the padded float64 LU factors and the row order
struct InverseLayout {
  double* A;
  int* perm;
  InverseLayout(Carver& ws, int m) {
    A = ws.take<double>((size_t)m * m);
    perm = ws.take<int>(m);
  }
};

}  // namespace vtc

using namespace vtc;

// ---- C ABI ---------------------------------------------------------------
extern "C" size_t vtc_mat_inverse_workspace_bytes(int64_t n) {
  if (n <= 0 || n > kInvMaxN) return 256;
  return measured_bytes<InverseLayout>(inv_padded(n));
}

extern "C" int vtc_mat_inverse(const float* a, int64_t n, float* a_inv,
                               int* status, void* workspace,
                               size_t workspace_bytes, void* stream) {
  VTC_REQUIRE(a && a_inv && status, "vtc_mat_inverse: null pointer");
  VTC_REQUIRE(n > 0, "vtc_mat_inverse: bad size");
  if (n > kInvMaxN) {
    set_error("vtc_mat_inverse: n = %lld exceeds the device LU limit of %d",
              (long long)n, kInvMaxN);
    return VTC_ERR_UNSUPPORTED;
  }
  const uintptr_t in0 = (uintptr_t)a, out0 = (uintptr_t)a_inv;
  const uintptr_t bytes = (uintptr_t)(n * n) * sizeof(float);
  VTC_REQUIRE(in0 + bytes <= out0 || out0 + bytes <= in0,
              "vtc_mat_inverse: a_inv must not alias a");
  if (!workspace || workspace_bytes < vtc_mat_inverse_workspace_bytes(n)) {
    set_error("vtc_mat_inverse: workspace too small");
    return VTC_ERR_WORKSPACE;
  }
  const int m = inv_padded(n);
  Carver carve(workspace);
  const InverseLayout L(carve, m);
  hipStream_t s = as_stream(stream);
  static unsigned long long configured = 0;
  if (first_use_on_this_device(&configured)) {
    VTC_HIP_CHECK(hipFuncSetAttribute(
        reinterpret_cast<const void*>(lu_factor_kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize,
        (int)inv_factor_lds_bytes(kInvMaxN)));
  }
  hipLaunchKernelGGL(lu_factor_kernel, dim3(1), dim3(kInvThreads),
                     inv_factor_lds_bytes(m), s, a, (int)n, m, L.A, L.perm,
                     status);
  VTC_LAUNCH_CHECK();
  hipLaunchKernelGGL(lu_solve_kernel, dim3((unsigned)ceil_div(n, kInvCols)),
                     dim3((unsigned)ceil_div(m, 64) * 64), 0, s,
                     (const double*)L.A, (const int*)L.perm, (int)n, m, a_inv);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}
