// ZCA whitening and PCA on the device (utils/image_processing.py:338-460 and
// training/pca.py:8-39 of the reference).
//
// Four pieces, each its own entry point:
//   column covariance   C = Xc^T Xc / D of a (D, n) float32 matrix, float64
//                       products and sums (centred on load: Xc = x - mu with
//                       the float64 column means mu); split over row slabs,
//                       slabs summed in a fixed order (bitwise reproducible)
//   symmetric eigen     parallel-ordered (round-robin) two-sided Jacobi in
//                       float64, one workgroup, n <= 256, A and V in an
//                       L2-resident workspace; bounded by max_sweeps
//   ZCA matrices        W = U diag(1/(sqrt(w)+eps)) U^T and its inverse
//                       U diag(sqrt(w)+eps) U^T, float64 sums rounded to f32
//   row transform       y = (x - a) M + c, float32 FMA chains over k in
//                       increasing order (the class of the reference's
//                       float32 numpy products); the offset is subtracted
//                       in the loader, before the product
#include "common.h"

namespace vtc {

// ---- column means and covariance ----------------------------------------
constexpr int kCovTile = 64;      // output tile edge (i and j)
constexpr int kCovChunk = 32;     // rows staged per LDS step
constexpr int kCovThreads = 256;  // 4 waves, each takes every 4th staged row
constexpr int kCovTargetBlocks = 1024;
constexpr int kMeanCols = 64;

__host__ __device__ static inline int64_t cov_tiles_1d(int64_t n) {
  return (n + kCovTile - 1) / kCovTile;
}
static inline int64_t cov_tiles(int64_t n) {
  const int64_t t = cov_tiles_1d(n);
  return t * (t + 1) / 2;  // upper triangle ti <= tj
}
static inline int64_t cov_slabs(int64_t rows, int64_t n) {
  int64_t s = ceil_div(kCovTargetBlocks, cov_tiles(n));
  const int64_t chunks = ceil_div(rows, kCovChunk);
  if (s > chunks) s = chunks;
  return s < 1 ? 1 : s;
}
static inline int64_t mean_slabs(int64_t rows) {
  int64_t s = ceil_div(rows, 1024);
  return s > 512 ? 512 : (s < 1 ? 1 : s);
}

// partial column sums: block (column block, slab), 4 row lanes x 64 columns
__global__ __launch_bounds__(256) void column_sum_kernel(
    const float* __restrict__ x, int64_t rows, int64_t n, int64_t rows_per,
    double* __restrict__ partial) {
  __shared__ double red[4][kMeanCols];
  const int t = threadIdx.x;
  const int64_t col = (int64_t)blockIdx.x * kMeanCols + (t & 63);
  const int64_t r0 = (int64_t)blockIdx.y * rows_per;
  int64_t r1 = r0 + rows_per;
  if (r1 > rows) r1 = rows;
  double s = 0.0;
  if (col < n)
    for (int64_t r = r0 + (t >> 6); r < r1; r += 4) s += (double)x[r * n + col];
  red[t >> 6][t & 63] = s;
  __syncthreads();
  if (t < 64 && col < n)
    partial[(int64_t)blockIdx.y * n + col] =
        ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

// means[c] = sum over slabs (in order) / rows; grand = mean of the means
__global__ __launch_bounds__(256) void column_mean_kernel(
    const double* __restrict__ partial, int64_t slabs, int64_t rows,
    int64_t n, double* __restrict__ means, double* __restrict__ grand) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  double own = 0.0;
  for (int64_t c = t; c < n; c += 256) {
    double s = 0.0;
    for (int64_t z = 0; z < slabs; ++z) s += partial[z * n + c];
    const double m = s / (double)rows;
    means[c] = m;
    own += m;
  }
  own = wave_sum(own);
  if ((t & 63) == 0) red[t >> 6] = own;
  __syncthreads();
  if (t == 0 && grand) *grand = (((red[0] + red[1]) + red[2]) + red[3]) / n;
}

__device__ __forceinline__ void cov_tile_of(int64_t idx, int64_t t1d,
                                            int64_t* ti, int64_t* tj) {
  int64_t i = 0;
  while (idx >= t1d - i) {
    idx -= t1d - i;
    ++i;
  }
  *ti = i;
  *tj = i + idx;
}

// partial[slab][tile][64][64] = sum over the slab's rows of xc[r,i] xc[r,j],
// i in tile row block ti, j in column block tj (ti <= tj).  Lane l of each
// wave owns the 8x8 sub-tile (l/8, l%8); the four waves take rows k = w mod 4
// of every staged chunk and are added in wave order at the end.
__global__ __launch_bounds__(kCovThreads) void covariance_partial_kernel(
    const float* __restrict__ x, int64_t rows, int64_t n, int center,
    const double* __restrict__ means, int64_t rows_per,
    double* __restrict__ partial) {
  // staging (2 x 16 KiB) while the rows stream, then the 32 KiB wave sum
  __shared__ double lds[kCovTile * kCovTile];
  static_assert(2 * kCovChunk * kCovTile <= kCovTile * kCovTile, "LDS");
  double (*sa)[kCovTile] = reinterpret_cast<double (*)[kCovTile]>(lds);
  double (*sb)[kCovTile] =
      reinterpret_cast<double (*)[kCovTile]>(lds + kCovChunk * kCovTile);
  double* red = lds;
  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  int64_t ti, tj;
  cov_tile_of(blockIdx.x, cov_tiles_1d(n), &ti, &tj);
  const int64_t i0 = ti * kCovTile, j0 = tj * kCovTile;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per;
  int64_t r1 = r0 + rows_per;
  if (r1 > rows) r1 = rows;

  // loader: column lane, rows wave + 4q
  const int64_t ci = i0 + lane, cj = j0 + lane;
  const bool ci_ok = ci < n, cj_ok = cj < n;
  const double mi = (ci_ok && center) ? means[ci] : 0.0;
  const double mj = (cj_ok && center) ? means[cj] : 0.0;

  double acc[8][8];
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[a][b] = 0.0;
  const int ri = (lane >> 3) * 8, rj = (lane & 7) * 8;

  for (int64_t rc = r0; rc < r1; rc += kCovChunk) {
#pragma unroll
    for (int q = 0; q < kCovChunk / 4; ++q) {
      const int k = wave + 4 * q;
      const int64_t r = rc + k;
      const bool rok = r < r1;
      sa[k][lane] = (rok && ci_ok) ? (double)x[r * n + ci] - mi : 0.0;
      sb[k][lane] = (rok && cj_ok) ? (double)x[r * n + cj] - mj : 0.0;
    }
    __syncthreads();
#pragma unroll 2
    for (int k = wave; k < kCovChunk; k += 4) {
      double av[8], bv[8];
#pragma unroll
      for (int a = 0; a < 8; ++a) av[a] = sa[k][ri + a];
#pragma unroll
      for (int b = 0; b < 8; ++b) bv[b] = sb[k][rj + b];
#pragma unroll
      for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = fma(av[a], bv[b], acc[a][b]);
    }
    __syncthreads();
  }
  // waves in order 0, 1, 2, 3
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) {
          const int e = (ri + a) * kCovTile + rj + b;
          red[e] = (w == 0) ? acc[a][b] : red[e] + acc[a][b];
        }
    }
    __syncthreads();
  }
  double* out = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) *
                              (kCovTile * kCovTile);
  for (int e = t; e < kCovTile * kCovTile; e += kCovThreads) out[e] = red[e];
}

// cov[i][j] = sum over slabs (in order) of the tile partial / rows; (i, j) and
// (j, i) read the same partial element, so the result is exactly symmetric
__global__ __launch_bounds__(256) void covariance_reduce_kernel(
    const double* __restrict__ partial, int64_t slabs, int64_t tiles,
    int64_t rows, int64_t n, double* __restrict__ cov) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n * n) return;
  int64_t i = e / n, j = e % n;
  if (i > j) {
    const int64_t s = i;
    i = j;
    j = s;
  }
  const int64_t t1d = cov_tiles_1d(n);
  const int64_t ti = i / kCovTile, tj = j / kCovTile;
  const int64_t tile = ti * t1d - ti * (ti - 1) / 2 + (tj - ti);
  const int64_t off = tile * (kCovTile * kCovTile) +
                      (i - ti * kCovTile) * kCovTile + (j - tj * kCovTile);
  double s = 0.0;
  for (int64_t z = 0; z < slabs; ++z)
    s += partial[z * tiles * (kCovTile * kCovTile) + off];
  cov[e] = s / (double)rows;
}

// ---- symmetric eigen-decomposition ----------------------------------------
constexpr int kEigMaxN = 256;
constexpr int kEigThreads = 1024;
constexpr int kEigBatch = 4;
constexpr double kEigTol = 1e-14;   // off(A)_F <= kEigTol * ||A||_F

// sum over the whole block; every thread receives it (fixed order)
__device__ __forceinline__ double eig_block_sum(double v, double* red) {
  v = wave_sum(v);
  const int t = threadIdx.x;
  __syncthreads();
  if ((t & 63) == 0) red[t >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < kEigThreads / 64; ++w) s += red[w];
  return s;
}

// pair i of round r of the circle ordering of m (even) indices
__device__ __forceinline__ void eig_pair(int r, int i, int m, int* p, int* q) {
  if (i == 0) {
    *p = m - 1;
    *q = r;
  } else {
    *p = (r + i) % (m - 1);
    *q = (r - i + (m - 1)) % (m - 1);
  }
}

// A, V: m x m float64 workspace (m = n rounded up to even; the padding row and
// column of A are zero and never rotate).  Rotation of pair (p, q) as in
// Numerical Recipes 11.1: theta = (a_qq - a_pp) / (2 a_pq),
// t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1/sqrt(t^2+1), s = t c,
// A <- J^T A J with J_pp = J_qq = c, J_pq = s, J_qp = -s.  The n/2 pairs of a
// round are disjoint: thread-owned 2x2 blocks A[{p_P,q_P}, {p_Q,q_Q}] take
// the left rotation of P and the right rotation of Q in one read-modify-write.
__global__ __launch_bounds__(kEigThreads) void jacobi_eig_kernel(
    const double* __restrict__ a_in, int n, int max_sweeps,
    double* __restrict__ A, double* __restrict__ V, double* eigvals,
    float* eigvecs, int* status) {
  __shared__ double pc[kEigMaxN / 2], ps[kEigMaxN / 2];
  __shared__ int pp[kEigMaxN / 2], pq[kEigMaxN / 2];
  __shared__ double red[kEigThreads / 64];
  __shared__ double diag[kEigMaxN];
  __shared__ int rank[kEigMaxN];
  const int t = threadIdx.x;
  const int m = n + (n & 1), h = m / 2;
  const int mm = m * m;

  // upper triangle of the input, mirrored; zero padding
  double fro = 0.0;
  for (int e = t; e < mm; e += kEigThreads) {
    const int i = e / m, j = e % m;
    double v = 0.0;
    if (i < n && j < n) v = (i <= j) ? a_in[i * n + j] : a_in[j * n + i];
    A[e] = v;
    V[e] = (i == j) ? 1.0 : 0.0;
    fro += v * v;
  }
  const double fro2 = eig_block_sum(fro, red);
  __syncthreads();

  int converged = 0, sweep = 0;
  for (;; ++sweep) {
    double off = 0.0;
    for (int e = t; e < mm; e += kEigThreads)
      if (e / m != e % m) off += A[e] * A[e];
    const double off2 = eig_block_sum(off, red);
    if (!(off2 > kEigTol * kEigTol * fro2)) {
      converged = (off2 == off2 && fro2 == fro2) ? 1 : 0;
      break;
    }
    if (sweep >= max_sweeps) break;
    for (int r = 0; r < m - 1; ++r) {
      if (t < h) {
        int p, q;
        eig_pair(r, t, m, &p, &q);
        const double apq = A[p * m + q];
        double c = 1.0, s = 0.0;
        if (apq != 0.0) {
          const double theta = (A[q * m + q] - A[p * m + p]) / (2.0 * apq);
          const double at = fabs(theta);
          double tt = (at > 1e150) ? 0.5 / at : 1.0 / (at + sqrt(at * at + 1.0));
          if (theta < 0.0) tt = -tt;
          c = 1.0 / sqrt(tt * tt + 1.0);
          s = tt * c;
        }
        pc[t] = c;
        ps[t] = s;
        pp[t] = p;
        pq[t] = q;
      }
      __syncthreads();
      // A blocks: (P, Q) over h x h
      for (int b0 = t; b0 < h * h; b0 += kEigThreads * kEigBatch) {
        double v[kEigBatch][4];
#pragma unroll
        for (int u = 0; u < kEigBatch; ++u) {
          const int b = b0 + u * kEigThreads;
          if (b < h * h) {
            const int P = b / h, Q = b % h;
            const int p = pp[P], q = pq[P], x = pp[Q], y = pq[Q];
            v[u][0] = A[p * m + x];
            v[u][1] = A[p * m + y];
            v[u][2] = A[q * m + x];
            v[u][3] = A[q * m + y];
          }
        }
#pragma unroll
        for (int u = 0; u < kEigBatch; ++u) {
          const int b = b0 + u * kEigThreads;
          if (b < h * h) {
            const int P = b / h, Q = b % h;
            const int p = pp[P], q = pq[P], x = pp[Q], y = pq[Q];
            const double c1 = pc[P], s1 = ps[P], c2 = pc[Q], s2 = ps[Q];
            // left: row p' = c p - s q, row q' = s p + c q
            const double px = c1 * v[u][0] - s1 * v[u][2];
            const double py = c1 * v[u][1] - s1 * v[u][3];
            const double qx = s1 * v[u][0] + c1 * v[u][2];
            const double qy = s1 * v[u][1] + c1 * v[u][3];
            // right: col x' = c x - s y, col y' = s x + c y
            double npx = c2 * px - s2 * py, npy = s2 * px + c2 * py;
            double nqx = c2 * qx - s2 * qy, nqy = s2 * qx + c2 * qy;
            if (P == Q && s1 != 0.0) {  // the rotated pair: exact zeros
              npy = 0.0;
              nqx = 0.0;
            }
            A[p * m + x] = npx;
            A[p * m + y] = npy;
            A[q * m + x] = nqx;
            A[q * m + y] = nqy;
          }
        }
      }
      // V <- V J: (row i, pair P) over m x h
      for (int b0 = t; b0 < m * h; b0 += kEigThreads * kEigBatch) {
        double v[kEigBatch][2];
#pragma unroll
        for (int u = 0; u < kEigBatch; ++u) {
          const int b = b0 + u * kEigThreads;
          if (b < m * h) {
            const int i = b / h, P = b % h;
            v[u][0] = V[i * m + pp[P]];
            v[u][1] = V[i * m + pq[P]];
          }
        }
#pragma unroll
        for (int u = 0; u < kEigBatch; ++u) {
          const int b = b0 + u * kEigThreads;
          if (b < m * h) {
            const int i = b / h, P = b % h;
            const double c = pc[P], s = ps[P];
            V[i * m + pp[P]] = c * v[u][0] - s * v[u][1];
            V[i * m + pq[P]] = s * v[u][0] + c * v[u][1];
          }
        }
      }
      __syncthreads();
    }
  }

  // descending order: rank = #{j : d_j > d_i or (d_j == d_i and j < i)}
  for (int i = t; i < n; i += kEigThreads) diag[i] = A[i * m + i];
  __syncthreads();
  for (int i = t; i < n; i += kEigThreads) {
    const double d = diag[i];
    int k = 0;
    for (int j = 0; j < n; ++j)
      k += (diag[j] > d || (diag[j] == d && j < i)) ? 1 : 0;
    rank[i] = k;
    eigvals[k] = d;
  }
  __syncthreads();
  // sign: the largest-magnitude float32 component of each vector is positive
  // (ties: the lower index); one wave per vector
  const int lane = t & 63, wave = t >> 6;
  for (int i = wave; i < n; i += kEigThreads / 64) {
    float best = -1.f;
    int at = 0;
    for (int k = lane; k < n; k += 64) {
      const float a = fabsf((float)V[k * m + i]);
      if (a > best) {  // k increases: ties keep the lower index
        best = a;
        at = k;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ob = __shfl_xor(best, off, 64);
      const int oa = __shfl_xor(at, off, 64);
      if (ob > best || (ob == best && oa < at)) {
        best = ob;
        at = oa;
      }
    }
    const bool flip = (float)V[at * m + i] < 0.f;
    const int col = rank[i];
    for (int k = lane; k < n; k += 64) {
      const float v = (float)V[k * m + i];
      eigvecs[k * n + col] = flip ? -v : v;
    }
  }
  if (t == 0) {
    status[0] = converged;
    status[1] = sweep;
  }
}

// ---- ZCA matrices ------------------------------------------------------
// w_mat[i][j] = sum_k U[i][k] U[j][k] / (sqrt(max(w_k, 0)) + eps), w_inv the
// same with the factor sqrt(max(w_k, 0)) + eps; float64 sums in k order
__global__ __launch_bounds__(256) void zca_matrices_kernel(
    const float* __restrict__ u, const double* __restrict__ w, int n,
    double eps, float* __restrict__ w_mat, float* __restrict__ w_inv) {
  __shared__ double fk[256], rk[256];
  const int e = blockIdx.x * 256 + threadIdx.x;
  const bool live = e < n * n;
  const int i = live ? e / n : 0, j = live ? e % n : 0;
  double s = 0.0, si = 0.0;
  for (int k0 = 0; k0 < n; k0 += 256) {
    __syncthreads();
    if (k0 + (int)threadIdx.x < n) {
      const double f = sqrt(fmax(w[k0 + threadIdx.x], 0.0)) + eps;
      fk[threadIdx.x] = f;
      rk[threadIdx.x] = 1.0 / f;
    }
    __syncthreads();
    const int k1 = (n - k0 < 256) ? n - k0 : 256;
    if (live)
      for (int k = 0; k < k1; ++k) {
        const double uu =
            (double)u[i * n + k0 + k] * (double)u[j * n + k0 + k];
        s += uu * rk[k];
        si += uu * fk[k];
      }
  }
  if (!live) return;
  if (w_mat) w_mat[e] = (float)s;
  if (w_inv) w_inv[e] = (float)si;
}

// ---- row transform -------------------------------------------------------
// y (rows, n) = (x - a) M + c.  Block tile 64 rows x 64 columns, K step 32;
// thread (tr, tc) = (t / 16, t % 16) owns rows 4 tr.. and columns 4 tc..;
// operands staged k-major in LDS (X transposed while it is stored).
constexpr int kRtBM = 64, kRtBN = 64, kRtBK = 32, kRtPitch = 68;

__global__ __launch_bounds__(256) void row_transform_kernel(
    const float* __restrict__ x, int64_t rows, int n,
    const float* __restrict__ offsets, const float* __restrict__ mat,
    float add, float* __restrict__ y, int vec) {
  __shared__ float sx[kRtBK][kRtPitch];
  __shared__ float sm[kRtBK][kRtPitch];
  const int t = threadIdx.x;
  const int tr = t >> 4, tc = t & 15;
  const int64_t row0 = (int64_t)blockIdx.x * kRtBM;
  const int col0 = blockIdx.y * kRtBN;
  // loaders: X row t/4, k (t%4)*8..+8 ; M k t/8, columns (t%8)*8..+8
  const int xr = t >> 2, xk = (t & 3) * 8;
  const int mk = t >> 3, mc = (t & 7) * 8;
  const int64_t grow = row0 + xr;
  const bool row_ok = grow < rows;
  const float* xrow = x + (row_ok ? grow : 0) * n;

  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;

  for (int k0 = 0; k0 < n; k0 += kRtBK) {
    float xv[8], mv[8];
    const int kx = k0 + xk;
    if (vec && row_ok && kx + 8 <= n) {  // n % 4 == 0: 16-byte aligned
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float4 a = *reinterpret_cast<const float4*>(xrow + kx + 4 * h);
        const float4 o =
            *reinterpret_cast<const float4*>(offsets + kx + 4 * h);
        xv[4 * h + 0] = sub_rn(a.x, o.x);
        xv[4 * h + 1] = sub_rn(a.y, o.y);
        xv[4 * h + 2] = sub_rn(a.z, o.z);
        xv[4 * h + 3] = sub_rn(a.w, o.w);
      }
    } else {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = kx + u;
        xv[u] = (row_ok && k < n) ? sub_rn(xrow[k], offsets[k]) : 0.f;
      }
    }
    const int kk = k0 + mk, cm = col0 + mc;
    if (vec && kk < n && cm + 8 <= n) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float4 b = *reinterpret_cast<const float4*>(
            mat + (int64_t)kk * n + cm + 4 * h);
        mv[4 * h + 0] = b.x;
        mv[4 * h + 1] = b.y;
        mv[4 * h + 2] = b.z;
        mv[4 * h + 3] = b.w;
      }
    } else {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int c = cm + u;
        mv[u] = (kk < n && c < n) ? mat[(int64_t)kk * n + c] : 0.f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 8; ++u) sx[xk + u][xr] = xv[u];
#pragma unroll
    for (int u = 0; u < 8; ++u) sm[mk][mc + u] = mv[u];
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < kRtBK; ++k) {
      const float4 a = *reinterpret_cast<const float4*>(&sx[k][tr * 4]);
      const float4 b = *reinterpret_cast<const float4*>(&sm[k][tc * 4]);
      const float av[4] = {a.x, a.y, a.z, a.w};
      const float bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t r = row0 + tr * 4 + i;
    if (r >= rows) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = col0 + tc * 4 + j;
      if (c < n) y[r * n + c] = add_rn(acc[i][j], add);
    }
  }
}

// Scratch of vtc_column_covariance.  own_means: the caller gave no means_f64,
// the column means live here.  One more piece has always been counted and is
// not used; it stays so that the queried size does not move.
struct CovarianceLayout {
  double* cov_part;
  double* mean_part;
  double* means = nullptr;
  CovarianceLayout(Carver& ws, int64_t rows, int64_t cols, bool own_means) {
    cov_part = ws.take<double>((size_t)cov_slabs(rows, cols) *
                               cov_tiles(cols) * kCovTile * kCovTile);
    mean_part = ws.take<double>((size_t)mean_slabs(rows) * cols);
    if (own_means) means = ws.take<double>(cols);
    ws.take<char>(256);
  }
};

// Scratch of vtc_sym_eig: the matrix and the rotations, padded to an even order
struct SymEigLayout {
  double* A;
  double* V;
  SymEigLayout(Carver& ws, int64_t n) {
    const int64_t m = n + (n & 1);
    A = ws.take<double>(m * m);
    V = ws.take<double>(m * m);
  }
};

}  // namespace vtc

using namespace vtc;

// ---- C ABI ---------------------------------------------------------------
extern "C" size_t vtc_column_covariance_workspace_bytes(int64_t rows,
                                                        int64_t cols) {
  if (rows <= 0 || cols <= 0) return 256;
  return measured_bytes<CovarianceLayout>(rows, cols, true);
}

extern "C" int vtc_column_covariance(const float* x, int64_t rows,
                                     int64_t cols, int center,
                                     double* means_f64, double* grand_mean_f64,
                                     double* cov_f64, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  VTC_REQUIRE(x && (cov_f64 || means_f64 || grand_mean_f64),
              "vtc_column_covariance: null pointer");
  VTC_REQUIRE(rows > 0 && cols > 0, "vtc_column_covariance: bad size");
  VTC_REQUIRE(cols <= 65536 && cols * cols < ((int64_t)1 << 31),
              "vtc_column_covariance: bad size");
  if (!workspace ||
      workspace_bytes < vtc_column_covariance_workspace_bytes(rows, cols)) {
    set_error("vtc_column_covariance: workspace too small");
    return VTC_ERR_WORKSPACE;
  }
  Carver carve(workspace);
  const int64_t cslabs = cov_slabs(rows, cols), tiles = cov_tiles(cols);
  const int64_t mslabs = mean_slabs(rows);
  const CovarianceLayout L(carve, rows, cols, means_f64 == nullptr);
  double* means = means_f64 ? means_f64 : L.means;
  hipStream_t s = as_stream(stream);
  const bool need_means = center || means_f64 || grand_mean_f64;
  if (need_means) {
    const int64_t per = ceil_div(rows, mslabs);
    hipLaunchKernelGGL(column_sum_kernel,
                       dim3((unsigned)ceil_div(cols, kMeanCols),
                            (unsigned)mslabs),
                       dim3(256), 0, s, x, rows, cols, per, L.mean_part);
    VTC_LAUNCH_CHECK();
    hipLaunchKernelGGL(column_mean_kernel, dim3(1), dim3(256), 0, s,
                       (const double*)L.mean_part, mslabs, rows, cols, means,
                       grand_mean_f64);
    VTC_LAUNCH_CHECK();
  }
  if (!cov_f64) return VTC_OK;
  const int64_t per = ceil_div(ceil_div(rows, cslabs), kCovChunk) * kCovChunk;
  const int64_t slabs = ceil_div(rows, per);
  hipLaunchKernelGGL(covariance_partial_kernel,
                     dim3((unsigned)tiles, (unsigned)slabs),
                     dim3(kCovThreads), 0, s, x, rows, cols, center ? 1 : 0,
                     (const double*)means, per, L.cov_part);
  VTC_LAUNCH_CHECK();
  hipLaunchKernelGGL(covariance_reduce_kernel,
                     dim3((unsigned)ceil_div(cols * cols, 256)), dim3(256), 0,
                     s, (const double*)L.cov_part, slabs, tiles, rows, cols,
                     cov_f64);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" size_t vtc_sym_eig_workspace_bytes(int64_t n) {
  if (n <= 0 || n > kEigMaxN) return 256;
  return measured_bytes<SymEigLayout>(n);
}

extern "C" int vtc_sym_eig(const double* a_f64, int64_t n, int max_sweeps,
                           double* eigvals_f64, float* eigvecs_f32,
                           int* status, void* workspace,
                           size_t workspace_bytes, void* stream) {
  VTC_REQUIRE(a_f64 && eigvals_f64 && eigvecs_f32 && status,
              "vtc_sym_eig: null pointer");
  VTC_REQUIRE(n > 0 && max_sweeps >= 0, "vtc_sym_eig: bad size");
  if (n > kEigMaxN) {
    set_error("vtc_sym_eig: n = %lld exceeds the single-workgroup Jacobi "
              "limit of %d", (long long)n, kEigMaxN);
    return VTC_ERR_UNSUPPORTED;
  }
  if (!workspace || workspace_bytes < vtc_sym_eig_workspace_bytes(n)) {
    set_error("vtc_sym_eig: workspace too small");
    return VTC_ERR_WORKSPACE;
  }
  Carver carve(workspace);
  const SymEigLayout L(carve, n);
  hipLaunchKernelGGL(jacobi_eig_kernel, dim3(1), dim3(kEigThreads), 0,
                     as_stream(stream), a_f64, (int)n, max_sweeps, L.A, L.V,
                     eigvals_f64, eigvecs_f32, status);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" int vtc_zca_matrices(const float* eigvecs_f32,
                                const double* eigvals_f64, int64_t n,
                                double eps, float* w_f32, float* w_inv_f32,
                                void* stream) {
  VTC_REQUIRE(eigvecs_f32 && eigvals_f64 && (w_f32 || w_inv_f32),
              "vtc_zca_matrices: null pointer");
  VTC_REQUIRE(n > 0 && n <= 4096, "vtc_zca_matrices: bad size");
  hipLaunchKernelGGL(zca_matrices_kernel,
                     dim3((unsigned)ceil_div(n * n, 256)), dim3(256), 0,
                     as_stream(stream), eigvecs_f32, eigvals_f64, (int)n, eps,
                     w_f32, w_inv_f32);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" int vtc_row_transform(const float* x, int64_t rows, int64_t n,
                                 const float* offsets, const float* m,
                                 float add, float* y, void* stream) {
  VTC_REQUIRE(x && offsets && m && y, "vtc_row_transform: null pointer");
  VTC_REQUIRE(rows > 0 && n > 0 && n <= 4096,
              "vtc_row_transform: bad size");
  VTC_REQUIRE(ceil_div(rows, kRtBM) < ((int64_t)1 << 31),
              "vtc_row_transform: bad size");
  // 16-byte loads: rows, offsets and matrix rows all start 16-byte aligned
  const int vec = (n % 4 == 0 && ((uintptr_t)x | (uintptr_t)offsets |
                                  (uintptr_t)m) % 16 == 0) ? 1 : 0;
  hipLaunchKernelGGL(row_transform_kernel,
                     dim3((unsigned)ceil_div(rows, kRtBM),
                          (unsigned)ceil_div(n, kRtBN)),
                     dim3(256), 0, as_stream(stream), x, rows, (int)n,
                     offsets, m, add, y, vec);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}
