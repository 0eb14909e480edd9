// Tiled contraction at float32 accuracy on the 16-bit matrix pipe: every f32
// value becomes three bf16 parts that sum to it exactly (split3_packed,
// split_operand.h) and a product keeps the six part products hh, hm, mh, hl,
// lh, mm on v_mfma_f32_16x16x32_bf16 -- the truncation is below 2^-24 of a
// product, under the rounding of the f32 result itself.  (The two-part splits
// of gemm_x3.h stop at 2^-16 / 2^-21 and miss the gradient gates.)
//
//   C[M,N] = A * B          B is k-major: B[k * ldb + col]
//   A_KC : A[row * lda + k] (k contiguous), else k-major: A[k * lda + row]
//
// Values are split while a tile is staged; nothing pre-split lives in HBM.
//
// Block = 4 waves (2x2), block tile 128x128, wave tile 64x64 (4x4 MFMA tiles),
// K step 32.  One LDS image [operand][part][128 rows][32 k] of bf16 (48 KiB,
// two blocks per CU), global loads one K step ahead in registers.  A k-major
// operand is transposed in registers: a thread loads a 4 k x 4 row block
// (4 x 16 bytes) and writes, per row, 4 consecutive k of each part
// (ds_write_b64), the same 8-byte pieces a k-contiguous operand writes.
//
// LDS banks.  Rows are 64 B; the 16-byte chunk index is XORed with
// (-(row >> 2)) & 3.  A fragment read (ds_read_b128, lane l: row l & 15, chunk
// l >> 4) is served in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19,
// 28-31}, ...: per group the pairs (row >> 2, chunk) are (0,c) (3,c) (1,c^1)
// (2,c^1), which the XOR sends to four different chunks, times four rows mod 4
// = all 16 slots of the 256-byte bank row: conflict-free.  Stores (banks mod
// 128 B, groups of 16 consecutive lanes): a k-contiguous operand writes two
// whole rows per group, conflict-free; a k-major operand has 8 row blocks x 2
// k pieces per group, two lanes per 8-byte slot: 2-way, 8 LDS cycles against
// the 6 the store costs anyway.
#pragma once

#include "common.h"
#include "gemm_f32.h"
#include "split_operand.h"

namespace vtc {

constexpr int kB3BM = 128, kB3BN = 128, kB3BK = 32;
constexpr int kB3PartBytes = 128 * 64;   // one part of one operand tile

struct GemmB3Args {
  const float* A;
  const float* B;
  int64_t M, N, K;
  int64_t lda, ldb;
  int64_t k_chunk;      // K range of a slice, a multiple of 4
  int slices;
  // epilogue.  MINUS: C = acc - X (both leading dimension ldc); else slab z of
  // a split-K product, C + z * slab_stride.
  float* C;
  const float* X;
  int64_t ldc, slab_stride;
};

__device__ __forceinline__ int b3_lds_off(int row, int chunk) {
  return row * 64 + ((chunk ^ ((0 - (row >> 2)) & 3)) << 4);
}

constexpr unsigned kB3Outside = 0x80000000u;   // past every resource: reads 0

// Thread -> piece of a 128-line x 32-k operand tile.
//   k contiguous: 4 loads, load i is line (tid + 256 i) >> 3, k piece
//     (tid + 256 i) & 7 (4 consecutive k).
//   k-major: one 4 k x 4 line block: lines 4 lq .. 4 lq + 3, k piece kq; 8
//     consecutive lanes read 128 consecutive bytes of one k row.
__device__ __forceinline__ void b3_kmajor_piece(int tid, int* lq, int* kq) {
  *lq = (tid & 7) | (((tid >> 4) & 3) << 3);
  *kq = ((tid >> 3) & 1) | ((tid >> 6) << 1);
}

// Tile loads are buffer loads: lines past the matrix and k past the slice get
// an offset outside the resource and read as zero -- no branches, so loads stay
// in flight across the products of the step before (gemm_x3.h).
template <bool KC>
__device__ __forceinline__ void b3_stage_load(const __amdgpu_buffer_rsrc_t& rs,
                                              unsigned ld, int lines_left,
                                              int k0, int k_len, int tid,
                                              u32x4 (&regs)[4]) {
  if (KC) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int f = tid + i * 256;
      const int line = f >> 3, k = k0 + (f & 7) * 4;
      const unsigned vo = (line < lines_left && k < k_len)
                              ? ((unsigned)line * ld + (unsigned)k) * 4u
                              : kB3Outside;
      regs[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, vo, 0, 0);
    }
  } else {
    int lq, kq;
    b3_kmajor_piece(tid, &lq, &kq);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + kq * 4 + j;
      const unsigned vo = (4 * lq < lines_left && k < k_len)
                              ? ((unsigned)k * ld + 4u * (unsigned)lq) * 4u
                              : kB3Outside;
      regs[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, vo, 0, 0);
    }
  }
}

// registers -> LDS as three bf16 parts; `base` = part 0 of the operand
template <bool KC>
__device__ __forceinline__ void b3_stage_store(char* base, int tid,
                                               const u32x4 (&regs)[4]) {
  int lq, kq;
  b3_kmajor_piece(tid, &lq, &kq);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int line, piece;
    float v[4];
    if (KC) {
      const int f = tid + i * 256;
      line = f >> 3;
      piece = f & 7;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = __uint_as_float(regs[i][j]);
    } else {
      line = 4 * lq + i;
      piece = kq;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = __uint_as_float(regs[j][i]);
    }
    uint2 h, m, l;
    split3_packed(v, h, m, l);
    const int off = b3_lds_off(line, piece >> 1) + 8 * (piece & 1);
    *reinterpret_cast<uint2*>(base + off) = h;
    *reinterpret_cast<uint2*>(base + kB3PartBytes + off) = m;
    *reinterpret_cast<uint2*>(base + 2 * kB3PartBytes + off) = l;
  }
}

// TWO_SETS: hh in one accumulator set and the five cross products in a second,
// added once at the end; else one set.
template <bool A_KC, bool MINUS, bool TWO_SETS>
__global__ __launch_bounds__(256, 2) void gemm_b3_kernel(GemmB3Args g) {
  // [A, B][h, m, l][128 rows][64 B]
  __shared__ __attribute__((aligned(16))) char lds[2][3][kB3PartBytes];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r16 = lane & 15, kc = lane >> 4;
  // Block -> (slice, tile).  Workgroups are dealt round-robin to the 8 XCDs
  // (one L2 each): block L runs on XCD L % 8.  The blocks that share operands
  // are made to run on one XCD back to back: without split-K the column tiles
  // of a row block (same rows of A); with it all tiles of a slice (same k rows
  // of both operands).
  const int64_t tiles_n = (g.N + kB3BN - 1) / kB3BN;
  const int64_t tiles_m = (g.M + kB3BM - 1) / kB3BM;
  const int64_t inner = g.slices > 1 ? tiles_m * tiles_n : tiles_n;
  const int64_t slot = (int64_t)blockIdx.x >> 3;
  const int64_t outer = (slot / inner) * 8 + (blockIdx.x & 7);
  const int64_t in = slot % inner;
  int64_t tile_m, tile_n;
  int z;
  if (g.slices > 1) {
    z = (int)outer;
    tile_m = in / tiles_n;
    tile_n = in % tiles_n;
    if (z >= g.slices) return;                     // whole block (grid padding)
  } else {
    z = 0;
    tile_m = outer;
    tile_n = in;
    if (tile_m >= tiles_m) return;
  }
  const int64_t m0 = tile_m * kB3BM;
  const int64_t n0 = tile_n * kB3BN;
  const int64_t k_begin = (int64_t)z * g.k_chunk;
  const int64_t k_stop = k_begin + g.k_chunk < g.K ? k_begin + g.k_chunk : g.K;
  const int k_len = k_stop > k_begin ? (int)(k_stop - k_begin) : 0;
  const int nk = (k_len + kB3BK - 1) / kB3BK;
  const int a_left = (int)(g.M - m0 < kB3BM ? g.M - m0 : kB3BM);
  const int b_left = (int)(g.N - n0 < kB3BN ? g.N - n0 : kB3BN);

  // one resource per operand tile: exactly the bytes the tile may read (an
  // empty slice: none)
  const int a_bytes =
      k_len == 0 ? 0
                 : (int)((A_KC ? ((int64_t)a_left - 1) * g.lda + k_len
                               : ((int64_t)k_len - 1) * g.lda + a_left) * 4);
  const int b_bytes =
      k_len == 0 ? 0 : (int)((((int64_t)k_len - 1) * g.ldb + b_left) * 4);
  const __amdgpu_buffer_rsrc_t ars = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(A_KC ? g.A + m0 * g.lda + k_begin : g.A + k_begin * g.lda + m0),
      0, a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(g.B + k_begin * g.ldb + n0), 0, b_bytes, 0x00020000);
  const unsigned lda = (unsigned)g.lda, ldb = (unsigned)g.ldb;

  constexpr int kSets = TWO_SETS ? 2 : 1;
  f32x4 acc[kSets][4][4];
#pragma unroll
  for (int t = 0; t < kSets; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][i][j][r] = 0.f;

  u32x4 ra[4], rb[4];
  b3_stage_load<A_KC>(ars, lda, a_left, 0, k_len, tid, ra);
  b3_stage_load<false>(brs, ldb, b_left, 0, k_len, tid, rb);
  for (int kt = 0; kt < nk; ++kt) {
    b3_stage_store<A_KC>(lds[0][0], tid, ra);
    b3_stage_store<false>(lds[1][0], tid, rb);
    __syncthreads();
    // the next step's operands (past the slice: all zero, nothing is fetched)
    b3_stage_load<A_KC>(ars, lda, a_left, (kt + 1) * kB3BK, k_len, tid, ra);
    b3_stage_load<false>(brs, ldb, b_left, (kt + 1) * kB3BK, k_len, tid, rb);
    uint4 af[4][3];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int p = 0; p < 3; ++p)
        af[mi][p] = *reinterpret_cast<const uint4*>(
            lds[0][p] + b3_lds_off(wm * 64 + mi * 16 + r16, kc));
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      uint4 bf[3];
#pragma unroll
      for (int p = 0; p < 3; ++p)
        bf[p] = *reinterpret_cast<const uint4*>(
            lds[1][p] + b3_lds_off(wn * 64 + ni * 16 + r16, kc));
      // (part of A, part of B): the small products first, hh last
      constexpr int pa[6] = {1, 2, 0, 1, 0, 0};
      constexpr int pb[6] = {1, 0, 2, 0, 1, 0};
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        constexpr int last = kSets - 1;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
          f32x4& c = acc[q == 5 ? 0 : last][mi][ni];
          c = mfma_k32<false>(af[mi][pa[q]], bf[pb[q]], c);
        }
      }
    }
    __syncthreads();
  }

  // C/D layout of the 16x16 MFMA: column = lane & 15, row = 4 (lane >> 4) + e
  const float* __restrict__ X = g.X;
  float* __restrict__ C = g.C;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int64_t row0 = m0 + wm * 64 + mi * 16 + 4 * kc;
    float x[4][4];
    if (MINUS) {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int64_t col = n0 + wn * 64 + ni * 16 + r16;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          x[ni][e] = (row0 + e < g.M && col < g.N)
                         ? X[(row0 + e) * g.ldc + col] : 0.f;
      }
    }
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int64_t col = n0 + wn * 64 + ni * 16 + r16;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = acc[0][mi][ni][e];
        if (TWO_SETS) v += acc[kSets - 1][mi][ni][e];
        if (row0 + e < g.M && col < g.N) {
          if (MINUS)
            C[(row0 + e) * g.ldc + col] = sub_rn(v, x[ni][e]);
          else
            C[(int64_t)z * g.slab_stride + (row0 + e) * g.ldc + col] = v;
        }
      }
    }
  }
}

// ---- the dictionary gradient of the fully-connected update on this kernel
// E = C D - X, then slabs[z] = (C^T E) over slice z of the batch.  `slices` and
// the K range of a slice are those of the exact-f32 route (gradient_slices,
// launch_gemm_f32), so the workspace and the slab reduction are shared.
//
// Preconditions (fc_gradient_b3_usable): 16-byte aligned pointers; n and s
// multiples of 64 (16-byte loads never straddle an edge, no K tail in the
// first product); every tile's byte range within a 2 GiB buffer resource.
constexpr int64_t kB3MinBatch = 1024;

static inline bool fc_gradient_b3_usable(const void* images,
                                         const void* dictionary,
                                         const void* codes, const void* grad,
                                         int64_t b, int64_t n, int64_t s,
                                         int slices) {
  const uintptr_t bits = reinterpret_cast<uintptr_t>(images) |
                         reinterpret_cast<uintptr_t>(dictionary) |
                         reinterpret_cast<uintptr_t>(codes) |
                         reinterpret_cast<uintptr_t>(grad);
  if (bits & 15) return false;
  if (n % 64 || s % 64 || b < kB3MinBatch || slices < 1) return false;
  const int64_t wide = n > s ? n : s;
  const int64_t chunk = ceil_div(ceil_div(b, slices), kGemmBK) * kGemmBK;
  const int64_t rows = chunk > 128 ? chunk : 128;
  return rows * wide * 4 < 0x7fffffffLL;
}

// Where the route is the default: from the batch at which it is measured
// faster than the exact-f32 pair (profiles/fc_gradient_b3.txt: from 8192 rows
// at n = 256, s = 1024, and in proportion to the work of a row below that).
static inline bool fc_gradient_b3_faster(int64_t b, int64_t n, int64_t s) {
  return b >= 8192 && (double)b * (double)n * (double)s >= 2147483648.0;
}

// two_sets: hh and the cross products in separate accumulators
int launch_fc_gradient_b3(const float* images, const float* dictionary,
                          const float* codes, float* E, float* slabs,
                          int slices, int64_t b, int64_t n, int64_t s,
                          bool two_sets, hipStream_t st);

}  // namespace vtc
