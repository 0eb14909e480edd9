/*
 * vtc_vq.h -- eighth header of libvtc_hip.so: the vector quantiser of the
 * `utils.quantization` module that the experiments of
 * spencerkent/vision-transform-codes import and the reference never shipped
 * (the "Mod2" / "Mod3" variants of
 * experiments/rate_distortion_sparse_coding.py quantise the sparse tail of a
 * code, 23 of 64 coefficients, as one vector).  DESIGN.md 4.16.
 *
 *   vectors (b, d), codebook -> vtc_vq_assign     -> indices, dequantised
 *   vectors, state           -> vtc_vq_lloyd_step -> state after one step
 *   indices [b]              -> vtc_vq_index_counts -> counts of every index
 *
 * One quantiser for all the rows of the (b, d) float32 vectors:
 *   codebook   float64 (kmax, d)  the codewords, row-major
 *   lengths    float64 [kmax]     bits per codeword
 *   k          int32   [1]        codewords in use; the slots i >= k are never
 *                                 read; a k outside [1, kmax] is clamped into
 *                                 it before any read
 *   zero_index int32   [1]        index of the codeword whose d components
 *                                 are all exactly 0.0, or -1
 * with 1 <= d <= VTC_VQ_MAX_DIM and 1 <= kmax <= VTC_VQ_MAX_CODEWORDS; a
 * larger d or kmax answers VTC_ERR_UNSUPPORTED.  b >= 1, and b * d is not
 * limited to 2^31.
 *
 * The assignment rule, shared by vtc_vq_assign and vtc_vq_lloyd_step: the
 * index of row x is the lowest i < k that minimises
 *   D_i + lambda * lengths[i],
 * where D_i starts from 0.0 and accumulates over t = 0 .. d - 1 in ascending
 * order, e = (double)x[t] - codebook[i, t], D_i = D_i + e * e: all float64,
 * every product and every sum rounded separately (never fused).  When
 * lambda == 0 the cost is D_i alone and `lengths` is not read.  The cells are
 * scanned in index order and a later cell wins only with a strictly smaller
 * cost, so ties go to the lowest index and -0.0 is assigned like 0.0.  A row
 * with any NaN component gets index -1, is a member of no cell, and is counted
 * once in status[0] (int64, zeroed by the call).  The distance is never formed
 * as |x|^2 - 2 x.c + |c|^2: that rounds differently and cancels for the
 * near-zero vectors that make up most of the data.
 *
 * The functions live in the same shared library as those of the other seven
 * headers and follow the conventions stated at the top of vtc_quality.h:
 * device pointers with the alignment of their element and no more (the
 * workspace 256 bytes), `stream` last, no allocation inside, null pointers,
 * bad sizes and a short workspace answered before any device work, every
 * output element written by the call itself.  Every output is bitwise
 * reproducible: floating-point sums run in a fixed order that depends on the
 * shape alone, there are no floating-point atomics.  Counts are integers.
 */
#ifndef VTC_VQ_H_
#define VTC_VQ_H_

#include "vtc_quality.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTC_VQ_ABI_VERSION 1

#define VTC_VQ_MAX_DIM 32
#define VTC_VQ_MAX_CODEWORDS 4096
#define VTC_VQ_ASSIGN_ROWS 256    /* rows of one workgroup of the scan */
#define VTC_VQ_TILE_DOUBLES 4096  /* one LDS tile of the codebook holds
                                   * 4096 / dp whole codewords, dp = d rounded
                                   * up to 4, 8, 16, 24 or 32 */
#define VTC_VQ_ROWS 2048          /* rows of one block of vtc_vq_lloyd_step */
#define VTC_VQ_LANES 16           /* interleaved partial sums of one block */
#define VTC_VQ_COST_LANES 1024    /* interleaved partial sums of D and R */

int vtc_vq_abi_version(void);

/* vectors: float32 (b, d).  lengths may be NULL (or hold +inf) when
 * lambda == 0.  lambda >= 0: a negative or NaN lambda is a bad argument.
 * Outputs:
 *   indices      int32 [b]        the rule above
 *   dequantized  float32 (b, d)   or NULL: the assigned codeword rounded once
 *                                 to float32, a whole row of NaN where the
 *                                 index is -1
 *   status       int64 [1]        the number of rows with a NaN component
 * No workspace. */
int vtc_vq_assign(const float* vectors, int64_t b, int32_t d,
                  const double* codebook, const double* lengths,
                  const int32_t* k, int32_t kmax, double lambda,
                  int32_t* indices, float* dequantized, int64_t* status,
                  void* stream);

/* The state of a Lloyd fit: the four arrays above and
 *   counts     int64   [kmax]  members of every codeword
 *   cost       float64 [3]     {J, D, R} of the last step
 *   active     int32   [1]     non-zero: the quantiser is still being fitted
 *   iterations int32   [1]     steps taken */
typedef struct vtc_vq_state {
  double* codebook;
  double* lengths;
  int64_t* counts;
  double* cost;
  int32_t* k;
  int32_t* zero_index;
  int32_t* active;
  int32_t* iterations;
} vtc_vq_state;

/* workspace: with c = ceil(b / 2048) blocks and pad() rounding up to 256
 * bytes, the indices and squared distances of the rows, the per-block sums of
 * the members, of their squared distances and their counts, the members and
 * the source cell of every new slot, and two records of the step:
 *   pad(4 b) + pad(8 b) + pad(8 c kmax d) + pad(8 c kmax) + pad(4 c kmax)
 *   + pad(8 kmax) + pad(4 kmax) + 256 + 256.
 * 0 for a shape the call refuses. */
size_t vtc_vq_lloyd_step_workspace_bytes(int64_t b, int32_t d, int32_t kmax);

/* One step: assign, accumulate, update.  `in` is read, `out` is written, all
 * eight arrays of both non-NULL; `out` may be `in` member for member (a step
 * in place), any other overlap is undefined.  The two structs are read on the
 * host during the call.
 *
 * With in->active[0] == 0 the state is copied from `in` to `out` bit for bit
 * (all kmax slots) and status[0] = 0.  Otherwise, with k0 = in->k[0]:
 *   - every row without NaN is assigned by the rule above from in->codebook
 *     and in->lengths (lengths are read even when lambda == 0: R needs them);
 *   - n_i = members of cell i, S_i = the component-wise sum of its members,
 *     D_i = the sum over its members of the D_i of the rule (the squared
 *     distance the scan formed), n = sum of n_i;
 *   - D = sum of D_i, R = sum over the cells with n_i > 0 of n_i * lengths_i,
 *     J = D + lambda * R, and J = D when lambda == 0;
 *   - cell i is kept iff n_i > 0, or pin_zero != 0 and i == in->zero_index[0];
 *     the kept cells move down to the slots 0 .. k' - 1 in order, out->k[0] =
 *     k';  codeword = S_i / n_i component by component, or exactly the zero
 *     vector for the pinned cell; length = -log2(n_i / n), +inf for a pinned
 *     cell without members; count = n_i; the slots i >= k' get codeword 0.0,
 *     length 0.0, count 0;
 *   - out->zero_index[0] = the new slot of cell in->zero_index[0] if it is
 *     kept and all d components of its new codeword are exactly 0.0, else -1;
 *   - out->cost = {J, D, R}; out->iterations[0] = in->iterations[0] + 1;
 *   - out->active[0] = 0 iff in->iterations[0] > 0 and
 *     (J_prev - J) <= epsilon * J_prev with J_prev = in->cost[0]; else 1.
 *     The first step never clears.
 *   - n == 0 (every row holds a NaN): the quantiser is copied as it was,
 *     cost = NaN, active = 0.
 * status[0]: the rows with a NaN component.
 *
 * Order of the float64 sums.  S_i (every component) and D_i: within a block
 * of 2048 rows, for g = 0 .. 15 the member rows whose row number within the
 * block is g mod 16, in ascending order, each sum started from 0.0; these
 * sixteen in ascending g; then the blocks in ascending order, started from
 * 0.0.  D and R: for p = 0 .. 1023 the cells i = p mod 1024 in ascending
 * order, each sum started from 0.0; these 1024 in ascending p, started from
 * 0.0.  n_i and n are integers. */
int vtc_vq_lloyd_step(const float* vectors, int64_t b, int32_t d,
                      int32_t kmax, double lambda, double epsilon,
                      int32_t pin_zero, const vtc_vq_state* in,
                      const vtc_vq_state* out, int64_t* status,
                      void* workspace, size_t workspace_bytes, void* stream);

/* indices: int32 [b].  counts: int64 [kmax], zeroed by the call: counts[i] =
 * rows with indices[r] == i; an index outside [0, kmax) is not counted.
 * (vtc_quant_index_counts stops at 1024 codewords.)  kmax > 4096 answers
 * VTC_ERR_UNSUPPORTED.  No workspace. */
int vtc_vq_index_counts(const int32_t* indices, int64_t b, int32_t kmax,
                        int64_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTC_VQ_H_ */
