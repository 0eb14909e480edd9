/*
 * vtc_quant.h -- seventh header of libvtc_hip.so: the scalar quantisers of
 * the `utils.quantization` module that the experiments of
 * spencerkent/vision-transform-codes import
 * (experiments/rate_distortion_sparse_coding.py:23) and the reference never
 * shipped.  DESIGN.md 4.15.
 *
 *   codes (b, s), codebooks -> vtc_quant_assign       -> indices, dequantised
 *   codes, state            -> vtc_quant_lloyd_step   -> state after one step
 *   indices (b, s)          -> vtc_quant_index_counts -> counts of every index
 *
 * Every column j of the codes has a quantiser of its own:
 *   codebooks  float64 (s, kmax)  the codewords
 *   lengths    float64 (s, kmax)  bits per codeword
 *   k          int32   [s]        codewords in use, 1 <= k[j] <= kmax; the
 *                                 slots i >= k[j] are never read
 *   zero_index int32   [s]        index of the codeword whose value is
 *                                 exactly 0.0, or -1
 * with 1 <= kmax <= VTC_QUANT_MAX_CODEWORDS.  A k[j] outside [1, kmax] is
 * clamped into it before any read.
 *
 * The assignment rule, shared by vtc_quant_assign and vtc_quant_lloyd_step:
 * the index of x in column j is the lowest i < k[j] that minimises
 *   d * d + lambda * lengths[j, i],     d = (double)x - codebooks[j, i],
 * in float64, the two products and the sum rounded separately (never fused).
 * When lambda == 0 the cost is d * d alone and `lengths` is not read.  The
 * cells are scanned in index order and a later cell wins only with a strictly
 * smaller cost, so ties go to the lowest index and -0.0 is assigned like
 * 0.0.  A NaN code gets index -1, is no member of any cell, and is counted in
 * status[0] (int64, zeroed by the call).
 *
 * The functions live in the same shared library as those of the other six
 * headers and follow the conventions stated at the top of vtc_quality.h:
 * device pointers with the alignment of their element and no more (the
 * workspace 256 bytes), `stream` last, no allocation inside, null pointers,
 * bad sizes and a short workspace answered before any device work, every
 * output element written by the call itself.  Every output is bitwise
 * reproducible: floating-point sums run in a fixed order that depends on the
 * shape alone, there are no floating-point atomics.  Counts are summed with
 * integer atomics or as integers, whose result does not depend on the order.
 */
#ifndef VTC_QUANT_H_
#define VTC_QUANT_H_

#include "vtc_quality.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTC_QUANT_ABI_VERSION 1

#define VTC_QUANT_MAX_CODEWORDS 1024
#define VTC_QUANT_ROWS 512   /* rows of one block of vtc_quant_lloyd_step */
#define VTC_QUANT_LANES 8    /* interleaved partial sums of one block */

int vtc_quant_abi_version(void);

/* codes: float32 (b, s), b >= 1, s >= 1; b * s is not limited to 2^31.
 * lengths may be NULL when lambda == 0.  lambda >= 0 (a negative or NaN
 * lambda is a bad argument).  Outputs:
 *   indices      int32 (b, s)    the rule above
 *   dequantized  float32 (b, s)  or NULL: the assigned codeword rounded once
 *                                to float32, NaN where the index is -1
 *   status       int64 [1]       the number of NaN codes
 * kmax > 1024 answers VTC_ERR_UNSUPPORTED.  No workspace. */
int vtc_quant_assign(const float* codes, int64_t b, int64_t s,
                     const double* codebooks, const double* lengths,
                     const int32_t* k, int32_t kmax, double lambda,
                     int32_t* indices, float* dequantized, int64_t* status,
                     void* stream);

/* The per-column state of a Lloyd fit: the four arrays above and
 *   counts     int64   (s, kmax)  members of every codeword
 *   cost       float64 (s, 3)     {J, D, R} of the last step
 *   active     int32   [s]        non-zero: the column is still being fitted
 *   iterations int32   [s]        steps taken */
typedef struct vtc_quant_state {
  double* codebooks;
  double* lengths;
  int64_t* counts;
  double* cost;
  int32_t* k;
  int32_t* zero_index;
  int32_t* active;
  int32_t* iterations;
} vtc_quant_state;

/* workspace: with n = ceil(b / 512) * s * kmax partials, the float64 sums of
 * the members, the float64 sums of their squared errors and the int32 member
 * counts, each array rounded up to 256 bytes: 2 pad(8 n) + pad(4 n).  0 for a
 * shape the call refuses. */
size_t vtc_quant_lloyd_step_workspace_bytes(int64_t b, int64_t s,
                                            int32_t kmax);

/* One step: assign, accumulate, update.  `in` is read, `out` is written, all
 * eight arrays of both non-NULL; `out` may be `in` member for member (a step
 * in place), any other overlap is undefined.  The two structs are read on the
 * host during the call.
 *
 * A column with in->active[j] == 0 is copied from `in` to `out` bit for bit
 * (all kmax slots) and takes no part in the sums.  For an active column, with
 * k0 = in->k[j]:
 *   - every non-NaN code is assigned by the rule above from in->codebooks and
 *     in->lengths (lengths are read even when lambda == 0: R needs them);
 *   - n_i = members of cell i, S_i = the sum of its members, D_i = the sum of
 *     d * d over its members, n = sum of n_i;
 *   - D = sum of D_i, R = sum over the cells with n_i > 0 of n_i * lengths_i
 *     (the bits of the assignment under the lengths it was made with),
 *     J = D + lambda * R, and J = D when lambda == 0;
 *   - cell i is kept iff n_i > 0, or pin_zero != 0 and i == in->zero_index[j];
 *     the kept cells move down to the slots 0 .. k' - 1 in order, out->k[j] =
 *     k';  codeword = S_i / n_i, or exactly 0.0 for the pinned cell; length =
 *     -log2(n_i / n), +inf for a pinned cell without members; count = n_i;
 *     the slots i >= k' get codeword 0.0, length 0.0, count 0;
 *   - out->zero_index[j] = the new slot of cell in->zero_index[j] if it is
 *     kept and its new codeword is exactly 0.0, else -1;
 *   - out->cost[j] = {J, D, R}; out->iterations[j] = in->iterations[j] + 1;
 *   - out->active[j] = 0 iff in->iterations[j] > 0 and
 *     (J_prev - J) <= epsilon * J_prev with J_prev = in->cost[j, 0]; else 1.
 *     The first step (in->iterations[j] == 0) never clears.
 *   - n == 0 (every code of the column NaN): the quantiser is copied as it
 *     was, cost = NaN, active = 0.
 * status[0]: NaN codes met in active columns.
 *
 * Order of the float64 sums.  S_i and D_i: within a block of 512 rows, for
 * g = 0 .. 7 the member rows whose row number within the block is g mod 8, in
 * ascending order, each sum started from 0.0; these eight in ascending g;
 * then the blocks in ascending order.  D and R: the cells in ascending order
 * of i.  n_i and n are integers. */
int vtc_quant_lloyd_step(const float* codes, int64_t b, int64_t s,
                         int32_t kmax, double lambda, double epsilon,
                         int32_t pin_zero, const vtc_quant_state* in,
                         const vtc_quant_state* out, int64_t* status,
                         void* workspace, size_t workspace_bytes,
                         void* stream);

/* indices: int32 (b, s).  counts: int64 (s, kmax), zeroed by the call:
 * counts[j, i] = rows with indices[r, j] == i; an index outside [0, kmax) is
 * not counted.  kmax > 1024 answers VTC_ERR_UNSUPPORTED.  No workspace. */
int vtc_quant_index_counts(const int32_t* indices, int64_t b, int64_t s,
                           int32_t kmax, int64_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTC_QUANT_H_ */
