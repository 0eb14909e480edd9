/*
 * vtc_vq_large.h -- twelfth header of libvtc_hip.so: the vector quantiser of
 * vtc_vq.h for codebooks of up to 131 072 codewords.  The experiment's live
 * block starts its Mod3 fit from vec_init_num_bins = 100000 candidates;
 * vtc_vq.h stops at VTC_VQ_MAX_CODEWORDS = 4096, and its entry points stay
 * exactly as they are.  DESIGN.md 4.20.
 *
 *   vectors (b, d), codebook -> vtc_vq_large_assign     -> indices, dequantised
 *   vectors, state           -> vtc_vq_large_lloyd_step -> state after one step
 *   indices [b]              -> vtc_vq_large_index_counts -> counts of every index
 *
 * The contract is the one written in vtc_vq.h, word for word, with
 * 1 <= kmax <= VTC_VQ_LARGE_MAX_CODEWORDS in place of VTC_VQ_MAX_CODEWORDS:
 * the quantiser's arrays, the assignment rule (float64 scan in index order,
 * every operation rounded separately, ties to the lowest index, NaN rows get
 * -1 and are counted in status), the semantics of a Lloyd step (pinning,
 * compaction in order, lengths, zero_index, the convergence test, the frozen
 * and all-NaN copies, a step in place), struct vtc_vq_state, the conventions
 * of vtc_quality.h (device pointers with the alignment of their element, the
 * workspace 256 bytes, `stream` last, no allocation inside, null pointers, bad
 * sizes and a short workspace answered before any device work, every output
 * element written by the call).  1 <= d <= VTC_VQ_MAX_DIM.  A larger d or kmax
 * answers VTC_ERR_UNSUPPORTED and names the limit.
 *
 * The order of the float64 sums is that of vtc_vq.h as well.  S_i (every
 * component) and D_i: within a block of VTC_VQ_ROWS = 2048 rows, for
 * g = 0 .. 15 the member rows whose row number within the block is g mod 16,
 * in ascending order, each sum started from 0.0; these sixteen in ascending g;
 * then the blocks in ascending order, started from 0.0.  D and R: for
 * p = 0 .. 1023 the cells i = p mod 1024 in ascending order, each sum started
 * from 0.0; these 1024 in ascending p, started from 0.0.
 *
 * A block in which a cell has no member is skipped here, where vtc_vq.h adds
 * that block's partial.  Such a partial started at +0.0 and had nothing added
 * to it, so it is +0.0; a running sum that started at +0.0 is never -0.0 (a
 * float64 sum is -0.0 only when both terms are), and s + (+0.0) == s bit for
 * bit for every other s.  Skipping the block therefore changes no bit, and
 * for kmax <= VTC_VQ_MAX_CODEWORDS every function below returns exactly the
 * bits of its vtc_vq_* twin.
 */
#ifndef VTC_VQ_LARGE_H_
#define VTC_VQ_LARGE_H_

#include "vtc_vq.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTC_VQ_LARGE_ABI_VERSION 1

#define VTC_VQ_LARGE_MAX_CODEWORDS 131072

int vtc_vq_large_abi_version(void);

/* vtc_vq_assign with 1 <= kmax <= 131072.  No workspace. */
int vtc_vq_large_assign(const float* vectors, int64_t b, int32_t d,
                        const double* codebook, const double* lengths,
                        const int32_t* k, int32_t kmax, double lambda,
                        int32_t* indices, float* dequantized, int64_t* status,
                        void* stream);

/* workspace: with c = ceil(b / 2048) blocks and pad() rounding up to 256
 * bytes, the indices and squared distances of the rows; for every block the
 * sorted list of the cells that have a member in it (at most 2048), how many
 * there are, and beside the list the sums of the members, of their squared
 * distances and their counts; the members and the summed distances of every
 * cell; the members and the source cell of every new slot; two records of the
 * step:
 *   pad(4 b) + pad(8 b)
 *   + pad(4 * 2048 c) + pad(4 c) + pad(8 * 2048 c d) + pad(8 * 2048 c)
 *   + pad(4 * 2048 c)
 *   + pad(8 kmax) + pad(8 kmax) + pad(8 kmax) + pad(4 kmax) + 256 + 256.
 * No term holds the product of c and kmax.  0 for a shape the call refuses. */
size_t vtc_vq_large_lloyd_step_workspace_bytes(int64_t b, int32_t d,
                                               int32_t kmax);

/* vtc_vq_lloyd_step with 1 <= kmax <= 131072: the same outputs, the same order
 * of the sums (above). */
int vtc_vq_large_lloyd_step(const float* vectors, int64_t b, int32_t d,
                            int32_t kmax, double lambda, double epsilon,
                            int32_t pin_zero, const vtc_vq_state* in,
                            const vtc_vq_state* out, int64_t* status,
                            void* workspace, size_t workspace_bytes,
                            void* stream);

/* vtc_vq_index_counts with 1 <= kmax <= 131072.  No workspace. */
int vtc_vq_large_index_counts(const int32_t* indices, int64_t b, int32_t kmax,
                              int64_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTC_VQ_LARGE_H_ */
