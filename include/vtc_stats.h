/*
 * vtc_stats.h -- sixth header of libvtc_hip.so: the numbers behind the
 * reference's code plots, utils/plotting.py:643-893 of
 * spencerkent/vision-transform-codes (display_code_marginal_densities,
 * display_2d_code_densities) and utils/misc.py:24-76 (rotational_average).
 * DESIGN.md 4.14.
 *
 *   codes (b, s) -> vtc_code_summary          -> kept, min, max, mean, variance
 *                                                of every column
 *   codes, ranges -> vtc_code_histogram       -> np.histogram of every column
 *   codes, pairs -> vtc_code_joint_histogram  -> np.histogramdd of column pairs
 *   images, map  -> vtc_binned_mean           -> the mean of every bin of a map
 *
 * The filter, shared by the three code entry points: `ignore` is float32
 * [n_ignore] on the DEVICE, 0 <= n_ignore <= 8 (NULL allowed when it is 0).  A
 * value x is KEPT iff x != v for every v of the list, the plain IEEE
 * comparison of the reference's filter_code_vals: ignoring 0.0 drops -0.0
 * too, a NaN in the list drops nothing, and a NaN value is always kept.
 *
 * The histogram contract is np.histogram(kept.astype(float64),
 * np.linspace(lo, hi, bins + 1)) with float64 edges:
 *   - e_i = lo + i * step, step = (hi - lo) / bins, the product and the sum
 *     rounded separately (never fused); e_bins = hi exactly;
 *   - bin i is [e_i, e_{i+1}), the last bin is closed on the right;
 *   - a kept finite value outside [lo, hi] is not counted, a non-finite value
 *     is not counted;
 *   - lo == hi: every kept value equal to it lands in the LAST bin;
 *   - lo or hi NaN, or lo > hi: the row of counts is zero.
 * The bin index is guessed as floor((x - lo) * bins / (hi - lo)) and then
 * moved down while x < e_k and up while x >= e_{k+1}: the comparison against
 * the edges decides, the guess only starts near it.
 *
 * The functions live in the same shared library as those of the other five
 * headers and follow the conventions stated at the top of vtc_quality.h:
 * device pointers with the alignment of their element and no more (the
 * workspace 256 bytes), `stream` last, no allocation inside, null pointers,
 * bad sizes and a short workspace answered before any device work, every
 * output element written by the call itself.  Every output is bitwise
 * reproducible: floating-point sums run in a fixed order that depends on the
 * shape alone, there are no floating-point atomics.  Counts are summed with
 * integer atomics, whose result does not depend on the order.
 */
#ifndef VTC_STATS_H_
#define VTC_STATS_H_

#include "vtc_quality.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTC_STATS_ABI_VERSION 1

#define VTC_STATS_MAX_IGNORE 8
#define VTC_STATS_MAX_BINS 4096        /* vtc_code_histogram, vtc_binned_mean */
#define VTC_STATS_MAX_JOINT_BINS 256   /* per axis */
#define VTC_STATS_SUMMARY_ROWS 512     /* rows of one partial sum */
#define VTC_STATS_JOINT_ROWS 4096      /* rows of one partial range */
#define VTC_STATS_BINNED_SAMPLES 4096  /* samples of one partial bin sum */

int vtc_stats_abi_version(void);

/* workspace: with n = ceil(b / 512) * s partials, one float64 array and four
 * 4-byte arrays of n elements, each rounded up to 256 bytes:
 * pad(8 n) + 4 pad(4 n).  0 for a shape the call refuses. */
size_t vtc_code_summary_workspace_bytes(int64_t b, int64_t s);

/* codes: float32 (b, s), b >= 1, s >= 1; b * s is not limited to 2^31.
 * Outputs, one per column:
 *   kept      int64    values the filter keeps
 *   nonfinite int64    kept values that are NaN or +-inf; they are left out of
 *                      lo, hi, mean and var
 *   lo, hi    float64  the float32 minimum / maximum of the kept finite
 *                      values, widened; NaN when there is none
 *   mean, var float64  over the n = kept - nonfinite finite kept values, ddof
 *                      = 0, two passes (the mean, then the squares of x - mean),
 *                      NaN when n = 0.
 * Order of the float64 sums: rows in blocks of 512; inside a block four
 * interleaved sums (rows r, r + 4, ... for r = 0 .. 3 of the block), added
 * 0 + 1 + 2 + 3; the blocks added in ascending order. */
int vtc_code_summary(const float* codes, int64_t b, int64_t s,
                     const float* ignore, int32_t n_ignore, int64_t* kept,
                     double* lo, double* hi, double* mean, double* var,
                     int64_t* nonfinite, void* workspace,
                     size_t workspace_bytes, void* stream);

/* workspace: step and bins / (hi - lo) of every column, two float64 arrays of
 * s elements, each rounded up to 256 bytes: 2 pad(8 s).  0 for a shape the
 * call refuses. */
size_t vtc_code_histogram_workspace_bytes(int64_t b, int64_t s, int32_t bins);

/* lo, hi: float64[s], the caller's range of every column (vtc_code_summary's,
 * or one shared range).  counts: int64 (s, bins), zeroed by the call.
 * 1 <= bins <= 4096; more answer VTC_ERR_UNSUPPORTED. */
int vtc_code_histogram(const float* codes, int64_t b, int64_t s,
                       const float* ignore, int32_t n_ignore, const double* lo,
                       const double* hi, int32_t bins, int64_t* counts,
                       void* workspace, size_t workspace_bytes, void* stream);

/* workspace: with n = n_pairs * ceil(b / 4096) partial ranges, five 4-byte
 * arrays of n elements, each rounded up to 256 bytes: 5 pad(4 n).  0 for a
 * shape the call refuses. */
size_t vtc_code_joint_histogram_workspace_bytes(int64_t b, int64_t n_pairs);

/* pairs: int32 (n_pairs, 2) column indices on the device, n_pairs >= 1.
 * max_column: 1 <= max_column <= s; a pair with an index outside
 * [0, max_column) is skipped: kept = -1, lo = hi = NaN, counts zero.
 * A row is kept for a pair iff both of its values are kept.  Outputs:
 *   kept   int64[n_pairs]            rows kept
 *   lo, hi float64 (n_pairs, 2)      minimum / maximum of each axis over the
 *                                    kept rows whose two values are finite;
 *                                    NaN when there is none
 *   counts int64 (n_pairs, bins, bins), first axis = first column of the pair;
 *          np.histogramdd over those rows with np.linspace(lo, hi, bins + 1)
 *          per axis, the rules above on each axis.
 * 1 <= bins <= 256; more answer VTC_ERR_UNSUPPORTED. */
int vtc_code_joint_histogram(const float* codes, int64_t b, int64_t s,
                             const int32_t* pairs, int64_t n_pairs,
                             int32_t max_column, const float* ignore,
                             int32_t n_ignore, int32_t bins, int64_t* kept,
                             double* lo, double* hi, int64_t* counts,
                             void* workspace, size_t workspace_bytes,
                             void* stream);

/* workspace: with c = ceil(h * w / 4096) blocks of samples, count * c * nbins
 * float64 partial sums and c * nbins int32 partial member counts, each array
 * rounded up to 256 bytes: pad(8 count c nbins) + pad(4 c nbins).  0 for a
 * shape the call refuses. */
size_t vtc_binned_mean_workspace_bytes(int64_t count, int32_t h, int32_t w,
                                       int32_t nbins);

/* images: (count, h, w) of `dtype`, VTC_DTYPE_F32 (widened on load) or
 * VTC_DTYPE_F64.  bin_of: int32 (h, w), the bin of every sample; a value
 * outside [0, nbins) belongs to no bin.  1 <= nbins <= 4096 (more answer
 * VTC_ERR_UNSUPPORTED).  means: float64 (count, nbins), the sum of the bin's
 * samples divided by their number, NaN for an empty bin; members: int64
 * [nbins].  Order of a sum: the samples of a block of 4096 in row-major order,
 * then the blocks in ascending order. */
int vtc_binned_mean(const void* images, int dtype, const int32_t* bin_of,
                    int64_t count, int32_t h, int32_t w, int32_t nbins,
                    double* means, int64_t* members, void* workspace,
                    size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTC_STATS_H_ */
