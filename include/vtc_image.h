/*
 * vtc_image.h -- second header of libvtc_hip.so: the image-level half of
 * utils/image_processing.py of spencerkent/vision-transform-codes, i.e. what a
 * caller needs after training to take a whole image through a learned
 * dictionary and back (whiten, tile, code, re-tile, unwhiten).
 *
 *   utils/image_processing.py:63-92    filter_fd                 -> vtc_img_filter_fd
 *   utils/image_processing.py:18-60    filter_sd (convolve2d 'same' 'symm',
 *                                      or two convolve1d 'reflect' passes)
 *                                                                -> vtc_img_filter_sd
 *   utils/image_processing.py:95-114   downsample                -> vtc_img_downsample
 *   utils/image_processing.py:597-648  patches_from_single_image -> vtc_img_tile_patches
 *   utils/image_processing.py:651-699  assemble_image_from_patches
 *                                                                -> vtc_img_assemble_patches
 *   utils/image_processing.py:311-335  unwhiten_center_surround  -> vtc_img_filter_fd with 1 / F
 *                                                                   (the Python layer forms 1 / F)
 *
 * The functions live in the same shared library as those of vtc_hip.h and
 * follow its conventions:
 *   - every pointer is a DEVICE pointer to a contiguous row-major array; sizes
 *     are element counts; `stream` is a hipStream_t passed as void* (NULL =
 *     the null stream).
 *   - alignment: a data pointer needs the alignment of its element and no
 *     more (4 bytes for float32 / int32, 8 for float64 -- a complex128 array
 *     is read as pairs of float64 --, 1 for uint8).  Every kernel here reads
 *     and writes the caller's arrays element by element; no entry point
 *     refuses a pointer for its alignment.  `workspace` must be 256-byte
 *     aligned.
 *   - functions only enqueue work on `stream` and return.  Every device
 *     operation of a call is issued on `stream`; calls on different streams of
 *     one device may be in flight together, provided they share no output and
 *     no workspace (vtc_hip.h, Conventions, "streams").
 *   - no allocation inside: scratch comes from the caller as `workspace`,
 *     sized by the matching *_workspace_bytes() query.  The hipFFT plans of
 *     vtc_img_filter_fd are the only per-process device state here: one pair
 *     per (device, stream, call shape), made at the first such call, bound to
 *     that stream then and kept, so that two streams never share a plan.
 *   - return value: VTC_OK or a VTC_ERR_* code of vtc_hip.h; vtc_last_error()
 *     gives text.  Null pointers, bad sizes and unsupported shapes are
 *     answered before any device work.
 *
 * Images are channel-last stacks (count, h, w, c) of `dtype` (enum vtc_dtype
 * of vtc_hip.h: float32 or uint8), each channel handled on its own, as the
 * reference's per-channel loops do.
 */
#ifndef VTC_IMAGE_H_
#define VTC_IMAGE_H_

#include "vtc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTC_IMAGE_ABI_VERSION 1

int vtc_image_abi_version(void);

/* ---- filter_fd ----------------------------------------------------------
 * out (count, h, w, c) float32 = real(ifft2(filter_dft * fft2(image padded
 * with zeros to (fh, fw))))[0:h, 0:w], transforms and product in float64,
 * one rounding to float32.  filter_dft: (fh, fw) complex128 (interleaved
 * re, im), fh >= h and fw >= w (smaller: VTC_ERR_INVALID_ARGUMENT, the
 * reference's "don't undersample DFT").  The filter may be any complex array:
 * the real part of the inverse transform of F X, X the spectrum of a real
 * image, is the inverse transform of Fh X with Fh[k] = (F[k] + conj(F[-k]))
 * / 2, so the call runs a real-to-complex / complex-to-real pair (hipFFT D2Z
 * / Z2D, opened at first use) on the half spectrum with the filter
 * symmetrised as it is read.  out must not alias images. */
size_t vtc_img_filter_fd_workspace_bytes(int64_t count, int32_t h, int32_t w,
                                         int32_t c, int32_t fh, int32_t fw);
int vtc_img_filter_fd(const void* images, int dtype, const double* filter_dft,
                      float* out, int64_t count, int32_t h, int32_t w,
                      int32_t c, int32_t fh, int32_t fw, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---- filter_sd ----------------------------------------------------------
 * Two routes, chosen by the pointers:
 *   filter != NULL (separable_vert = separable_horz = NULL): the general
 *     (fh, fw) float64 filter.  scipy's convolve2d(image, filter, 'same',
 *     boundary='symm') per channel: a true convolution, out[y, x] = sum_{j,i}
 *     filter[j, i] * image[y + (fh-1)/2 - j, x + (fw-1)/2 - i] (integer
 *     division: the centring of 'same' for even sizes), indices reflected
 *     about the image edge with the edge sample repeated; float64 sums in a
 *     fixed order (j, i descending), one rounding to float32.  One LDS tile
 *     of the image with its reflected halo and the filter per workgroup; no
 *     workspace (NULL, 0).
 *   separable_vert (fh) and separable_horz (fw) != NULL, float64: the
 *     reference's two convolve1d(mode='reflect') passes, centre n / 2.  The
 *     horizontal pass is stored in the image's own element type, as scipy
 *     does -- float32 rounded to nearest, uint8 truncated toward zero and
 *     wrapped modulo 256 --, the vertical pass runs on that in float64 and
 *     rounds to float32.  workspace: the intermediate, count*h*w*c float32.
 *     `filter` is ignored.
 * Restriction: 1 <= fh <= min(h, 63) and 1 <= fw <= min(w, 63); a filter
 * larger than the image in either axis or beyond 63 taps per axis answers
 * VTC_ERR_UNSUPPORTED.  out must not alias images. */
size_t vtc_img_filter_sd_workspace_bytes(int64_t count, int32_t h, int32_t w,
                                         int32_t c, int32_t fh, int32_t fw,
                                         int separable);
int vtc_img_filter_sd(const void* images, int dtype, const double* filter,
                      const double* separable_vert,
                      const double* separable_horz, float* out, int64_t count,
                      int32_t h, int32_t w, int32_t c, int32_t fh, int32_t fw,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- tiling -------------------------------------------------------------
 * Pure moves: patches and images have the element type `dtype`.
 * patches (count, k, ph, pw, c), k = (h / ph) * (w / pw): patch (i, j) of the
 * row-major grid is images[n, i*ph:(i+1)*ph, j*pw:(j+1)*pw, :]; pixels right
 * of and below the last whole patch are ignored.  ph <= h, pw <= w. */
int vtc_img_tile_patches(const void* images, int dtype, void* patches,
                         int64_t count, int32_t h, int32_t w, int32_t c,
                         int32_t ph, int32_t pw, void* stream);
/* image (out_h, out_w, c) = zeros, then patch p (ph, pw, c) written at
 * (positions[2p], positions[2p+1]) = (row, column) of its upper left corner,
 * for p = 0 .. k-1 in that order: where patches overlap the one with the
 * larger index is kept, as in the reference's loop.  positions: (k, 2) int32
 * in the caller's order.  A patch that does not lie inside the image is
 * skipped, never written out of bounds.
 * positions_disjoint != 0: the caller has checked that no two patches
 * overlap; the patches are then scattered in parallel after a memset.
 * 0: every output element looks for the last patch that covers it (k
 * comparisons per element, no write races, any table). */
int vtc_img_assemble_patches(const void* patches, int dtype,
                             const int32_t* positions, void* image, int64_t k,
                             int32_t ph, int32_t pw, int32_t c, int32_t out_h,
                             int32_t out_w, int positions_disjoint,
                             void* stream);

/* ---- downsample ---------------------------------------------------------
 * out (count, ceil(h / factor), ceil(w / factor), c) = images[:, ::factor,
 * ::factor, :], element type kept.  factor >= 1. */
int vtc_img_downsample(const void* images, int dtype, void* out, int64_t count,
                       int32_t h, int32_t w, int32_t c, int32_t factor,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTC_IMAGE_H_ */
