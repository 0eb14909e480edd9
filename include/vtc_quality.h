/*
 * vtc_quality.h -- fifth header of libvtc_hip.so: the structural similarity
 * index of utils/plotting.py:42-64 of spencerkent/vision-transform-codes
 * (compute_ssim), the second distortion measure of its rate-distortion
 * experiments beside pSNR.  DESIGN.md 4.13.
 *
 *   two image stacks, one range per image -> vtc_ssim -> mean SSIM per image,
 *                                                        the SSIM maps
 *
 * The reference calls skimage.measure.compare_ssim(target, reconstruction,
 * data_range=R, gaussian_weights=True, sigma=1.5,
 * use_sample_covariance=False), which for 2-d images is, all in float64:
 *   1. the window: 11 taps per axis, exp(-k^2 / (2 * 1.5^2)) for k = -5 .. 5
 *      divided by their sum, applied as scipy.ndimage.gaussian_filter does:
 *      separably, the vertical axis first, boundary 'reflect' (the edge sample
 *      repeated);
 *   2. ux, uy, uxx, uyy, uxy: the filters of X, Y, X*X, Y*Y, X*Y;
 *      vx = uxx - ux*ux, vy = uyy - uy*uy, vxy = uxy - ux*uy;
 *   3. C1 = (0.01 R)^2, C2 = (0.03 R)^2,
 *      S = ((2 ux uy + C1) (2 vxy + C2)) / ((ux^2 + uy^2 + C1) (vx + vy + C2));
 *   4. the mean of S[5:h-5, 5:w-5].
 *
 * The functions live in the same shared library as those of vtc_hip.h,
 * vtc_image.h, vtc_codec.h and vtc_decode.h and follow their conventions:
 *   - every pointer is a DEVICE pointer to a contiguous row-major array;
 *     `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *   - alignment: a pointer needs the alignment of its element and no more
 *     (4 bytes for float32, 8 for float64).  `workspace` must be 256-byte
 *     aligned.
 *   - functions only enqueue work on `stream` and return; every device
 *     operation of a call is issued on `stream`.
 *   - no allocation inside: scratch comes from the caller as `workspace`,
 *     sized by the matching *_workspace_bytes() query.  No per-process state.
 *   - return value: VTC_OK or a VTC_ERR_* code of vtc_hip.h; vtc_last_error()
 *     gives text.  Null pointers, bad sizes and a short workspace are answered
 *     before any device work.
 *   - every output is bitwise reproducible from run to run and independent of
 *     the other images of the stack: all sums run in a fixed order, there are
 *     no floating-point atomics.
 */
#ifndef VTC_QUALITY_H_
#define VTC_QUALITY_H_

#include "vtc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTC_QUALITY_ABI_VERSION 1

/* float64 images: the element type this header adds to enum vtc_dtype of
 * vtc_hip.h (VTC_DTYPE_F32 = 0, VTC_DTYPE_U8 = 1). */
enum vtc_quality_dtype { VTC_DTYPE_F64 = 2 };

#define VTC_SSIM_RADIUS 5   /* the window has 2 * 5 + 1 taps per axis */

int vtc_quality_abi_version(void);

/* workspace: one float64 partial sum per 16 x 32 output tile of every image,
 * count * ceil(h / 16) * ceil(w / 32) of them, rounded up to 256 bytes.  0 for
 * a shape vtc_ssim refuses. */
size_t vtc_ssim_workspace_bytes(int64_t count, int32_t h, int32_t w);

/* x, y: (count, h, w) stacks of `dtype`, VTC_DTYPE_F32 or VTC_DTYPE_F64; a
 * float32 sample is widened to float64 as it is read, so that its squares and
 * products are exact.  data_range: float64[count], R of each image.
 * mean_out: float64[count].  map_out: NULL, or float64 (count, h, w), the
 * whole map S, uncropped (scikit-image's full=True); it must not overlap x or
 * y.  count >= 1 (else VTC_ERR_INVALID_ARGUMENT); h < 11 or w < 11, where the
 * reference raises ValueError, answers VTC_ERR_UNSUPPORTED.
 * Every product and sum is a separate float64 operation, never fused: two
 * identical images give exactly 1.0 in every sample.  R = 0 or a non-finite
 * sample gives what the formula gives (NaN), as in the reference. */
int vtc_ssim(const void* x, const void* y, int dtype, const double* data_range,
             double* mean_out, double* map_out, int64_t count, int32_t h,
             int32_t w, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTC_QUALITY_H_ */
