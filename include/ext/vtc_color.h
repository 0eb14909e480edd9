/*
 * vtc_color.h -- fourteenth header of libvtc_hip.so: the colour step of an
 * image-level rate-distortion point.  RGB <-> a luma / chroma space (or any
 * learned 3 x 3 colour basis), chroma planes down to reduced resolution and
 * back.  The reference has no colour path (its dataset_generation.py:149-150
 * leaves 'Kodak' at "This is next"); the arithmetic below is this header's
 * own and is stated to the operation, so that a float64 restatement agrees
 * with it bit for bit.  DESIGN.md 4.22.
 *
 *   RGB (count, h, w, 3) -> vtc_color_transform  -> YCbCr, one plane each
 *   Cb, Cr (count, h, w) -> vtc_plane_downsample -> (count, ceil(h / fv),
 *                                                    ceil(w / fh))
 *   ... each plane coded and decoded (vtc_image.h, vtc_codec.h, vtc_decode.h)
 *   Cb, Cr reduced       -> vtc_plane_upsample   -> (count, h, w)
 *   YCbCr                -> vtc_color_transform  -> RGB
 *
 * This header lives under include/ext/ like vtc_index_ans_split.h; include/
 * itself keeps the twelve headers it has.  The functions live in the same
 * shared library as those of the other thirteen headers and follow the
 * conventions of vtc_image.h: every data pointer is a DEVICE pointer to a
 * contiguous row-major float32 array and needs the alignment of its element
 * and no more, `stream` last, functions only enqueue work on `stream`, no
 * workspace, no allocation inside, no atomics.  Null pointers, bad sizes and
 * unsupported factors, layouts or modes are answered before any device work
 * with the argument named in vtc_last_error(): VTC_ERR_INVALID_ARGUMENT for a
 * null pointer, a size below 1, overlapping arrays and sizes that contradict
 * each other, VTC_ERR_UNSUPPORTED for a size, factor, layout or mode the
 * kernels do not take.  count = 0 is a bad size, as in vtc_image.h.
 * h * w <= 2^31 - 1 (of the larger plane); count is not limited to 2^31.
 * No inline assembly.
 *
 * ARITHMETIC, all three calls: float32 in, float32 out.  Every operation is
 * an IEEE float64 operation rounded on its own (no fused multiply-add), in
 * the order written below; the result is rounded once to float32 at the
 * store.  Every output element is written by exactly one thread from inputs
 * alone: bitwise reproducible, whatever the grid and whichever of the two
 * access paths a pointer's alignment selects.
 */
#ifndef VTC_COLOR_H_
#define VTC_COLOR_H_

#include "../vtc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTC_COLOR_ABI_VERSION 1

/* channel-last (count, h, w, 3): the layout of vtc_image.h and of the
 * training-set builder */
#define VTC_COLOR_HWC 0
/* planar (count, 3, h, w): the layout of the convolutional engine; with
 * count = 1 three planes back to back */
#define VTC_COLOR_CHW 1

#define VTC_UPSAMPLE_REPLICATE 0
#define VTC_UPSAMPLE_TRIANGLE 1

int vtc_color_abi_version(void);

/* ---- a 3 x 3 affine map per pixel ----------------------------------------
 * With t_j = (double)in_j - pre[j], j = 0, 1, 2:
 *   out_i = ((m[3i] * t_0 + m[3i + 1] * t_1) + m[3i + 2] * t_2) + post[i]
 * and then, when clamp != 0, v < lo ? lo : (v > hi ? hi : v): a NaN stays a
 * NaN.  lo and hi are ignored when clamp == 0; lo <= hi otherwise.
 * matrix[9] (row-major), pre[3] and post[3] are HOST pointers to doubles;
 * they are read before the call returns and travel as kernel arguments.
 * in_layout and out_layout are chosen independently.  out must not overlap
 * in (both are count * h * w * 3 floats); equal pointers are refused.
 * Forward JFIF is matrix = the YCbCr rows, pre = 0, post = (0, o, o);
 * inverse JFIF is matrix = the RGB rows, pre = (0, o, o), post = 0.
 * When both arrays can be reached 16 bytes at a time (a 16-byte aligned base
 * pointer, and h * w a multiple of 4 for a planar array) each lane takes 4
 * pixels as three 16-byte loads and three 16-byte stores; otherwise one pixel
 * per lane, element by element.  Both paths give the same bits. */
int vtc_color_transform(const float* in, int in_layout, float* out,
                        int out_layout, int64_t count, int32_t h, int32_t w,
                        const double* matrix, const double* pre,
                        const double* post, int clamp, double lo, double hi,
                        void* stream);

/* ---- box mean ------------------------------------------------------------
 * out (count, ceil(h / fv), ceil(w / fh)); fv, fh in {1, 2, 4}.  Output
 * (Y, X) is the sum, accumulated from 0.0 in row-major order, of in[y][x] for
 * y in [Y fv, min(h, (Y + 1) fv)) and inside each row x in [X fh,
 * min(w, (X + 1) fh)), divided by the number of pixels summed: a ragged edge
 * averages what is there.  out must not overlap in.
 * The grid of all three calls is capped at 2048 blocks of 256 threads and
 * strides from there; VTC_COLOR_MAX_BLOCKS=<n> in the environment lowers the
 * cap (a test's way to make a small array turn the loops over). */
int vtc_plane_downsample(const float* in, float* out, int64_t count,
                         int32_t h, int32_t w, int32_t fv, int32_t fh,
                         void* stream);

/* ---- back to full resolution ---------------------------------------------
 * in (count, h_in, w_in) -> out (count, h_out, w_out) with
 * ceil(h_out / fv) == h_in and ceil(w_out / fh) == w_in; fv, fh in {1, 2, 4}.
 * VTC_UPSAMPLE_REPLICATE: out[y][x] = in[y / fv][x / fh].
 * VTC_UPSAMPLE_TRIANGLE: centre-aligned linear interpolation clamped to the
 *   edge.  Per axis (f the factor, n the input size, y the output index):
 *     u = (y + 0.5) / f - 0.5 (exact in binary), i0 = floor(u), t = u - i0,
 *     a = clamp(i0, 0, n - 1), b = clamp(i0 + 1, 0, n - 1);
 *   out[y][x] = (1 - t_v) * ((1 - t_h) * p(a_v, a_h) + t_h * p(a_v, b_h))
 *             +      t_v  * ((1 - t_h) * p(b_v, a_h) + t_h * p(b_v, b_h)),
 *   operations in exactly that order.  For f = 2 the weights are libjpeg's
 *   3/4 and 1/4; for f = 1 the plane passes through unchanged (t = 0; the
 *   products with the zero weight still take place, so -0.0 comes out as 0.0
 *   and an infinity as NaN).
 * out must not overlap in. */
int vtc_plane_upsample(const float* in, float* out, int64_t count,
                       int32_t h_in, int32_t w_in, int32_t h_out,
                       int32_t w_out, int32_t fv, int32_t fh, int mode,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTC_COLOR_H_ */
