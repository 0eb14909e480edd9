/*
 * vtc_codec.h -- third header of libvtc_hip.so: the JPEG source coding of
 * utils/jpeg.py of spencerkent/vision-transform-codes (quantise, run-length
 * symbols, Huffman lengths, packed streams), i.e. what a rate-distortion point
 * needs once the codes exist: how many bits they cost.
 *
 *   utils/jpeg.py:133-238  generate_jpg_binary_stream (symbols)
 *                                               -> vtc_jpeg_symbol_counts
 *   utils/jpeg.py:133-238  generate_jpg_binary_stream (len of the stream)
 *                                               -> vtc_jpeg_stream_bits
 *   utils/jpeg.py:133-238  generate_jpg_binary_stream (the stream)
 *                                               -> vtc_jpeg_bit_offsets,
 *                                                  vtc_jpeg_pack
 *   examples/train_jpeg.py np.rint(codes / binwidths) and its inverse
 *                                               -> vtc_jpeg_quantize,
 *                                                  vtc_jpeg_dequantize
 *
 * The Huffman tables themselves (at most 272 symbols) are built on the host
 * from the device counts (utils/jpeg.py of this project).
 *
 * The functions live in the same shared library as those of vtc_hip.h and
 * vtc_image.h and follow their conventions:
 *   - every pointer is a DEVICE pointer to a contiguous row-major array;
 *     `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *   - alignment: a pointer needs the alignment of its element and no more
 *     (4 bytes for int32 / float32, 8 for uint64 / int64 / double, 1 for
 *     uint8).  `workspace` must be 256-byte aligned.
 *   - functions only enqueue work on `stream` and return; every device
 *     operation of a call is issued on `stream`.
 *   - no allocation inside: scratch comes from the caller as `workspace`,
 *     sized by the matching *_workspace_bytes() query.  No per-process state.
 *   - return value: VTC_OK or a VTC_ERR_* code of vtc_hip.h; vtc_last_error()
 *     gives text.  Null pointers and bad sizes are answered before any device
 *     work.
 *   - every output is bitwise reproducible from run to run: counts and flags
 *     are integer atomics, packed bits are OR-ed into disjoint positions.
 *
 * Levels: int32 (d, s) row-major.  One patch is one row of s quantiser levels
 * relative to the zero codeword, in scan order (v[0] is the DC level).
 * 1 <= s <= 4096 (VTC_JPEG_MAX_S), d >= 1.
 *
 * Symbols: an AC symbol is the byte run << 4 | size (0x00 = end of block,
 * 0xF0 = sixteen zeros), a DC symbol is the category 0..15.  Symbol ids, for
 * status[1]: AC byte b has id b, DC category c has id 256 + c.
 *
 * status: int32[2], overwritten by the symbol, bits and pack calls.
 *   [0]  number of levels with |v| > 32767 (size category above 15;
 *        INT32_MIN counts).  Such a level is coded as size 15 with its low 15
 *        value bits, so every other output stays defined, but the stream is
 *        not the reference's.  vtc_jpeg_pack adds the number of stream bits it
 *        dropped because they fell outside `out`.
 *   [1]  0, or 1 + the smallest symbol id that was used and has length 0 in
 *        the tables handed in (such a symbol contributes no bits).
 */
#ifndef VTC_CODEC_H_
#define VTC_CODEC_H_

#include "vtc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTC_CODEC_ABI_VERSION 1
#define VTC_JPEG_MAX_S 4096

int vtc_codec_abi_version(void);

/* ---- quantise / dequantise ------------------------------------------------
 * codes (d, s) float32; binwidths double[s] in scan order; order int32[s]
 * (scan position k reads code column order[k]) or NULL for the identity.
 *   levels[p, k] = nearbyint((double)codes[p, order[k]] / binwidths[k]),
 * ties to even -- np.rint(codes.astype(float64)[:, order] / binwidths)
 * exactly --, saturated to the int32 range, NaN -> INT32_MIN.  An order entry
 * outside [0, s) reads nothing and gives INT32_MIN. */
int vtc_jpeg_quantize(const float* codes, const double* binwidths,
                      const int32_t* order, int32_t* levels, int64_t d,
                      int32_t s, void* stream);
/* codes[p, order[k]] = (float)((double)levels[p, k] * binwidths[k]), one
 * rounding.  order must be a permutation of 0..s-1 for every code to be
 * written; an entry outside [0, s) writes nothing. */
int vtc_jpeg_dequantize(const int32_t* levels, const double* binwidths,
                        const int32_t* order, float* codes, int64_t d,
                        int32_t s, void* stream);

/* ---- symbol statistics ----------------------------------------------------
 * ac_counts uint64[256] indexed by run << 4 | size, dc_counts uint64[16]
 * indexed by category: how often each symbol occurs in the d streams.  Both
 * are overwritten.  status[1] is set to 0. */
int vtc_jpeg_symbol_counts(const int32_t* levels, int64_t d, int32_t s,
                           uint64_t* ac_counts, uint64_t* dc_counts,
                           int32_t* status, void* stream);

/* ---- stream lengths -------------------------------------------------------
 * ac_len uint8[256], dc_len uint8[16]: codeword lengths in bits, 0 = symbol
 * absent from the table.  bits int32[d]: length of each patch's stream
 * (Huffman codewords plus value bits, AC part, end of block, then DC). */
int vtc_jpeg_stream_bits(const int32_t* levels, int64_t d, int32_t s,
                         const uint8_t* ac_len, const uint8_t* dc_len,
                         int32_t* bits, int32_t* status, void* stream);

/* offsets int64[d + 1]: exclusive prefix sum of bits, offsets[d] the total.
 * workspace: one int64 per tile of 2048 rows. */
size_t vtc_jpeg_bit_offsets_workspace_bytes(int64_t d);
int vtc_jpeg_bit_offsets(const int32_t* bits, int64_t d, int64_t* offsets,
                         void* workspace, size_t workspace_bytes,
                         void* stream);

/* ---- packed streams -------------------------------------------------------
 * ac_code uint64[256], dc_code uint64[16]: each codeword in the low `len`
 * bits, first stream bit the most significant of them, len <= 64 (of a longer
 * one only 64 bits are written).  The call zero-fills all out_bytes of out,
 * then writes patch p's stream from bit offsets[p] on: stream bit j is bit
 * 7 - j % 8 of byte j / 8 (np.unpackbits order).  Bits that would fall
 * outside [0, 8 * out_bytes) -- out too short for offsets[d], or an offset
 * that is negative -- are dropped, never written, and counted in status[0]. */
int vtc_jpeg_pack(const int32_t* levels, int64_t d, int32_t s,
                  const uint64_t* ac_code, const uint8_t* ac_len,
                  const uint64_t* dc_code, const uint8_t* dc_len,
                  const int64_t* offsets, uint8_t* out, size_t out_bytes,
                  int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTC_CODEC_H_ */
