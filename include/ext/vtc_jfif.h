/*
 * vtc_jfif.h -- fifteenth header of libvtc_hip.so: the device half of a
 * baseline JFIF writer (ITU-T T.81 sequential DCT, Huffman, 8-bit), so that
 * the JPEG point of a rate-distortion curve is the size of a file any decoder
 * opens.  vtc_codec.h keeps the reference's pseudo-JPEG rules; the rules here
 * are the standard's and are this header's own.  DESIGN.md 4.23.
 *
 *   plane (h, w)  -> vtc_jfif_forward_dct   -> levels (rows, 64), zigzag order
 *   levels        -> vtc_jfif_symbol_counts -> counts; the host builds the
 *                                              length-limited tables
 *   levels        -> vtc_jfif_block_bits    -> bits per block
 *   bits          -> vtc_jpeg_bit_offsets (vtc_codec.h) -> offsets
 *   levels        -> vtc_jfif_pack          -> one bit-contiguous segment
 *   segment       -> vtc_jfif_stuff_bytes   -> 0x00 after every 0xFF
 *   levels        -> vtc_jfif_inverse_dct   -> the plane a decoder shows
 *
 * The markers and header segments of the file are written on the host
 * (utils/jfif.py).  Restart intervals, progressive and arithmetic modes and
 * 12-bit samples are not provided.
 *
 * This header lives under include/ext/ like vtc_color.h.  The functions live
 * in the same shared library as those of the other headers and follow the
 * conventions of vtc_codec.h: every pointer is a DEVICE pointer to a
 * contiguous row-major array and needs the alignment of its element and no
 * more (1 byte for uint8, 2 for uint16, 4 for int32 / float32, 8 for uint64 /
 * int64 / double); `workspace` must be 256-byte aligned; `stream` last;
 * functions only enqueue work on `stream`; no allocation inside, scratch comes
 * from the caller, sized by the matching *_workspace_bytes() query; null
 * pointers and bad sizes are answered before any device work
 * (VTC_ERR_INVALID_ARGUMENT, VTC_ERR_WORKSPACE) with text in vtc_last_error().
 * Every output is bitwise reproducible: counts and flags are integer atomics,
 * packed bits are OR-ed into disjoint positions, every other output element
 * is written by exactly one thread.  No inline assembly, no float atomics.
 *
 * Levels: int32 (d, 64) row-major, one 8 x 8 block per row in zigzag order
 * (T.81 figure A.6), v[0] the DC level.  Rows are in scan (MCU) order.
 *   pred int32[d]: the row that holds the previous block of the same
 *     component in scan order, or -1 for the first one; a value outside
 *     [0, d) is read as -1.
 *   table_sel uint8[d]: which of the two (DC, AC) table pairs codes the row;
 *     0 selects pair 0, anything else pair 1.
 *
 * Symbols (T.81 F.1.2): DIFF = v[0] - (pred >= 0 ? levels[pred][0] : 0), in
 * 64-bit arithmetic; the DC symbol is the bit length of |DIFF|, 0 .. 11.  For
 * every nonzero v[i], i >= 1, z is the number of zeros since the previous
 * nonzero AC index (index 0 counts as the start: the first has z = i - 1);
 * the block emits z / 16 symbols 0xF0, then (z % 16) << 4 | size with size
 * the bit length of |v[i]|, 1 .. 10.  The end-of-block symbol 0x00 is emitted
 * only when the last nonzero index is below 63 (an all-zero AC part emits it).
 * The value bits of a number of size n are its low n bits when it is
 * positive, the low n bits of (number - 1) when it is negative.  Stream order
 * of a block: DC codeword, DIFF bits, the AC tokens in ascending index each
 * followed by its value bits, end of block.
 * Symbol ids, for status[1]: AC byte b of pair t has id 272 t + b, DC
 * category c of pair t has id 272 t + 256 + c.
 *
 * status: int32[2], overwritten by the symbol, bits and pack calls.
 *   [0]  number of levels whose size exceeds 10 (AC) or DIFFs whose size
 *        exceeds 11 (DC).  Such a number is coded at the cap with its low 10
 *        (11) value bits, so every other output stays defined, but the file
 *        is not a baseline file.  vtc_jfif_pack adds the number of stream
 *        bits it dropped because they fell outside `raw`.
 *   [1]  0, or 1 + the smallest symbol id that was used and has length 0 in
 *        the tables handed in (such a symbol contributes no bits).
 */
#ifndef VTC_JFIF_H_
#define VTC_JFIF_H_

#include "../vtc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTC_JFIF_ABI_VERSION 1
/* bytes per tile of vtc_jfif_stuff_bytes */
#define VTC_JFIF_STUFF_TILE 2048

int vtc_jfif_abi_version(void);

/* ---- plane -> levels --------------------------------------------------------
 * plane float32 (h, w).  The plane is extended to bh x bw blocks of 8 x 8 by
 * replicating its last row and column: 8 bh >= h, 8 bw >= w, bh bw < 2^31.
 * All arithmetic is IEEE float64, every operation rounded on its own:
 *   s[y][x]  = rint(x < 0 ? 0 : (x > 255 ? 255 : x)) - 128
 *   t[y][u]  = sum over k = 0 .. 7, ascending, of s[y][k] * basis[8 u + k]
 *   c[v][u]  = sum over k = 0 .. 7, ascending, of t[k][u] * basis[8 v + k]
 * (each sum starts from its k = 0 product), basis double[64] with
 * basis[8 u + k] = c(u) / 2 * cos((2 k + 1) u pi / 16), c(0) = 1 / sqrt(2),
 * c(u > 0) = 1, computed once by the caller;
 *   level    = rint(c[v][u] / q[zz]), ties to even, zz the zigzag index of
 *              (v, u), q uint16[64] in zigzag order, saturated to int32,
 *              NaN -> INT32_MIN (a q entry of 0 saturates, it never faults).
 * levels int32 (rows, 64): block (by, bx) is written at row
 * row_of_block[by bw + bx] (int32[bh bw]); an entry outside [0, rows) writes
 * nothing.  Rows that no entry names are left as they are. */
int vtc_jfif_forward_dct(const float* plane, int32_t h, int32_t w, int32_t bh,
                         int32_t bw, const double* basis, const uint16_t* q,
                         const int32_t* row_of_block, int32_t* levels,
                         int64_t rows, void* stream);

/* ---- levels -> plane --------------------------------------------------------
 * The way back, columns first:
 *   c[v][u]  = (double)level * q[zz]      (an entry of row_of_block outside
 *                                          [0, rows) reads zeros)
 *   t[y][u]  = sum over k = 0 .. 7, ascending, of c[k][u] * basis[8 k + y]
 *   p[y][x]  = sum over k = 0 .. 7, ascending, of t[y][k] * basis[8 k + x]
 *   sample   = r < 0 ? 0 : (r > 255 ? 255 : r) with r = rint(p[y][x] + 128),
 *              stored as float32
 * cropped to (h, w): every element of plane is written exactly once. */
int vtc_jfif_inverse_dct(const int32_t* levels, int64_t rows,
                         const int32_t* row_of_block, int32_t bh, int32_t bw,
                         const double* basis, const uint16_t* q, float* plane,
                         int32_t h, int32_t w, void* stream);

/* ---- symbol statistics ------------------------------------------------------
 * ac_counts uint64[2][256] indexed by [pair][run << 4 | size], dc_counts
 * uint64[2][16] indexed by [pair][category]; both overwritten.  status[1] is
 * set to 0.  d >= 1. */
int vtc_jfif_symbol_counts(const int32_t* levels, int64_t d,
                           const int32_t* pred, const uint8_t* table_sel,
                           uint64_t* ac_counts, uint64_t* dc_counts,
                           int32_t* status, void* stream);

/* ---- block lengths ----------------------------------------------------------
 * ac_len uint8[2][256], dc_len uint8[2][16]: codeword lengths in bits, at
 * most 16 (a longer one is read as 16), 0 = symbol absent from the table.
 * bits int32[d]: codewords plus value bits of each block.  The offsets come
 * from vtc_jpeg_bit_offsets. */
int vtc_jfif_block_bits(const int32_t* levels, int64_t d, const int32_t* pred,
                        const uint8_t* table_sel, const uint8_t* ac_len,
                        const uint8_t* dc_len, int32_t* bits, int32_t* status,
                        void* stream);

/* ---- the entropy-coded segment ----------------------------------------------
 * ac_code uint16[2][256], dc_code uint16[2][16]: each codeword in the low
 * `len` bits, first stream bit the most significant of them.  offsets
 * int64[d + 1].  The call zero-fills all raw_bytes of raw, writes block p
 * from bit offsets[p] on -- stream bit j is bit 7 - j % 8 of byte j / 8 -- and
 * sets the bits from offsets[d] up to the next byte boundary to 1 (T.81
 * F.1.2.3).  Bits that would fall outside [0, 8 raw_bytes) are dropped, never
 * written, and counted in status[0]. */
int vtc_jfif_pack(const int32_t* levels, int64_t d, const int32_t* pred,
                  const uint8_t* table_sel, const uint16_t* ac_code,
                  const uint8_t* ac_len, const uint16_t* dc_code,
                  const uint8_t* dc_len, const int64_t* offsets, uint8_t* raw,
                  size_t raw_bytes, int32_t* status, void* stream);

/* ---- byte stuffing ----------------------------------------------------------
 * out uint8[capacity] receives raw uint8[n] with a 0x00 inserted after every
 * 0xFF: byte i goes to i + (number of 0xFF among raw[0 .. i)).  out_len
 * int64[1] (device) receives n + (number of 0xFF), whether or not that fits;
 * bytes that would land at or beyond capacity are dropped, never written, and
 * counted in status[0] (int32[1], saturated at INT32_MAX).  Bytes of out at
 * or beyond out_len are left as they are.  n >= 0, capacity >= 0; raw may be
 * null when n = 0 and out when capacity = 0; out must not overlap raw.
 * Tiles of VTC_JFIF_STUFF_TILE bytes count their 0xFF bytes, one block scans
 * the tile sums, each tile rescans and stores: no atomics, no zero-fill.
 * workspace: one int64 per tile. */
size_t vtc_jfif_stuff_bytes_workspace_bytes(int64_t n);
int vtc_jfif_stuff_bytes(const uint8_t* raw, int64_t n, uint8_t* out,
                         int64_t capacity, int64_t* out_len, int32_t* status,
                         void* workspace, size_t workspace_bytes,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTC_JFIF_H_ */
