/*
 * vtc_decode.h -- fourth header of libvtc_hip.so: the decoder of the packed
 * JPEG streams that vtc_jpeg_pack (vtc_codec.h) writes.  The reference,
 * utils/jpeg.py of spencerkent/vision-transform-codes, only ever measures
 * len(stream) and has no decoder; this one is the inverse of the coding rules
 * of generate_jpg_binary_stream (utils/jpeg.py:133-238), stated in DESIGN.md
 * 4.11 and 4.12.
 *
 *   packed bits, offsets, the two Huffman tables  -> vtc_jpeg_unpack -> levels
 *
 * The functions live in the same shared library as those of vtc_hip.h,
 * vtc_image.h and vtc_codec.h and follow their conventions:
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
 *   - every output is bitwise reproducible from run to run: a row is decoded
 *     by one lane, counts and flags are integer atomics.
 *
 * Levels, symbols and symbol ids are those of vtc_codec.h: int32 (d, s)
 * row-major, v[0] the DC level; AC byte b has id b, DC category c id 256 + c.
 * 1 <= s <= VTC_JPEG_MAX_S, d >= 1.
 *
 * Row p occupies stream bits offsets[p] up to, not including, offsets[p + 1];
 * stream bit j is bit 7 - j % 8 of byte j / 8.  Starting from v = 0 and
 * pos = 1, AC codewords are read until 0x00: 0xF0 adds 16 to pos; a byte b
 * with size = b & 15 > 0 adds b >> 4 to pos, reads `size` value bits into
 * v[pos] and adds 1 to pos.  Then one DC codeword of category c and c value
 * bits into v[0].  Value bits with a leading 1 are the magnitude, with a
 * leading 0 its complement: the value is bits - (2^size - 1).  The row must
 * end exactly at offsets[p + 1].
 *
 * A row is malformed when a value would land at pos >= s, an AC byte of size
 * 0 other than 0x00 and 0xF0 occurs, no codeword matches, a read would pass
 * offsets[p + 1] or leave [0, 8 * packed_bytes), bits are left over, or
 * offsets[p] > offsets[p + 1].  Such a row keeps the levels decoded before
 * the fault, the rest of it stays zero, and nothing is read or written out
 * of bounds.
 *
 * status: int64[3], overwritten.
 *   [0]  number of malformed rows.
 *   [1]  0, or 1 + the smallest malformed row index.
 *   [2]  0, or 1 + the smallest symbol id whose codeword equals another's or
 *        is a prefix of another's (AC and DC table each on its own).  Then no
 *        row is decoded: levels is all zero and [0], [1] are 0.
 */
#ifndef VTC_DECODE_H_
#define VTC_DECODE_H_

#include "vtc_codec.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTC_DECODE_ABI_VERSION 1

int vtc_decode_abi_version(void);

/* workspace: the decoding tables of one call -- the at most 272 codewords
 * left-aligned to 64 bits and sorted, uint64[272]; their length and symbol
 * id, uint16[272]; a first-level lookup of 2^10 uint16 entries per table;
 * int32[4] of counts and the prefix flag.  Each array is rounded up to 256
 * bytes. */
size_t vtc_jpeg_unpack_workspace_bytes(void);

/* ac_code uint64[256], ac_len uint8[256], dc_code uint64[16], dc_len
 * uint8[16]: the arrays vtc_jpeg_pack takes (each codeword in the low `len`
 * bits, first stream bit the most significant of them, len <= 64 and a larger
 * one read as 64, 0 = symbol absent).  packed uint8[packed_bytes]; offsets
 * int64[d + 1]; levels int32 (d, s) is zero-filled, then every row's nonzero
 * levels are stored; status as above. */
int vtc_jpeg_unpack(const uint8_t* packed, size_t packed_bytes,
                    const int64_t* offsets, int64_t d, int32_t s,
                    const uint64_t* ac_code, const uint8_t* ac_len,
                    const uint64_t* dc_code, const uint8_t* dc_len,
                    int32_t* levels, int64_t* status, void* workspace,
                    size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTC_DECODE_H_ */
