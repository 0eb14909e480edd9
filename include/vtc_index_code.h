/*
 * vtc_index_code.h -- ninth header of libvtc_hip.so: prefix codes for the
 * indices of the quantisers of vtc_quant.h and vtc_vq.h.  The experiment
 * (experiments/rate_distortion_sparse_coding.py:763-827 of
 * spencerkent/vision-transform-codes) trains one Huffman table per index
 * stream on the training codes and charges the test codes what those tables
 * cost; this header measures that cost and writes the bits.  DESIGN.md 4.17.
 *
 *   indices (b, m), len         -> vtc_index_code_bits -> bits per row, per column
 *   bits per row                -> vtc_jpeg_bit_offsets (vtc_codec.h) -> offsets
 *   indices, code, len, offsets -> vtc_index_code_pack -> packed streams
 *
 * Data.
 *   indices  int32  (b, m)     m index streams ("columns") per row: a column
 *                              is one scalar quantiser, or the vector quantiser
 *   code     uint64 (m, kmax)  column j has its own prefix code over the symbols
 *                              0 .. kmax - 1: the codeword of symbol i in the
 *                              low len[j, i] bits of code[j, i]; higher bits
 *                              are not read
 *   len      uint8  (m, kmax)  0 .. 64 bits, or VTC_INDEX_CODE_ABSENT: the table
 *                              lacks the symbol (65 .. 254 are read as absent)
 * A length of 0 is legal: the table of one symbol, whose codeword is the empty
 * string.  1 <= m <= VTC_INDEX_CODE_MAX_COLUMNS and 1 <= kmax <=
 * VTC_INDEX_CODE_MAX_SYMBOLS, larger ones answer VTC_ERR_UNSUPPORTED; b >= 1,
 * and b * m is not limited to 2^31.
 *
 * An entry indices[r, j] is uncodable when it is negative (the -1 of a NaN
 * code), is >= kmax, or has an absent length.  It contributes no bits and is
 * counted.  Both calls report in
 *   status   int64  [3]        zeroed by the call:
 *                              [0] the number of uncodable entries,
 *                              [1] 1 + the smallest flat position r * m + j of
 *                                  one, 0 when there is none,
 *                              [2] stream bits dropped by vtc_index_code_pack
 *                                  (0 from vtc_index_code_bits).
 *
 * The functions live in the same shared library as those of the other eight
 * headers and follow the conventions stated at the top of vtc_quality.h:
 * device pointers with the alignment of their element and no more (`packed`
 * any byte address), `stream` last, no allocation inside and no workspace,
 * null pointers and bad sizes answered before any device work, every output
 * element written by the call itself.  All outputs are sums, minima and ORs of
 * integers: bitwise reproducible from run to run.
 */
#ifndef VTC_INDEX_CODE_H_
#define VTC_INDEX_CODE_H_

#include "vtc_quality.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTC_INDEX_CODE_ABI_VERSION 1

#define VTC_INDEX_CODE_ABSENT 255
#define VTC_INDEX_CODE_MAX_COLUMNS 4096
#define VTC_INDEX_CODE_MAX_SYMBOLS 4096

int vtc_index_code_abi_version(void);

/* row_bits     int32 [b]  the sum over j of len[j, indices[r, j]]: the length
 *                         of row r's stream (at most 4096 * 64 bits)
 * column_bits  int64 [m]  the same lengths summed down each column: the rate
 *                         broken down by coefficient */
int vtc_index_code_bits(const int32_t* indices, int64_t b, int32_t m,
                        const uint8_t* len, int32_t kmax, int32_t* row_bits,
                        int64_t* column_bits, int64_t* status, void* stream);

/* offsets: int64 [b + 1], e.g. vtc_jpeg_bit_offsets of row_bits.  Row r's
 * stream is the codewords of its columns 0 .. m - 1 in that order, each most
 * significant bit first, written from stream bit offsets[r] on; a row may use
 * the bits below offsets[r + 1].  Stream bit i is bit 7 - i % 8 of byte i / 8
 * of `packed`, the layout of vtc_jpeg_pack.
 * packed: uint8 [packed_bytes], zeroed by the call; packed_bytes >= 0.
 * Bits that would fall outside [0, 8 * packed_bytes) or at or beyond
 * offsets[r + 1] are dropped and counted in status[2]; a row whose offset is
 * negative or above offsets[r + 1] is dropped whole. */
int vtc_index_code_pack(const int32_t* indices, int64_t b, int32_t m,
                        const uint64_t* code, const uint8_t* len, int32_t kmax,
                        const int64_t* offsets, uint8_t* packed,
                        int64_t packed_bytes, int64_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTC_INDEX_CODE_H_ */
