/*
 * vtc_index_decode.h -- tenth header of libvtc_hip.so: the decoder of the
 * packed index streams that vtc_index_code_pack (vtc_index_code.h) writes.
 * The reference's experiment only ever measures the length of those streams
 * and has no decoder; this one is the inverse of the packer's layout, stated
 * in DESIGN.md 4.17 and 4.18.
 *
 *   packed bits, offsets, the m tables -> vtc_index_code_unpack -> indices
 *
 * The functions live in the same shared library as those of the other nine
 * headers and follow the conventions of vtc_decode.h: device pointers with
 * the alignment of their element and no more (`packed` any byte address),
 * `workspace` 256-byte aligned and sized by the query, `stream` last, no
 * allocation inside, every device operation on `stream`, null pointers and bad
 * sizes answered before any device work.  Every output is an integer that is
 * stored once or reduced by integer atomics: bitwise reproducible.
 *
 * code uint64 (m, kmax), len uint8 (m, kmax), m, kmax, offsets int64 [b + 1]
 * and the bit layout are exactly those of vtc_index_code_pack: a length of
 * 0 .. 64 is a codeword (0 the empty codeword of a one-symbol column),
 * 65 .. 255 means absent; stream bit i is bit 7 - i % 8 of byte i / 8 of
 * `packed`.  1 <= m <= VTC_INDEX_CODE_MAX_COLUMNS, 1 <= kmax <=
 * VTC_INDEX_CODE_MAX_SYMBOLS, larger ones answer VTC_ERR_UNSUPPORTED; b >= 1
 * and b * m is not limited to 2^31.  packed_bytes >= 0; `packed` must not be
 * null but is never read when packed_bytes is 0.
 *
 * Row r starts at stream bit offsets[r] and reads exactly m codewords, column
 * 0 first, each under its own column's table.  It may use the bits below
 * min(offsets[r + 1], 8 * packed_bytes).  A one-symbol column yields its
 * symbol and consumes nothing.  Bits left over before offsets[r + 1] are NOT
 * an error (the packer's contract allows gaps between rows): the caller
 * compares row_bits[r] with offsets[r + 1] - offsets[r] where it wants none.
 *
 * A row is malformed when offsets[r] < 0 or offsets[r] > offsets[r + 1], when
 * no codeword of a column matches (a column with no codeword at all included),
 * or when a codeword would pass the row's end or the buffer.  Such a row keeps
 * the indices decoded before the fault, the rest of it is -1 (the value the
 * packer treats as uncodable), and its row_bits is the bits consumed up to
 * there.  Nothing is read or stored out of bounds.
 *
 * status: int64[3], overwritten.
 *   [0]  number of malformed rows.
 *   [1]  0, or 1 + the smallest malformed row index.
 *   [2]  0, or 1 + the smallest flat table position j * kmax + i whose
 *        codeword equals another codeword of column j or is a prefix of one.
 *        Then no row is decoded: indices is all -1, row_bits all 0 and [0],
 *        [1] are 0.
 */
#ifndef VTC_INDEX_DECODE_H_
#define VTC_INDEX_DECODE_H_

#include "vtc_index_code.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTC_INDEX_DECODE_ABI_VERSION 1

/* bits of the first-level lookup of a column: K */
#define VTC_INDEX_DECODE_LOOKUP_BITS 10

int vtc_index_decode_abi_version(void);

/* workspace: the decoding tables of one call, each array rounded up to 256
 * bytes, in this order:
 *   uint64 [m * kmax]  column j's codewords left-aligned to 64 bits and sorted
 *                      by (word, length, symbol), from j * kmax on
 *   uint32 [m * kmax]  their meta words: bit 31 valid, bits 12 .. 18 the
 *                      length 0 .. 64, bits 0 .. 11 the symbol
 *   uint32 [m * 2^K]   the first-level lookup, K = 10: the meta word of the
 *                      codeword of at most K bits that a K-bit prefix starts
 *                      with, 0 (valid bit clear) when there is none
 *   int32  [m]         the number of codewords of each column
 *   int32  [1]         the smallest bad table position, INT32_MAX when none
 * Host-only; 0 for sizes that vtc_index_code_unpack refuses. */
size_t vtc_index_code_unpack_workspace_bytes(int32_t m, int32_t kmax);

/* indices int32 (b, m) and row_bits int32 [b]: every element written by the
 * call; status as above. */
int vtc_index_code_unpack(const uint8_t* packed, int64_t packed_bytes,
                          const int64_t* offsets, int64_t b, int32_t m,
                          const uint64_t* code, const uint8_t* len, int32_t kmax,
                          int32_t* indices, int32_t* row_bits, int64_t* status,
                          void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTC_INDEX_DECODE_H_ */
