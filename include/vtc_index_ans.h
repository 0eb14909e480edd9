/*
 * vtc_index_ans.h -- eleventh header of libvtc_hip.so: a table-driven range
 * coder (rANS) for the (b, m) int32 index arrays of vtc_quant.h / vtc_vq.h,
 * and its decoder.  A prefix code (vtc_index_code.h) cannot spend less than
 * one bit per symbol, which for sparse codes is the dominant cost; this coder
 * reaches the cost sum log2(2^15 / f) of its frequencies to within the flush
 * of a stream.  DESIGN.md 4.19.
 *
 *   indices (b, m), freq        -> vtc_index_ans_sizes  -> bytes per stream
 *   bytes per stream            -> vtc_jpeg_bit_offsets (vtc_codec.h; a plain
 *                                  exclusive prefix sum of int32 into int64)
 *                                                       -> byte offsets
 *   indices, freq, sizes, offsets -> vtc_index_ans_pack -> packed streams
 *   packed, offsets, freq       -> vtc_index_ans_unpack -> indices
 *
 * The functions live in the same shared library as those of the other ten
 * headers and follow the conventions of vtc_index_code.h / vtc_index_decode.h:
 * device pointers with the alignment of their element and no more (`packed`
 * any byte address), `workspace` 256-byte aligned and sized by the host-only
 * query, `stream` last, no allocation inside, every device operation on
 * `stream`, null pointers and bad sizes answered before any device work, every
 * output element written by the call.  Integers only: bitwise reproducible.
 *
 * THE CODE
 *
 * Model.
 *  - `freq` is uint16 (m, kmax).
 *  - Column j's frequencies sum to exactly 2^15 (VTC_INDEX_ANS_PROB_BITS = 15).
 *  - Limits are 1 <= m, kmax <= 4096, as in the Huffman coder.
 *  - A frequency of 0 means the symbol is absent.
 *  - A one-symbol column has frequency 2^15.  It costs no bits and never
 *    changes a state.
 *  - Each call derives the exclusive cumulative sums `cum` (uint16 (m, kmax))
 *    into its workspace: one block per column, integer scan.
 *  - A column whose sum is not 2^15 sets status[2] = 1 + j (smallest such j).
 *    Then nothing is coded or decoded: sizes are 0 and indices are -1 (and
 *    status[0], status[1] are 0, `packed` all zero, used_bytes 0).  This is the
 *    bad-table rule of DESIGN.md 4.18.
 *
 * Streams.
 *  - The caller picks rows_per_stream R, with R >= 1 and R * m <= 2^24.
 *  - Stream s covers rows s R ... min(b, (s + 1) R) - 1.  There are
 *    n = ceil(b / R) streams, and the last may be shorter.
 *  - Symbols are in row-major order: flat position t = (r - s R) * m + j.
 *  - b * m is not limited to 2^31.
 *
 * Interleave.
 *  - A stream carries 64 independent rANS states.  Position t belongs to state
 *    t % 64, so one wave codes one stream, whatever m is.
 *  - In step q, lane l handles position 64 q + l under column (64 q + l) % m.
 *  - Lanes past the end of the stream idle.
 *  - This one rule covers m = 1, m = 42, m = 65 and m = 4096.
 *
 * Arithmetic.
 *  - State is 32-bit.  The lower bound is L = 2^16.  Words are 16-bit.  The
 *    start state is L.
 *  - Encode a symbol (f, c) as follows.
 *    - If (uint64)x >= (uint64)f << 17, emit x & 0xFFFF and set x >>= 16.  At
 *      most once suffices.  The compare must be 64-bit because f = 2^15 gives
 *      2^32.
 *    - Then x = ((x / f) << 15) + x % f + c.
 *  - Decode as follows.
 *    - slot = x & 32767.
 *    - The symbol is the largest i with cum[j, i] <= slot.  This rule skips
 *      absent symbols correctly, including trailing ones.
 *    - x = f * (x >> 15) + slot - c.
 *    - If x < L, set x = (x << 16) | next word.  One word always suffices.
 *
 * Layout, as the decoder reads it forward from the stream's first byte.
 *  - First come 64 little-endian uint32 end states, lanes 0 ... 63, always 256
 *    bytes.
 *  - Then come the 16-bit little-endian words.
 *  - Within a step, the lanes that need a word take consecutive words in
 *    ascending lane order (ballot + popcount of the lower lanes).  The cursor
 *    advances by the popcount.
 *  - The encoder is the exact inverse.  It walks steps from last to first and
 *    fills the words back to front.
 *  - A stream's length is 256 + 2 * words bytes.
 *
 * Uncodable entries.  An entry is uncodable when it is negative, >= kmax or
 * of frequency 0.  As in vtc_index_code.h, it contributes nothing and leaves
 * its lane's state alone.  It is counted in status[0], and status[1] holds 1 +
 * the first flat position r * m + j.
 *
 * FREQUENCIES FROM COUNTS (utils.index_coding.index_ans_frequencies; host,
 * pure integers, deterministic).  For column j with k_j codewords in use:
 *  1. The weight w_i is count_i, or 1 when count_i = 0, for every i < k_j (so
 *     every index the codebook can produce is codable); w_i = 0 for i >= k_j.
 *  2. f_i = max(1, floor(w_i * 2^15 / W)) for i < k_j, where W = sum w_i.
 *  3. The difference d = 2^15 - sum f is given out, or taken back, one unit at
 *     a time, going round the symbols in order of (-w_i, i) and skipping
 *     symbols at f = 1 when taking.  It terminates because k <= 4096 < 2^15.
 *
 * status: int64 [3], overwritten by every call.
 *   sizes, pack   [0] uncodable entries, [1] 0 or 1 + the first one's flat
 *                 position, [2] 0, or 1 + the smallest bad column; from pack
 *                 otherwise the number of streams skipped or not written as
 *                 the coder sizes them (below).
 *   unpack        [0] malformed streams, [1] 0 or 1 + the first one,
 *                 [2] 0 or 1 + the smallest bad column.
 */
#ifndef VTC_INDEX_ANS_H_
#define VTC_INDEX_ANS_H_

#include "vtc_index_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTC_INDEX_ANS_ABI_VERSION 1

#define VTC_INDEX_ANS_PROB_BITS 15
#define VTC_INDEX_ANS_LANES 64
/* log2 of the most symbols of one stream: rows_per_stream * m <= 2^24 */
#define VTC_INDEX_ANS_MAX_STREAM_BITS 24
/* log2 of the buckets of the decoder's per-column search index: B */
#define VTC_INDEX_ANS_BUCKET_BITS 8

int vtc_index_ans_abi_version(void);

/* workspace of all three calls, each array rounded up to 256 bytes:
 *   uint16 [m * kmax]  cum: the exclusive cumulative sums of each column
 *   uint16 [m * 2^B]   B = 8: for bucket g of column j, the largest i with
 *                      cum[j, i] <= g * 2^(15 - B) -- where the decoder's
 *                      search for a slot of that bucket starts
 *   int32  [1]         the smallest bad column, INT32_MAX when none
 * Host-only; 0 for sizes the calls refuse (m or kmax outside 1 .. 4096). */
size_t vtc_index_ans_workspace_bytes(int32_t m, int32_t kmax);

/* The coder run without stores.  stream_bytes int32 [n], n = ceil(b / R):
 * 256 + 2 * words of every stream. */
int vtc_index_ans_sizes(const int32_t* indices, int64_t b, int32_t m,
                        const uint16_t* freq, int32_t kmax,
                        int32_t rows_per_stream, int32_t* stream_bytes,
                        int64_t* status, void* workspace,
                        size_t workspace_bytes, void* stream);

/* stream_bytes int32 [n] as vtc_index_ans_sizes wrote it; offsets int64
 * [n + 1] in bytes, e.g. vtc_jpeg_bit_offsets of stream_bytes.  packed uint8
 * [packed_bytes] is zeroed by the call; packed_bytes >= 0.
 * Stream s occupies [offsets[s], offsets[s] + stream_bytes[s]).  If that range
 * is not inside [0, packed_bytes) or not at or below offsets[s + 1] (or
 * stream_bytes[s] is below 256 or odd), the stream is skipped whole before any
 * store and counted in status[2].  Every store is bounded to the slot, also
 * when stream_bytes[s] is not the coder's own size: such a stream is counted
 * in status[2] and its contents are unspecified.  The words are stored
 * bytewise. */
int vtc_index_ans_pack(const int32_t* indices, int64_t b, int32_t m,
                       const uint16_t* freq, int32_t kmax,
                       int32_t rows_per_stream, const int32_t* stream_bytes,
                       const int64_t* offsets, uint8_t* packed,
                       int64_t packed_bytes, int64_t* status, void* workspace,
                       size_t workspace_bytes, void* stream);

/* indices int32 (b, m) and used_bytes int32 [n]: every element written.
 * Stream s starts at byte offsets[s] and is read only below
 * min(offsets[s + 1], packed_bytes).  A stream is malformed when
 *  - its offsets are negative or decreasing, or its slot is shorter than 256
 *    bytes: all its indices are -1 and its used_bytes is 0;
 *  - it runs out of words: positions from that step on are -1, used_bytes is
 *    256 + 2 * the words read before that step;
 *  - any of its 64 states is not L after the last step (rANS's free integrity
 *    check): the indices stay as decoded, each in [0, kmax).
 * Bytes left over in a slot are not an error: used_bytes reports what was
 * read.  Whatever the bytes, nothing is read or stored out of bounds and
 * every loop is bounded by the symbol count.  `packed` must not be null but is
 * never read when packed_bytes is 0. */
int vtc_index_ans_unpack(const uint8_t* packed, int64_t packed_bytes,
                         const int64_t* offsets, int64_t b, int32_t m,
                         const uint16_t* freq, int32_t kmax,
                         int32_t rows_per_stream, int32_t* indices,
                         int32_t* used_bytes, int64_t* status, void* workspace,
                         size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTC_INDEX_ANS_H_ */
