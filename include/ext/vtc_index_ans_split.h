/*
 * vtc_index_ans_split.h -- thirteenth header of libvtc_hip.so: the range coder
 * of vtc_index_ans.h for ONE index column of up to 131 072 symbols, the index
 * stream of the large vector quantiser (vtc_vq_large.h), and its decoder.  A
 * 15-bit frequency table cannot hold more than 32 768 symbols at frequency
 * >= 1, so an index is split into two symbols, each under a 15-bit table of
 * its own.  DESIGN.md 4.21.
 *
 *   indices [b], freq_hi, freq_lo -> vtc_index_ans_split_sizes -> bytes per
 *                                                                 stream
 *   bytes per stream   -> vtc_jpeg_bit_offsets (vtc_codec.h; a plain exclusive
 *                         prefix sum of int32 into int64)  -> byte offsets
 *   indices, tables, sizes, offsets -> vtc_index_ans_split_pack -> packed
 *   packed, offsets, tables         -> vtc_index_ans_split_unpack -> indices
 *
 * This header is an extension of vtc_index_ans.h and lives under
 * include/ext/; include/ itself keeps the twelve headers it has.  The
 * functions live in the same shared library as those of the other twelve
 * headers and follow the conventions of vtc_index_ans.h: device pointers with
 * the alignment of their element and no more (`packed` any byte address),
 * `workspace` 256-byte aligned and sized by the host-only query, `stream`
 * last, no allocation inside, every device operation on `stream`, null
 * pointers, bad sizes and a short workspace answered before any device work,
 * every output element written by the call.  Integers only: bitwise
 * reproducible.  No inline assembly.
 *
 * THE CODE
 *
 * Split.
 *  - Index i is coded as two symbols under the same lane state:
 *    hi = i >> 8 (VTC_INDEX_ANS_SPLIT_LO_BITS = 8) and lo = i & 255.
 *  - By the chain rule P(i) = P(hi) * P(lo | hi), so any distribution over the
 *    indices is representable; each factor is quantised to 15 bits.
 *
 * Model.
 *  - `indices` is int32 [b], one column.  1 <= kmax <= 131 072
 *    (VTC_INDEX_ANS_SPLIT_MAX_SYMBOLS).  H = ceil(kmax / 256) <= 512.
 *  - `freq_hi` is uint16 [H]; `freq_lo` is uint16 (H, 256), row h the
 *    frequencies of lo given hi = h.
 *  - `freq_hi` sums to exactly 2^15 (VTC_INDEX_ANS_PROB_BITS of
 *    vtc_index_ans.h).
 *  - Every row h with freq_hi[h] > 0 sums to exactly 2^15 and is 0 at every l
 *    with 256 h + l >= kmax.  Rows with freq_hi[h] = 0 are not read.
 *  - A frequency of 0 means the symbol is absent.  A one-symbol table has
 *    frequency 2^15; it costs no bits and never changes a state.
 *  - Each call derives the exclusive cumulative sums of both tables into its
 *    workspace: one block per table row, integer scan.
 *
 * Bad tables.
 *  - status[2] = 1 when freq_hi does not sum to 2^15.
 *  - Otherwise status[2] = 2 + h for the smallest row h with freq_hi[h] > 0
 *    whose sum is not 2^15 or which is not 0 at some l with 256 h + l >= kmax.
 *  - Then nothing is coded or decoded: sizes are 0, `packed` all zero, indices
 *    -1, used_bytes 0, status[0] = status[1] = 0.
 *
 * Streams.
 *  - The caller picks rows_per_stream R with 1 <= R <= 2^24
 *    (VTC_INDEX_ANS_MAX_STREAM_BITS).
 *  - Stream s covers rows s R ... min(b, (s + 1) R) - 1.  There are
 *    n = ceil(b / R) streams, and the last may be shorter.
 *  - b is not limited to 2^31.
 *
 * Interleave.
 *  - A stream carries 64 independent rANS states (VTC_INDEX_ANS_LANES).
 *    Position t within a stream belongs to state t % 64, so one wave codes one
 *    stream.
 *  - Step q handles positions 64 q ... 64 q + 63.  Lanes past the end of the
 *    stream idle.
 *
 * Arithmetic (the primitives of vtc_index_ans.h, unchanged).
 *  - State is 32-bit.  The lower bound is L = 2^16.  Words are 16-bit.  The
 *    start state is L.
 *  - Encode a symbol (f, c) as follows.
 *    - If (uint64)x >= (uint64)f << 17, emit x & 0xFFFF and set x >>= 16.  At
 *      most once suffices.  The compare must be 64-bit because f = 2^15 gives
 *      2^32.
 *    - Then x = ((x / f) << 15) + x % f + c.
 *  - Decode under a table (freq, cum) as follows.
 *    - slot = x & 32767.
 *    - The symbol is the largest i with cum[i] <= slot.  This rule skips
 *      absent symbols correctly, including trailing ones.
 *    - x = f * (x >> 15) + slot - c.
 *    - If x < L, set x = (x << 16) | next word.  One word always suffices.
 *  - The decoder runs two phases per step.
 *    - Phase A: every active lane decodes hi under freq_hi, then renormalises.
 *    - Phase B: every active lane decodes lo under row hi of freq_lo, then
 *      renormalises.
 *    - The index is 256 hi + lo.
 *  - The encoder is the exact inverse.  It walks the steps from last to first.
 *    Within a step it encodes lo for all lanes, then hi for all lanes.
 *
 * Layout, as the decoder reads it forward from the stream's first byte.
 *  - First come 64 little-endian uint32 end states, lanes 0 ... 63, always 256
 *    bytes.
 *  - Then come the 16-bit little-endian words.
 *  - Within a step the phase-A words precede the phase-B words.
 *  - Within a phase, the lanes that need a word take consecutive words in
 *    ascending lane order (ballot + popcount of the lower lanes).  The cursor
 *    advances by the popcount.
 *  - The encoder fills the words back to front.
 *  - A stream's length is 256 + 2 * words bytes.
 *
 * Uncodable entries.  An entry is uncodable when it is negative, >= kmax, has
 * freq_hi[hi] = 0 or has freq_lo[hi, lo] = 0.  It contributes nothing in
 * either phase and leaves its lane's state alone.  It is counted in status[0],
 * and status[1] holds 1 + the first one's row.
 *
 * FREQUENCIES FROM COUNTS (utils.index_coding.index_ans_split_frequencies;
 * host, pure integers, deterministic).  For k codewords in use of kmax:
 *  1. The weight w_i is count_i, or 1 when count_i = 0, for every i < k (so
 *     every index the codebook can produce is codable); w_i = 0 for i >= k.
 *  2. Lo row h: steps 1-3 of vtc_index_ans.h on the counts of block h, indices
 *     256 h ... 256 h + 255, with k_h = clamp(k - 256 h, 0, 256) symbols in
 *     use.  A row with k_h = 0 is all zero.
 *  3. Hi: W_h = sum of w_i over block h.  Steps 2-3 of vtc_index_ans.h on the
 *     W_h of the ceil(k / 256) blocks in use; 0 beyond.
 *
 * status: int64 [3], overwritten by every call.
 *   sizes, pack   [0] uncodable entries, [1] 0 or 1 + the first one's row,
 *                 [2] 0, or the bad-table word above; from pack otherwise the
 *                 number of streams skipped or not written as the coder sizes
 *                 them (below).
 *   unpack        [0] malformed streams, [1] 0 or 1 + the first one,
 *                 [2] 0 or the bad-table word.
 */
#ifndef VTC_INDEX_ANS_SPLIT_H_
#define VTC_INDEX_ANS_SPLIT_H_

#include "../vtc_index_ans.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTC_INDEX_ANS_SPLIT_ABI_VERSION 1

#define VTC_INDEX_ANS_SPLIT_MAX_SYMBOLS 131072
/* an index's low symbol: its last 8 bits */
#define VTC_INDEX_ANS_SPLIT_LO_BITS 8

int vtc_index_ans_split_abi_version(void);

/* workspace of all three calls, each array rounded up to 256 bytes, with
 * H = ceil(kmax / 256):
 *   uint16 [H]        the exclusive cumulative sums of freq_hi
 *   uint16 [H * 256]  the exclusive cumulative sums of every row of freq_lo
 *                     (rows with freq_hi[h] = 0 are left as they were)
 *   int32  [1]        the bad-table word, INT32_MAX when none
 * Host-only; 0 for sizes the calls refuse (kmax outside 1 .. 131 072). */
size_t vtc_index_ans_split_workspace_bytes(int32_t kmax);

/* The coder run without stores.  stream_bytes int32 [n], n = ceil(b / R):
 * 256 + 2 * words of every stream. */
int vtc_index_ans_split_sizes(const int32_t* indices, int64_t b,
                              const uint16_t* freq_hi, const uint16_t* freq_lo,
                              int32_t kmax, int32_t rows_per_stream,
                              int32_t* stream_bytes, int64_t* status,
                              void* workspace, size_t workspace_bytes,
                              void* stream);

/* stream_bytes int32 [n] as vtc_index_ans_split_sizes wrote it; offsets int64
 * [n + 1] in bytes, e.g. vtc_jpeg_bit_offsets of stream_bytes.  packed uint8
 * [packed_bytes] is zeroed by the call; packed_bytes >= 0.
 * Stream s occupies [offsets[s], offsets[s] + stream_bytes[s]).  If that range
 * is not inside [0, packed_bytes) or not at or below offsets[s + 1] (or
 * stream_bytes[s] is below 256 or odd), the stream is skipped whole before any
 * store and counted in status[2].  Every store is bounded to the slot, also
 * when stream_bytes[s] is not the coder's own size: such a stream is counted
 * in status[2] and its contents are unspecified.  The words are stored
 * bytewise.  These are the rules of vtc_index_ans_pack. */
int vtc_index_ans_split_pack(const int32_t* indices, int64_t b,
                             const uint16_t* freq_hi, const uint16_t* freq_lo,
                             int32_t kmax, int32_t rows_per_stream,
                             const int32_t* stream_bytes,
                             const int64_t* offsets, uint8_t* packed,
                             int64_t packed_bytes, int64_t* status,
                             void* workspace, size_t workspace_bytes,
                             void* stream);

/* indices int32 [b] and used_bytes int32 [n]: every element written.
 * Stream s starts at byte offsets[s] and is read only below
 * min(offsets[s + 1], packed_bytes).  A stream is malformed when
 *  - its offsets are negative or decreasing, or its slot is shorter than 256
 *    bytes: all its indices are -1 and its used_bytes is 0;
 *  - it runs out of words, in either phase of a step: positions from that
 *    step on are -1, used_bytes is 256 + 2 * the words read before that step;
 *  - any of its 64 states is not L after the last step (rANS's free integrity
 *    check): the indices stay as decoded, each in [0, kmax).
 * Bytes left over in a slot are not an error: used_bytes reports what was
 * read.  Whatever the bytes, nothing is read or stored out of bounds, every
 * loop is bounded by the symbol count, and every search by 9 probes (hi) or 8
 * probes (lo).  `packed` must not be null but is never read when packed_bytes
 * is 0.  These are the rules of vtc_index_ans_unpack. */
int vtc_index_ans_split_unpack(const uint8_t* packed, int64_t packed_bytes,
                               const int64_t* offsets, int64_t b,
                               const uint16_t* freq_hi,
                               const uint16_t* freq_lo, int32_t kmax,
                               int32_t rows_per_stream, int32_t* indices,
                               int32_t* used_bytes, int64_t* status,
                               void* workspace, size_t workspace_bytes,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTC_INDEX_ANS_SPLIT_H_ */
