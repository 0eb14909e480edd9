/*
 * vtc_jfif_decode.h -- sixteenth header of libvtc_hip.so: the device half of
 * a baseline JFIF reader (ITU-T T.81 sequential DCT, Huffman, 8-bit, one
 * interleaved scan, no restart intervals), the way back from the bytes the
 * fifteenth header writes -- or any other baseline encoder.  DESIGN.md 4.24.
 *
 *   stuffed bytes -> vtc_jfif_unstuff_bytes -> the entropy-coded segment
 *   segment       -> vtc_jfif_unpack        -> levels (rows, 64), DIFF in
 *                                              column 0
 *   levels        -> vtc_jfif_dc_accumulate -> absolute DC levels
 *   levels        -> the inverse DCT of the fifteenth header -> planes
 *
 * The markers and header segments of the file are walked on the host
 * (utils/jfif.py).  Restart intervals, progressive and arithmetic modes,
 * 12-bit samples and four-component files are not provided.
 *
 * This header lives under include/ext/ like the fifteenth.  The functions live
 * in the same shared library and follow the same conventions: every pointer
 * is a DEVICE pointer to a contiguous row-major array and needs the alignment
 * of its element and no more (1 byte for uint8, 2 for uint16, 4 for int32, 8
 * for int64); `workspace` must be 256-byte aligned; `stream` last; functions
 * only enqueue work on `stream` and never wait for it; no allocation inside,
 * scratch comes from the caller, sized by the matching *_workspace_bytes()
 * query; null pointers and bad sizes are answered before any device work
 * (VTC_ERR_INVALID_ARGUMENT, VTC_ERR_WORKSPACE) with text in
 * vtc_last_error().  Every output is bitwise reproducible: every output
 * element is written by exactly one thread, the status words are integer
 * minima.  No inline assembly, no float atomics.
 *
 * The bit stream: stream bit j is bit 7 - j % 8 of byte j / 8; a read at or
 * beyond bit 8 seg_bytes gives 1.
 *
 * Tables, as the pack call of the fifteenth header takes them: ac_code
 * uint16[2][256] and ac_len uint8[2][256] indexed by [table][run << 4 |
 * size], dc_code uint16[2][16] and dc_len uint8[2][16] indexed by
 * [table][category]; each codeword in the low `len` bits, first stream bit the
 * most significant of them; length 0 = symbol absent, a length above 16 is
 * read as 16.  Each table must be prefix-free; one that is not decodes as some
 * fixed code of its codewords, never out of bounds.
 *
 * Tokens (T.81 F.2.2).  A block is a DC token -- a codeword of the DC table
 * naming a category 0 .. 11, then that many value bits -- and AC tokens of the
 * AC table until index 63 is written or an end of block is read: byte
 * run << 4 | size with size 1 .. 10 skips `run` zeros and reads `size` value
 * bits for the next coefficient, 0xF0 skips sixteen zeros (it may end exactly
 * at index 63), 0x00 ends the block; no end of block follows index 63.  Value
 * bits v of size n give v when their first bit is 1 and v - 2^n + 1 otherwise
 * (EXTEND).  A token is MALFORMED when no codeword of at most 16 bits matches,
 * the DC category is above 11, the AC size is above 10, the AC byte has size
 * 0 and run 1 .. 14, or a coefficient or a 0xF0 run would pass index 63.
 */
#ifndef VTC_JFIF_DECODE_H_
#define VTC_JFIF_DECODE_H_

#include "../vtc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VTC_JFIF_DECODE_ABI_VERSION 1
/* bytes per subsequence of vtc_jfif_unpack: one lane decodes one */
#define VTC_JFIF_SUBSEQ_BYTES 128
/* subsequences per workgroup of vtc_jfif_unpack */
#define VTC_JFIF_SUBSEQ_PER_GROUP 256
/* chain elements per tile of vtc_jfif_dc_accumulate */
#define VTC_JFIF_DC_TILE 256
/* block positions of one MCU, at most */
#define VTC_JFIF_MAX_SLOTS 10

int vtc_jfif_decode_abi_version(void);

/* ---- byte unstuffing --------------------------------------------------------
 * The inverse of the stuffing call of the fifteenth header.  in uint8[n].
 *   marker_at = the smallest i with in[i] == 0xFF and (i + 1 >= n or
 *               in[i + 1] != 0x00); n when there is none.
 * Every byte i < marker_at goes to out[i - (number of FF 00 pairs wholly
 * before i)], except a 0x00 that directly follows a 0xFF, which goes nowhere.
 * out_len int64[2] (device) receives the unstuffed length and marker_at,
 * whether or not the output fits; bytes that would land at or beyond capacity
 * are dropped, never written, and counted in status[0] (int32[1], saturated at
 * INT32_MAX).  Bytes of out at or beyond the unstuffed length are left as they
 * are.  n >= 0, capacity >= 0; `in` may be null when n = 0 and out when
 * capacity = 0; out must not overlap in.
 * Tiles of VTC_JFIF_STUFF_TILE (2048) bytes count their stuffed zeros and find
 * their first marker, one block scans the tiles, each tile rescans and
 * stores: no atomics, no zero-fill.  A pair that straddles two tiles is
 * counted in the tile of its 0x00.
 * workspace: two int64 arrays of one entry per tile, and two words. */
size_t vtc_jfif_unstuff_bytes_workspace_bytes(int64_t n);
int vtc_jfif_unstuff_bytes(const uint8_t* in, int64_t n, uint8_t* out,
                           int64_t capacity, int64_t* out_len, int32_t* status,
                           void* workspace, size_t workspace_bytes,
                           void* stream);

/* ---- the entropy-coded segment -> levels ------------------------------------
 * seg uint8[seg_bytes], 1 <= seg_bytes < 2^31.  slot_dc and slot_ac
 * uint8[nslots], 1 <= nslots <= VTC_JFIF_MAX_SLOTS: the table (0, or 1 for
 * anything else) of each block position inside an MCU; block r of the scan
 * uses position r % nslots.  levels int32 (rows, 64), 1 <= rows < 2^31, is
 * zero-filled, then every nonzero level of blocks 0 .. rows - 1 is stored, in
 * zigzag order; column 0 receives DIFF, not the DC level
 * (vtc_jfif_dc_accumulate).
 *
 * The sequential decoder this call equals: from bit 0, block after block,
 * until `rows` blocks are complete or a token would START at or beyond bit
 * 8 seg_bytes.  status int64[4], overwritten:
 *   [0]  0, or 1 + the bit position of the first malformed token on that path
 *   [1]  blocks completed, at most rows; when [0] is set, the blocks completed
 *        before that token
 *   [2]  the bit position just after block `rows`, or -1 if the stream ended
 *        first or [0] is set.  A last token that needed bits beyond the end
 *        (read as ones) leaves a position above 8 seg_bytes.
 *   [3]  synchronisation rounds taken (below)
 * Rows completed before the first malformed token are the sequential
 * decoder's; later rows may hold anything.  Nothing is read or written out of
 * bounds whatever the bytes are.
 *
 * Method: self-synchronising parallel decoding.  The segment is cut into
 * subsequences of VTC_JFIF_SUBSEQ_BYTES bytes, one lane each.  The state at a
 * boundary is (bit position of the next token, coefficient index with 0 = a DC
 * token is next, block position in the MCU).  Subsequence 0 starts at
 * (0, 0, 0), every other one from the guess (its first bit, 0, 0); a lane
 * decodes until its position reaches the end of its subsequence and records
 * its exit state and the blocks it completed; every round decodes each
 * subsequence again from the exit state its predecessor recorded in the round
 * before, until a round changes no exit state.  On a guessed state a
 * malformed token consumes its codeword (one bit when none matches) and ends
 * the block: a function of state and bits that always advances.
 * VTC_JFIF_SUBSEQ_PER_GROUP subsequences share a workgroup, which iterates to
 * its own fixed point in LDS; the kernel is enqueued once per workgroup of
 * the segment, and in launch l a workgroup whose incoming state equals the
 * one it last decoded from copies its exit state and stops, so after launch l
 * workgroups 0 .. l are final.  No workgroup waits for another.  [3] is the
 * sum over launches of the largest number of rounds, in any workgroup of the
 * launch, that changed an exit state.  Then one block scans the block counts
 * and a last pass decodes from the true states and stores.
 * workspace: the decode tables, six arrays of one or two words per workgroup
 * and two words per subsequence. */
size_t vtc_jfif_unpack_workspace_bytes(int64_t seg_bytes);
int vtc_jfif_unpack(const uint8_t* seg, int64_t seg_bytes,
                    const uint8_t* slot_dc, const uint8_t* slot_ac,
                    int32_t nslots, const uint16_t* ac_code,
                    const uint8_t* ac_len, const uint16_t* dc_code,
                    const uint8_t* dc_len, int32_t* levels, int64_t rows,
                    int64_t* status, void* workspace, size_t workspace_bytes,
                    void* stream);

/* ---- DC prediction undone ---------------------------------------------------
 * levels int32 (d, 64), column 0 updated in place.  order int32[d]: the rows
 * sorted by component, then by scan order; start uint8[d]: non-zero where a
 * component's chain begins.  For j ascending:
 *   acc = start[j] ? 0 : acc;  acc += levels[order[j]][0]  (32-bit, wrapping);
 *   levels[order[j]][0] = acc
 * with acc = 0 before j = 0.  An entry of order outside [0, d) adds 0 and
 * writes nothing; the entries inside must be distinct.  A segmented inclusive
 * scan: tiles of VTC_JFIF_DC_TILE elements reduce, one block scans the tile
 * carries, each tile rescans and stores.  d >= 1.
 * workspace: two int32 per tile. */
size_t vtc_jfif_dc_accumulate_workspace_bytes(int64_t d);
int vtc_jfif_dc_accumulate(int32_t* levels, int64_t d, const int32_t* order,
                           const uint8_t* start, void* workspace,
                           size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTC_JFIF_DECODE_H_ */
