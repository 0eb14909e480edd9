// The rANS stream coder shared by the two index range coders, index_ans.hip
// (m columns, one table each) and index_ans_split.hip (one column, a hi and a
// lo symbol per index).  It states the stream format of
// include/vtc_index_ans.h: 64 interleaved 32-bit states, L = 2^16, 16-bit
// words, a 256-byte header of end states, the words in decoder order with lane
// order inside a step.  ONE WAVE codes ONE STREAM: lane l holds state l.
// Nothing here knows how a symbol's (f, c) is found: that is the model, and
// each .hip file states its own.
#pragma once

#include <limits.h>

#include "../../include/vtc_index_ans.h"
#include "common.h"

namespace vtc {
namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / 64;
constexpr int kProbBits = VTC_INDEX_ANS_PROB_BITS;
constexpr unsigned kProbScale = 1u << kProbBits;
constexpr unsigned kLower = 1u << 16;            // L
constexpr int kHeaderBytes = 4 * VTC_INDEX_ANS_LANES;
constexpr int64_t kMaxStreamSymbols = (int64_t)1 << VTC_INDEX_ANS_MAX_STREAM_BITS;
typedef unsigned long long u64;
constexpr u64 kNoPosition = ~0ull;

static_assert(VTC_INDEX_ANS_LANES == 64, "one wave codes one stream");

// ---- status -------------------------------------------------------------------
// `bad` is a word of the workspace: what status[2] is to receive for a bad
// table, INT_MAX when none (the *_cum_kernel of the model takes the minimum).
__global__ void ans_begin_kernel(int32_t* bad, u64* status) {
  *bad = INT_MAX;
  status[0] = 0;
  status[1] = kNoPosition;   // minimum of flat positions, rows or streams
  status[2] = 0;
}

__global__ void ans_end_kernel(const int32_t* bad, u64* status) {
  status[1] = status[1] == kNoPosition ? 0 : status[1] + 1;
  if (*bad != INT_MAX) status[2] = (u64)*bad;
}

// ---- tables -------------------------------------------------------------------
// The largest i in [lo, hi] with cum[i] <= slot, given cum[lo] <= slot; at most
// ceil(log2(hi - lo + 1)) probes, none when lo == hi.
__device__ __forceinline__ int symbol_of(const uint16_t* cum, int lo, int hi,
                                         unsigned slot) {
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cum[mid] <= slot)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// The exclusive integer scan of one frequency row by one block, and the row's
// total to every thread (a good row's is kProbScale).  Thread t owns the `per`
// consecutive symbols from t * per on; the 256 partial sums are scanned in LDS
// (Hillis-Steele, 8 rounds).  All sums are 32-bit: `length` is at most 4096,
// a frequency at most 65535.  The stored uint16 is exact for a row that passes
// the check (its sums are at most 2^15); a bad row's is never read.
__device__ __forceinline__ unsigned scan_row(const uint16_t* freq,
                                             uint16_t* cum, int length,
                                             unsigned (&part)[2][kBlock]) {
  const int tid = threadIdx.x;
  const int per = (length + kBlock - 1) / kBlock;
  const int from = tid * per;
  const int to = from + per < length ? from + per : length;
  unsigned own = 0;   // at most 16 terms: not worth the vectoriser's registers
#pragma clang loop vectorize(disable) interleave(disable)
  for (int i = from; i < to; ++i) own += freq[i];
  part[0][tid] = own;
  __syncthreads();
  int in = 0;
  for (int off = 1; off < kBlock; off <<= 1) {
    unsigned v = part[in][tid];
    if (tid >= off) v += part[in][tid - off];
    part[in ^ 1][tid] = v;
    in ^= 1;
    __syncthreads();
  }
  unsigned run = part[in][tid] - own;   // exclusive
  for (int i = from; i < to; ++i) {
    cum[i] = (uint16_t)run;
    run += freq[i];
  }
  return part[in][kBlock - 1];
}

// ---- streams ------------------------------------------------------------------
struct StreamSpan {
  int64_t base;   // flat position of the stream's first symbol
  int count;      // its symbols, 1 .. 2^24
  int steps;      // ceil(count / 64)
};

// Stream s of `rows` rows of `symbols_per_row` symbols each, the last stream
// what is left of b.
__device__ __forceinline__ StreamSpan stream_span(int64_t s, int64_t b,
                                                  int rows,
                                                  int symbols_per_row) {
  StreamSpan span;
  const int64_t row0 = s * rows;
  const int64_t left = b - row0;
  const int64_t here = left < rows ? left : rows;
  span.base = row0 * symbols_per_row;
  span.count = (int)(here * symbols_per_row);   // <= 2^24
  span.steps = (span.count + 63) >> 6;
  return span;
}

__device__ __forceinline__ unsigned lower_lanes(u64 mask, int lane) {
  return (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
}

// ---- encoding -------------------------------------------------------------------
// pack: the stream's slot, and the words the caller's size leaves room for.
// sizes: no slot, and the cursor counts down from 0.
struct EncodeSlot {
  uint8_t* slot;
  int room;   // words
};

// False when the caller's size and offsets admit no slot: counted in
// status[2], and the whole wave leaves.
__device__ __forceinline__ bool open_pack_slot(
    EncodeSlot& out, int64_t s, const int32_t* __restrict__ sizes_in,
    const int64_t* __restrict__ offsets, uint8_t* __restrict__ packed,
    int64_t packed_bytes, int lane, u64* __restrict__ status) {
  const int64_t from = offsets[s], to = offsets[s + 1];
  const int64_t size = sizes_in[s];
  const bool fits = size >= kHeaderBytes && (size & 1) == 0 && from >= 0 &&
                    from <= packed_bytes - size && from + size <= to;
  if (!fits) {
    if (lane == 0) atomicAdd(&status[2], 1ull);
    return false;
  }
  out.slot = packed + from;
  out.room = (int)((size - kHeaderBytes) >> 1);
  return true;
}

// One phase of one step of a stream's encoder: the lanes with f != 0 code the
// symbol (f, c); the words they emit lie in front of everything emitted so
// far, in lane order.
template <bool kStore>
__device__ __forceinline__ void encode_phase(unsigned f, unsigned c,
                                             unsigned& x, int& cursor,
                                             uint8_t* slot, int room, int lane,
                                             bool& strayed) {
  const bool emit = f != 0 && (u64)x >= ((u64)f << (kProbBits + 2));
  const u64 mask = __ballot(emit);
  cursor -= __popcll(mask);
  if (emit) {
    if (kStore) {
      const int w = cursor + (int)lower_lanes(mask, lane);
      if (w >= 0 && w < room) {
        uint8_t* at = slot + kHeaderBytes + 2 * (int64_t)w;
        at[0] = (uint8_t)x;
        at[1] = (uint8_t)(x >> 8);
      } else {
        strayed = true;
      }
    }
    x >>= 16;
  }
  if (f != 0) x = ((x / f) << kProbBits) + x % f + c;
}

// The end of a stream's encoder.  pack: the end states into the header, and
// the stream counted in status[2] when words were lost at the front or the
// size is larger than the coder's own.  sizes: the stream's bytes.  Both: the
// lanes' uncodable entries into status[0], the smallest of their positions
// into status[1].
template <bool kStore>
__device__ __forceinline__ void finish_encode(
    unsigned x, int cursor, bool strayed, int uncodable, u64 first,
    uint8_t* slot, int64_t s, int lane, int32_t* __restrict__ sizes_out,
    u64* __restrict__ status) {
  if (kStore) {
    uint8_t* at = slot + 4 * lane;   // room >= 0: the header is inside the slot
    at[0] = (uint8_t)x;
    at[1] = (uint8_t)(x >> 8);
    at[2] = (uint8_t)(x >> 16);
    at[3] = (uint8_t)(x >> 24);
    if (__ballot(strayed || cursor != 0) && lane == 0)
      atomicAdd(&status[2], 1ull);
  } else if (lane == 0) {
    sizes_out[s] = kHeaderBytes - 2 * cursor;   // cursor = -words
  }
  const int count = wave_sum_int(uncodable);
  if (count) {   // the whole wave
    first = wave_min(first);
    if (lane == 0) {
      atomicAdd(&status[0], (u64)count);
      atomicMin(&status[1], first);
    }
  }
}

// ---- decoding -------------------------------------------------------------------
__device__ __forceinline__ unsigned load_le(const uint8_t* __restrict__ at,
                                            int bytes) {
  unsigned v = 0;
  for (int i = 0; i < bytes; ++i) v |= (unsigned)at[i] << (8 * i);
  return v;
}

struct DecodeSlot {
  const uint8_t* slot;
  int room;      // words of the slot, at most max_words
  bool opened;   // the header is inside the slot: `x` is the lane's end state
};

// With good tables (`decoding`), the slot that the offsets give stream s, cut
// at packed_bytes, and the lane's state out of its header; not opened where
// the offsets decrease or leave no room for a header: that stream is malformed.
__device__ __forceinline__ DecodeSlot open_decode_slot(
    bool decoding, int64_t s, const int64_t* __restrict__ offsets,
    const uint8_t* __restrict__ packed, int64_t packed_bytes,
    int64_t max_words, int lane, unsigned& x) {
  const int64_t from = offsets[s], next = offsets[s + 1];
  const int64_t stop = next < packed_bytes ? next : packed_bytes;
  DecodeSlot in = {packed, 0, decoding};
  if (decoding && (from < 0 || from > next || stop - from < kHeaderBytes))
    in.opened = false;
  x = kLower;
  if (in.opened) {
    in.slot = packed + from;
    const int64_t words = (stop - from - kHeaderBytes) >> 1;
    in.room = words < max_words ? (int)words : (int)max_words;
    x = load_le(in.slot + 4 * lane, 4);
    // No instruction: the load is waited for here.  Left to its first use,
    // the wait sits in the step loop, where it also waits for the store of
    // the step before.
    asm volatile("" : "+v"(x));
  }
  return in;
}

// The renormalisation of one phase: the lanes with `need` take the next words
// in lane order.  False when the slot has too few: the whole wave stops, and
// nothing was read.
__device__ __forceinline__ bool refill(bool need, unsigned& x, int& cursor,
                                       const uint8_t* __restrict__ slot,
                                       int room, int lane) {
  const u64 mask = __ballot(need);
  const int taken = __popcll(mask);
  if (cursor + taken > room) return false;
  if (need) {
    const int w = cursor + (int)lower_lanes(mask, lane);   // < room
    x = x << 16 | load_le(slot + kHeaderBytes + 2 * (int64_t)w, 2);
  }
  cursor += taken;
  return true;
}

// The end of a stream's decoder: the free integrity check (every state back at
// L; a stream that ran dry is already malformed), the bytes it read, and a
// malformed stream into status[0] and status[1].
__device__ __forceinline__ void finish_decode(
    bool alive, bool malformed, unsigned x, bool opened, int cursor, int64_t s,
    int lane, int32_t* __restrict__ used_bytes, u64* __restrict__ status) {
  if (alive && __ballot(x != kLower)) malformed = true;
  if (lane == 0) {
    used_bytes[s] = opened ? kHeaderBytes + 2 * cursor : 0;
    if (malformed) {
      atomicAdd(&status[0], 1ull);
      atomicMin(&status[1], (u64)s);
    }
  }
}

// ---- host side ------------------------------------------------------------------
// The streams of b rows, `rows` each; VTC_OK when the grid takes them, the
// error text set otherwise.  (That a stream holds at most kMaxStreamSymbols
// symbols is the model's check: its text names the model's arguments.)
int check_streams(const char* who, int64_t b, int32_t rows, int64_t* streams) {
  *streams = ceil_div(b, rows);
  if (ceil_div(*streams, kWavesPerBlock) >= (int64_t)1 << 31) {
    set_error("%s: b = %lld, too many streams", who, (long long)b);
    return VTC_ERR_UNSUPPORTED;
  }
  return VTC_OK;
}

int check_workspace(const char* who, size_t need, const void* workspace,
                    size_t workspace_bytes) {
  if (!workspace || workspace_bytes < need) {
    set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
              need);
    return VTC_ERR_WORKSPACE;
  }
  return VTC_OK;
}

}  // namespace
}  // namespace vtc
