// The bit writer shared by the packers of jpeg_codec.hip, index_code.hip and
// jfif.hip, and the bit reader of one lane shared by the decoders of
// jpeg_decode.hip and index_decode.hip (through prefix_table.h, which
// jfif_decode.hip includes as well: six users).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vtc {
namespace {

typedef unsigned long long u64;

// `words` is `out` rounded down to a 4-byte boundary and positions count bits
// from there: the caller's bytes are bits [lo, limit).  Writes the low n bits
// of `value`, most significant first, from `pos` on, in pieces that stay
// inside one 32-bit word; a piece is OR-ed in as the big-endian image of its
// bits, so byte j / 8 receives stream bit j at bit 7 - j % 8.  Bits outside
// [lo, limit) are dropped and counted; a word that holds no byte of the
// caller's is never addressed, and in the first and last word the bytes that
// are not the caller's receive zeros only (OR leaves them as they are).
__device__ __forceinline__ int put_bits(unsigned* words, int64_t lo,
                                        int64_t limit, int64_t pos,
                                        unsigned long long value, int n) {
  int dropped = 0;
  if (n > 64) n = 64;
  while (n > 0) {
    const int o = (int)(pos & 31);
    const int take = min(32 - o, n);
    int keep = take;
    if (pos < lo || pos >= limit)
      keep = 0;
    else if (pos + take > limit)
      keep = (int)(limit - pos);
    dropped += take - keep;
    if (keep > 0) {
      uint32_t piece = (uint32_t)(value >> (n - take));
      if (take < 32) piece &= (1u << take) - 1u;
      piece >>= take - keep;
      const uint32_t be = piece << (32 - o - keep);
      if (be) atomicOr(&words[pos >> 5], __builtin_bswap32(be));
    }
    pos += take;
    n -= take;
  }
  return dropped;
}

// ---- the bit reader of one lane ---------------------------------------------
// `win` holds the next `have` stream bits from `pos` on, left-aligned, zeros
// behind them.  A byte is loaded only when its index is below `nbytes` and
// its first bit below `end`; what a caller may use of the window is avail():
// the bits that are loaded AND belong to the row.
struct BitReader {
  const uint8_t* bytes;
  int64_t nbytes;   // packed_bytes
  int64_t end;      // the row's end, at most 8 * nbytes
  int64_t pos;      // >= 0
  int64_t next;     // index of the next byte to load
  u64 win;
  int have;

  __device__ __forceinline__ bool loadable() const {
    return next < nbytes && next * 8 < end;
  }
  __device__ __forceinline__ void seek(int64_t to) {
    pos = to;
    next = to >> 3;
    win = 0;
    have = 0;
    const int skip = (int)(to & 7);
    if (skip && loadable()) {   // the bits before `to` fall off the top
      win = (u64)bytes[next] << (56 + skip);
      have = 8 - skip;
      ++next;
    }
  }
  __device__ __forceinline__ void refill() {
    while (have <= 56 && loadable()) {
      win |= (u64)bytes[next] << (56 - have);
      have += 8;
      ++next;
    }
  }
  // After refill(): the 64 bits from pos on.  refill() stops at 57..64 bits;
  // the top of one more byte completes them, without being consumed.
  __device__ __forceinline__ u64 window64() const {
    if (have >= 57 && have < 64 && loadable())
      return win | (u64)bytes[next] >> (have - 56);
    return win;
  }
  __device__ __forceinline__ int64_t avail() const {
    const int64_t left = end - pos;
    return left < have ? left : have;
  }
  // the same for window64()
  __device__ __forceinline__ int64_t avail64() const {
    const int64_t left = end - pos;
    const int loaded = have >= 57 && have < 64 && loadable() ? 64 : have;
    return left < loaded ? left : loaded;
  }
  __device__ __forceinline__ void consume(int n) {
    if (n < have) {
      win <<= n;
      have -= n;
      pos += n;
    } else {
      seek(pos + n);
    }
  }
};

}  // namespace
}  // namespace vtc
