// The bit writer shared by the packers of jpeg_codec.hip and index_code.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vtc {
namespace {

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

}  // namespace
}  // namespace vtc
