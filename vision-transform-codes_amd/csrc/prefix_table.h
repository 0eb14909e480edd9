// The decode table of a prefix code, stated once for the three Huffman readers
// (jpeg_decode.hip, index_decode.hip, jfif_decode.hip).  DESIGN.md 4.12 gives
// the rules and why they hold.
//
// A table is two sorted arrays and a first-level lookup.  Codeword `code` of
// `len` bits becomes the key left_align(code, len); a meta word packs what the
// codeword stands for.  Sorted by (key, length, symbol), a codeword that is a
// prefix of another stands directly before one it is a prefix of, so
// neighbours suffice to find a violation; and the codeword a window starts
// with is the largest key <= the window, provided the window really starts
// with it.  The lookup answers that question in one read for every codeword
// of at most kLutBits bits.
//
// A reader fixes the types and the packing in a policy P:
//   P::Key        unsigned type of a left-aligned codeword; its width is the
//                 longest codeword
//   P::Meta       unsigned type a meta word is kept in (in registers it is an
//                 unsigned); 0 is "no codeword"
//   P::kLutBits   bits of the first-level lookup
//   P::make(len, symbol)   the meta word, the length above the symbol
//   P::valid(m), P::len(m), P::symbol(m)
// An absent entry of a table has meta word 0 and one key for all of them.
#pragma once

#include <limits.h>

#include "bitstream.h"

namespace vtc {

template <class P>
struct PrefixTable {
  typedef typename P::Key Key;
  typedef typename P::Meta Meta;
  static constexpr int kKeyBits = 8 * (int)sizeof(Key);
  static constexpr int kLutBits = P::kLutBits;
  static constexpr int kLutSize = 1 << kLutBits;

  // whether the empty codeword (length 0) is one; no shift by the full width
  // is ever taken for it
  static constexpr bool kHasEmpty = P::valid(P::make(0, 0));

  // make() then len() and symbol() give back what went in
  static __host__ __device__ constexpr bool round_trips(int len, int symbol) {
    return P::valid(P::make(len, symbol)) && !P::valid(0) &&
           P::len(P::make(len, symbol)) == len &&
           P::symbol(P::make(len, symbol)) == symbol;
  }

  // The key of a codeword: bits above `len` fall off, a length above the
  // width reads as the width.  (No shift by the full width is taken.)
  static __device__ __forceinline__ Key left_align(u64 code, int len) {
    if (len > kKeyBits) len = kKeyBits;
    return len ? (Key)(code << (kKeyBits - len)) : (Key)0;
  }

  // The order of the sorted arrays: codewords before absent entries, then
  // (key, length, symbol).  The order of the codewords is total, so the sorted
  // arrays do not depend on the algorithm; absent entries are all alike.
  static __device__ __forceinline__ bool sorts_before(Key ka, Meta ma, Key kb,
                                                      Meta mb) {
    if (P::valid(ma) != P::valid(mb)) return P::valid(ma);
    if (ka != kb) return ka < kb;
    return ma < mb;   // the length sits above the symbol
  }

  // Bitonic sort of entries 0 .. n2 - 1 of key[] and meta[] in LDS, n2 a power
  // of two, by a block of kThreads threads; the absent entries come last.
  // Barriers: the caller's before, one after every stage here.
  template <int kThreads>
  static __device__ __forceinline__ void sort(Key* key, Meta* meta, int n2) {
    for (int k = 2; k <= n2; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = threadIdx.x; t < n2 / 2; t += kThreads) {
          // the t-th index with bit j clear, and its partner
          const int i = (t & ~(j - 1)) << 1 | (t & (j - 1));
          const int p = i | j;
          const Key ka = key[i], kb = key[p];
          const Meta ma = meta[i], mb = meta[p];
          const bool ascending = (i & k) == 0;
          const bool swap = ascending ? sorts_before(kb, mb, ka, ma)
                                      : sorts_before(ka, ma, kb, mb);
          if (swap) {
            key[i] = kb;
            meta[i] = mb;
            key[p] = ka;
            meta[p] = ma;
          }
        }
        __syncthreads();
      }
    }
  }

  // Sorted codewords i and i + 1 of one table: the smallest symbol that
  // offends, INT_MAX when the first is no prefix of the second.  Equal
  // codewords offend both; the empty codeword is a prefix of everything.
  static __device__ __forceinline__ int prefix_violation(const Key* key,
                                                         const Meta* meta,
                                                         int i) {
    const int la = P::len(meta[i]), lb = P::len(meta[i + 1]);
    if (la > lb) return INT_MAX;
    if (!(kHasEmpty && la == 0) &&
        (Key)(key[i] ^ key[i + 1]) >> (kKeyBits - la))
      return INT_MAX;
    const int a = P::symbol(meta[i]), b = P::symbol(meta[i + 1]);
    return la == lb && b < a ? b : a;
  }

  // First level: sorted codewords first, first + stride, ... below n, each of
  // at most kLutBits bits, put their meta word on the 1 << (kLutBits - len)
  // prefixes that start with them.  Prefix-free codewords own disjoint
  // ranges: any threads may share the work.  Where ranges overlap the later
  // codeword in sorted order wins, which needs ONE thread (first 0, stride 1).
  static __device__ __forceinline__ void fill_lookup(Meta* lut, const Key* key,
                                                     const Meta* meta, int n,
                                                     int first, int stride) {
    for (int r = first; r < n; r += stride) {
      const int l = P::len(meta[r]);
      if (l > kLutBits) continue;
      const int from = (int)(key[r] >> (kKeyBits - kLutBits));
      const int span = 1 << (kLutBits - l);   // from + span <= kLutSize
      for (int q = 0; q < span; ++q) lut[from + q] = meta[r];
    }
  }

  // The codeword the window `w` starts with, as a meta word; 0 when none
  // does.  lut, key, meta: one table's arrays; n: its codewords.
  static __device__ __forceinline__ unsigned match(const Meta* lut,
                                                   const Key* key,
                                                   const Meta* meta, int n,
                                                   Key w) {
    const unsigned e = lut[w >> (kKeyBits - kLutBits)];
    if (P::valid(e)) return e;
    int lo = 0, hi = n;   // lo: number of codewords <= w
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (key[mid] <= w)
        lo = mid + 1;
      else
        hi = mid;
    }
    if (lo == 0) return 0;
    const unsigned m = meta[lo - 1];
    const int l = P::len(m);
    if (!(kHasEmpty && l == 0) && (Key)(key[lo - 1] ^ w) >> (kKeyBits - l))
      return 0;
    return m;
  }

  // One codeword off a lane's bit reader (64-bit keys): its meta word, or 0
  // when no codeword matches or the match passes the row's end or the buffer;
  // nothing is consumed then.
  static __device__ __forceinline__ unsigned read(BitReader& r,
                                                  const Meta* lut,
                                                  const Key* key,
                                                  const Meta* meta, int n) {
    r.refill();
    const unsigned m = match(lut, key, meta, n, r.window64());
    if (!P::valid(m) || P::len(m) > r.avail64()) return 0;
    r.consume(P::len(m));
    return m;
  }
};

}  // namespace vtc
