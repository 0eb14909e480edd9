// One axis of a spatial filter with scipy's 'symm' / 'reflect' boundary: the
// reflection rule and the float64 tap sum shared by the Gaussian window of
// local_norm.hip and the caller's filters of image_tools.hip.
#pragma once

#include "common.h"

namespace vtc {

// numpy's 'symmetric' padding: index i folds with period 2n, i mod 2n in
// [n, 2n) mirroring to 2n - 1 - i, which stays right for windows wider than
// the image.
__device__ __forceinline__ int fold(int i, int n) {
  const int p = 2 * n;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

// sum over k = 0 .. count-1, in that order, of at(fold(p + k - lead, n)) *
// tap(k) in float64: a correlation whose first tap sits `lead` samples before
// position p of an axis of n samples.  A convolution is the same sum over the
// reversed taps.
template <class Tap, class At>
__device__ __forceinline__ double tap_sum(Tap tap, int count, int lead, int p,
                                          int n, At at) {
  double acc = 0.0;
  for (int k = 0; k < count; ++k) acc += at(fold(p + k - lead, n)) * tap(k);
  return acc;
}

}  // namespace vtc
