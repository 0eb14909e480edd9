// Sums and minima over one block of kThreads threads, and the one-block loop
// that turns tile sums into tile prefixes: the scans of jpeg_codec.hip (row
// offsets), jfif.hip (byte stuffing) and jfif_decode.hip (byte unstuffing,
// blocks before a subsequence).  Every function must be reached by the whole
// block; each ends behind a barrier, so its LDS words are free for the next
// call.
#pragma once

#include "common.h"

namespace vtc {

// Exclusive prefix of `v` over the block's threads; *total = block sum.
template <int kThreads>
__device__ __forceinline__ long long block_exclusive_scan(long long v,
                                                          long long* total) {
  constexpr int kWaves = kThreads / 64;
  __shared__ long long wave_sums[kWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  long long incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const long long o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  if (lane == 63) wave_sums[wave] = incl;
  __syncthreads();
  long long before = 0, all = 0;
  for (int w = 0; w < kWaves; ++w) {
    if (w < wave) before += wave_sums[w];
    all += wave_sums[w];
  }
  __syncthreads();   // wave_sums is reused by the next call
  *total = all;
  return before + incl - v;
}

// Minimum of `v` over the block's threads.
template <int kThreads>
__device__ __forceinline__ long long block_min(long long v) {
  constexpr int kWaves = kThreads / 64;
  __shared__ long long wave_mins[kWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const long long o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  if (lane == 0) wave_mins[wave] = v;
  __syncthreads();
  long long all = wave_mins[0];
  for (int w = 1; w < kWaves; ++w)
    all = wave_mins[w] < all ? wave_mins[w] : all;
  __syncthreads();
  return all;
}

// One block: sums[i] = sum of sums[0 .. i - 1] for i < tiles; returns the sum
// of all.  A thread rewrites only the entries it read.
template <int kThreads>
__device__ __forceinline__ long long block_prefix_tile_sums(long long* sums,
                                                            int64_t tiles) {
  long long carry = 0;
  for (int64_t base = 0; base < tiles; base += kThreads) {
    const int64_t i = base + threadIdx.x;
    const long long v = i < tiles ? sums[i] : 0;
    long long total;
    const long long before = block_exclusive_scan<kThreads>(v, &total);
    if (i < tiles) sums[i] = carry + before;
    carry += total;
  }
  return carry;
}

}  // namespace vtc
