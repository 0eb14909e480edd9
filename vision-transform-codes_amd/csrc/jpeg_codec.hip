// JPEG source coding of utils/jpeg.py on the device (include/vtc_codec.h):
// quantise, run-length symbols and their counts, stream lengths, offsets,
// packed streams.  DESIGN.md 4.11 states the coding rules.
//
// One wave walks one patch (row of s levels) 64 coefficients at a time: lane k
// of chunk c holds level c * 64 + k, __ballot(level != 0) is the chunk's mask
// of nonzero AC levels, the previous nonzero of a lane is the highest set bit
// of the mask below it -- or, when there is none, the last nonzero of the
// earlier chunks, carried in a wave-uniform register (0 at the start: the run
// before the first AC level counts from index 1 whatever v[0] is).  A lane
// with a nonzero level owns one token: z / 16 copies of 0xF0, the symbol
// (z % 16) << 4 | size, and size value bits.  Lane 0 of chunk 0 also owns the
// end-of-block symbol and the DC part, which follow the AC part.
//
// Every wave walks kRowsPerWave consecutive rows, so a 256-thread block covers
// 256 rows and its 32-bit LDS bins (at most 4096 increments per row) cannot
// wrap.  All three row kernels share lane_token(): what one counts, the other
// measures and the third writes.
#include <limits.h>

#include "../../include/vtc_codec.h"
#include "bitstream.h"
#include "block_scan.h"
#include "common.h"

namespace vtc {
namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / 64;
constexpr int kRowsPerWave = 64;
constexpr int kRowsPerBlock = kWavesPerBlock * kRowsPerWave;
constexpr int kSymbols = 256 + 16;   // AC bytes, then DC categories
constexpr int kDcBase = 256;
constexpr int kEob = 0x00, kZrl = 0xF0;
constexpr int kScanItems = 8;
constexpr int kScanTile = kBlock * kScanItems;

// What lane `lane` of chunk `chunk` contributes to the stream of one row.
struct LaneToken {
  bool ac;          // a nonzero level at index >= 1: owns an AC token
  bool over;        // |level| > 32767
  int z;            // zeros since the previous nonzero AC level
  int size;         // bit length of |level|, clamped to 15
  uint32_t value;   // the `size` value bits
};

// Must be reached by the whole wave (it ballots).  `carry`: index of the last
// nonzero AC level of the earlier chunks of this row, 0 when there is none.
__device__ __forceinline__ LaneToken lane_token(const int32_t* row, int s,
                                                int chunk, int lane,
                                                int& carry) {
  LaneToken t;
  const int idx = chunk * 64 + lane;
  const bool active = idx < s;
  const int32_t v = active ? row[idx] : 0;
  const uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
  int size = 32 - __clz((int)a);
  if (a == 0) size = 0;
  t.over = size > 15;
  if (t.over) size = 15;
  t.size = size;
  t.value = (v < 0 ? ~a : a) & ((1u << size) - 1u);
  t.ac = active && idx >= 1 && v != 0;
  const unsigned long long mask = __ballot(t.ac);
  const unsigned long long below = mask & ((1ull << lane) - 1ull);
  const int prev = below ? chunk * 64 + 63 - __clzll((long long)below) : carry;
  t.z = idx - prev - 1;
  if (mask) carry = chunk * 64 + 63 - __clzll((long long)mask);
  return t;
}

__global__ void status_begin_kernel(int32_t* status) {
  status[0] = 0;
  status[1] = INT_MAX;
}
__global__ void status_end_kernel(int32_t* status) {
  if (status[1] == INT_MAX) status[1] = 0;
}

// ---- counts ---------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void symbol_counts_kernel(
    const int32_t* __restrict__ levels, int64_t d, int s,
    unsigned long long* __restrict__ ac_counts,
    unsigned long long* __restrict__ dc_counts, int32_t* __restrict__ status) {
  __shared__ unsigned bins[kSymbols];
  for (int i = threadIdx.x; i < kSymbols; i += kBlock) bins[i] = 0;
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t row0 =
      ((int64_t)blockIdx.x * kWavesPerBlock + wave) * kRowsPerWave;
  const int chunks = (s + 63) >> 6;
  int over = 0;
  for (int r = 0; r < kRowsPerWave && row0 + r < d; ++r) {
    const int32_t* row = levels + (row0 + r) * s;
    int carry = 0;
    for (int chunk = 0; chunk < chunks; ++chunk) {
      const LaneToken t = lane_token(row, s, chunk, lane, carry);
      over += t.over;
      if (t.ac) {
        atomicAdd(&bins[(t.z & 15) << 4 | t.size], 1u);
        if (t.z >> 4) atomicAdd(&bins[kZrl], (unsigned)(t.z >> 4));
      }
      if (chunk == 0 && lane == 0) {
        atomicAdd(&bins[kEob], 1u);
        atomicAdd(&bins[kDcBase + t.size], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kSymbols; i += kBlock) {
    const unsigned n = bins[i];
    if (n)
      atomicAdd(i < kDcBase ? &ac_counts[i] : &dc_counts[i - kDcBase],
                (unsigned long long)n);
  }
  over = wave_sum_int(over);
  if (lane == 0 && over) atomicAdd(&status[0], over);
}

// Bits of one lane's AC token under the table `len` (LDS, kSymbols bytes); a
// used symbol of length 0 lowers `missing` to 1 + its id.
__device__ __forceinline__ int ac_token_bits(const LaneToken& t,
                                             const uint8_t* len,
                                             int& missing) {
  if (!t.ac) return 0;
  const int sym = (t.z & 15) << 4 | t.size;
  const int ls = len[sym];
  if (!ls) missing = min(missing, sym + 1);
  int bits = ls + t.size;
  const int zrl = t.z >> 4;
  if (zrl) {
    const int lf = len[kZrl];
    if (!lf) missing = min(missing, kZrl + 1);
    bits += zrl * lf;
  }
  return bits;
}

// ---- stream lengths -------------------------------------------------------
__global__ __launch_bounds__(kBlock) void stream_bits_kernel(
    const int32_t* __restrict__ levels, int64_t d, int s,
    const uint8_t* __restrict__ ac_len, const uint8_t* __restrict__ dc_len,
    int32_t* __restrict__ bits, int32_t* __restrict__ status) {
  __shared__ uint8_t len[kSymbols];
  for (int i = threadIdx.x; i < kSymbols; i += kBlock)
    len[i] = i < kDcBase ? ac_len[i] : dc_len[i - kDcBase];
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t row0 =
      ((int64_t)blockIdx.x * kWavesPerBlock + wave) * kRowsPerWave;
  const int chunks = (s + 63) >> 6;
  int over = 0, missing = INT_MAX;
  for (int r = 0; r < kRowsPerWave && row0 + r < d; ++r) {
    const int32_t* row = levels + (row0 + r) * s;
    int carry = 0, total = 0;
    for (int chunk = 0; chunk < chunks; ++chunk) {
      const LaneToken t = lane_token(row, s, chunk, lane, carry);
      over += t.over;
      total += ac_token_bits(t, len, missing);
      if (chunk == 0 && lane == 0) {
        const int le = len[kEob], ld = len[kDcBase + t.size];
        if (!le) missing = min(missing, kEob + 1);
        if (!ld) missing = min(missing, kDcBase + t.size + 1);
        total += le + ld + t.size;
      }
    }
    total = wave_sum_int(total);
    if (lane == 0) bits[row0 + r] = total;
  }
  over = wave_sum_int(over);
  if (lane == 0 && over) atomicAdd(&status[0], over);
  missing = wave_min(missing);
  if (lane == 0 && missing != INT_MAX) atomicMin(&status[1], missing);
}

// ---- packing --------------------------------------------------------------
// put_bits(): bitstream.h
__global__ __launch_bounds__(kBlock) void pack_kernel(
    const int32_t* __restrict__ levels, int64_t d, int s,
    const unsigned long long* __restrict__ ac_code,
    const uint8_t* __restrict__ ac_len,
    const unsigned long long* __restrict__ dc_code,
    const uint8_t* __restrict__ dc_len, const int64_t* __restrict__ offsets,
    uint8_t* out, int64_t out_bytes, int32_t* __restrict__ status) {
  __shared__ uint8_t len[kSymbols];
  __shared__ unsigned long long code[kSymbols];
  for (int i = threadIdx.x; i < kSymbols; i += kBlock) {
    len[i] = i < kDcBase ? ac_len[i] : dc_len[i - kDcBase];
    code[i] = i < kDcBase ? ac_code[i] : dc_code[i - kDcBase];
  }
  __syncthreads();
  const uintptr_t address = reinterpret_cast<uintptr_t>(out);
  unsigned* words = reinterpret_cast<unsigned*>(address & ~(uintptr_t)3);
  const int64_t lo = (int64_t)(address & 3) * 8;
  const int64_t limit = lo + out_bytes * 8;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t row0 =
      ((int64_t)blockIdx.x * kWavesPerBlock + wave) * kRowsPerWave;
  const int chunks = (s + 63) >> 6;
  int over = 0, missing = INT_MAX, dropped = 0;
  for (int r = 0; r < kRowsPerWave && row0 + r < d; ++r) {
    const int32_t* row = levels + (row0 + r) * s;
    // a negative offset stays negative: lo <= 24
    const int64_t base = offsets[row0 + r] < 0 ? offsets[row0 + r]
                                               : offsets[row0 + r] + lo;
    int carry = 0, dc_size = 0;
    uint32_t dc_value = 0;
    int64_t run = 0;
    for (int chunk = 0; chunk < chunks; ++chunk) {
      const LaneToken t = lane_token(row, s, chunk, lane, carry);
      over += t.over;
      if (chunk == 0) {   // lane 0 keeps the DC part for the end
        dc_size = t.size;
        dc_value = t.value;
      }
      const int mine = ac_token_bits(t, len, missing);
      int incl = mine;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
      }
      if (t.ac) {
        int64_t pos = base + run + (incl - mine);
        const int lf = len[kZrl];
        for (int k = t.z >> 4; k > 0; --k) {
          dropped += put_bits(words, lo, limit, pos, code[kZrl], lf);
          pos += min(lf, 64);
        }
        const int sym = (t.z & 15) << 4 | t.size;
        dropped += put_bits(words, lo, limit, pos, code[sym], len[sym]);
        pos += min((int)len[sym], 64);
        dropped += put_bits(words, lo, limit, pos, t.value, t.size);
      }
      run += __shfl(incl, 63, 64);
    }
    if (lane == 0) {
      int64_t pos = base + run;
      const int le = len[kEob], ld = len[kDcBase + dc_size];
      if (!le) missing = min(missing, kEob + 1);
      if (!ld) missing = min(missing, kDcBase + dc_size + 1);
      dropped += put_bits(words, lo, limit, pos, code[kEob], le);
      pos += min(le, 64);
      dropped += put_bits(words, lo, limit, pos, code[kDcBase + dc_size], ld);
      pos += min(ld, 64);
      dropped += put_bits(words, lo, limit, pos, dc_value, dc_size);
    }
  }
  over = wave_sum_int(over + dropped);
  if (lane == 0 && over) atomicAdd(&status[0], over);
  missing = wave_min(missing);
  if (lane == 0 && missing != INT_MAX) atomicMin(&status[1], missing);
}

// ---- offsets: exclusive scan in three steps (block_scan.h) -------------------
__device__ __forceinline__ long long scan_thread_sum(const int32_t* bits,
                                                     int64_t d, int64_t first) {
  long long sum = 0;
  for (int k = 0; k < kScanItems; ++k)
    if (first + k < d) sum += bits[first + k];
  return sum;
}

// step 1: sums[b] = sum of tile b
__global__ __launch_bounds__(kBlock) void scan_tile_sums_kernel(
    const int32_t* __restrict__ bits, int64_t d, long long* __restrict__ sums) {
  const int64_t first =
      (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  long long total;
  block_exclusive_scan<kBlock>(scan_thread_sum(bits, d, first), &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// step 2 (one block): sums[b] = sum of the tiles before b
__global__ __launch_bounds__(kBlock) void scan_sums_kernel(
    long long* __restrict__ sums, int64_t tiles) {
  block_prefix_tile_sums<kBlock>(sums, tiles);
}

// step 3: offsets of tile b, and offsets[d] from the thread that holds row d-1
__global__ __launch_bounds__(kBlock) void scan_write_kernel(
    const int32_t* __restrict__ bits, int64_t d,
    const long long* __restrict__ sums, long long* __restrict__ offsets) {
  const int64_t first =
      (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  long long total;
  long long at = sums[blockIdx.x] + block_exclusive_scan<kBlock>(
                                        scan_thread_sum(bits, d, first), &total);
  for (int k = 0; k < kScanItems; ++k) {
    const int64_t i = first + k;
    if (i >= d) break;
    offsets[i] = at;
    at += bits[i];
    if (i == d - 1) offsets[d] = at;
  }
}

struct OffsetsLayout {
  long long* sums;
  OffsetsLayout(Carver& c, int64_t d) {
    sums = c.take<long long>((size_t)ceil_div(d, kScanTile));
  }
};

// ---- quantise / dequantise --------------------------------------------------
__global__ __launch_bounds__(kBlock) void quantize_kernel(
    const float* __restrict__ codes, const double* __restrict__ binwidths,
    const int32_t* __restrict__ order, int32_t* __restrict__ levels,
    int64_t total, int s) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total;
       i += stride) {
    const int k = (int)(i % s);
    const int from = order ? order[k] : k;
    int32_t level = INT_MIN;
    if ((unsigned)from < (unsigned)s) {
      const double q = rint((double)codes[i - k + from] / binwidths[k]);
      if (q >= 2147483647.0)
        level = INT_MAX;
      else if (q > -2147483648.0)   // false for NaN
        level = (int32_t)q;
    }
    levels[i] = level;
  }
}

__global__ __launch_bounds__(kBlock) void dequantize_kernel(
    const int32_t* __restrict__ levels, const double* __restrict__ binwidths,
    const int32_t* __restrict__ order, float* __restrict__ codes,
    int64_t total, int s) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total;
       i += stride) {
    const int k = (int)(i % s);
    const int to = order ? order[k] : k;
    if ((unsigned)to < (unsigned)s)
      codes[i - k + to] = (float)((double)levels[i] * binwidths[k]);
  }
}

int check_rows(const char* who, int64_t d, int32_t s, int64_t* blocks) {
  VTC_REQUIRE(d > 0, "%s: bad size d = %lld", who, (long long)d);
  VTC_REQUIRE(s >= 1 && s <= VTC_JPEG_MAX_S,
              "%s: bad size s = %d (1 .. %d)", who, s, VTC_JPEG_MAX_S);
  *blocks = ceil_div(d, kRowsPerBlock);
  VTC_REQUIRE(*blocks < (int64_t)1 << 31, "%s: too many rows", who);
  return VTC_OK;
}

int elementwise_blocks(int64_t total) {
  const int64_t blocks = ceil_div(total, kBlock);
  return (int)(blocks < 65536 ? blocks : 65536);
}

}  // namespace
}  // namespace vtc

using namespace vtc;

extern "C" int vtc_codec_abi_version(void) { return VTC_CODEC_ABI_VERSION; }

extern "C" int vtc_jpeg_quantize(const float* codes, const double* binwidths,
                                 const int32_t* order, int32_t* levels,
                                 int64_t d, int32_t s, void* stream) {
  const char* who = "vtc_jpeg_quantize";
  VTC_REQUIRE(codes && binwidths && levels, "%s: null pointer", who);
  int64_t unused;
  const int rc = check_rows(who, d, s, &unused);
  if (rc != VTC_OK) return rc;
  const int64_t total = d * s;
  quantize_kernel<<<elementwise_blocks(total), kBlock, 0, as_stream(stream)>>>(
      codes, binwidths, order, levels, total, s);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" int vtc_jpeg_dequantize(const int32_t* levels,
                                   const double* binwidths,
                                   const int32_t* order, float* codes,
                                   int64_t d, int32_t s, void* stream) {
  const char* who = "vtc_jpeg_dequantize";
  VTC_REQUIRE(levels && binwidths && codes, "%s: null pointer", who);
  int64_t unused;
  const int rc = check_rows(who, d, s, &unused);
  if (rc != VTC_OK) return rc;
  const int64_t total = d * s;
  dequantize_kernel<<<elementwise_blocks(total), kBlock, 0,
                      as_stream(stream)>>>(levels, binwidths, order, codes,
                                           total, s);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" int vtc_jpeg_symbol_counts(const int32_t* levels, int64_t d,
                                      int32_t s, uint64_t* ac_counts,
                                      uint64_t* dc_counts, int32_t* status,
                                      void* stream) {
  const char* who = "vtc_jpeg_symbol_counts";
  VTC_REQUIRE(levels && ac_counts && dc_counts && status, "%s: null pointer",
              who);
  int64_t blocks;
  const int rc = check_rows(who, d, s, &blocks);
  if (rc != VTC_OK) return rc;
  hipStream_t st = as_stream(stream);
  VTC_HIP_CHECK(hipMemsetAsync(ac_counts, 0, 256 * sizeof(uint64_t), st));
  VTC_HIP_CHECK(hipMemsetAsync(dc_counts, 0, 16 * sizeof(uint64_t), st));
  status_begin_kernel<<<1, 1, 0, st>>>(status);
  symbol_counts_kernel<<<(int)blocks, kBlock, 0, st>>>(
      levels, d, s, reinterpret_cast<unsigned long long*>(ac_counts),
      reinterpret_cast<unsigned long long*>(dc_counts), status);
  status_end_kernel<<<1, 1, 0, st>>>(status);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" int vtc_jpeg_stream_bits(const int32_t* levels, int64_t d,
                                    int32_t s, const uint8_t* ac_len,
                                    const uint8_t* dc_len, int32_t* bits,
                                    int32_t* status, void* stream) {
  const char* who = "vtc_jpeg_stream_bits";
  VTC_REQUIRE(levels && ac_len && dc_len && bits && status,
              "%s: null pointer", who);
  int64_t blocks;
  const int rc = check_rows(who, d, s, &blocks);
  if (rc != VTC_OK) return rc;
  hipStream_t st = as_stream(stream);
  status_begin_kernel<<<1, 1, 0, st>>>(status);
  stream_bits_kernel<<<(int)blocks, kBlock, 0, st>>>(levels, d, s, ac_len,
                                                     dc_len, bits, status);
  status_end_kernel<<<1, 1, 0, st>>>(status);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" size_t vtc_jpeg_bit_offsets_workspace_bytes(int64_t d) {
  if (d <= 0) return 0;
  return measured_bytes<OffsetsLayout>(d);
}

extern "C" int vtc_jpeg_bit_offsets(const int32_t* bits, int64_t d,
                                    int64_t* offsets, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  const char* who = "vtc_jpeg_bit_offsets";
  VTC_REQUIRE(bits && offsets, "%s: null pointer", who);
  VTC_REQUIRE(d > 0, "%s: bad size d = %lld", who, (long long)d);
  const int64_t tiles = ceil_div(d, kScanTile);
  VTC_REQUIRE(tiles < (int64_t)1 << 31, "%s: too many rows", who);
  const size_t need = vtc_jpeg_bit_offsets_workspace_bytes(d);
  if (!workspace || workspace_bytes < need) {
    set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
              need);
    return VTC_ERR_WORKSPACE;
  }
  Carver carve(workspace);
  const OffsetsLayout ws(carve, d);
  hipStream_t st = as_stream(stream);
  long long* out = reinterpret_cast<long long*>(offsets);
  scan_tile_sums_kernel<<<(int)tiles, kBlock, 0, st>>>(bits, d, ws.sums);
  scan_sums_kernel<<<1, kBlock, 0, st>>>(ws.sums, tiles);
  scan_write_kernel<<<(int)tiles, kBlock, 0, st>>>(bits, d, ws.sums, out);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" int vtc_jpeg_pack(const int32_t* levels, int64_t d, int32_t s,
                             const uint64_t* ac_code, const uint8_t* ac_len,
                             const uint64_t* dc_code, const uint8_t* dc_len,
                             const int64_t* offsets, uint8_t* out,
                             size_t out_bytes, int32_t* status, void* stream) {
  const char* who = "vtc_jpeg_pack";
  VTC_REQUIRE(levels && ac_code && ac_len && dc_code && dc_len && offsets &&
                  out && status, "%s: null pointer", who);
  int64_t blocks;
  const int rc = check_rows(who, d, s, &blocks);
  if (rc != VTC_OK) return rc;
  VTC_REQUIRE(out_bytes > 0 && out_bytes < (size_t)1 << 59,
              "%s: bad size out_bytes = %zu", who, out_bytes);
  hipStream_t st = as_stream(stream);
  VTC_HIP_CHECK(hipMemsetAsync(out, 0, out_bytes, st));
  status_begin_kernel<<<1, 1, 0, st>>>(status);
  pack_kernel<<<(int)blocks, kBlock, 0, st>>>(
      levels, d, s, reinterpret_cast<const unsigned long long*>(ac_code),
      ac_len, reinterpret_cast<const unsigned long long*>(dc_code), dc_len,
      offsets, out, (int64_t)out_bytes, status);
  status_end_kernel<<<1, 1, 0, st>>>(status);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}
