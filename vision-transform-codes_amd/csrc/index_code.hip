// Prefix codes for quantiser indices on the device (include/vtc_index_code.h):
// the bits every row and every column costs under per-column tables, and the
// packed streams.  DESIGN.md 4.17.
//
// Every row has exactly m symbols, so a lane's place in the stream is a scan
// of lengths and nothing else.  One wave step covers
//   m < 64:   G = 64 / m consecutive rows; lane l holds row l / m of the step
//             and column l % m, the lanes from G * m on idle (none when m
//             divides 64: m = 1 codes 64 rows per step).  The step's G * m
//             indices are consecutive in memory, one coalesced load.
//   m >= 64:  one row, in chunks of 64 columns with a running carry, as the
//             JPEG packer walks a patch.
// The wave scans the lengths with __shfl_up; a lane's position inside its row
// is its exclusive scan value minus that of the row's head lane (lane
// l - l % m, lane 0 when m >= 64), fetched with one __shfl.  The lane that
// holds column m - 1 knows the row's total.  Both kernels share step_entry()
// and scan_lengths(): what one measures the other writes.
//
// The tables (up to m * kmax * 9 bytes) do not fit in LDS in general: lengths
// and codewords are gathered from global memory, where they stay cache
// resident (each column's table is read by every row).  LDS holds the block's
// per-column partial sums only, 4 * m bytes.
#include "../../include/vtc_index_code.h"
#include "bitstream.h"
#include "common.h"

namespace vtc {
namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / 64;
constexpr int kStepsPerWave = 16;
constexpr int kMaxColumns = VTC_INDEX_CODE_MAX_COLUMNS;
constexpr int kMaxSymbols = VTC_INDEX_CODE_MAX_SYMBOLS;
constexpr unsigned long long kNoPosition = ~0ull;

// Rows of one wave step.
__host__ __device__ inline int rows_per_step(int m) {
  return m < 64 ? 64 / m : 1;
}

// Where a lane sits in a wave step; fixed for the whole kernel.
struct LaneMap {
  int group;    // rows of one step
  int chunks;   // 64-column chunks of one row
  int row;      // the lane's row within the step
  int col;      // its column in chunk 0
  int head;     // the lane that holds column 0 of the same row
  bool live;    // false for the idle lanes from G * m on
};

__device__ __forceinline__ LaneMap lane_map(int m, int lane) {
  LaneMap w;
  w.group = rows_per_step(m);
  if (m < 64) {
    w.chunks = 1;
    w.row = lane / m;
    w.col = lane - w.row * m;
    w.head = lane - w.col;
    w.live = lane < w.group * m;
  } else {
    w.chunks = (m + 63) >> 6;
    w.row = 0;
    w.col = lane;
    w.head = 0;
    w.live = true;
  }
  return w;
}

// Inclusive scan of `v` over the wave.
__device__ __forceinline__ int scan_lengths(int v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(v, off, 64);
    if (lane >= off) v += o;
  }
  return v;
}

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Uncodable entries seen by one lane.
struct Uncodable {
  int count = 0;
  unsigned long long first = kNoPosition;   // smallest flat position
};

// The entry at flat position `flat` of column `col`: its length in bits, 0 for
// an inactive lane and for an uncodable entry (which is recorded); *at is the
// entry's place in the (m, kmax) tables.
__device__ __forceinline__ int step_entry(const int32_t* __restrict__ indices,
                                          const uint8_t* __restrict__ len,
                                          int kmax, bool active, int64_t flat,
                                          int col, Uncodable& bad, int* at) {
  *at = 0;
  if (!active) return 0;
  const int32_t index = indices[flat];
  int bits = VTC_INDEX_CODE_ABSENT;
  if ((unsigned)index < (unsigned)kmax) {
    *at = col * kmax + index;   // < 4096 * 4096
    bits = len[*at];
  }
  if (bits > 64) {
    ++bad.count;
    if ((unsigned long long)flat < bad.first)
      bad.first = (unsigned long long)flat;
    return 0;
  }
  return bits;
}

__device__ __forceinline__ void report(const Uncodable& bad, long long dropped,
                                       int lane, unsigned long long* status) {
  const long long count = wave_sum_ll(bad.count);
  const unsigned long long first = wave_min(bad.first);
  dropped = wave_sum_ll(dropped);
  if (lane != 0) return;
  if (count) {
    atomicAdd(&status[0], (unsigned long long)count);
    atomicMin(&status[1], first);
  }
  if (dropped) atomicAdd(&status[2], (unsigned long long)dropped);
}

__global__ void status_begin_kernel(unsigned long long* status) {
  status[0] = 0;
  status[1] = kNoPosition;
  status[2] = 0;
}
__global__ void status_end_kernel(unsigned long long* status) {
  status[1] = status[1] == kNoPosition ? 0 : status[1] + 1;
}

// ---- bits -------------------------------------------------------------------
// The block's column sums collect in 32-bit LDS words (a block covers at most
// 4096 rows of at most 64 bits) and leave through one global atomic per column
// and block.  With m <= 64 a lane keeps its column for the whole kernel and
// sums it in a register first.
__global__ __launch_bounds__(kBlock) void bits_kernel(
    const int32_t* __restrict__ indices, int64_t b, int m,
    const uint8_t* __restrict__ len, int kmax, int32_t* __restrict__ row_bits,
    unsigned long long* __restrict__ column_bits,
    unsigned long long* __restrict__ status) {
  __shared__ unsigned column_sum[kMaxColumns];
  for (int i = threadIdx.x; i < m; i += kBlock) column_sum[i] = 0;
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const LaneMap w = lane_map(m, lane);
  const int64_t row0 = ((int64_t)blockIdx.x * kWavesPerBlock + wave) *
                       kStepsPerWave * w.group;
  Uncodable bad;
  unsigned own = 0;
  for (int step = 0; step < kStepsPerWave; ++step) {
    const int64_t first_row = row0 + (int64_t)step * w.group;
    if (first_row >= b) break;   // the whole wave
    const int64_t row = first_row + w.row;
    int run = 0;
    for (int chunk = 0; chunk < w.chunks; ++chunk) {
      const int col = w.col + chunk * 64;
      const bool active = w.live && row < b && col < m;
      int at;
      const int mine =
          step_entry(indices, len, kmax, active, row * m + col, col, bad, &at);
      if (w.chunks == 1)
        own += mine;
      else if (mine)
        atomicAdd(&column_sum[col], (unsigned)mine);
      const int incl = scan_lengths(mine, lane);
      const int head = __shfl(incl - mine, w.head, 64);
      if (active && col == m - 1) row_bits[row] = run + incl - head;
      run += __shfl(incl, 63, 64);
    }
  }
  if (w.chunks == 1 && w.live && own) atomicAdd(&column_sum[w.col], own);
  __syncthreads();
  for (int i = threadIdx.x; i < m; i += kBlock) {
    const unsigned n = column_sum[i];
    if (n) atomicAdd(&column_bits[i], (unsigned long long)n);
  }
  report(bad, 0, lane, status);
}

// ---- packing ------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void pack_kernel(
    const int32_t* __restrict__ indices, int64_t b, int m,
    const unsigned long long* __restrict__ code,
    const uint8_t* __restrict__ len, int kmax,
    const int64_t* __restrict__ offsets, uint8_t* packed, int64_t packed_bytes,
    unsigned long long* __restrict__ status) {
  const uintptr_t address = reinterpret_cast<uintptr_t>(packed);
  unsigned* words = reinterpret_cast<unsigned*>(address & ~(uintptr_t)3);
  const int64_t lo = (int64_t)(address & 3) * 8;
  const int64_t all_bits = packed_bytes * 8;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const LaneMap w = lane_map(m, lane);
  const int64_t row0 = ((int64_t)blockIdx.x * kWavesPerBlock + wave) *
                       kStepsPerWave * w.group;
  Uncodable bad;
  long long dropped = 0;
  for (int step = 0; step < kStepsPerWave; ++step) {
    const int64_t first_row = row0 + (int64_t)step * w.group;
    if (first_row >= b) break;   // the whole wave
    const int64_t row = first_row + w.row;
    // the row's window [base, limit) in bits from `words`; empty (every bit
    // dropped) for a negative or decreasing offset or a row past the output
    int64_t base = 0, limit = lo;
    if (w.live && row < b) {
      const int64_t from = offsets[row], to = offsets[row + 1];
      if (from >= 0 && from <= to && from < all_bits) {
        base = lo + from;
        limit = lo + (to < all_bits ? to : all_bits);
      }
    }
    int run = 0;
    for (int chunk = 0; chunk < w.chunks; ++chunk) {
      const int col = w.col + chunk * 64;
      const bool active = w.live && row < b && col < m;
      int at;
      const int mine =
          step_entry(indices, len, kmax, active, row * m + col, col, bad, &at);
      const int incl = scan_lengths(mine, lane);
      const int head = __shfl(incl - mine, w.head, 64);
      if (mine)
        dropped += put_bits(words, lo, limit, base + run + (incl - mine) - head,
                            code[at], mine);
      run += __shfl(incl, 63, 64);
    }
  }
  report(bad, dropped, lane, status);
}

int check_shape(const char* who, int64_t b, int32_t m, int32_t kmax,
                int64_t* blocks) {
  VTC_REQUIRE(b >= 1, "%s: bad size b = %lld", who, (long long)b);
  VTC_REQUIRE(m >= 1, "%s: bad size m = %d", who, m);
  VTC_REQUIRE(kmax >= 1, "%s: bad size kmax = %d", who, kmax);
  if (m > kMaxColumns) {
    set_error("%s: m = %d, at most %d", who, m, kMaxColumns);
    return VTC_ERR_UNSUPPORTED;
  }
  if (kmax > kMaxSymbols) {
    set_error("%s: kmax = %d, at most %d", who, kmax, kMaxSymbols);
    return VTC_ERR_UNSUPPORTED;
  }
  *blocks = ceil_div(b, (int64_t)kWavesPerBlock * kStepsPerWave *
                            rows_per_step(m));
  if (*blocks >= (int64_t)1 << 31) {
    set_error("%s: b = %lld, too many rows", who, (long long)b);
    return VTC_ERR_UNSUPPORTED;
  }
  return VTC_OK;
}

}  // namespace
}  // namespace vtc

using namespace vtc;

extern "C" int vtc_index_code_abi_version(void) {
  return VTC_INDEX_CODE_ABI_VERSION;
}

extern "C" int vtc_index_code_bits(const int32_t* indices, int64_t b,
                                   int32_t m, const uint8_t* len, int32_t kmax,
                                   int32_t* row_bits, int64_t* column_bits,
                                   int64_t* status, void* stream) {
  const char* who = "vtc_index_code_bits";
  VTC_REQUIRE(indices && len && row_bits && column_bits && status,
              "%s: null pointer", who);
  int64_t blocks;
  const int rc = check_shape(who, b, m, kmax, &blocks);
  if (rc != VTC_OK) return rc;
  hipStream_t st = as_stream(stream);
  unsigned long long* report_to = reinterpret_cast<unsigned long long*>(status);
  VTC_HIP_CHECK(hipMemsetAsync(column_bits, 0, (size_t)m * sizeof(int64_t), st));
  status_begin_kernel<<<1, 1, 0, st>>>(report_to);
  bits_kernel<<<(int)blocks, kBlock, 0, st>>>(
      indices, b, m, len, kmax, row_bits,
      reinterpret_cast<unsigned long long*>(column_bits), report_to);
  status_end_kernel<<<1, 1, 0, st>>>(report_to);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" int vtc_index_code_pack(const int32_t* indices, int64_t b,
                                   int32_t m, const uint64_t* code,
                                   const uint8_t* len, int32_t kmax,
                                   const int64_t* offsets, uint8_t* packed,
                                   int64_t packed_bytes, int64_t* status,
                                   void* stream) {
  const char* who = "vtc_index_code_pack";
  VTC_REQUIRE(indices && code && len && offsets && packed && status,
              "%s: null pointer", who);
  int64_t blocks;
  const int rc = check_shape(who, b, m, kmax, &blocks);
  if (rc != VTC_OK) return rc;
  VTC_REQUIRE(packed_bytes >= 0 && packed_bytes < (int64_t)1 << 59,
              "%s: bad size packed_bytes = %lld", who, (long long)packed_bytes);
  hipStream_t st = as_stream(stream);
  unsigned long long* report_to = reinterpret_cast<unsigned long long*>(status);
  if (packed_bytes)
    VTC_HIP_CHECK(hipMemsetAsync(packed, 0, (size_t)packed_bytes, st));
  status_begin_kernel<<<1, 1, 0, st>>>(report_to);
  pack_kernel<<<(int)blocks, kBlock, 0, st>>>(
      indices, b, m, reinterpret_cast<const unsigned long long*>(code), len,
      kmax, offsets, packed, packed_bytes, report_to);
  status_end_kernel<<<1, 1, 0, st>>>(report_to);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}
