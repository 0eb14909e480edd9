// Decoder of the packed JPEG streams (include/vtc_decode.h): packed bits back
// to levels.  DESIGN.md 4.12 states the rules and why the shape is this one.
//
// Decoding is serial inside a row -- where a codeword starts is known only
// once the one before it has been read -- and parallel across rows.  So one
// LANE owns one row: 64 consecutive rows per wave, 256 per block.  (The
// packer's shape, one wave per row, would leave 63 lanes idle here.)  The
// streams of neighbouring rows are adjacent in memory, so the byte loads of a
// wave fall in one short range.  Lanes diverge on the number of tokens of
// their rows; that is inherent.
//
// Three steps per call, all on the caller's stream:
//   1. levels is zero-filled (rows are sparse: a lane stores its nonzero
//      levels only, a dense row write would be s * 4 bytes apart across lanes)
//   2. decode_tables_kernel, one block: the decode tables of prefix_table.h
//      for the at most 272 codewords, with a first-level lookup of 10 bits
//      per table, into the caller's workspace
//   3. unpack_kernel: the tables go to LDS, every lane walks its row
//
// A codeword of at most 10 bits is found by one LDS read; a longer one by
// predecessor search in the sorted array.
#include <limits.h>

#include "../../include/vtc_decode.h"
#include "bitstream.h"
#include "common.h"
#include "prefix_table.h"

namespace vtc {
namespace {

constexpr int kBlock = 256;
constexpr int kAcSymbols = 256, kDcSymbols = 16;
constexpr int kSymbols = kAcSymbols + kDcSymbols;   // AC bytes, DC categories
constexpr int kDcBase = kAcSymbols;
constexpr int kEob = 0x00, kZrl = 0xF0;
constexpr int kMaxCodeBits = 64;

// meta word of a codeword: length << 9 | symbol id (ids below 272, lengths
// 1..64); 0 is no codeword.
struct JpegCode {
  typedef u64 Key;
  typedef uint16_t Meta;
  static constexpr int kLutBits = 10;
  static __host__ __device__ constexpr unsigned make(int len, int id) {
    return (unsigned)len << 9 | (unsigned)id;
  }
  static __host__ __device__ constexpr bool valid(unsigned m) {
    return m != 0;
  }
  static __host__ __device__ constexpr int len(unsigned m) {
    return m >> 9;
  }
  static __host__ __device__ constexpr int symbol(unsigned m) {
    return m & 511;
  }
};
typedef PrefixTable<JpegCode> Table;
constexpr int kLutSize = Table::kLutSize;
static_assert(Table::round_trips(1, 0) && Table::round_trips(64, 0) &&
                  Table::round_trips(1, 271) && Table::round_trips(64, 271),
              "length << 9 | id");

struct DecodeLayout {
  u64* code;        // [272] left-aligned, sorted: AC from 0, DC from 256
  uint16_t* meta;   // [272] meta words of the sorted codewords
  uint16_t* lut;    // [2][1024] meta word of the codeword a prefix starts with
  int32_t* head;    // [4] AC count, DC count, 1 + bad symbol id or 0, unused
  explicit DecodeLayout(Carver& c) {
    code = c.take<u64>(kSymbols);
    meta = c.take<uint16_t>(kSymbols);
    lut = c.take<uint16_t>(2 * kLutSize);
    head = c.take<int32_t>(4);
  }
};

// ---- table preparation (prefix_table.h) -------------------------------------
__global__ __launch_bounds__(kBlock) void decode_tables_kernel(
    const u64* __restrict__ ac_code, const uint8_t* __restrict__ ac_len,
    const u64* __restrict__ dc_code, const uint8_t* __restrict__ dc_len,
    DecodeLayout ws, u64* __restrict__ status) {
  __shared__ u64 key[kSymbols];
  __shared__ uint16_t meta[kSymbols];
  __shared__ uint16_t lut[2 * kLutSize];
  __shared__ int count[2], bad;
  const int tid = threadIdx.x;
  if (tid < 2) count[tid] = 0;
  if (tid == 0) bad = INT_MAX;
  for (int i = tid; i < 2 * kLutSize; i += kBlock) lut[i] = 0;
  __syncthreads();
  for (int i = tid; i < kSymbols; i += kBlock) {
    int l = i < kDcBase ? ac_len[i] : dc_len[i - kDcBase];
    if (l > kMaxCodeBits) l = kMaxCodeBits;
    const u64 c = i < kDcBase ? ac_code[i] : dc_code[i - kDcBase];
    key[i] = Table::left_align(c, l);
    meta[i] = l ? JpegCode::make(l, i) : 0;
    if (l) atomicAdd(&count[i >= kDcBase], 1);
  }
  __syncthreads();
  Table::sort<kBlock>(key, meta, kAcSymbols);   // each table on its own
  Table::sort<kBlock>(key + kDcBase, meta + kDcBase, kDcSymbols);

  for (int i = tid; i < kSymbols; i += kBlock) {
    const int table = i >= kDcBase;
    const int r = i - (table ? kDcBase : 0);
    if (r + 1 >= count[table]) continue;
    const int offender = Table::prefix_violation(key, meta, i);
    if (offender != INT_MAX) atomicMin(&bad, offender);
  }
  __syncthreads();
  if (bad == INT_MAX) {   // prefix-free: the ranges are disjoint
    Table::fill_lookup(lut, key, meta, count[0], tid, kBlock);
    Table::fill_lookup(lut + kLutSize, key + kDcBase, meta + kDcBase, count[1],
                       tid, kBlock);
  }
  __syncthreads();

  for (int i = tid; i < kSymbols; i += kBlock) {
    ws.code[i] = key[i];
    ws.meta[i] = meta[i];
  }
  for (int i = tid; i < 2 * kLutSize; i += kBlock) ws.lut[i] = lut[i];
  if (tid == 0) {
    const int flag = bad == INT_MAX ? 0 : bad + 1;
    ws.head[0] = count[0];
    ws.head[1] = count[1];
    ws.head[2] = flag;
    ws.head[3] = 0;
    status[0] = 0;
    status[1] = ULLONG_MAX;   // minimum of 1 + row; unpack_end_kernel
    status[2] = (u64)flag;
  }
}

__global__ void unpack_end_kernel(u64* status) {
  if (status[1] == ULLONG_MAX) status[1] = 0;
}

// BitReader, the bit reader of one lane: bitstream.h

// Reads one codeword of a table: its symbol id, or -1 (no match, or the match
// passes the row's end or the buffer).
__device__ __forceinline__ int read_symbol(BitReader& r, const uint16_t* lut,
                                           const u64* code,
                                           const uint16_t* meta, int n) {
  const unsigned m = Table::read(r, lut, code, meta, n);
  return m ? JpegCode::symbol(m) : -1;
}

// Reads `size` value bits, 1..15; false when they pass the end.
__device__ __forceinline__ bool read_value(BitReader& r, int size,
                                           int32_t* value) {
  r.refill();
  if (size > r.avail()) return false;
  const int32_t bits = (int32_t)(r.win >> (kMaxCodeBits - size));
  r.consume(size);
  *value = (bits >> (size - 1)) ? bits : bits - ((1 << size) - 1);
  return true;
}

// One row.  false: malformed; what was decoded before the fault is stored.
__device__ __forceinline__ bool unpack_row(
    BitReader& r, int64_t begin, int64_t stop, int32_t* __restrict__ row,
    int s, const uint16_t* lut, const u64* code, const uint16_t* meta,
    int n_ac, int n_dc) {
  if (begin < 0 || begin > stop) return false;
  r.seek(begin);
  int k = 1;
  for (;;) {   // every turn consumes at least one bit of a finite row
    const int b = read_symbol(r, lut, code, meta, n_ac);
    if (b < 0) return false;
    if (b == kEob) break;
    if (b == kZrl) {
      if (k < s) k += 16;   // beyond s only "beyond s" matters: no overflow
      continue;
    }
    const int size = b & 15;
    if (size == 0) return false;
    if (k < s) k += b >> 4;
    if (k >= s) return false;
    int32_t v;
    if (!read_value(r, size, &v)) return false;
    row[k] = v;   // 1 <= k < s
    ++k;
  }
  const int c = read_symbol(r, lut + kLutSize, code + kDcBase, meta + kDcBase,
                            n_dc);
  if (c < 0) return false;
  if (c > kDcBase) {
    int32_t v;
    if (!read_value(r, c - kDcBase, &v)) return false;
    row[0] = v;
  }
  return r.pos == stop;
}

__global__ __launch_bounds__(kBlock) void unpack_kernel(
    const uint8_t* __restrict__ packed, int64_t packed_bytes,
    const long long* __restrict__ offsets, int64_t d, int s, DecodeLayout ws,
    int32_t* __restrict__ levels, u64* __restrict__ status) {
  __shared__ u64 code[kSymbols];
  __shared__ uint16_t meta[kSymbols];
  __shared__ uint16_t lut[2 * kLutSize];
  if (ws.head[2]) return;   // not prefix-free: nothing is decoded
  const int n_ac = ws.head[0], n_dc = ws.head[1];
  for (int i = threadIdx.x; i < kSymbols; i += kBlock) {
    code[i] = ws.code[i];
    meta[i] = ws.meta[i];
  }
  for (int i = threadIdx.x; i < 2 * kLutSize; i += kBlock) lut[i] = ws.lut[i];
  __syncthreads();

  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  bool malformed = false;
  if (p < d) {
    const int64_t begin = offsets[p], stop = offsets[p + 1];
    const int64_t limit = packed_bytes * 8;
    BitReader r;
    r.bytes = packed;
    r.nbytes = packed_bytes;
    r.end = stop < limit ? stop : limit;
    malformed = !unpack_row(r, begin, stop, levels + p * s, s, lut, code, meta,
                            n_ac, n_dc);
  }
  // rows of a wave are consecutive: its first malformed row is its lowest lane
  const u64 mask = __ballot(malformed);
  if (mask && (threadIdx.x & 63) == 0) {
    atomicAdd(&status[0], (u64)__popcll(mask));
    atomicMin(&status[1], (u64)(p + __ffsll((long long)mask)));
  }
}

int check_rows(const char* who, int64_t d, int32_t s, int64_t* blocks) {
  VTC_REQUIRE(d > 0, "%s: bad size d = %lld", who, (long long)d);
  VTC_REQUIRE(s >= 1 && s <= VTC_JPEG_MAX_S,
              "%s: bad size s = %d (1 .. %d)", who, s, VTC_JPEG_MAX_S);
  *blocks = ceil_div(d, kBlock);
  VTC_REQUIRE(*blocks < (int64_t)1 << 31, "%s: too many rows", who);
  return VTC_OK;
}

}  // namespace
}  // namespace vtc

using namespace vtc;

extern "C" int vtc_decode_abi_version(void) { return VTC_DECODE_ABI_VERSION; }

extern "C" size_t vtc_jpeg_unpack_workspace_bytes(void) {
  return measured_bytes<DecodeLayout>();
}

extern "C" int vtc_jpeg_unpack(const uint8_t* packed, size_t packed_bytes,
                               const int64_t* offsets, int64_t d, int32_t s,
                               const uint64_t* ac_code, const uint8_t* ac_len,
                               const uint64_t* dc_code, const uint8_t* dc_len,
                               int32_t* levels, int64_t* status,
                               void* workspace, size_t workspace_bytes,
                               void* stream) {
  const char* who = "vtc_jpeg_unpack";
  VTC_REQUIRE(packed && offsets && ac_code && ac_len && dc_code && dc_len &&
                  levels && status, "%s: null pointer", who);
  int64_t blocks;
  const int rc = check_rows(who, d, s, &blocks);
  if (rc != VTC_OK) return rc;
  VTC_REQUIRE(packed_bytes > 0 && packed_bytes < (size_t)1 << 59,
              "%s: bad size packed_bytes = %zu", who, packed_bytes);
  const size_t need = vtc_jpeg_unpack_workspace_bytes();
  if (!workspace || workspace_bytes < need) {
    set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
              need);
    return VTC_ERR_WORKSPACE;
  }
  Carver carve(workspace);
  const DecodeLayout ws(carve);
  hipStream_t st = as_stream(stream);
  u64* flags = reinterpret_cast<u64*>(status);
  VTC_HIP_CHECK(hipMemsetAsync(levels, 0,
                               (size_t)d * (size_t)s * sizeof(int32_t), st));
  decode_tables_kernel<<<1, kBlock, 0, st>>>(
      reinterpret_cast<const u64*>(ac_code), ac_len,
      reinterpret_cast<const u64*>(dc_code), dc_len, ws, flags);
  unpack_kernel<<<(int)blocks, kBlock, 0, st>>>(
      packed, (int64_t)packed_bytes, reinterpret_cast<const long long*>(offsets),
      d, s, ws, levels, flags);
  unpack_end_kernel<<<1, 1, 0, st>>>(flags);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}
