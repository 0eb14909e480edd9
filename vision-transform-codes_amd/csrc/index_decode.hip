// Decoder of the packed index streams (include/vtc_index_decode.h): packed
// bits back to the (b, m) indices that vtc_index_code_pack wrote.  DESIGN.md
// 4.18 states the rules and why the shape is this one.
//
// Decoding is serial inside a row and parallel across rows, so one LANE owns
// one row: 64 consecutive rows per wave, 256 per block, the shape of
// jpeg_decode.hip.  Unlike there every row has exactly m codewords: all lanes
// of a wave are on the same column at the same time and read the same column's
// table; there is no divergence on the number of tokens.
//
// Four launches per call, all on the caller's stream:
//   1. index_unpack_begin_kernel: status and the workspace's prefix flag
//   2. index_tables_kernel, one block per column: the column's decode table
//      of prefix_table.h, into the workspace (sorted over the next power of
//      two by 1024 threads: the launch's time is the latency of this one sort)
//   3. index_unpack_kernel: every lane walks its row; a wave collects 64 rows
//      x kTile columns in LDS and stores them with consecutive lanes on
//      consecutive addresses
//   4. index_unpack_end_kernel: the minimum of status[1] and the flag into
//      status[2]
//
// A codeword of at most kLutBits bits is one read of the column's lookup; a
// longer one is found by predecessor search in the sorted array.  The tables
// (up to 4096 * 4096 * 12 bytes plus lookups) stay in global memory, where
// they are cache resident: every row reads them.
#include <limits.h>

#include "../../include/vtc_index_decode.h"
#include "bitstream.h"
#include "common.h"
#include "prefix_table.h"

namespace vtc {
namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / 64;
constexpr int kTableBlock = 1024;   // threads that sort one column's table
constexpr int kMaxColumns = VTC_INDEX_CODE_MAX_COLUMNS;
constexpr int kMaxSymbols = VTC_INDEX_CODE_MAX_SYMBOLS;
constexpr int kMaxCodeBits = 64;
constexpr int kTile = 32;               // columns a wave collects before it stores
constexpr int kTileStride = kTile + 1;  // odd: lane-per-row writes hit 64 banks

// meta word of a codeword: an explicit valid bit (the empty codeword of symbol
// 0 would otherwise be 0, "no codeword"), length 0 .. 64, symbol 0 .. 4095.
struct IndexCode {
  typedef u64 Key;
  typedef uint32_t Meta;
  static constexpr int kLutBits = VTC_INDEX_DECODE_LOOKUP_BITS;
  static constexpr unsigned kValid = 1u << 31;
  static __host__ __device__ constexpr unsigned make(int len, int symbol) {
    return kValid | (unsigned)len << 12 | (unsigned)symbol;
  }
  static __host__ __device__ constexpr bool valid(unsigned m) {
    return m & kValid;
  }
  static __host__ __device__ constexpr int len(unsigned m) {
    return m >> 12 & 127u;
  }
  static __host__ __device__ constexpr int symbol(unsigned m) {
    return m & 4095u;
  }
};
typedef PrefixTable<IndexCode> Table;
constexpr int kLutBits = Table::kLutBits;
constexpr int kLutSize = Table::kLutSize;
static_assert(Table::round_trips(0, 0) && Table::round_trips(64, 4095) &&
                  Table::round_trips(0, 4095) && Table::round_trips(64, 0),
              "valid | length << 12 | symbol");

struct IndexDecodeLayout {
  u64* code;        // [m * kmax] left-aligned, sorted, column j from j * kmax
  uint32_t* meta;   // [m * kmax] meta words of the sorted codewords
  uint32_t* lut;    // [m << kLutBits] meta word of the codeword a prefix starts with
  int32_t* count;   // [m] codewords of each column
  int32_t* bad;     // [1] smallest bad table position, INT_MAX when none
  IndexDecodeLayout(Carver& c, int m, int kmax) {
    code = c.take<u64>((size_t)m * kmax);
    meta = c.take<uint32_t>((size_t)m * kmax);
    lut = c.take<uint32_t>((size_t)m << kLutBits);
    count = c.take<int32_t>(m);
    bad = c.take<int32_t>(1);
  }
};

__global__ void index_unpack_begin_kernel(IndexDecodeLayout ws, u64* status) {
  *ws.bad = INT_MAX;
  status[0] = 0;
  status[1] = ULLONG_MAX;   // minimum of 1 + row; index_unpack_end_kernel
  status[2] = 0;
}

__global__ void index_unpack_end_kernel(IndexDecodeLayout ws, u64* status) {
  if (status[1] == ULLONG_MAX) status[1] = 0;
  const int bad = *ws.bad;
  status[2] = bad == INT_MAX ? 0 : (u64)bad + 1;
}

// ---- table preparation (prefix_table.h) -------------------------------------
__global__ __launch_bounds__(kTableBlock) void index_tables_kernel(
    const u64* __restrict__ code, const uint8_t* __restrict__ len, int kmax,
    IndexDecodeLayout ws) {
  __shared__ u64 key[kMaxSymbols];
  __shared__ uint32_t meta[kMaxSymbols];
  __shared__ uint32_t lut[kLutSize];
  __shared__ int count, bad;
  const int tid = threadIdx.x;
  const int column = blockIdx.x;
  const int base = column * kmax;   // < 4096 * 4096
  int n2 = 1;
  while (n2 < kmax) n2 <<= 1;       // <= kMaxSymbols
  if (tid == 0) {
    count = 0;
    bad = INT_MAX;
  }
  for (int i = tid; i < kLutSize; i += kTableBlock) lut[i] = 0;
  __syncthreads();
  int mine = 0;
  for (int i = tid; i < n2; i += kTableBlock) {
    const int l = i < kmax ? len[base + i] : VTC_INDEX_CODE_ABSENT;
    if (l <= kMaxCodeBits) {
      key[i] = Table::left_align(code[base + i], l);
      meta[i] = IndexCode::make(l, i);
      ++mine;
    } else {
      key[i] = ~0ull;
      meta[i] = 0;
    }
  }
  if (mine) atomicAdd(&count, mine);
  __syncthreads();

  Table::sort<kTableBlock>(key, meta, n2);
  const int n = count;   // the codewords are entries 0 .. n - 1

  for (int i = tid; i + 1 < n; i += kTableBlock) {
    const int offender = Table::prefix_violation(key, meta, i);
    if (offender != INT_MAX) atomicMin(&bad, base + offender);
  }
  __syncthreads();
  if (bad == INT_MAX)   // prefix-free: the ranges are disjoint
    Table::fill_lookup(lut, key, meta, n, tid, kTableBlock);
  __syncthreads();

  for (int i = tid; i < kmax; i += kTableBlock) {
    ws.code[base + i] = key[i];
    ws.meta[base + i] = meta[i];
  }
  for (int i = tid; i < kLutSize; i += kTableBlock)
    ws.lut[((size_t)column << kLutBits) + i] = lut[i];
  if (tid == 0) {
    ws.count[column] = n;
    if (bad != INT_MAX) atomicMin(ws.bad, bad);
  }
}

// ---- decoding -----------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void index_unpack_kernel(
    const uint8_t* __restrict__ packed, int64_t packed_bytes,
    const long long* __restrict__ offsets, int64_t b, int m, int kmax,
    IndexDecodeLayout ws, int32_t* __restrict__ indices,
    int32_t* __restrict__ row_bits, u64* __restrict__ status) {
  __shared__ int32_t tiles[kWavesPerBlock][64 * kTileStride];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int32_t* tile = tiles[wave];
  const int64_t wave_row = ((int64_t)blockIdx.x * kWavesPerBlock + wave) * 64;
  const int64_t p = wave_row + lane;
  const bool decoding = *ws.bad == INT_MAX;   // else nothing is decoded

  BitReader r;
  r.bytes = packed;
  r.nbytes = packed_bytes;
  r.end = 0;
  r.seek(0);
  int64_t begin = 0;
  bool ok = false, malformed = false;
  if (decoding && p < b) {
    begin = offsets[p];
    const int64_t stop = offsets[p + 1], limit = packed_bytes * 8;
    if (begin < 0 || begin > stop) {
      malformed = true;
      begin = 0;
    } else {
      ok = true;
      r.end = stop < limit ? stop : limit;
      r.seek(begin);
    }
  }

  for (int j0 = 0; j0 < m; j0 += kTile) {   // the same turns in every wave
    const int width = m - j0 < kTile ? m - j0 : kTile;
    for (int c = 0; c < width; ++c) {
      const int j = j0 + c;
      int32_t symbol = -1;
      if (ok) {
        const unsigned e = Table::read(
            r, ws.lut + ((size_t)j << kLutBits), ws.code + (size_t)j * kmax,
            ws.meta + (size_t)j * kmax, ws.count[j]);
        if (!IndexCode::valid(e)) {
          ok = false;   // no codeword, or one that passes the end
          malformed = true;
        } else {
          symbol = IndexCode::symbol(e);
        }
      }
      tile[lane * kTileStride + c] = symbol;
    }
    __syncthreads();
    // 64 rows x width columns, consecutive lanes on consecutive columns; with
    // m <= kTile the wave's whole 64 * m block is contiguous
    for (int e = lane; e < 64 * width; e += 64) {
      const int row = width == kTile ? e >> 5 : e / width;
      const int c = e - row * width;
      if (wave_row + row < b)   // j0 + c < m by construction
        indices[(wave_row + row) * m + j0 + c] = tile[row * kTileStride + c];
    }
    __syncthreads();
  }
  if (p < b) row_bits[p] = decoding ? (int32_t)(r.pos - begin) : 0;

  // rows of a wave are consecutive: its first malformed row is its lowest lane
  const u64 mask = __ballot(malformed);
  if (mask && lane == 0) {
    atomicAdd(&status[0], (u64)__popcll(mask));
    atomicMin(&status[1], (u64)(p + __ffsll((long long)mask)));
  }
}

// VTC_OK when the call takes the shape; sets the error text otherwise.
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
  *blocks = ceil_div(b, kBlock);
  if (*blocks >= (int64_t)1 << 31) {
    set_error("%s: b = %lld, too many rows", who, (long long)b);
    return VTC_ERR_UNSUPPORTED;
  }
  return VTC_OK;
}

}  // namespace
}  // namespace vtc

using namespace vtc;

extern "C" int vtc_index_decode_abi_version(void) {
  return VTC_INDEX_DECODE_ABI_VERSION;
}

extern "C" size_t vtc_index_code_unpack_workspace_bytes(int32_t m,
                                                        int32_t kmax) {
  if (m < 1 || m > kMaxColumns || kmax < 1 || kmax > kMaxSymbols) return 0;
  return measured_bytes<IndexDecodeLayout>(m, kmax);
}

extern "C" int vtc_index_code_unpack(const uint8_t* packed,
                                     int64_t packed_bytes,
                                     const int64_t* offsets, int64_t b,
                                     int32_t m, const uint64_t* code,
                                     const uint8_t* len, int32_t kmax,
                                     int32_t* indices, int32_t* row_bits,
                                     int64_t* status, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  const char* who = "vtc_index_code_unpack";
  VTC_REQUIRE(packed && offsets && code && len && indices && row_bits && status,
              "%s: null pointer", who);
  int64_t blocks;
  const int rc = check_shape(who, b, m, kmax, &blocks);
  if (rc != VTC_OK) return rc;
  VTC_REQUIRE(packed_bytes >= 0 && packed_bytes < (int64_t)1 << 59,
              "%s: bad size packed_bytes = %lld", who, (long long)packed_bytes);
  const size_t need = vtc_index_code_unpack_workspace_bytes(m, kmax);
  if (!workspace || workspace_bytes < need) {
    set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
              need);
    return VTC_ERR_WORKSPACE;
  }
  Carver carve(workspace);
  const IndexDecodeLayout ws(carve, m, kmax);
  hipStream_t st = as_stream(stream);
  u64* flags = reinterpret_cast<u64*>(status);
  index_unpack_begin_kernel<<<1, 1, 0, st>>>(ws, flags);
  index_tables_kernel<<<m, kTableBlock, 0, st>>>(
      reinterpret_cast<const u64*>(code), len, kmax, ws);
  index_unpack_kernel<<<(int)blocks, kBlock, 0, st>>>(
      packed, packed_bytes, reinterpret_cast<const long long*>(offsets), b, m,
      kmax, ws, indices, row_bits, flags);
  index_unpack_end_kernel<<<1, 1, 0, st>>>(ws, flags);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}
