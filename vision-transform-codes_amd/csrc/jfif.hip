// The device half of a baseline JFIF writer (include/ext/vtc_jfif.h): plane to
// quantiser levels and back, the T.81 run-length symbols with DC prediction
// and their counts, block lengths, one bit-contiguous entropy-coded segment,
// and the 0xFF byte-stuffing pass.  DESIGN.md 4.23 states the rules and the
// bounds of every index.
//
// DCT kernels: one wave per 8 x 8 block, lane 8 y + x holds sample (y, x);
// both passes of the separable transform exchange values with __shfl and read
// the 8 x 8 basis from LDS.  Every product and every sum is a float64
// operation of its own (-ffp-contract=off), in ascending k.
//
// Row kernels: one wave per block (row of 64 levels), lane i holds level i.
// Lane 0 owns the DC token (DIFF against levels[pred][0]) and the end of
// block, a lane i >= 1 with a nonzero level owns one AC token whose run comes
// from __ballot and clz as in jpeg_codec.hip.  lane_token() states the rule
// once: what the count kernel counts, the length kernel measures and the pack
// kernel writes.  A wave walks kRowsPerWave consecutive rows, so the 32-bit
// LDS bins of a workgroup (at most 64 increments per row) cannot wrap.
#include <limits.h>

#include "../../include/ext/vtc_jfif.h"
#include "bitstream.h"
#include "block_scan.h"
#include "common.h"

namespace vtc {
namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / 64;
constexpr int kRowsPerWave = 8;
constexpr int kRowsPerBlock = kWavesPerBlock * kRowsPerWave;
constexpr int kPairSymbols = 256 + 16;      // AC bytes, then DC categories
constexpr int kSymbols = 2 * kPairSymbols;  // two table pairs
constexpr int kDcBase = 256;
constexpr int kEob = 0x00, kZrl = 0xF0;
constexpr int kAcCap = 10, kDcCap = 11;
constexpr int kMaxCodeBits = 16;
constexpr int kStuffItems = VTC_JFIF_STUFF_TILE / kBlock;
static_assert(kStuffItems * kBlock == VTC_JFIF_STUFF_TILE, "tile = block * 8");

// zigzag index of the coefficient at (v, u), indexed by 8 v + u (T.81 A.6)
__constant__ uint8_t kZigzagOf[64] = {
    0,  1,  5,  6,  14, 15, 27, 28,   //
    2,  4,  7,  13, 16, 26, 29, 42,   //
    3,  8,  12, 17, 25, 30, 41, 43,   //
    9,  11, 18, 24, 31, 40, 44, 53,   //
    10, 19, 23, 32, 39, 45, 52, 54,   //
    20, 22, 33, 38, 46, 51, 55, 60,   //
    21, 34, 37, 47, 50, 56, 59, 61,   //
    35, 36, 48, 49, 57, 58, 62, 63};

// ---- DCT ------------------------------------------------------------------
// sum over k, ascending, of a[from + k * step] * basis[row * 8 + k] (or
// basis[k * 8 + row] when `transposed`), the operand fetched from the lane
// that holds it.  Must be reached by the whole wave.
template <bool kTransposed>
__device__ __forceinline__ double lane_dot8(double mine, int from, int step,
                                            const double* basis, int row) {
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double a = __shfl(mine, from + k * step, 64);
    const double c = kTransposed ? basis[k * 8 + row] : basis[row * 8 + k];
    const double p = a * c;
    acc = k == 0 ? p : acc + p;
  }
  return acc;
}

__global__ __launch_bounds__(kBlock) void forward_dct_kernel(
    const float* __restrict__ plane, int h, int w, int bh, int bw,
    const double* __restrict__ basis, const uint16_t* __restrict__ q,
    const int32_t* __restrict__ row_of_block, int32_t* __restrict__ levels,
    int64_t rows) {
  __shared__ double cs[64];
  if (threadIdx.x < 64) cs[threadIdx.x] = basis[threadIdx.x];
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int y = lane >> 3, x = lane & 7;
  const int zz = kZigzagOf[lane];
  const double qz = (double)q[zz];
  const int64_t blocks = (int64_t)bh * bw;
  const int64_t stride = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t b = (int64_t)blockIdx.x * kWavesPerBlock + wave; b < blocks;
       b += stride) {
    const int by = (int)(b / bw), bx = (int)(b % bw);
    // replicate the last row and column: 0 <= py < h, 0 <= px < w
    const int py = min(by * 8 + y, h - 1), px = min(bx * 8 + x, w - 1);
    const double raw = (double)plane[(int64_t)py * w + px];
    const double s =
        rint(raw < 0.0 ? 0.0 : (raw > 255.0 ? 255.0 : raw)) - 128.0;
    // rows: lane (y, u = x) sums s[y][k] * basis[u][k]
    const double t = lane_dot8<false>(s, y * 8, 1, cs, x);
    // columns: lane (v = y, u = x) sums t[k][u] * basis[v][k]
    const double c = lane_dot8<false>(t, x, 8, cs, y);
    const double r = rint(c / qz);
    int32_t level = INT_MIN;
    if (r >= 2147483647.0)
      level = INT_MAX;
    else if (r > -2147483648.0)   // false for NaN
      level = (int32_t)r;
    const int32_t row = row_of_block[b];
    if (row >= 0 && (int64_t)row < rows) levels[(int64_t)row * 64 + zz] = level;
  }
}

__global__ __launch_bounds__(kBlock) void inverse_dct_kernel(
    const int32_t* __restrict__ levels, int64_t rows,
    const int32_t* __restrict__ row_of_block, int bh, int bw,
    const double* __restrict__ basis, const uint16_t* __restrict__ q,
    float* __restrict__ plane, int h, int w) {
  __shared__ double cs[64];
  if (threadIdx.x < 64) cs[threadIdx.x] = basis[threadIdx.x];
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int y = lane >> 3, x = lane & 7;
  const int zz = kZigzagOf[lane];
  const double qz = (double)q[zz];
  const int64_t blocks = (int64_t)bh * bw;
  const int64_t stride = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t b = (int64_t)blockIdx.x * kWavesPerBlock + wave; b < blocks;
       b += stride) {
    const int by = (int)(b / bw), bx = (int)(b % bw);
    const int32_t row = row_of_block[b];
    double c = 0.0;
    if (row >= 0 && (int64_t)row < rows)
      c = (double)levels[(int64_t)row * 64 + zz] * qz;
    // columns: lane (y, u = x) sums c[k][u] * basis[k][y]
    const double t = lane_dot8<true>(c, x, 8, cs, y);
    // rows: lane (y, x) sums t[y][k] * basis[k][x]
    const double p = lane_dot8<true>(t, y * 8, 1, cs, x);
    const double r = rint(p + 128.0);
    const int py = by * 8 + y, px = bx * 8 + x;
    if (py < h && px < w)
      plane[(int64_t)py * w + px] =
          (float)(r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r));
  }
}

// ---- the token rule ---------------------------------------------------------
// What lane `lane` contributes to the stream of one row.
struct LaneToken {
  bool dc;          // lane 0: owns the DC token
  bool ac;          // a nonzero level at index >= 1: owns an AC token
  bool over;        // size above the cap (10 for AC, 11 for DC)
  bool eob;         // wave-uniform: the last nonzero index is below 63
  int sel;          // wave-uniform: 0 or 1, the table pair of the row
  int z;            // zeros since the previous nonzero AC level
  int size;         // bit length of |number|, clamped to the cap
  uint32_t value;   // the `size` value bits
};

// Must be reached by the whole wave (it ballots).  0 <= row < d.
__device__ __forceinline__ LaneToken lane_token(const int32_t* levels,
                                                int64_t d, int64_t row,
                                                const int32_t* pred,
                                                const uint8_t* table_sel,
                                                int lane) {
  LaneToken t;
  const int32_t v = levels[row * 64 + lane];
  long long n = v;
  int cap = kAcCap;
  t.dc = lane == 0;
  if (t.dc) {
    cap = kDcCap;
    const int32_t p = pred[row];
    if (p >= 0 && (int64_t)p < d) n -= levels[(int64_t)p * 64];
  }
  const unsigned long long a =
      n < 0 ? 0ull - (unsigned long long)n : (unsigned long long)n;
  int size = a ? 64 - __clzll((long long)a) : 0;
  t.over = size > cap;
  if (t.over) size = cap;
  t.size = size;
  t.value = (uint32_t)(n < 0 ? n - 1 : n) & ((1u << size) - 1u);
  t.ac = lane >= 1 && v != 0;
  t.sel = table_sel[row] ? 1 : 0;
  const unsigned long long mask = __ballot(t.ac);
  const unsigned long long below = mask & ((1ull << lane) - 1ull);
  const int prev = below ? 63 - __clzll((long long)below) : 0;
  t.z = lane - prev - 1;
  t.eob = !(mask >> 63);
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
    const int32_t* __restrict__ levels, int64_t d,
    const int32_t* __restrict__ pred, const uint8_t* __restrict__ table_sel,
    unsigned long long* __restrict__ ac_counts,
    unsigned long long* __restrict__ dc_counts, int32_t* __restrict__ status) {
  __shared__ unsigned bins[kSymbols];
  for (int i = threadIdx.x; i < kSymbols; i += kBlock) bins[i] = 0;
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t row0 =
      ((int64_t)blockIdx.x * kWavesPerBlock + wave) * kRowsPerWave;
  int over = 0;
  for (int r = 0; r < kRowsPerWave && row0 + r < d; ++r) {
    const LaneToken t = lane_token(levels, d, row0 + r, pred, table_sel, lane);
    unsigned* pair = bins + t.sel * kPairSymbols;
    over += t.over;
    if (t.ac) {
      atomicAdd(&pair[(t.z & 15) << 4 | t.size], 1u);
      if (t.z >> 4) atomicAdd(&pair[kZrl], (unsigned)(t.z >> 4));
    }
    if (t.dc) {
      atomicAdd(&pair[kDcBase + t.size], 1u);
      if (t.eob) atomicAdd(&pair[kEob], 1u);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kSymbols; i += kBlock) {
    const unsigned n = bins[i];
    const int sel = i / kPairSymbols, j = i % kPairSymbols;
    if (n)
      atomicAdd(j < kDcBase ? &ac_counts[sel * 256 + j]
                            : &dc_counts[sel * 16 + j - kDcBase],
                (unsigned long long)n);
  }
  over = wave_sum_int(over);
  if (lane == 0 && over) atomicAdd(&status[0], over);
}

// The two table pairs side by side in LDS: pair t at [272 t, 272 t + 272).
__device__ __forceinline__ void load_lengths(uint8_t* len,
                                             const uint8_t* ac_len,
                                             const uint8_t* dc_len) {
  for (int i = threadIdx.x; i < kSymbols; i += kBlock) {
    const int sel = i / kPairSymbols, j = i % kPairSymbols;
    const int l = j < kDcBase ? ac_len[sel * 256 + j]
                              : dc_len[sel * 16 + j - kDcBase];
    len[i] = (uint8_t)min(l, kMaxCodeBits);
  }
}

// Bits of one lane's token (the end of block excluded) under the pair `len`
// (LDS, kPairSymbols bytes); a used symbol of length 0 lowers `missing` to
// 1 + its id, ids of `len` starting at `id0`.
__device__ __forceinline__ int token_bits(const LaneToken& t,
                                          const uint8_t* len, int id0,
                                          int& missing) {
  int bits = 0;
  if (t.dc) {
    const int sym = kDcBase + t.size;
    const int ld = len[sym];
    if (!ld) missing = min(missing, id0 + sym + 1);
    bits = ld + t.size;
  } else if (t.ac) {
    const int sym = (t.z & 15) << 4 | t.size;
    const int ls = len[sym];
    if (!ls) missing = min(missing, id0 + sym + 1);
    bits = ls + t.size;
    const int zrl = t.z >> 4;
    if (zrl) {
      const int lf = len[kZrl];
      if (!lf) missing = min(missing, id0 + kZrl + 1);
      bits += zrl * lf;
    }
  }
  return bits;
}

// ---- block lengths ----------------------------------------------------------
__global__ __launch_bounds__(kBlock) void block_bits_kernel(
    const int32_t* __restrict__ levels, int64_t d,
    const int32_t* __restrict__ pred, const uint8_t* __restrict__ table_sel,
    const uint8_t* __restrict__ ac_len, const uint8_t* __restrict__ dc_len,
    int32_t* __restrict__ bits, int32_t* __restrict__ status) {
  __shared__ uint8_t len[kSymbols];
  load_lengths(len, ac_len, dc_len);
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t row0 =
      ((int64_t)blockIdx.x * kWavesPerBlock + wave) * kRowsPerWave;
  int over = 0, missing = INT_MAX;
  for (int r = 0; r < kRowsPerWave && row0 + r < d; ++r) {
    const LaneToken t = lane_token(levels, d, row0 + r, pred, table_sel, lane);
    const int id0 = t.sel * kPairSymbols;
    const uint8_t* pair = len + id0;
    over += t.over;
    int total = token_bits(t, pair, id0, missing);
    if (t.dc && t.eob) {
      const int le = pair[kEob];
      if (!le) missing = min(missing, id0 + kEob + 1);
      total += le;
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
    const int32_t* __restrict__ levels, int64_t d,
    const int32_t* __restrict__ pred, const uint8_t* __restrict__ table_sel,
    const uint16_t* __restrict__ ac_code, const uint8_t* __restrict__ ac_len,
    const uint16_t* __restrict__ dc_code, const uint8_t* __restrict__ dc_len,
    const int64_t* __restrict__ offsets, uint8_t* raw, int64_t raw_bytes,
    int32_t* __restrict__ status) {
  __shared__ uint8_t len[kSymbols];
  __shared__ uint16_t code[kSymbols];
  load_lengths(len, ac_len, dc_len);
  for (int i = threadIdx.x; i < kSymbols; i += kBlock) {
    const int sel = i / kPairSymbols, j = i % kPairSymbols;
    code[i] = j < kDcBase ? ac_code[sel * 256 + j]
                          : dc_code[sel * 16 + j - kDcBase];
  }
  __syncthreads();
  const uintptr_t address = reinterpret_cast<uintptr_t>(raw);
  unsigned* words = reinterpret_cast<unsigned*>(address & ~(uintptr_t)3);
  const int64_t lo = (int64_t)(address & 3) * 8;
  const int64_t limit = lo + raw_bytes * 8;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t row0 =
      ((int64_t)blockIdx.x * kWavesPerBlock + wave) * kRowsPerWave;
  int over = 0, missing = INT_MAX, dropped = 0;
  for (int r = 0; r < kRowsPerWave && row0 + r < d; ++r) {
    const LaneToken t = lane_token(levels, d, row0 + r, pred, table_sel, lane);
    const int id0 = t.sel * kPairSymbols;
    const uint8_t* plen = len + id0;
    const uint16_t* pcode = code + id0;
    over += t.over;
    // a negative offset stays negative: lo <= 24
    const int64_t base = offsets[row0 + r] < 0 ? offsets[row0 + r]
                                               : offsets[row0 + r] + lo;
    const int mine = token_bits(t, plen, id0, missing);
    int incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    int64_t pos = base + (incl - mine);
    if (t.dc) {
      const int sym = kDcBase + t.size;
      dropped += put_bits(words, lo, limit, pos, pcode[sym], plen[sym]);
      pos += plen[sym];
      dropped += put_bits(words, lo, limit, pos, t.value, t.size);
    } else if (t.ac) {
      const int lf = plen[kZrl];
      for (int k = t.z >> 4; k > 0; --k) {
        dropped += put_bits(words, lo, limit, pos, pcode[kZrl], lf);
        pos += lf;
      }
      const int sym = (t.z & 15) << 4 | t.size;
      dropped += put_bits(words, lo, limit, pos, pcode[sym], plen[sym]);
      pos += plen[sym];
      dropped += put_bits(words, lo, limit, pos, t.value, t.size);
    }
    const int total = __shfl(incl, 63, 64);
    if (t.dc && t.eob) {
      const int le = plen[kEob];
      if (!le) missing = min(missing, id0 + kEob + 1);
      dropped += put_bits(words, lo, limit, base + total, pcode[kEob], le);
    }
  }
  // the pad bits of the last byte, all ones
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t end = offsets[d];
    const int pad = (int)((8 - (end & 7)) & 7);
    if (end >= 0 && pad)
      dropped += put_bits(words, lo, limit, end + lo, 0x7Fu, pad);
  }
  over = wave_sum_int(over + dropped);
  if (lane == 0 && over) atomicAdd(&status[0], over);
  missing = wave_min(missing);
  if (lane == 0 && missing != INT_MAX) atomicMin(&status[1], missing);
}

// ---- byte stuffing: count, scan, scatter (block_scan.h) ---------------------
// The thread's kStuffItems bytes from `first` on (zeros beyond n) and how many
// of them are 0xFF.
__device__ __forceinline__ int load_stuff_items(const uint8_t* raw, int64_t n,
                                                int64_t first, uint8_t* b) {
  int marks = 0;
#pragma unroll
  for (int k = 0; k < kStuffItems; ++k) {
    b[k] = first + k < n ? raw[first + k] : (uint8_t)0;
    marks += b[k] == 0xFF;
  }
  return marks;
}

// step 1: sums[tile] = number of 0xFF bytes of the tile
__global__ __launch_bounds__(kBlock) void stuff_tile_sums_kernel(
    const uint8_t* __restrict__ raw, int64_t n, long long* __restrict__ sums) {
  const int64_t first = (int64_t)blockIdx.x * VTC_JFIF_STUFF_TILE +
                        (int64_t)threadIdx.x * kStuffItems;
  uint8_t b[kStuffItems];
  long long total;
  block_exclusive_scan<kBlock>(load_stuff_items(raw, n, first, b), &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// step 2 (one block): sums[tile] = 0xFF bytes before the tile; the length of
// the stuffed string and the number of bytes that do not fit
__global__ __launch_bounds__(kBlock) void stuff_scan_kernel(
    long long* __restrict__ sums, int64_t tiles, int64_t n, int64_t capacity,
    long long* __restrict__ out_len, int32_t* __restrict__ status) {
  const long long carry = block_prefix_tile_sums<kBlock>(sums, tiles);
  if (threadIdx.x == 0) {
    const long long length = n + carry;
    const long long lost = length > capacity ? length - capacity : 0;
    out_len[0] = length;
    status[0] = lost > INT_MAX ? INT_MAX : (int32_t)lost;
  }
}

// step 3: byte i goes to i + (0xFF bytes before i), a zero behind every 0xFF;
// only positions below capacity are written
__global__ __launch_bounds__(kBlock) void stuff_write_kernel(
    const uint8_t* __restrict__ raw, int64_t n,
    const long long* __restrict__ sums, uint8_t* __restrict__ out,
    int64_t capacity) {
  const int64_t first = (int64_t)blockIdx.x * VTC_JFIF_STUFF_TILE +
                        (int64_t)threadIdx.x * kStuffItems;
  uint8_t b[kStuffItems];
  const int marks = load_stuff_items(raw, n, first, b);
  long long total;
  long long at =
      first + sums[blockIdx.x] + block_exclusive_scan<kBlock>(marks, &total);
#pragma unroll
  for (int k = 0; k < kStuffItems; ++k) {
    if (first + k >= n) break;
    if (at < capacity) out[at] = b[k];
    ++at;
    if (b[k] == 0xFF) {
      if (at < capacity) out[at] = 0;
      ++at;
    }
  }
}

struct StuffLayout {
  long long* sums;
  StuffLayout(Carver& c, int64_t n) {
    sums = c.take<long long>((size_t)ceil_div(n, VTC_JFIF_STUFF_TILE));
  }
};

int check_rows(const char* who, int64_t d, int64_t* blocks) {
  VTC_REQUIRE(d > 0, "%s: bad size d = %lld", who, (long long)d);
  *blocks = ceil_div(d, kRowsPerBlock);
  VTC_REQUIRE(*blocks < (int64_t)1 << 31, "%s: too many rows", who);
  return VTC_OK;
}

int check_plane(const char* who, int32_t h, int32_t w, int32_t bh, int32_t bw,
                int64_t rows, int* grid) {
  VTC_REQUIRE(h >= 1 && w >= 1, "%s: bad size h = %d, w = %d", who, h, w);
  VTC_REQUIRE(bh >= 1 && bw >= 1 && (int64_t)bh * 8 >= h &&
                  (int64_t)bw * 8 >= w,
              "%s: bad size bh = %d, bw = %d: the block grid must cover the "
              "%d x %d plane", who, bh, bw, h, w);
  VTC_REQUIRE((int64_t)bh * bw < (int64_t)1 << 31, "%s: too many blocks", who);
  VTC_REQUIRE(rows >= 1 && rows < (int64_t)1 << 31, "%s: bad size rows = %lld",
              who, (long long)rows);
  const int64_t blocks = ceil_div((int64_t)bh * bw, kWavesPerBlock);
  *grid = (int)(blocks < 65536 ? blocks : 65536);
  return VTC_OK;
}

}  // namespace
}  // namespace vtc

using namespace vtc;

extern "C" int vtc_jfif_abi_version(void) { return VTC_JFIF_ABI_VERSION; }

extern "C" int vtc_jfif_forward_dct(const float* plane, int32_t h, int32_t w,
                                    int32_t bh, int32_t bw,
                                    const double* basis, const uint16_t* q,
                                    const int32_t* row_of_block,
                                    int32_t* levels, int64_t rows,
                                    void* stream) {
  const char* who = "vtc_jfif_forward_dct";
  VTC_REQUIRE(plane && basis && q && row_of_block && levels,
              "%s: null pointer", who);
  int grid;
  const int rc = check_plane(who, h, w, bh, bw, rows, &grid);
  if (rc != VTC_OK) return rc;
  forward_dct_kernel<<<grid, kBlock, 0, as_stream(stream)>>>(
      plane, h, w, bh, bw, basis, q, row_of_block, levels, rows);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" int vtc_jfif_inverse_dct(const int32_t* levels, int64_t rows,
                                    const int32_t* row_of_block, int32_t bh,
                                    int32_t bw, const double* basis,
                                    const uint16_t* q, float* plane, int32_t h,
                                    int32_t w, void* stream) {
  const char* who = "vtc_jfif_inverse_dct";
  VTC_REQUIRE(levels && row_of_block && basis && q && plane,
              "%s: null pointer", who);
  int grid;
  const int rc = check_plane(who, h, w, bh, bw, rows, &grid);
  if (rc != VTC_OK) return rc;
  inverse_dct_kernel<<<grid, kBlock, 0, as_stream(stream)>>>(
      levels, rows, row_of_block, bh, bw, basis, q, plane, h, w);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" int vtc_jfif_symbol_counts(const int32_t* levels, int64_t d,
                                      const int32_t* pred,
                                      const uint8_t* table_sel,
                                      uint64_t* ac_counts, uint64_t* dc_counts,
                                      int32_t* status, void* stream) {
  const char* who = "vtc_jfif_symbol_counts";
  VTC_REQUIRE(levels && pred && table_sel && ac_counts && dc_counts && status,
              "%s: null pointer", who);
  int64_t blocks;
  const int rc = check_rows(who, d, &blocks);
  if (rc != VTC_OK) return rc;
  hipStream_t st = as_stream(stream);
  VTC_HIP_CHECK(hipMemsetAsync(ac_counts, 0, 2 * 256 * sizeof(uint64_t), st));
  VTC_HIP_CHECK(hipMemsetAsync(dc_counts, 0, 2 * 16 * sizeof(uint64_t), st));
  status_begin_kernel<<<1, 1, 0, st>>>(status);
  symbol_counts_kernel<<<(int)blocks, kBlock, 0, st>>>(
      levels, d, pred, table_sel,
      reinterpret_cast<unsigned long long*>(ac_counts),
      reinterpret_cast<unsigned long long*>(dc_counts), status);
  status_end_kernel<<<1, 1, 0, st>>>(status);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" int vtc_jfif_block_bits(const int32_t* levels, int64_t d,
                                   const int32_t* pred,
                                   const uint8_t* table_sel,
                                   const uint8_t* ac_len,
                                   const uint8_t* dc_len, int32_t* bits,
                                   int32_t* status, void* stream) {
  const char* who = "vtc_jfif_block_bits";
  VTC_REQUIRE(levels && pred && table_sel && ac_len && dc_len && bits &&
                  status, "%s: null pointer", who);
  int64_t blocks;
  const int rc = check_rows(who, d, &blocks);
  if (rc != VTC_OK) return rc;
  hipStream_t st = as_stream(stream);
  status_begin_kernel<<<1, 1, 0, st>>>(status);
  block_bits_kernel<<<(int)blocks, kBlock, 0, st>>>(
      levels, d, pred, table_sel, ac_len, dc_len, bits, status);
  status_end_kernel<<<1, 1, 0, st>>>(status);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" int vtc_jfif_pack(const int32_t* levels, int64_t d,
                             const int32_t* pred, const uint8_t* table_sel,
                             const uint16_t* ac_code, const uint8_t* ac_len,
                             const uint16_t* dc_code, const uint8_t* dc_len,
                             const int64_t* offsets, uint8_t* raw,
                             size_t raw_bytes, int32_t* status, void* stream) {
  const char* who = "vtc_jfif_pack";
  VTC_REQUIRE(levels && pred && table_sel && ac_code && ac_len && dc_code &&
                  dc_len && offsets && raw && status, "%s: null pointer", who);
  int64_t blocks;
  const int rc = check_rows(who, d, &blocks);
  if (rc != VTC_OK) return rc;
  VTC_REQUIRE(raw_bytes > 0 && raw_bytes < (size_t)1 << 59,
              "%s: bad size raw_bytes = %zu", who, raw_bytes);
  hipStream_t st = as_stream(stream);
  VTC_HIP_CHECK(hipMemsetAsync(raw, 0, raw_bytes, st));
  status_begin_kernel<<<1, 1, 0, st>>>(status);
  pack_kernel<<<(int)blocks, kBlock, 0, st>>>(
      levels, d, pred, table_sel, ac_code, ac_len, dc_code, dc_len, offsets,
      raw, (int64_t)raw_bytes, status);
  status_end_kernel<<<1, 1, 0, st>>>(status);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" size_t vtc_jfif_stuff_bytes_workspace_bytes(int64_t n) {
  if (n <= 0) return 0;
  return measured_bytes<StuffLayout>(n);
}

extern "C" int vtc_jfif_stuff_bytes(const uint8_t* raw, int64_t n,
                                    uint8_t* out, int64_t capacity,
                                    int64_t* out_len, int32_t* status,
                                    void* workspace, size_t workspace_bytes,
                                    void* stream) {
  const char* who = "vtc_jfif_stuff_bytes";
  VTC_REQUIRE(out_len && status, "%s: null pointer", who);
  VTC_REQUIRE(n >= 0 && n < (int64_t)1 << 40, "%s: bad size n = %lld", who,
              (long long)n);
  VTC_REQUIRE(capacity >= 0 && capacity < (int64_t)1 << 41,
              "%s: bad size capacity = %lld", who, (long long)capacity);
  VTC_REQUIRE((raw || n == 0) && (out || capacity == 0), "%s: null pointer",
              who);
  if (n > 0 && capacity > 0) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(raw);
    const uintptr_t b = reinterpret_cast<uintptr_t>(out);
    VTC_REQUIRE(a + (uintptr_t)n <= b || b + (uintptr_t)capacity <= a,
                "%s: out overlaps raw", who);
  }
  const int64_t tiles = ceil_div(n, VTC_JFIF_STUFF_TILE);
  const size_t need = vtc_jfif_stuff_bytes_workspace_bytes(n);
  if (need && (!workspace || workspace_bytes < need)) {
    set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
              need);
    return VTC_ERR_WORKSPACE;
  }
  Carver carve(need ? workspace : nullptr);
  const StuffLayout ws(carve, n);
  hipStream_t st = as_stream(stream);
  long long* length = reinterpret_cast<long long*>(out_len);
  if (tiles)
    stuff_tile_sums_kernel<<<(int)tiles, kBlock, 0, st>>>(raw, n, ws.sums);
  stuff_scan_kernel<<<1, kBlock, 0, st>>>(ws.sums, tiles, n, capacity, length,
                                          status);
  if (tiles)
    stuff_write_kernel<<<(int)tiles, kBlock, 0, st>>>(raw, n, ws.sums, out,
                                                      capacity);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}
