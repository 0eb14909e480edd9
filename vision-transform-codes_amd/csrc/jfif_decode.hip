// The device half of a baseline JFIF reader (include/ext/vtc_jfif_decode.h):
// stuffed bytes back to the entropy-coded segment, the segment back to
// quantiser levels, DC prediction undone.  DESIGN.md 4.24 states the rules and
// the bounds of every index.
//
// Unpacking.  A JFIF scan is one bit-contiguous segment without offsets, so a
// codeword's start is known only once everything before it has been read.
// The segment is cut into subsequences of kSubseqBytes bytes, one LANE each,
// 256 per workgroup; every lane but the first starts from a guess and the
// guesses are corrected, round after round, until no exit state changes
// (self-synchronising Huffman decoding).  Inside a workgroup the rounds run in
// LDS between barriers; across workgroups the kernel is enqueued once per
// workgroup of the segment, exit states double-buffered by launch parity, and
// a workgroup whose incoming state is the one it last decoded from copies its
// exit state and leaves.  Nothing waits for another workgroup.
//
// One step() states the token rule for the synchronisation rounds and for the
// storing pass.  The workgroup's 32 KiB of the segment are staged in LDS as
// big-endian words, one pad word per subsequence, so lanes that stand at the
// same offset of their subsequences read 32 different banks; the four decode
// tables (prefix_table.h, first level on 9 bits) are in LDS too.
#include <limits.h>

#include "../../include/ext/vtc_jfif.h"
#include "../../include/ext/vtc_jfif_decode.h"
#include "block_scan.h"
#include "common.h"
#include "prefix_table.h"

namespace vtc {
namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / 64;

// ---- byte unstuffing: count, scan, scatter (block_scan.h) -------------------
constexpr int kStuffItems = VTC_JFIF_STUFF_TILE / kBlock;
static_assert(kStuffItems * kBlock == VTC_JFIF_STUFF_TILE, "tile = block * 8");

// The thread's kStuffItems bytes from `first` on, the byte before them and the
// byte behind them, as b[0 .. kStuffItems + 1]; a position outside [0, n)
// reads 0x01, which is neither a marker byte nor a stuffed zero.
__device__ __forceinline__ void load_unstuff_items(const uint8_t* in,
                                                   int64_t n, int64_t first,
                                                   uint8_t* b) {
#pragma unroll
  for (int k = 0; k < kStuffItems + 2; ++k) {
    const int64_t i = first + k - 1;
    b[k] = i >= 0 && i < n ? in[i] : (uint8_t)1;
  }
}

// Of the thread's bytes below `limit`: how many are stuffed zeros (a 0x00
// directly behind a 0xFF); *marker = the first 0xFF of them that no 0x00
// follows, or n.
__device__ __forceinline__ int scan_unstuff_items(const uint8_t* b, int64_t n,
                                                  int64_t first,
                                                  int64_t limit,
                                                  long long* marker) {
  int zeros = 0;
  long long at = n;
#pragma unroll
  for (int k = 0; k < kStuffItems; ++k) {
    const int64_t i = first + k;
    if (i >= n) break;
    if (i < limit && b[k + 1] == 0x00 && b[k] == 0xFF) ++zeros;
    if (at == n && b[k + 1] == 0xFF && b[k + 2] != 0x00) at = i;
  }
  *marker = at;
  return zeros;
}

struct UnstuffLayout {
  long long* sums;   // [tiles] stuffed zeros of the tile, then those before it
  long long* marks;  // [tiles] the tile's first marker, or n
  long long* head;   // [2] marker_at, unused
  UnstuffLayout(Carver& c, int64_t n) {
    const size_t tiles = (size_t)ceil_div(n, VTC_JFIF_STUFF_TILE);
    sums = c.take<long long>(tiles);
    marks = c.take<long long>(tiles);
    head = c.take<long long>(2);
  }
};

// step 1: per tile, the stuffed zeros and the first marker
__global__ __launch_bounds__(kBlock) void unstuff_tile_kernel(
    const uint8_t* __restrict__ in, int64_t n, UnstuffLayout ws) {
  const int64_t first = (int64_t)blockIdx.x * VTC_JFIF_STUFF_TILE +
                        (int64_t)threadIdx.x * kStuffItems;
  uint8_t b[kStuffItems + 2];
  load_unstuff_items(in, n, first, b);
  long long marker, total;
  const int zeros = scan_unstuff_items(b, n, first, n, &marker);
  block_exclusive_scan<kBlock>(zeros, &total);
  marker = block_min<kBlock>(marker);
  if (threadIdx.x == 0) {
    ws.sums[blockIdx.x] = total;
    ws.marks[blockIdx.x] = marker;
  }
}

// step 2 (one block): sums[tile] = stuffed zeros before the tile; marker_at;
// the zeros of the marker's own tile that lie before it; lengths and status
__global__ __launch_bounds__(kBlock) void unstuff_scan_kernel(
    const uint8_t* __restrict__ in, int64_t n, UnstuffLayout ws, int64_t tiles,
    int64_t capacity, long long* __restrict__ out_len,
    int32_t* __restrict__ status) {
  const long long carry = block_prefix_tile_sums<kBlock>(ws.sums, tiles);
  long long marker = n;
  for (int64_t base = 0; base < tiles; base += kBlock) {
    const int64_t i = base + threadIdx.x;
    const long long lowest = block_min<kBlock>(i < tiles ? ws.marks[i] : n);
    marker = lowest < marker ? lowest : marker;
  }
  __syncthreads();   // sums[] of this block are visible to all its threads
  long long zeros = carry;
  if (marker < n) {   // 0 <= marker < n: its tile exists
    const int64_t tile = marker / VTC_JFIF_STUFF_TILE;
    const int64_t first =
        tile * VTC_JFIF_STUFF_TILE + (int64_t)threadIdx.x * kStuffItems;
    uint8_t b[kStuffItems + 2];
    load_unstuff_items(in, n, first, b);
    long long unused, inside;
    block_exclusive_scan<kBlock>(
        scan_unstuff_items(b, n, first, marker, &unused), &inside);
    zeros = ws.sums[tile] + inside;
  }
  if (threadIdx.x == 0) {
    const long long length = marker - zeros;
    const long long lost = length > capacity ? length - capacity : 0;
    out_len[0] = length;
    out_len[1] = marker;
    status[0] = lost > INT_MAX ? INT_MAX : (int32_t)lost;
    if (tiles) ws.head[0] = marker;
  }
}

// step 3: byte i < marker_at goes to i - (stuffed zeros before i), a stuffed
// zero nowhere; only positions below capacity are written
__global__ __launch_bounds__(kBlock) void unstuff_write_kernel(
    const uint8_t* __restrict__ in, int64_t n, UnstuffLayout ws,
    uint8_t* __restrict__ out, int64_t capacity) {
  const long long marker = ws.head[0];
  const int64_t first = (int64_t)blockIdx.x * VTC_JFIF_STUFF_TILE +
                        (int64_t)threadIdx.x * kStuffItems;
  if ((int64_t)blockIdx.x * VTC_JFIF_STUFF_TILE >= marker) return;  // uniform
  uint8_t b[kStuffItems + 2];
  load_unstuff_items(in, n, first, b);
  long long unused, total;
  const int zeros = scan_unstuff_items(b, n, first, marker, &unused);
  long long at = first - ws.sums[blockIdx.x] -
                 block_exclusive_scan<kBlock>(zeros, &total);
#pragma unroll
  for (int k = 0; k < kStuffItems; ++k) {
    if (first + k >= marker) break;
    if (b[k + 1] == 0x00 && b[k] == 0xFF) continue;
    if (at < capacity) out[at] = b[k + 1];   // 0 <= at <= first + k
    ++at;
  }
}

// ---- DC prediction undone: a segmented inclusive scan -----------------------
// The scan's element is (flag, sum): flag = a chain starts here or before,
// inside the span; sum = the sum since the last start of the span.
struct Seg {
  uint32_t flag, sum;
};
__device__ __forceinline__ Seg seg_join(Seg left, Seg right) {
  Seg r;
  r.flag = left.flag | right.flag;
  r.sum = right.flag ? right.sum : left.sum + right.sum;   // wraps
  return r;
}

// Inclusive segmented scan of `v` over the block; *total = the whole block.
__device__ __forceinline__ Seg block_segmented_scan(Seg v, Seg* total) {
  __shared__ Seg wave_tot[kWavesPerBlock];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    Seg o;
    o.flag = __shfl_up(v.flag, off, 64);
    o.sum = __shfl_up(v.sum, off, 64);
    if (lane >= off) v = seg_join(o, v);
  }
  if (lane == 63) wave_tot[wave] = v;
  __syncthreads();
  Seg before = {0u, 0u}, all = {0u, 0u};
  for (int w = 0; w < kWavesPerBlock; ++w) {
    if (w < wave) before = seg_join(before, wave_tot[w]);
    all = seg_join(all, wave_tot[w]);
  }
  __syncthreads();
  *total = all;
  return seg_join(before, v);
}

struct DcLayout {
  uint32_t* flag;   // [tiles]
  uint32_t* sum;    // [tiles] the tile's total, then the carry into the tile
  DcLayout(Carver& c, int64_t d) {
    const size_t tiles = (size_t)ceil_div(d, VTC_JFIF_DC_TILE);
    flag = c.take<uint32_t>(tiles);
    sum = c.take<uint32_t>(tiles);
  }
};

__device__ __forceinline__ Seg dc_element(const int32_t* levels, int64_t d,
                                          const int32_t* order,
                                          const uint8_t* start, int64_t j,
                                          int64_t* row) {
  Seg v = {0u, 0u};
  *row = -1;
  if (j < d) {
    const int32_t r = order[j];
    v.flag = start[j] ? 1u : 0u;
    if (r >= 0 && (int64_t)r < d) {
      *row = r;
      v.sum = (uint32_t)levels[(int64_t)r * 64];
    }
  }
  return v;
}

static_assert(VTC_JFIF_DC_TILE == kBlock, "one chain element per thread");

__global__ __launch_bounds__(kBlock) void dc_tile_kernel(
    const int32_t* __restrict__ levels, int64_t d,
    const int32_t* __restrict__ order, const uint8_t* __restrict__ start,
    DcLayout ws) {
  int64_t row;
  const Seg v = dc_element(levels, d, order, start,
                           (int64_t)blockIdx.x * kBlock + threadIdx.x, &row);
  Seg total;
  block_segmented_scan(v, &total);
  if (threadIdx.x == 0) {
    ws.flag[blockIdx.x] = total.flag;
    ws.sum[blockIdx.x] = total.sum;
  }
}

// one block: sum[tile] = the accumulator that enters the tile
__global__ __launch_bounds__(kBlock) void dc_scan_kernel(DcLayout ws,
                                                         int64_t tiles) {
  Seg carry = {0u, 0u};
  for (int64_t base = 0; base < tiles; base += kBlock) {
    const int64_t i = base + threadIdx.x;
    Seg v = {0u, 0u};
    if (i < tiles) {
      v.flag = ws.flag[i];
      v.sum = ws.sum[i];
    }
    Seg total;
    const Seg incl = seg_join(carry, block_segmented_scan(v, &total));
    // exclusive: what the tiles before i leave behind
    Seg left;
    left.flag = __shfl_up(incl.flag, 1, 64);
    left.sum = __shfl_up(incl.sum, 1, 64);
    __shared__ Seg edge[kWavesPerBlock];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 63) edge[wave] = incl;
    __syncthreads();
    if (lane == 0) left = wave ? edge[wave - 1] : carry;
    __syncthreads();
    if (i < tiles) ws.sum[i] = left.sum;
    carry = seg_join(carry, total);
  }
}

__global__ __launch_bounds__(kBlock) void dc_write_kernel(
    int32_t* levels, int64_t d, const int32_t* __restrict__ order,
    const uint8_t* __restrict__ start, DcLayout ws) {
  int64_t row;
  const Seg v = dc_element(levels, d, order, start,
                           (int64_t)blockIdx.x * kBlock + threadIdx.x, &row);
  Seg total, carry;
  carry.flag = 0u;
  carry.sum = ws.sum[blockIdx.x];
  const Seg incl = seg_join(carry, block_segmented_scan(v, &total));
  // every read of column 0 of this tile's rows happened above: rows are
  // distinct, so no other thread reads or writes levels[row][0]
  if (row >= 0) levels[row * 64] = (int32_t)incl.sum;
}

// ---- unpacking: tables ------------------------------------------------------
constexpr int kSubseqBytes = VTC_JFIF_SUBSEQ_BYTES;
constexpr int kSubseqWords = kSubseqBytes / 4;
constexpr int kSubseqBits = kSubseqBytes * 8;
static_assert(VTC_JFIF_SUBSEQ_PER_GROUP == kBlock, "one lane per subsequence");
static_assert(kSubseqWords == 32, "one pad word per 32 words: bank = offset");
constexpr int kGroupBytes = kSubseqBytes * kBlock;
constexpr int kGroupBits = kGroupBytes * 8;
// a token starts below the group's last bit and is at most 27 bits long: the
// 32-bit window at its start ends inside word kGroupWords
constexpr int kGroupWords = kGroupBytes / 4;
constexpr int kStagedWords = kGroupWords + 2;
constexpr int kStagedPadded = kStagedWords + kStagedWords / 32 + 1;

constexpr int kTables = 4;   // DC 0, DC 1, AC 0, AC 1
constexpr int kDcSymbols = 16, kAcSymbols = 256;
constexpr int kCodes = 2 * kDcSymbols + 2 * kAcSymbols;
constexpr int kMaxCodeBits = 16;
constexpr int kEob = 0x00, kZrl = 0xF0;
constexpr int kAcCap = 10, kDcCap = 11;

__host__ __device__ constexpr int table_base(int t) {
  return t < 2 ? t * kDcSymbols : 2 * kDcSymbols + (t - 2) * kAcSymbols;
}

// meta word of a codeword: length << 8 | symbol (lengths 1 .. 16); 0 is no
// codeword.
struct JfifCode {
  typedef uint16_t Key;
  typedef uint16_t Meta;
  static constexpr int kLutBits = 9;
  static __host__ __device__ constexpr unsigned make(int len, int symbol) {
    return (unsigned)len << 8 | (unsigned)symbol;
  }
  static __host__ __device__ constexpr bool valid(unsigned m) {
    return m != 0;
  }
  static __host__ __device__ constexpr int len(unsigned m) {
    return m >> 8;
  }
  static __host__ __device__ constexpr int symbol(unsigned m) {
    return m & 255;
  }
};
typedef PrefixTable<JfifCode> Table;
constexpr int kLutSize = Table::kLutSize;
static_assert(Table::round_trips(1, 0) && Table::round_trips(16, 255) &&
                  Table::round_trips(1, 255) && Table::round_trips(16, 0),
              "length << 8 | symbol");

// The state at a boundary: bit position << 10 | coefficient index << 4 | block
// position.  Inside a workgroup positions count from the group's first bit
// and fit 32 bits; between workgroups they are absolute, 64 bits.
constexpr uint32_t kNoState = 0xFFFFFFFFu;
constexpr u64 kNoState64 = ~0ull;

struct UnpackLayout {
  uint16_t* key;     // [kCodes] left-aligned codewords, each table sorted
  uint16_t* meta;    // [kCodes] length << 8 | symbol of the sorted codewords
  uint16_t* lut;     // [kTables][kLutSize] meta word a 9-bit prefix starts with
  int32_t* count;    // [kTables] codewords of each table
  u64* exit;         // [2][groups] exit state of each workgroup, by parity
  u64* seen;         // [groups] the incoming state it last decoded from
  int32_t* blocks;   // [groups] blocks its subsequences completed
  long long* first;  // [groups] blocks before the workgroup
  int32_t* rounds;   // [groups] per launch: the most rounds of a workgroup
  uint32_t* entry;   // [groups * 256] true entry state of each subsequence
  uint32_t* before;  // [groups * 256] blocks before it inside its workgroup
  u64* head;         // [4] 1 + first malformed bit, subsequence << 32 | row of
                     //     it, position after block `rows`, unused
  UnpackLayout(Carver& c, int64_t seg_bytes) {
    const size_t groups = (size_t)ceil_div(seg_bytes, kGroupBytes);
    key = c.take<uint16_t>(kCodes);
    meta = c.take<uint16_t>(kCodes);
    lut = c.take<uint16_t>(kTables * kLutSize);
    count = c.take<int32_t>(kTables);
    exit = c.take<u64>(2 * groups);
    seen = c.take<u64>(groups);
    blocks = c.take<int32_t>(groups);
    first = c.take<long long>(groups);
    rounds = c.take<int32_t>(groups);
    entry = c.take<uint32_t>(groups * kBlock);
    before = c.take<uint32_t>(groups * kBlock);
    head = c.take<u64>(4);
  }
};

// One block: the four decode tables of prefix_table.h, and the
// cross-workgroup state set to "nothing decoded yet".  A table that is not
// prefix-free is not reported: it decodes by the same rule.
__global__ __launch_bounds__(kBlock) void unpack_tables_kernel(
    const uint16_t* __restrict__ ac_code, const uint8_t* __restrict__ ac_len,
    const uint16_t* __restrict__ dc_code, const uint8_t* __restrict__ dc_len,
    UnpackLayout ws, int64_t groups) {
  __shared__ uint16_t key[kCodes], meta[kCodes];
  __shared__ uint16_t lut[kTables * kLutSize];
  __shared__ int count[kTables];
  const int tid = threadIdx.x;
  if (tid < kTables) count[tid] = 0;
  for (int i = tid; i < kTables * kLutSize; i += kBlock) lut[i] = 0;
  __syncthreads();
  for (int i = tid; i < kCodes; i += kBlock) {
    const int t = i < table_base(2) ? i / kDcSymbols
                                    : 2 + (i - table_base(2)) / kAcSymbols;
    int l = t < 2 ? dc_len[i] : ac_len[i - table_base(2)];
    if (l > kMaxCodeBits) l = kMaxCodeBits;
    const unsigned c = t < 2 ? dc_code[i] : ac_code[i - table_base(2)];
    key[i] = Table::left_align(c, l);
    meta[i] = l ? JfifCode::make(l, i - table_base(t)) : 0;
    if (l) atomicAdd(&count[t], 1);
  }
  __syncthreads();
  for (int t = 0; t < kTables; ++t)   // each table on its own
    Table::sort<kBlock>(key + table_base(t), meta + table_base(t),
                        t < 2 ? kDcSymbols : kAcSymbols);
  // where ranges overlap the later codeword wins: one thread per table, so
  // the lookup is a function of the tables alone
  if (tid < kTables)
    Table::fill_lookup(lut + tid * kLutSize, key + table_base(tid),
                       meta + table_base(tid), count[tid], 0, 1);
  __syncthreads();
  for (int i = tid; i < kCodes; i += kBlock) {
    ws.key[i] = key[i];
    ws.meta[i] = meta[i];
  }
  for (int i = tid; i < kTables * kLutSize; i += kBlock) ws.lut[i] = lut[i];
  if (tid < kTables) ws.count[tid] = count[tid];
  // before launch 0 the "previous" exit of workgroup g is the guess for g + 1
  for (int64_t g = tid; g < groups; g += kBlock) {
    ws.exit[groups + g] = (u64)((g + 1) * (int64_t)kGroupBits) << 10;
    ws.exit[g] = 0;
    ws.seen[g] = kNoState64;
    ws.blocks[g] = 0;
    ws.first[g] = 0;
    ws.rounds[g] = 0;
  }
  if (tid == 0) {
    ws.head[0] = kNoState64;
    ws.head[1] = kNoState64;
    ws.head[2] = kNoState64;
    ws.head[3] = 0;
  }
}

// ---- unpacking: what a workgroup keeps in LDS -------------------------------
struct GroupShared {
  uint32_t words[kStagedPadded];   // big-endian words of the group's bytes
  uint16_t key[kCodes];
  uint16_t meta[kCodes];
  uint16_t lut[kTables * kLutSize];
  int count[kTables];
  uint32_t exit[kBlock];
};

// The table of each block position of the MCU, bit `slot` of a mask: read
// once per thread, so the token loop has no lookup in front of its lookup.
struct Slots {
  unsigned dc, ac;
  int n;
  __device__ __forceinline__ Slots(const uint8_t* slot_dc,
                                   const uint8_t* slot_ac, int nslots)
      : dc(0), ac(0), n(nslots) {
    for (int i = 0; i < nslots; ++i) {   // nslots <= VTC_JFIF_MAX_SLOTS
      dc |= (slot_dc[i] ? 1u : 0u) << i;
      ac |= (slot_ac[i] ? 1u : 0u) << i;
    }
  }
};

__device__ __forceinline__ int padded(int word) { return word + (word >> 5); }

// Stages words [0, kStagedWords) of the group that starts at byte `base`.  A
// byte at or beyond seg_bytes reads 0xFF (stream bits beyond the end are 1).
// Global loads are aligned words that hold at least one byte of seg.
__device__ __forceinline__ void stage_group(GroupShared& sh,
                                            const uint8_t* seg,
                                            int64_t seg_bytes, int64_t base,
                                            const UnpackLayout& ws) {
  const uintptr_t address = reinterpret_cast<uintptr_t>(seg);
  const int skew = (int)((address + (uintptr_t)base) & 3);
  // aligned word j of the source holds bytes base - skew + 4 j .. + 3
  const uint32_t* source = reinterpret_cast<const uint32_t*>(
      (address + (uintptr_t)base) & ~(uintptr_t)3);
  const int64_t lo = -base, hi = seg_bytes - base;   // seg is bytes [lo, hi)
  for (int i = threadIdx.x; i < kStagedWords; i += kBlock) {
    u64 pair = ~0ull;   // little-endian image of bytes 4 i - skew .. + 7
    const int64_t b0 = (int64_t)4 * i - skew;
    uint32_t w0 = 0xFFFFFFFFu, w1 = 0xFFFFFFFFu;
    if (b0 + 3 >= lo && b0 < hi) w0 = source[i];
    if (skew && b0 + 7 >= lo && b0 + 4 < hi) w1 = source[i + 1];
    pair = (u64)w1 << 32 | w0;
    uint32_t word = (uint32_t)(pair >> (8 * skew));
    // bytes outside seg: ones
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t b = (int64_t)4 * i + k;
      if (b < lo || b >= hi) word |= 0xFFu << (8 * k);
    }
    sh.words[padded(i)] = __builtin_bswap32(word);
  }
  for (int i = threadIdx.x; i < kCodes; i += kBlock) {
    sh.key[i] = ws.key[i];
    sh.meta[i] = ws.meta[i];
  }
  for (int i = threadIdx.x; i < kTables * kLutSize; i += kBlock)
    sh.lut[i] = ws.lut[i];
  if (threadIdx.x < kTables) sh.count[threadIdx.x] = ws.count[threadIdx.x];
}

// The 32 stream bits from bit p of the group on, 0 <= p < kGroupBits + 32.
struct Window {
  const uint32_t* words;
  int at;          // index of the word in `a`, -2 = none
  uint32_t a, b;
  __device__ __forceinline__ uint32_t peek(int p) {
    const int i = p >> 5;   // i + 1 < kStagedWords
    if (i != at) {
      a = i == at + 1 ? b : words[padded(i)];
      b = words[padded(i + 1)];
      at = i;
    }
    const int s = p & 31;
    return s ? a << s | b >> (32 - s) : a;
  }
};

// The codeword of table t that the 16 bits `w` start with, as its meta word;
// 0 when none does.
__device__ __forceinline__ unsigned match(const GroupShared& sh, int t,
                                          unsigned w) {
  return Table::match(sh.lut + t * kLutSize, sh.key + table_base(t),
                      sh.meta + table_base(t), sh.count[t], (uint16_t)w);
}

__device__ __forceinline__ int32_t extend(uint32_t window, int len, int size) {
  // the `size` bits behind the codeword; len + size <= 27
  const int32_t bits = (int32_t)((window << len) >> (32 - size));
  return (bits >> (size - 1)) ? bits : bits - ((1 << size) - 1);
}

struct State {
  int p;      // bit position inside the group
  int z;      // 0: a DC token is next; 1 .. 63: index of the next coefficient
  int slot;   // block position inside the MCU
  __device__ __forceinline__ uint32_t pack() const {
    return (uint32_t)p << 10 | (uint32_t)z << 4 | (uint32_t)slot;
  }
  __device__ static __forceinline__ State unpack(uint32_t v) {
    State s;
    s.p = (int)(v >> 10);
    s.z = (int)(v >> 4 & 63);
    s.slot = (int)(v & 15);
    return s;
  }
};

// What one token did.
struct Token {
  bool malformed;   // consumed its codeword (one bit without one), ended block
  bool ended;       // the block is complete
  int index;        // where `value` belongs, -1: no level
  int32_t value;
};

// One token from state s.  s.p advances by 1 .. 27 bits whatever the bits are.
__device__ __forceinline__ Token step(const GroupShared& sh, Window& win,
                                      State& s, const Slots& slots) {
  Token t;
  t.malformed = false;
  t.ended = false;
  t.index = -1;
  t.value = 0;
  const uint32_t w = win.peek(s.p);
  const bool dc = s.z == 0;
  // s.slot < slots.n <= 10 in every state the kernels make; 15 at the most
  const int table = dc ? (int)(slots.dc >> s.slot & 1u)
                       : 2 + (int)(slots.ac >> s.slot & 1u);
  const unsigned m = match(sh, table, w >> 16);
  const int len = m ? JfifCode::len(m) : 1, symbol = JfifCode::symbol(m);
  int advance = len;
  if (!m) {
    t.malformed = true;
  } else if (dc) {
    if (symbol > kDcCap) {
      t.malformed = true;
    } else {
      if (symbol) {
        t.index = 0;
        t.value = extend(w, len, symbol);
      }
      advance += symbol;
      s.z = 1;
    }
  } else {
    const int run = symbol >> 4, size = symbol & 15;
    if (size == 0) {
      if (symbol == kEob) {
        t.ended = true;
      } else if (symbol == kZrl && s.z + 16 <= 64) {
        s.z += 16;
        t.ended = s.z == 64;
      } else {
        t.malformed = true;
      }
    } else if (size > kAcCap || s.z + run > 63) {
      t.malformed = true;
    } else {
      t.index = s.z + run;   // 1 .. 63
      t.value = extend(w, len, size);
      advance += size;
      s.z = t.index + 1;
      t.ended = s.z == 64;
    }
  }
  s.p += advance;
  if (t.malformed) t.ended = true;
  if (t.ended) {
    s.z = 0;
    s.slot = s.slot + 1 >= slots.n ? 0 : s.slot + 1;
  }
  return t;
}

// ---- unpacking: the synchronisation rounds ----------------------------------
// Launch `launch` of `groups`.  reads exit[(launch + 1) & 1], writes
// exit[launch & 1].
__global__ __launch_bounds__(kBlock) void unpack_sync_kernel(
    const uint8_t* __restrict__ seg, int64_t seg_bytes,
    const uint8_t* __restrict__ slot_dc, const uint8_t* __restrict__ slot_ac,
    int nslots, UnpackLayout ws, int64_t groups, int launch) {
  __shared__ GroupShared sh;
  const int64_t g = blockIdx.x;
  const u64* prev = ws.exit + (size_t)((launch + 1) & 1) * groups;
  u64* cur = ws.exit + (size_t)(launch & 1) * groups;
  const u64 incoming = g == 0 ? 0ull : prev[g - 1];
  const u64 seen = ws.seen[g];
  if (incoming == seen) {   // uniform: nothing to do
    if (threadIdx.x == 0) cur[g] = prev[g];
    return;
  }
  const int64_t base = g * kGroupBytes;
  stage_group(sh, seg, seg_bytes, base, ws);
  const Slots slots(slot_dc, slot_ac, nslots);
  const int tid = threadIdx.x;
  const int64_t left = seg_bytes - base;   // >= 1
  const int lanes = (int)(left < kGroupBytes ? ceil_div(left, kSubseqBytes)
                                             : kBlock);   // 1 .. 256
  const bool active = tid < lanes;
  // the subsequence's last bit + 1, inside the group
  const int end = (int)(left * 8 < (int64_t)(tid + 1) * kSubseqBits
                            ? left * 8
                            : (int64_t)(tid + 1) * kSubseqBits);
  // incoming: an exit state of the group before, 0 <= p - base bits < 27
  const uint32_t in0 = (uint32_t)(incoming - ((u64)(base * 8) << 10));
  uint32_t my_in = (uint32_t)(tid * kSubseqBits) << 10;   // the guess
  if (seen != kNoState64 && active) my_in = ws.entry[g * kBlock + tid];
  if (tid == 0) my_in = in0;
  sh.exit[tid] = kNoState;
  __syncthreads();

  Window win;
  win.words = sh.words;
  win.at = -2;
  uint32_t my_exit = kNoState;
  int my_blocks = 0, rounds = 0;
  bool dirty = true;
  // at most lanes + 1 turns: after turn r lanes 0 .. r are final, and the
  // turn after the last change ends the loop; the count only states the bound
  for (int turn = 0; turn <= kBlock; ++turn) {
    bool changed = false;
    if (active && dirty) {
      State s = State::unpack(my_in);
      int blocks = 0;
      while (s.p < end) blocks += step(sh, win, s, slots).ended;
      const uint32_t e = s.pack();
      changed = e != my_exit;
      my_exit = e;
      my_blocks = blocks;
      sh.exit[tid] = e;
    }
    if (!__syncthreads_or(changed)) break;
    ++rounds;
    const uint32_t next = tid == 0 ? my_in : sh.exit[tid - 1];
    dirty = next != my_in;
    my_in = next;
    __syncthreads();   // every read of exit[] before the next turn's writes
  }

  long long total;
  const long long mine =
      block_exclusive_scan<kBlock>(active ? my_blocks : 0, &total);
  if (active) {
    ws.entry[g * kBlock + tid] = my_in;
    ws.before[g * kBlock + tid] = (uint32_t)mine;
  }
  if (tid == lanes - 1) {
    // absolute again
    cur[g] = (u64)my_exit + ((u64)(base * 8) << 10);
    ws.seen[g] = incoming;
    ws.blocks[g] = (int32_t)total;
    atomicMax(&ws.rounds[launch], rounds);
  }
}

// one block: first[g] = blocks before workgroup g
__global__ __launch_bounds__(kBlock) void unpack_scan_kernel(UnpackLayout ws,
                                                             int64_t groups) {
  long long carry = 0;
  for (int64_t base = 0; base < groups; base += kBlock) {
    const int64_t i = base + threadIdx.x;
    long long total;
    const long long before =
        block_exclusive_scan<kBlock>(i < groups ? ws.blocks[i] : 0, &total);
    if (i < groups) ws.first[i] = carry + before;
    carry += total;
  }
  if (threadIdx.x == 0) ws.head[3] = (u64)carry;
}

// ---- unpacking: the storing pass --------------------------------------------
__global__ __launch_bounds__(kBlock) void unpack_store_kernel(
    const uint8_t* __restrict__ seg, int64_t seg_bytes,
    const uint8_t* __restrict__ slot_dc, const uint8_t* __restrict__ slot_ac,
    int nslots, UnpackLayout ws, int32_t* __restrict__ levels, int64_t rows) {
  __shared__ GroupShared sh;
  const int64_t g = blockIdx.x;
  if (ws.first[g] >= rows) return;   // uniform
  const int64_t base = g * kGroupBytes;
  stage_group(sh, seg, seg_bytes, base, ws);
  const Slots slots(slot_dc, slot_ac, nslots);
  __syncthreads();
  const int tid = threadIdx.x;
  const int64_t left = seg_bytes - base;
  const int lanes = (int)(left < kGroupBytes ? ceil_div(left, kSubseqBytes)
                                             : kBlock);
  if (tid >= lanes) return;
  const int end = (int)(left * 8 < (int64_t)(tid + 1) * kSubseqBits
                            ? left * 8
                            : (int64_t)(tid + 1) * kSubseqBits);
  const int64_t sub = g * kBlock + tid;
  int64_t row = ws.first[g] + ws.before[sub];
  State s = State::unpack(ws.entry[sub]);
  Window win;
  win.words = sh.words;
  win.at = -2;
  bool reported = false;
  while (s.p < end && row < rows) {   // 0 <= row < rows at every store
    const int at = s.p;
    const Token t = step(sh, win, s, slots);
    if (t.index >= 0 && t.value != 0) levels[row * 64 + t.index] = t.value;
    if (t.malformed && !reported) {
      reported = true;
      atomicMin(&ws.head[0], (u64)(base * 8 + at) + 1ull);
      atomicMin(&ws.head[1], (u64)sub << 32 | (u64)row);
    }
    if (t.ended) {
      ++row;
      // one lane completes block `rows` on the true path
      if (row == rows) ws.head[2] = (u64)(base * 8 + s.p);
    }
  }
}

__global__ void unpack_end_kernel(UnpackLayout ws, int64_t groups,
                                  int64_t rows, long long* status) {
  const bool bad = ws.head[0] != kNoState64;
  const long long total = (long long)ws.head[3];
  long long rounds = 0;
  for (int64_t l = 0; l < groups; ++l) rounds += ws.rounds[l];
  status[0] = bad ? (long long)ws.head[0] : 0;
  status[1] = bad ? (long long)(ws.head[1] & 0xFFFFFFFFull)
                  : (total < rows ? total : rows);
  status[2] = bad || ws.head[2] == kNoState64 ? -1 : (long long)ws.head[2];
  status[3] = rounds;
}

int check_workspace(const char* who, size_t need, void* workspace,
                    size_t workspace_bytes) {
  if (need && (!workspace || workspace_bytes < need)) {
    set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
              need);
    return VTC_ERR_WORKSPACE;
  }
  return VTC_OK;
}

}  // namespace
}  // namespace vtc

using namespace vtc;

extern "C" int vtc_jfif_decode_abi_version(void) {
  return VTC_JFIF_DECODE_ABI_VERSION;
}

extern "C" size_t vtc_jfif_unstuff_bytes_workspace_bytes(int64_t n) {
  if (n <= 0) return 0;
  return measured_bytes<UnstuffLayout>(n);
}

extern "C" int vtc_jfif_unstuff_bytes(const uint8_t* in, int64_t n,
                                      uint8_t* out, int64_t capacity,
                                      int64_t* out_len, int32_t* status,
                                      void* workspace, size_t workspace_bytes,
                                      void* stream) {
  const char* who = "vtc_jfif_unstuff_bytes";
  VTC_REQUIRE(out_len && status, "%s: null pointer", who);
  VTC_REQUIRE(n >= 0 && n < (int64_t)1 << 40, "%s: bad size n = %lld", who,
              (long long)n);
  VTC_REQUIRE(capacity >= 0 && capacity < (int64_t)1 << 41,
              "%s: bad size capacity = %lld", who, (long long)capacity);
  VTC_REQUIRE((in || n == 0) && (out || capacity == 0), "%s: null pointer",
              who);
  if (n > 0 && capacity > 0) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(in);
    const uintptr_t b = reinterpret_cast<uintptr_t>(out);
    VTC_REQUIRE(a + (uintptr_t)n <= b || b + (uintptr_t)capacity <= a,
                "%s: out overlaps in", who);
  }
  const int64_t tiles = ceil_div(n, VTC_JFIF_STUFF_TILE);
  const size_t need = vtc_jfif_unstuff_bytes_workspace_bytes(n);
  const int rc = check_workspace(who, need, workspace, workspace_bytes);
  if (rc != VTC_OK) return rc;
  Carver carve(need ? workspace : nullptr);
  const UnstuffLayout ws(carve, n);
  hipStream_t st = as_stream(stream);
  if (tiles)
    unstuff_tile_kernel<<<(int)tiles, kBlock, 0, st>>>(in, n, ws);
  unstuff_scan_kernel<<<1, kBlock, 0, st>>>(
      in, n, ws, tiles, capacity, reinterpret_cast<long long*>(out_len),
      status);
  if (tiles && capacity > 0)
    unstuff_write_kernel<<<(int)tiles, kBlock, 0, st>>>(in, n, ws, out,
                                                        capacity);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" size_t vtc_jfif_unpack_workspace_bytes(int64_t seg_bytes) {
  if (seg_bytes <= 0 || seg_bytes >= (int64_t)1 << 31) return 0;
  return measured_bytes<UnpackLayout>(seg_bytes);
}

extern "C" int vtc_jfif_unpack(const uint8_t* seg, int64_t seg_bytes,
                               const uint8_t* slot_dc, const uint8_t* slot_ac,
                               int32_t nslots, const uint16_t* ac_code,
                               const uint8_t* ac_len, const uint16_t* dc_code,
                               const uint8_t* dc_len, int32_t* levels,
                               int64_t rows, int64_t* status, void* workspace,
                               size_t workspace_bytes, void* stream) {
  const char* who = "vtc_jfif_unpack";
  VTC_REQUIRE(seg && slot_dc && slot_ac && ac_code && ac_len && dc_code &&
                  dc_len && levels && status, "%s: null pointer", who);
  VTC_REQUIRE(seg_bytes >= 1 && seg_bytes < (int64_t)1 << 31,
              "%s: bad size seg_bytes = %lld", who, (long long)seg_bytes);
  VTC_REQUIRE(nslots >= 1 && nslots <= VTC_JFIF_MAX_SLOTS,
              "%s: bad size nslots = %d (1 .. %d)", who, nslots,
              VTC_JFIF_MAX_SLOTS);
  VTC_REQUIRE(rows >= 1 && rows < (int64_t)1 << 31,
              "%s: bad size rows = %lld", who, (long long)rows);
  const size_t need = vtc_jfif_unpack_workspace_bytes(seg_bytes);
  const int rc = check_workspace(who, need, workspace, workspace_bytes);
  if (rc != VTC_OK) return rc;
  Carver carve(workspace);
  const UnpackLayout ws(carve, seg_bytes);
  const int64_t groups = ceil_div(seg_bytes, kGroupBytes);   // <= 65536
  hipStream_t st = as_stream(stream);
  VTC_HIP_CHECK(hipMemsetAsync(levels, 0, (size_t)rows * 64 * sizeof(int32_t),
                               st));
  unpack_tables_kernel<<<1, kBlock, 0, st>>>(ac_code, ac_len, dc_code, dc_len,
                                             ws, groups);
  // launch l makes workgroups 0 .. l final; a workgroup that is final already
  // leaves at once.  No host read: the call only enqueues.
  for (int64_t launch = 0; launch < groups; ++launch)
    unpack_sync_kernel<<<(int)groups, kBlock, 0, st>>>(
        seg, seg_bytes, slot_dc, slot_ac, nslots, ws, groups, (int)launch);
  unpack_scan_kernel<<<1, kBlock, 0, st>>>(ws, groups);
  unpack_store_kernel<<<(int)groups, kBlock, 0, st>>>(
      seg, seg_bytes, slot_dc, slot_ac, nslots, ws, levels, rows);
  unpack_end_kernel<<<1, 1, 0, st>>>(ws, groups, rows,
                                     reinterpret_cast<long long*>(status));
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" size_t vtc_jfif_dc_accumulate_workspace_bytes(int64_t d) {
  if (d <= 0) return 0;
  return measured_bytes<DcLayout>(d);
}

extern "C" int vtc_jfif_dc_accumulate(int32_t* levels, int64_t d,
                                      const int32_t* order,
                                      const uint8_t* start, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  const char* who = "vtc_jfif_dc_accumulate";
  VTC_REQUIRE(levels && order && start, "%s: null pointer", who);
  VTC_REQUIRE(d >= 1 && d < (int64_t)1 << 31, "%s: bad size d = %lld", who,
              (long long)d);
  const size_t need = vtc_jfif_dc_accumulate_workspace_bytes(d);
  const int rc = check_workspace(who, need, workspace, workspace_bytes);
  if (rc != VTC_OK) return rc;
  Carver carve(workspace);
  const DcLayout ws(carve, d);
  const int64_t tiles = ceil_div(d, VTC_JFIF_DC_TILE);
  hipStream_t st = as_stream(stream);
  dc_tile_kernel<<<(int)tiles, kBlock, 0, st>>>(levels, d, order, start, ws);
  dc_scan_kernel<<<1, kBlock, 0, st>>>(ws, tiles);
  dc_write_kernel<<<(int)tiles, kBlock, 0, st>>>(levels, d, order, start, ws);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}
