// Range coding (rANS) of ONE index column of up to 131 072 symbols on the
// device (include/ext/vtc_index_ans_split.h): stream sizes, the packed streams and
// the way back.  DESIGN.md 4.21 states the code; the header is the contract.
//
// The coder is that of index_ans.hip with every index i coded
// as two symbols under the same lane state: hi = i >> 8 under freq_hi [H] and
// lo = i & 255 under row hi of freq_lo (H, 256), H = ceil(kmax / 256) <= 512.
// ONE WAVE codes ONE STREAM: in step q lane l holds position 64 q + l, the
// step's 64 indices are consecutive in memory, and the words of a phase go to
// consecutive places in lane order (ballot + popcount of the lower lanes).
// 256-thread blocks, 4 streams.
//
// Launches per call, all on the caller's stream:
//   1. split_begin_kernel: status and the workspace's bad-table word
//   2. split_cum_kernel, one block per table row (the hi row, then the H lo
//      rows): exclusive integer scan of the row's frequencies into the
//      workspace, and the checks of the row
//   3. split_encode_kernel<stores> or split_decode_kernel
//   4. split_end_kernel: status[1] and the bad-table word into status[2]
// (vtc_index_ans_split_pack zero-fills `packed` first.)
//
// The encoder walks the steps from last to first and codes lo, then hi, in
// each; what it measures (sizes) and what it writes (pack) is one function,
// the stores a template flag.  A step's fetch (index, then the two frequencies
// and cumulative sums gathered from global memory) does not depend on the
// states, so the next step's fetch is issued before the current step's
// arithmetic.  The decoder's phase B depends on its phase A within a lane (the
// row of the lo table is the decoded hi): that is the code, not a defect.  Its
// hi table (frequencies and cumulative sums, 2 KiB) is staged in LDS once per
// block; the 256 KiB of lo tables stay in global memory, where every stream
// reads the same rows.  Both searches are plain binary searches, at most 9
// probes over the H hi symbols and 8 over the 256 lo symbols; no bucket index
// as 4.19's is built (DESIGN.md 4.21 says why).
#include <limits.h>

#include "../../include/ext/vtc_index_ans_split.h"
#include "common.h"

namespace vtc {
namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / 64;
constexpr int kMaxSymbols = VTC_INDEX_ANS_SPLIT_MAX_SYMBOLS;
constexpr int kLoBits = VTC_INDEX_ANS_SPLIT_LO_BITS;
constexpr int kLoSymbols = 1 << kLoBits;                // 256
constexpr int kMaxHi = kMaxSymbols / kLoSymbols;        // 512
constexpr int kProbBits = VTC_INDEX_ANS_PROB_BITS;
constexpr unsigned kProbScale = 1u << kProbBits;
constexpr unsigned kLower = 1u << 16;            // L
constexpr int kHeaderBytes = 4 * VTC_INDEX_ANS_LANES;
constexpr int64_t kMaxStreamSymbols = (int64_t)1 << VTC_INDEX_ANS_MAX_STREAM_BITS;
constexpr int kBadHi = 1;        // status[2] of a bad freq_hi; 2 + h of a row
typedef unsigned long long u64;
constexpr u64 kNoPosition = ~0ull;

static_assert(VTC_INDEX_ANS_LANES == 64, "one wave codes one stream");
static_assert(kLoSymbols == kBlock, "split_cum_kernel: one thread per lo symbol");
static_assert(kMaxHi <= 2 * kBlock, "split_cum_kernel: two hi symbols a thread");

__host__ __device__ constexpr int hi_symbols(int kmax) {
  return (kmax + kLoSymbols - 1) >> kLoBits;
}

struct SplitLayout {
  uint16_t* cum_hi;   // [H] exclusive cumulative sums of freq_hi
  uint16_t* cum_lo;   // [H * 256] the same of every row of freq_lo
  int32_t* bad;       // [1] the bad-table word, INT_MAX when none
  SplitLayout(Carver& c, int kmax) {
    const int h = hi_symbols(kmax);
    cum_hi = c.take<uint16_t>((size_t)h);
    cum_lo = c.take<uint16_t>((size_t)h * kLoSymbols);
    bad = c.take<int32_t>(1);
  }
};

__global__ void split_begin_kernel(SplitLayout ws, u64* status) {
  *ws.bad = INT_MAX;
  status[0] = 0;
  status[1] = kNoPosition;   // minimum of rows or streams
  status[2] = 0;
}

__global__ void split_end_kernel(SplitLayout ws, u64* status) {
  status[1] = status[1] == kNoPosition ? 0 : status[1] + 1;
  const int bad = *ws.bad;
  if (bad != INT_MAX) status[2] = (u64)bad;
}

// ---- tables -------------------------------------------------------------------
// The largest i in [lo, hi] with cum[i] <= slot, given cum[lo] <= slot; at most
// ceil(log2(hi - lo + 1)) probes.
__device__ __forceinline__ int symbol_of(const uint16_t* cum, int lo, int hi,
                                         unsigned slot) {
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cum[mid] <= slot)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// Block 0 scans freq_hi (H <= 512 symbols, at most two a thread), block 1 + h
// row h of freq_lo (256 symbols, one a thread); the 256 partial sums are
// scanned in LDS (Hillis-Steele, 8 rounds).  All sums are 32-bit: at most
// 512 * 65535.  The stored uint16 is exact for a row that passes the check
// (its sums are at most 2^15); a bad table's is never read.  A row with
// freq_hi[h] = 0 is neither read nor scanned: no symbol leads to it.
__global__ __launch_bounds__(kBlock) void split_cum_kernel(
    const uint16_t* __restrict__ freq_hi, const uint16_t* __restrict__ freq_lo,
    int kmax, SplitLayout ws) {
  __shared__ unsigned part[2][kBlock];
  __shared__ int past;   // a lo row's nonzero entries at or beyond kmax
  const int tid = threadIdx.x;
  const bool is_hi = blockIdx.x == 0;
  const int row = (int)blockIdx.x - 1;
  if (!is_hi && freq_hi[row] == 0) return;   // the whole block
  const int length = is_hi ? hi_symbols(kmax) : kLoSymbols;
  const uint16_t* freq = is_hi ? freq_hi : freq_lo + row * kLoSymbols;
  uint16_t* cum = is_hi ? ws.cum_hi : ws.cum_lo + row * kLoSymbols;
  const int per = (length + kBlock - 1) / kBlock;
  const int from = tid * per;
  const int to = from + per < length ? from + per : length;
  if (tid == 0) past = 0;
  unsigned own = 0;
  bool beyond = false;
  for (int i = from; i < to; ++i) {
    const unsigned f = freq[i];
    own += f;
    if (!is_hi && f != 0 && row * kLoSymbols + i >= kmax) beyond = true;
  }
  part[0][tid] = own;
  __syncthreads();
  if (beyond) past = 1;   // every writer stores the same value
  int in = 0;
  for (int off = 1; off < kBlock; off <<= 1) {
    unsigned v = part[in][tid];
    if (tid >= off) v += part[in][tid - off];
    part[in ^ 1][tid] = v;
    in ^= 1;
    __syncthreads();
  }
  unsigned run = part[in][tid] - own;   // exclusive
  for (int i = from; i < to; ++i) {
    cum[i] = (uint16_t)run;
    run += freq[i];
  }
  if (tid == kBlock - 1 && (part[in][tid] != kProbScale || past))
    atomicMin(ws.bad, is_hi ? kBadHi : kBadHi + 1 + row);
}

// ---- shared pieces --------------------------------------------------------------
struct StreamSpan {
  int64_t base;   // row of the stream's first symbol
  int count;      // its symbols, 1 .. 2^24
  int steps;      // ceil(count / 64)
};

__device__ __forceinline__ StreamSpan stream_span(int64_t s, int64_t b,
                                                  int rows) {
  StreamSpan span;
  span.base = s * rows;
  const int64_t left = b - span.base;
  span.count = (int)(left < rows ? left : rows);   // <= 2^24
  span.steps = (span.count + 63) >> 6;
  return span;
}

__device__ __forceinline__ unsigned lower_lanes(u64 mask, int lane) {
  return (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
}

__device__ __forceinline__ u64 wave_min_u64(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const u64 o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ---- encoding -------------------------------------------------------------------
// What a lane needs of one step.  f_hi == 0: nothing to code (idle or
// uncodable); a codable entry has both frequencies above 0.
struct Entry {
  unsigned f_hi, c_hi, f_lo, c_lo;
  bool uncodable;
};

__device__ __forceinline__ Entry fetch(const int32_t* __restrict__ indices,
                                       const uint16_t* __restrict__ freq_hi,
                                       const uint16_t* __restrict__ freq_lo,
                                       const SplitLayout& ws, int kmax,
                                       const StreamSpan& span, int t) {
  Entry e = {0u, 0u, 0u, 0u, false};
  if (t >= span.count) return e;
  const int32_t index = indices[span.base + t];
  if ((unsigned)index < (unsigned)kmax) {   // index < H * 256
    const int hi = index >> kLoBits;
    const unsigned f_hi = freq_hi[hi];
    if (f_hi != 0) {   // the row was scanned
      e.f_lo = freq_lo[index];
      e.c_lo = ws.cum_lo[index];
      if (e.f_lo != 0) {
        e.f_hi = f_hi;
        e.c_hi = ws.cum_hi[hi];
      }
    }
  }
  e.uncodable = e.f_hi == 0;
  return e;
}

// One phase of one step of a stream's encoder: the lanes with f != 0 code the
// symbol (f, c); the words they emit lie in front of everything emitted so
// far, in lane order.
template <bool kStore>
__device__ __forceinline__ void encode_phase(unsigned f, unsigned c,
                                             unsigned& x, int& cursor,
                                             uint8_t* slot, int room, int lane,
                                             bool& strayed) {
  const bool emit = f != 0 && (u64)x >= ((u64)f << (kProbBits + 2));
  const u64 mask = __ballot(emit);
  cursor -= __popcll(mask);
  if (emit) {
    if (kStore) {
      const int w = cursor + (int)lower_lanes(mask, lane);
      if (w >= 0 && w < room) {
        uint8_t* at = slot + kHeaderBytes + 2 * (int64_t)w;
        at[0] = (uint8_t)x;
        at[1] = (uint8_t)(x >> 8);
      } else {
        strayed = true;
      }
    }
    x >>= 16;
  }
  if (f != 0) x = ((x / f) << kProbBits) + x % f + c;
}

template <bool kStore>
__global__ __launch_bounds__(kBlock) void split_encode_kernel(
    const int32_t* __restrict__ indices, int64_t b,
    const uint16_t* __restrict__ freq_hi, const uint16_t* __restrict__ freq_lo,
    int kmax, int rows, int64_t streams, SplitLayout ws,
    int32_t* __restrict__ sizes_out, const int32_t* __restrict__ sizes_in,
    const int64_t* __restrict__ offsets, uint8_t* __restrict__ packed,
    int64_t packed_bytes, u64* __restrict__ status) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  if (s >= streams) return;   // the whole wave
  if (*ws.bad != INT_MAX) {   // nothing is coded
    if (!kStore && lane == 0) sizes_out[s] = 0;
    return;
  }
  const StreamSpan span = stream_span(s, b, rows);

  // pack: the slot, and the words the caller's size leaves room for
  uint8_t* slot = nullptr;
  int room = 0;       // words
  bool strayed = false;
  if (kStore) {
    const int64_t from = offsets[s], to = offsets[s + 1];
    const int64_t size = sizes_in[s];
    const bool fits = size >= kHeaderBytes && (size & 1) == 0 && from >= 0 &&
                      from <= packed_bytes - size && from + size <= to;
    if (!fits) {
      if (lane == 0) atomicAdd(&status[2], 1ull);
      return;
    }
    slot = packed + from;
    room = (int)((size - kHeaderBytes) >> 1);
  }

  int t = (span.steps - 1) * 64 + lane;
  unsigned x = kLower;
  int cursor = room;   // pack: words still free in front; sizes: counts down
  int uncodable = 0;
  u64 first = kNoPosition;

  Entry e = fetch(indices, freq_hi, freq_lo, ws, kmax, span, t);
  for (int q = span.steps - 1; q >= 0; --q) {
    const int t_here = t;
    const Entry now = e;
    t -= 64;
    if (q > 0) e = fetch(indices, freq_hi, freq_lo, ws, kmax, span, t);

    if (now.uncodable) {
      ++uncodable;
      first = (u64)(span.base + t_here);   // steps descend: the last one kept
    }                                      // is the smallest
    // the decoder reads hi first, so the encoder codes lo first
    const unsigned f_lo = now.f_hi != 0 ? now.f_lo : 0u;
    encode_phase<kStore>(f_lo, now.c_lo, x, cursor, slot, room, lane, strayed);
    encode_phase<kStore>(now.f_hi, now.c_hi, x, cursor, slot, room, lane,
                         strayed);
  }

  if (kStore) {
    uint8_t* at = slot + 4 * lane;   // room >= 0: the header is inside the slot
    at[0] = (uint8_t)x;
    at[1] = (uint8_t)(x >> 8);
    at[2] = (uint8_t)(x >> 16);
    at[3] = (uint8_t)(x >> 24);
    // words lost at the front, or a size larger than the coder's own
    if (__ballot(strayed || cursor != 0) && lane == 0)
      atomicAdd(&status[2], 1ull);
  } else if (lane == 0) {
    sizes_out[s] = kHeaderBytes - 2 * cursor;   // cursor = -words
  }

  const int count = wave_sum_int(uncodable);
  if (count) {   // the whole wave
    first = wave_min_u64(first);
    if (lane == 0) {
      atomicAdd(&status[0], (u64)count);
      atomicMin(&status[1], first);
    }
  }
}

// ---- decoding -------------------------------------------------------------------
__device__ __forceinline__ unsigned load_le(const uint8_t* __restrict__ at,
                                            int bytes) {
  unsigned v = 0;
  for (int i = 0; i < bytes; ++i) v |= (unsigned)at[i] << (8 * i);
  return v;
}

// The renormalisation of one phase: the lanes with `need` take the next words
// in lane order.  False when the slot has too few: the whole wave stops.
__device__ __forceinline__ bool refill(bool need, unsigned& x, int& cursor,
                                       const uint8_t* __restrict__ slot,
                                       int room, int lane) {
  const u64 mask = __ballot(need);
  const int taken = __popcll(mask);
  if (cursor + taken > room) return false;
  if (need) {
    const int w = cursor + (int)lower_lanes(mask, lane);   // < room
    x = x << 16 | load_le(slot + kHeaderBytes + 2 * (int64_t)w, 2);
  }
  cursor += taken;
  return true;
}

__global__ __launch_bounds__(kBlock) void split_decode_kernel(
    const uint8_t* __restrict__ packed, int64_t packed_bytes,
    const int64_t* __restrict__ offsets, int64_t b,
    const uint16_t* __restrict__ freq_hi, const uint16_t* __restrict__ freq_lo,
    int kmax, int rows, int64_t streams, SplitLayout ws,
    int32_t* __restrict__ indices, int32_t* __restrict__ used_bytes,
    u64* __restrict__ status) {
  __shared__ uint16_t hi_freq[kMaxHi];
  __shared__ uint16_t hi_cum[kMaxHi];
  const bool decoding = *ws.bad == INT_MAX;
  const int top = hi_symbols(kmax);   // H <= kMaxHi
  if (decoding)   // the block's hi table; a bad table's sums are not read
    for (int i = threadIdx.x; i < top; i += kBlock) {
      hi_freq[i] = freq_hi[i];
      hi_cum[i] = ws.cum_hi[i];
    }
  __syncthreads();

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  if (s >= streams) return;   // the whole wave
  const StreamSpan span = stream_span(s, b, rows);

  const int64_t from = offsets[s], next = offsets[s + 1];
  const int64_t stop = next < packed_bytes ? next : packed_bytes;
  bool malformed = false;
  bool alive = decoding;
  int room = 0;   // words of the slot
  if (decoding && (from < 0 || from > next || stop - from < kHeaderBytes)) {
    malformed = true;
    alive = false;
  }
  const uint8_t* slot = packed;
  unsigned x = kLower;
  const bool opened = alive;   // the header is inside the slot
  if (opened) {
    slot = packed + from;
    // a slot holds at most 2^25 words that a stream can use
    const int64_t words = (stop - from - kHeaderBytes) >> 1;
    room = words < 2 * kMaxStreamSymbols ? (int)words
                                         : (int)(2 * kMaxStreamSymbols);
    x = load_le(slot + 4 * lane, 4);
  }

  int t = lane;
  int cursor = 0;
  for (int q = 0; q < span.steps; ++q) {
    const bool active = t < span.count;
    const int before = cursor;   // a step that runs dry reads nothing
    int32_t symbol = -1;
    if (alive) {
      int hi = 0;
      bool need = false;
      if (active) {   // phase A
        const unsigned at = x & (kProbScale - 1);
        hi = symbol_of(hi_cum, 0, top - 1, at);
        // hi_freq[hi] > 0: the sum is 2^15
        x = hi_freq[hi] * (x >> kProbBits) + at - hi_cum[hi];   // < 2^32
        need = x < kLower;
      }
      alive = refill(need, x, cursor, slot, room, lane);
      need = false;
      if (alive && active) {   // phase B: row hi was scanned and checked
        const int row = hi << kLoBits;
        const unsigned at = x & (kProbScale - 1);
        const int lo = symbol_of(ws.cum_lo + row, 0, kLoSymbols - 1, at);
        x = freq_lo[row + lo] * (x >> kProbBits) + at - ws.cum_lo[row + lo];
        need = x < kLower;
        symbol = row + lo;   // < kmax: the row is 0 from kmax on
      }
      if (alive) alive = refill(need, x, cursor, slot, room, lane);
      if (!alive) {   // out of words: the whole wave
        malformed = true;
        symbol = -1;
        cursor = before;
      }
    }
    if (active) indices[span.base + t] = symbol;
    t += 64;
  }

  // the free integrity check; a stream that ran dry is already counted
  if (alive && __ballot(x != kLower)) malformed = true;
  if (lane == 0) {
    used_bytes[s] = opened ? kHeaderBytes + 2 * cursor : 0;
    if (malformed) {
      atomicAdd(&status[0], 1ull);
      atomicMin(&status[1], (u64)s);
    }
  }
}

// VTC_OK when the calls take the shape; sets the error text otherwise.
int check_shape(const char* who, int64_t b, int32_t kmax, int32_t rows,
                int64_t* streams) {
  VTC_REQUIRE(b >= 1, "%s: bad size b = %lld", who, (long long)b);
  VTC_REQUIRE(kmax >= 1, "%s: bad size kmax = %d", who, kmax);
  VTC_REQUIRE(rows >= 1, "%s: bad size rows_per_stream = %d", who, rows);
  if (kmax > kMaxSymbols) {
    set_error("%s: kmax = %d, at most %d", who, kmax, kMaxSymbols);
    return VTC_ERR_UNSUPPORTED;
  }
  if (rows > kMaxStreamSymbols) {
    set_error("%s: rows_per_stream = %d, at most %lld", who, rows,
              (long long)kMaxStreamSymbols);
    return VTC_ERR_UNSUPPORTED;
  }
  *streams = ceil_div(b, rows);
  if (ceil_div(*streams, kWavesPerBlock) >= (int64_t)1 << 31) {
    set_error("%s: b = %lld, too many streams", who, (long long)b);
    return VTC_ERR_UNSUPPORTED;
  }
  return VTC_OK;
}

int check_workspace(const char* who, int32_t kmax, const void* workspace,
                    size_t workspace_bytes) {
  const size_t need = vtc_index_ans_split_workspace_bytes(kmax);
  if (!workspace || workspace_bytes < need) {
    set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
              need);
    return VTC_ERR_WORKSPACE;
  }
  return VTC_OK;
}

}  // namespace
}  // namespace vtc

using namespace vtc;

extern "C" int vtc_index_ans_split_abi_version(void) {
  return VTC_INDEX_ANS_SPLIT_ABI_VERSION;
}

extern "C" size_t vtc_index_ans_split_workspace_bytes(int32_t kmax) {
  if (kmax < 1 || kmax > kMaxSymbols) return 0;
  return measured_bytes<SplitLayout>(kmax);
}

extern "C" int vtc_index_ans_split_sizes(
    const int32_t* indices, int64_t b, const uint16_t* freq_hi,
    const uint16_t* freq_lo, int32_t kmax, int32_t rows_per_stream,
    int32_t* stream_bytes, int64_t* status, void* workspace,
    size_t workspace_bytes, void* stream) {
  const char* who = "vtc_index_ans_split_sizes";
  VTC_REQUIRE(indices && freq_hi && freq_lo && stream_bytes && status,
              "%s: null pointer", who);
  int64_t streams;
  int rc = check_shape(who, b, kmax, rows_per_stream, &streams);
  if (rc != VTC_OK) return rc;
  rc = check_workspace(who, kmax, workspace, workspace_bytes);
  if (rc != VTC_OK) return rc;
  Carver carve(workspace);
  const SplitLayout ws(carve, kmax);
  hipStream_t st = as_stream(stream);
  u64* flags = reinterpret_cast<u64*>(status);
  const int blocks = (int)ceil_div(streams, kWavesPerBlock);
  split_begin_kernel<<<1, 1, 0, st>>>(ws, flags);
  split_cum_kernel<<<1 + hi_symbols(kmax), kBlock, 0, st>>>(freq_hi, freq_lo,
                                                            kmax, ws);
  split_encode_kernel<false><<<blocks, kBlock, 0, st>>>(
      indices, b, freq_hi, freq_lo, kmax, rows_per_stream, streams, ws,
      stream_bytes, nullptr, nullptr, nullptr, 0, flags);
  split_end_kernel<<<1, 1, 0, st>>>(ws, flags);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" int vtc_index_ans_split_pack(
    const int32_t* indices, int64_t b, const uint16_t* freq_hi,
    const uint16_t* freq_lo, int32_t kmax, int32_t rows_per_stream,
    const int32_t* stream_bytes, const int64_t* offsets, uint8_t* packed,
    int64_t packed_bytes, int64_t* status, void* workspace,
    size_t workspace_bytes, void* stream) {
  const char* who = "vtc_index_ans_split_pack";
  VTC_REQUIRE(indices && freq_hi && freq_lo && stream_bytes && offsets &&
                  packed && status,
              "%s: null pointer", who);
  int64_t streams;
  int rc = check_shape(who, b, kmax, rows_per_stream, &streams);
  if (rc != VTC_OK) return rc;
  VTC_REQUIRE(packed_bytes >= 0 && packed_bytes < (int64_t)1 << 59,
              "%s: bad size packed_bytes = %lld", who, (long long)packed_bytes);
  rc = check_workspace(who, kmax, workspace, workspace_bytes);
  if (rc != VTC_OK) return rc;
  Carver carve(workspace);
  const SplitLayout ws(carve, kmax);
  hipStream_t st = as_stream(stream);
  u64* flags = reinterpret_cast<u64*>(status);
  const int blocks = (int)ceil_div(streams, kWavesPerBlock);
  if (packed_bytes)
    VTC_HIP_CHECK(hipMemsetAsync(packed, 0, (size_t)packed_bytes, st));
  split_begin_kernel<<<1, 1, 0, st>>>(ws, flags);
  split_cum_kernel<<<1 + hi_symbols(kmax), kBlock, 0, st>>>(freq_hi, freq_lo,
                                                            kmax, ws);
  split_encode_kernel<true><<<blocks, kBlock, 0, st>>>(
      indices, b, freq_hi, freq_lo, kmax, rows_per_stream, streams, ws,
      nullptr, stream_bytes, offsets, packed, packed_bytes, flags);
  split_end_kernel<<<1, 1, 0, st>>>(ws, flags);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" int vtc_index_ans_split_unpack(
    const uint8_t* packed, int64_t packed_bytes, const int64_t* offsets,
    int64_t b, const uint16_t* freq_hi, const uint16_t* freq_lo, int32_t kmax,
    int32_t rows_per_stream, int32_t* indices, int32_t* used_bytes,
    int64_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "vtc_index_ans_split_unpack";
  VTC_REQUIRE(packed && offsets && freq_hi && freq_lo && indices &&
                  used_bytes && status,
              "%s: null pointer", who);
  int64_t streams;
  int rc = check_shape(who, b, kmax, rows_per_stream, &streams);
  if (rc != VTC_OK) return rc;
  VTC_REQUIRE(packed_bytes >= 0 && packed_bytes < (int64_t)1 << 59,
              "%s: bad size packed_bytes = %lld", who, (long long)packed_bytes);
  rc = check_workspace(who, kmax, workspace, workspace_bytes);
  if (rc != VTC_OK) return rc;
  Carver carve(workspace);
  const SplitLayout ws(carve, kmax);
  hipStream_t st = as_stream(stream);
  u64* flags = reinterpret_cast<u64*>(status);
  const int blocks = (int)ceil_div(streams, kWavesPerBlock);
  split_begin_kernel<<<1, 1, 0, st>>>(ws, flags);
  split_cum_kernel<<<1 + hi_symbols(kmax), kBlock, 0, st>>>(freq_hi, freq_lo,
                                                            kmax, ws);
  split_decode_kernel<<<blocks, kBlock, 0, st>>>(
      packed, packed_bytes, offsets, b, freq_hi, freq_lo, kmax,
      rows_per_stream, streams, ws, indices, used_bytes, flags);
  split_end_kernel<<<1, 1, 0, st>>>(ws, flags);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}
