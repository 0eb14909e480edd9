// Range coding (rANS) of quantiser indices on the device
// (include/vtc_index_ans.h): stream sizes, the packed streams and the way back.
// DESIGN.md 4.19 states the code; the header is the contract.
//
// A stream carries 64 interleaved states and position t belongs to state
// t % 64, so ONE WAVE codes ONE STREAM whatever m is: in step q lane l holds
// position 64 q + l, the step's 64 indices are consecutive in memory (one
// coalesced access), and the words of a step go to consecutive places in lane
// order (ballot + popcount of the lower lanes).  256-thread blocks, 4 streams.
//
// Launches per call, all on the caller's stream:
//   1. ans_begin_kernel: status and the workspace's bad-column flag
//   2. ans_cum_kernel, one block per column: exclusive integer scan of the
//      column's frequencies into the workspace, and the check of their sum
//   3. ans_encode_kernel<stores> or ans_decode_kernel
//   4. ans_end_kernel: status[1] and the bad column into status[2]
// (vtc_index_ans_pack zero-fills `packed` first.)
//
// The encoder walks the steps from last to first.  What it measures
// (vtc_index_ans_sizes) and what it writes (vtc_index_ans_pack) is one
// function, the stores a template flag.  The fetch of a step (index, then
// frequency and cumulative sum gathered from global memory, where every stream
// reads the same tables) does not depend on the states, so the next step's
// fetch is issued before the current step's arithmetic.  The decoder's symbol
// search is the serial part of its step: a per-column index of 256 buckets
// (the symbol of every 128th slot, built by ans_cum_kernel) bounds it, and a
// binary search over the column's `cum` finishes it, at most 12 probes and
// none where one symbol covers the bucket.
#include <limits.h>

#include "../../include/vtc_index_ans.h"
#include "common.h"

namespace vtc {
namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / 64;
constexpr int kMaxColumns = VTC_INDEX_CODE_MAX_COLUMNS;
constexpr int kMaxSymbols = VTC_INDEX_CODE_MAX_SYMBOLS;
constexpr int kProbBits = VTC_INDEX_ANS_PROB_BITS;
constexpr unsigned kProbScale = 1u << kProbBits;
constexpr unsigned kLower = 1u << 16;            // L
constexpr int kHeaderBytes = 4 * VTC_INDEX_ANS_LANES;
constexpr int64_t kMaxStreamSymbols = (int64_t)1 << VTC_INDEX_ANS_MAX_STREAM_BITS;
constexpr int kBucketBits = VTC_INDEX_ANS_BUCKET_BITS;
constexpr int kBuckets = 1 << kBucketBits;             // of a column's 2^15 slots
constexpr int kBucketShift = kProbBits - kBucketBits;
typedef unsigned long long u64;
constexpr u64 kNoPosition = ~0ull;

static_assert(VTC_INDEX_ANS_LANES == 64, "one wave codes one stream");
static_assert(kBuckets == kBlock, "ans_cum_kernel: one thread per bucket");

struct IndexAnsLayout {
  uint16_t* cum;   // [m * kmax] exclusive cumulative sums, column j from j * kmax
  uint16_t* first; // [m * kBuckets] the symbol of a bucket's first slot
  int32_t* bad;    // [1] smallest bad column, INT_MAX when none
  IndexAnsLayout(Carver& c, int m, int kmax) {
    cum = c.take<uint16_t>((size_t)m * kmax);
    first = c.take<uint16_t>((size_t)m * kBuckets);
    bad = c.take<int32_t>(1);
  }
};

__global__ void ans_begin_kernel(IndexAnsLayout ws, u64* status) {
  *ws.bad = INT_MAX;
  status[0] = 0;
  status[1] = kNoPosition;   // minimum of flat positions or streams
  status[2] = 0;
}

__global__ void ans_end_kernel(IndexAnsLayout ws, u64* status) {
  status[1] = status[1] == kNoPosition ? 0 : status[1] + 1;
  const int bad = *ws.bad;
  if (bad != INT_MAX) status[2] = (u64)bad + 1;
}

// ---- tables -------------------------------------------------------------------
// The largest i in [lo, hi] with cum[i] <= slot, given cum[lo] <= slot; at most
// ceil(log2(hi - lo + 1)) probes, none when lo == hi.
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

// Thread t owns the `per` consecutive symbols from t * per on; the 256 partial
// sums are scanned in LDS (Hillis-Steele, 8 rounds).  All sums are 32-bit: at
// most 4096 * 65535.  The stored uint16 is exact for a column that passes the
// check (its sums are at most 2^15); a bad column's is never read.
// Then thread g finds the symbol of slot g << kBucketShift, the decoder's way
// in: the symbol of any slot of bucket g lies between first[g] and
// first[g + 1], which for the large frequencies of a sparse model are equal.
__global__ __launch_bounds__(kBlock) void ans_cum_kernel(
    const uint16_t* __restrict__ freq, int kmax, IndexAnsLayout ws) {
  __shared__ unsigned part[2][kBlock];
  const int tid = threadIdx.x;
  const int column = blockIdx.x;
  const int base = column * kmax;   // < 4096 * 4096
  const int per = (kmax + kBlock - 1) / kBlock;
  const int from = tid * per;
  const int to = from + per < kmax ? from + per : kmax;
  unsigned own = 0;
  for (int i = from; i < to; ++i) own += freq[base + i];
  part[0][tid] = own;
  __syncthreads();
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
    ws.cum[base + i] = (uint16_t)run;
    run += freq[base + i];
  }
  if (tid == kBlock - 1 && part[in][tid] != kProbScale)
    atomicMin(ws.bad, column);
  __syncthreads();   // the block's cum is in global memory
  ws.first[column * kBuckets + tid] = (uint16_t)symbol_of(
      ws.cum + base, 0, kmax - 1, (unsigned)tid << kBucketShift);
}

// ---- shared pieces --------------------------------------------------------------
struct StreamSpan {
  int64_t base;   // flat position of the stream's first symbol
  int count;      // its symbols, 1 .. 2^24
  int steps;      // ceil(count / 64)
};

__device__ __forceinline__ StreamSpan stream_span(int64_t s, int64_t b, int m,
                                                  int rows) {
  StreamSpan span;
  const int64_t row0 = s * rows;
  const int64_t left = b - row0;
  const int64_t here = left < rows ? left : rows;
  span.base = row0 * m;
  span.count = (int)(here * m);   // <= rows * m <= 2^24
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
// What a lane needs of one step.  f == 0: nothing to code (idle or uncodable).
struct Entry {
  unsigned f, c;
  bool uncodable;
};

__device__ __forceinline__ Entry fetch(const int32_t* __restrict__ indices,
                                       const uint16_t* __restrict__ freq,
                                       const uint16_t* __restrict__ cum,
                                       int kmax, const StreamSpan& span, int t,
                                       int column) {
  Entry e = {0u, 0u, false};
  if (t >= span.count) return e;
  const int32_t index = indices[span.base + t];
  if ((unsigned)index < (unsigned)kmax) {
    const int at = column * kmax + index;   // < 4096 * 4096
    e.f = freq[at];
    e.c = cum[at];
  }
  e.uncodable = e.f == 0;
  return e;
}

template <bool kStore>
__global__ __launch_bounds__(kBlock) void ans_encode_kernel(
    const int32_t* __restrict__ indices, int64_t b, int m,
    const uint16_t* __restrict__ freq, int kmax, int rows, int64_t streams,
    IndexAnsLayout ws, int32_t* __restrict__ sizes_out,
    const int32_t* __restrict__ sizes_in, const int64_t* __restrict__ offsets,
    uint8_t* __restrict__ packed, int64_t packed_bytes,
    u64* __restrict__ status) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  if (s >= streams) return;   // the whole wave
  if (*ws.bad != INT_MAX) {   // nothing is coded
    if (!kStore && lane == 0) sizes_out[s] = 0;
    return;
  }
  const StreamSpan span = stream_span(s, b, m, rows);

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

  const int back = 64 % m;   // a lane's column moves by this much per step
  int t = (span.steps - 1) * 64 + lane;
  int column = t % m;
  unsigned x = kLower;
  int cursor = room;   // pack: words still free in front; sizes: counts down
  int uncodable = 0;
  u64 first = kNoPosition;

  Entry e = fetch(indices, freq, ws.cum, kmax, span, t, column);
  for (int q = span.steps - 1; q >= 0; --q) {
    const int t_here = t;
    const Entry now = e;
    t -= 64;
    column -= back;
    if (column < 0) column += m;
    if (q > 0) e = fetch(indices, freq, ws.cum, kmax, span, t, column);

    if (now.uncodable) {
      ++uncodable;
      first = (u64)(span.base + t_here);   // steps descend: the last
    }                                            // one kept is the smallest
    const bool emit =
        now.f != 0 && (u64)x >= ((u64)now.f << (kProbBits + 2));
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
    if (now.f != 0) x = ((x / now.f) << kProbBits) + x % now.f + now.c;
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

__global__ __launch_bounds__(kBlock) void ans_decode_kernel(
    const uint8_t* __restrict__ packed, int64_t packed_bytes,
    const int64_t* __restrict__ offsets, int64_t b, int m,
    const uint16_t* __restrict__ freq, int kmax, int rows, int64_t streams,
    IndexAnsLayout ws, int32_t* __restrict__ indices,
    int32_t* __restrict__ used_bytes, u64* __restrict__ status) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  if (s >= streams) return;   // the whole wave
  const StreamSpan span = stream_span(s, b, m, rows);
  const bool decoding = *ws.bad == INT_MAX;

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
    // a slot holds at most 2^24 words that a stream can use
    const int64_t words = (stop - from - kHeaderBytes) >> 1;
    room = words < kMaxStreamSymbols ? (int)words : (int)kMaxStreamSymbols;
    x = load_le(slot + 4 * lane, 4);
  }

  const int ahead = 64 % m;
  int t = lane;
  int column = t % m;
  int cursor = 0;
  for (int q = 0; q < span.steps; ++q) {
    const bool active = t < span.count;
    int32_t symbol = -1;
    bool need = false;
    if (alive && active) {
      const uint16_t* cum = ws.cum + column * kmax;
      const uint16_t* first = ws.first + column * kBuckets;
      const unsigned at = x & (kProbScale - 1);
      const unsigned bucket = at >> kBucketShift;
      const int lo = first[bucket];   // cum[lo] <= bucket's first slot <= at
      const int hi = bucket + 1 < kBuckets ? first[bucket + 1] : kmax - 1;
      symbol = symbol_of(cum, lo, hi, at);
      const unsigned f = freq[column * kmax + symbol];   // > 0: the sum is 2^15
      x = f * (x >> kProbBits) + at - cum[symbol];       // < 2^32
      need = x < kLower;
    }
    const u64 mask = __ballot(need);
    const int taken = __popcll(mask);
    if (alive && cursor + taken > room) {   // out of words: the whole wave
      alive = false;
      malformed = true;
      symbol = -1;
    }
    if (alive) {
      if (need) {
        const int w = cursor + (int)lower_lanes(mask, lane);   // < room
        x = x << 16 | load_le(slot + kHeaderBytes + 2 * (int64_t)w, 2);
      }
      cursor += taken;
    }
    if (active) indices[span.base + t] = symbol;
    t += 64;
    column += ahead;
    if (column >= m) column -= m;
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
int check_shape(const char* who, int64_t b, int32_t m, int32_t kmax,
                int32_t rows, int64_t* streams) {
  VTC_REQUIRE(b >= 1, "%s: bad size b = %lld", who, (long long)b);
  VTC_REQUIRE(m >= 1, "%s: bad size m = %d", who, m);
  VTC_REQUIRE(kmax >= 1, "%s: bad size kmax = %d", who, kmax);
  VTC_REQUIRE(rows >= 1, "%s: bad size rows_per_stream = %d", who, rows);
  if (m > kMaxColumns) {
    set_error("%s: m = %d, at most %d", who, m, kMaxColumns);
    return VTC_ERR_UNSUPPORTED;
  }
  if (kmax > kMaxSymbols) {
    set_error("%s: kmax = %d, at most %d", who, kmax, kMaxSymbols);
    return VTC_ERR_UNSUPPORTED;
  }
  if ((int64_t)rows * m > kMaxStreamSymbols) {
    set_error("%s: rows_per_stream * m = %lld, at most %lld", who,
              (long long)rows * m, (long long)kMaxStreamSymbols);
    return VTC_ERR_UNSUPPORTED;
  }
  *streams = ceil_div(b, rows);
  if (ceil_div(*streams, kWavesPerBlock) >= (int64_t)1 << 31) {
    set_error("%s: b = %lld, too many streams", who, (long long)b);
    return VTC_ERR_UNSUPPORTED;
  }
  return VTC_OK;
}

int check_workspace(const char* who, int32_t m, int32_t kmax,
                    const void* workspace, size_t workspace_bytes) {
  const size_t need = vtc_index_ans_workspace_bytes(m, kmax);
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

extern "C" int vtc_index_ans_abi_version(void) {
  return VTC_INDEX_ANS_ABI_VERSION;
}

extern "C" size_t vtc_index_ans_workspace_bytes(int32_t m, int32_t kmax) {
  if (m < 1 || m > kMaxColumns || kmax < 1 || kmax > kMaxSymbols) return 0;
  return measured_bytes<IndexAnsLayout>(m, kmax);
}

extern "C" int vtc_index_ans_sizes(const int32_t* indices, int64_t b,
                                   int32_t m, const uint16_t* freq,
                                   int32_t kmax, int32_t rows_per_stream,
                                   int32_t* stream_bytes, int64_t* status,
                                   void* workspace, size_t workspace_bytes,
                                   void* stream) {
  const char* who = "vtc_index_ans_sizes";
  VTC_REQUIRE(indices && freq && stream_bytes && status, "%s: null pointer",
              who);
  int64_t streams;
  int rc = check_shape(who, b, m, kmax, rows_per_stream, &streams);
  if (rc != VTC_OK) return rc;
  rc = check_workspace(who, m, kmax, workspace, workspace_bytes);
  if (rc != VTC_OK) return rc;
  Carver carve(workspace);
  const IndexAnsLayout ws(carve, m, kmax);
  hipStream_t st = as_stream(stream);
  u64* flags = reinterpret_cast<u64*>(status);
  const int blocks = (int)ceil_div(streams, kWavesPerBlock);
  ans_begin_kernel<<<1, 1, 0, st>>>(ws, flags);
  ans_cum_kernel<<<m, kBlock, 0, st>>>(freq, kmax, ws);
  ans_encode_kernel<false><<<blocks, kBlock, 0, st>>>(
      indices, b, m, freq, kmax, rows_per_stream, streams, ws, stream_bytes,
      nullptr, nullptr, nullptr, 0, flags);
  ans_end_kernel<<<1, 1, 0, st>>>(ws, flags);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" int vtc_index_ans_pack(const int32_t* indices, int64_t b, int32_t m,
                                  const uint16_t* freq, int32_t kmax,
                                  int32_t rows_per_stream,
                                  const int32_t* stream_bytes,
                                  const int64_t* offsets, uint8_t* packed,
                                  int64_t packed_bytes, int64_t* status,
                                  void* workspace, size_t workspace_bytes,
                                  void* stream) {
  const char* who = "vtc_index_ans_pack";
  VTC_REQUIRE(indices && freq && stream_bytes && offsets && packed && status,
              "%s: null pointer", who);
  int64_t streams;
  int rc = check_shape(who, b, m, kmax, rows_per_stream, &streams);
  if (rc != VTC_OK) return rc;
  VTC_REQUIRE(packed_bytes >= 0 && packed_bytes < (int64_t)1 << 59,
              "%s: bad size packed_bytes = %lld", who, (long long)packed_bytes);
  rc = check_workspace(who, m, kmax, workspace, workspace_bytes);
  if (rc != VTC_OK) return rc;
  Carver carve(workspace);
  const IndexAnsLayout ws(carve, m, kmax);
  hipStream_t st = as_stream(stream);
  u64* flags = reinterpret_cast<u64*>(status);
  const int blocks = (int)ceil_div(streams, kWavesPerBlock);
  if (packed_bytes)
    VTC_HIP_CHECK(hipMemsetAsync(packed, 0, (size_t)packed_bytes, st));
  ans_begin_kernel<<<1, 1, 0, st>>>(ws, flags);
  ans_cum_kernel<<<m, kBlock, 0, st>>>(freq, kmax, ws);
  ans_encode_kernel<true><<<blocks, kBlock, 0, st>>>(
      indices, b, m, freq, kmax, rows_per_stream, streams, ws, nullptr,
      stream_bytes, offsets, packed, packed_bytes, flags);
  ans_end_kernel<<<1, 1, 0, st>>>(ws, flags);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

extern "C" int vtc_index_ans_unpack(const uint8_t* packed, int64_t packed_bytes,
                                    const int64_t* offsets, int64_t b,
                                    int32_t m, const uint16_t* freq,
                                    int32_t kmax, int32_t rows_per_stream,
                                    int32_t* indices, int32_t* used_bytes,
                                    int64_t* status, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  const char* who = "vtc_index_ans_unpack";
  VTC_REQUIRE(packed && offsets && freq && indices && used_bytes && status,
              "%s: null pointer", who);
  int64_t streams;
  int rc = check_shape(who, b, m, kmax, rows_per_stream, &streams);
  if (rc != VTC_OK) return rc;
  VTC_REQUIRE(packed_bytes >= 0 && packed_bytes < (int64_t)1 << 59,
              "%s: bad size packed_bytes = %lld", who, (long long)packed_bytes);
  rc = check_workspace(who, m, kmax, workspace, workspace_bytes);
  if (rc != VTC_OK) return rc;
  Carver carve(workspace);
  const IndexAnsLayout ws(carve, m, kmax);
  hipStream_t st = as_stream(stream);
  u64* flags = reinterpret_cast<u64*>(status);
  const int blocks = (int)ceil_div(streams, kWavesPerBlock);
  ans_begin_kernel<<<1, 1, 0, st>>>(ws, flags);
  ans_cum_kernel<<<m, kBlock, 0, st>>>(freq, kmax, ws);
  ans_decode_kernel<<<blocks, kBlock, 0, st>>>(
      packed, packed_bytes, offsets, b, m, freq, kmax, rows_per_stream,
      streams, ws, indices, used_bytes, flags);
  ans_end_kernel<<<1, 1, 0, st>>>(ws, flags);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}
