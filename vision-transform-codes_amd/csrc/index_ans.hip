// Range coding (rANS) of quantiser indices on the device
// (include/vtc_index_ans.h): stream sizes, the packed streams and the way back.
// DESIGN.md 4.19 states the code; the header is the contract.
//
// The stream format and its coder (one wave codes one stream, the words of a
// step in lane order) are stated in ans_stream.h.  This file states the model:
// m columns with one frequency table each, position t of a stream under the
// table of column t % m.  In step q lane l holds position 64 q + l, so the
// step's 64 indices are consecutive in memory (one coalesced access) and a
// lane's column moves by 64 % m per step.  256-thread blocks, 4 streams.
//
// Launches per call, all on the caller's stream:
//   1. ans_begin_kernel: status and the workspace's bad-column word
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
#include "ans_stream.h"

namespace vtc {
namespace {

constexpr int kMaxColumns = VTC_INDEX_CODE_MAX_COLUMNS;
constexpr int kMaxSymbols = VTC_INDEX_CODE_MAX_SYMBOLS;
constexpr int kBucketBits = VTC_INDEX_ANS_BUCKET_BITS;
constexpr int kBuckets = 1 << kBucketBits;             // of a column's 2^15 slots
constexpr int kBucketShift = kProbBits - kBucketBits;

static_assert(kBuckets == kBlock, "ans_cum_kernel: one thread per bucket");

struct IndexAnsLayout {
  uint16_t* cum;   // [m * kmax] exclusive cumulative sums, column j from j * kmax
  uint16_t* first; // [m * kBuckets] the symbol of a bucket's first slot
  int32_t* bad;    // [1] 1 + the smallest bad column, INT_MAX when none
  IndexAnsLayout() = default;
  IndexAnsLayout(Carver& c, int m, int kmax) {
    cum = c.take<uint16_t>((size_t)m * kmax);
    first = c.take<uint16_t>((size_t)m * kBuckets);
    bad = c.take<int32_t>(1);
  }
};

// ---- tables -------------------------------------------------------------------
// The column's scan (scan_row); then thread g finds the symbol of slot
// g << kBucketShift, the decoder's way in: the symbol of any slot of bucket g
// lies between first[g] and first[g + 1], which for the large frequencies of a
// sparse model are equal.
__global__ __launch_bounds__(kBlock) void ans_cum_kernel(
    const uint16_t* __restrict__ freq, int kmax, IndexAnsLayout ws) {
  __shared__ unsigned part[2][kBlock];
  const int tid = threadIdx.x;
  const int column = blockIdx.x;
  const int base = column * kmax;   // < 4096 * 4096
  const unsigned total = scan_row(freq + base, ws.cum + base, kmax, part);
  if (tid == kBlock - 1 && total != kProbScale) atomicMin(ws.bad, column + 1);
  __syncthreads();   // the block's cum is in global memory
  ws.first[column * kBuckets + tid] = (uint16_t)symbol_of(
      ws.cum + base, 0, kmax - 1, (unsigned)tid << kBucketShift);
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
  const StreamSpan span = stream_span(s, b, rows, m);
  EncodeSlot out = {nullptr, 0};
  if (kStore && !open_pack_slot(out, s, sizes_in, offsets, packed,
                                packed_bytes, lane, status))
    return;

  const int back = 64 % m;   // a lane's column moves by this much per step
  int t = (span.steps - 1) * 64 + lane;
  int column = t % m;
  unsigned x = kLower;
  int cursor = out.room;   // pack: words still free in front; sizes: counts down
  bool strayed = false;
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
    encode_phase<kStore>(now.f, now.c, x, cursor, out.slot, out.room, lane,
                         strayed);
  }
  finish_encode<kStore>(x, cursor, strayed, uncodable, first, out.slot, s, lane,
                        sizes_out, status);
}

// ---- decoding -------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void ans_decode_kernel(
    const uint8_t* __restrict__ packed, int64_t packed_bytes,
    const int64_t* __restrict__ offsets, int64_t b, int m,
    const uint16_t* __restrict__ freq, int kmax, int rows, int64_t streams,
    IndexAnsLayout ws, int32_t* __restrict__ indices,
    int32_t* __restrict__ used_bytes, u64* __restrict__ status) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  if (s >= streams) return;   // the whole wave
  const StreamSpan span = stream_span(s, b, rows, m);
  const bool decoding = *ws.bad == INT_MAX;
  unsigned x;
  // a slot holds at most 2^24 words that a stream can use
  const DecodeSlot in = open_decode_slot(decoding, s, offsets, packed,
                                         packed_bytes, kMaxStreamSymbols, lane,
                                         x);
  bool alive = in.opened;
  bool malformed = decoding && !in.opened;

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
    if (alive && !refill(need, x, cursor, in.slot, in.room, lane)) {
      alive = false;   // out of words: the whole wave
      malformed = true;
      symbol = -1;
    }
    if (active) indices[span.base + t] = symbol;
    t += 64;
    column += ahead;
    if (column >= m) column -= m;
  }
  finish_decode(alive, malformed, x, in.opened, cursor, s, lane, used_bytes,
                status);
}

// ---- host side ------------------------------------------------------------------
// What an entry point needs for its launches.
struct AnsCall {
  IndexAnsLayout ws;
  int64_t streams;
  int blocks;
  hipStream_t st;
  u64* flags;
};

// The checks that the three calls share, in their order (shape, packed_bytes,
// workspace), then the carve.  VTC_OK, or the error with its text set.
int open_call(const char* who, int64_t b, int32_t m, int32_t kmax, int32_t rows,
              int64_t packed_bytes, int64_t* status, void* workspace,
              size_t workspace_bytes, void* stream, AnsCall* call) {
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
  int rc = check_streams(who, b, rows, &call->streams);
  if (rc != VTC_OK) return rc;
  VTC_REQUIRE(packed_bytes >= 0 && packed_bytes < (int64_t)1 << 59,
              "%s: bad size packed_bytes = %lld", who, (long long)packed_bytes);
  rc = check_workspace(who, vtc_index_ans_workspace_bytes(m, kmax), workspace,
                       workspace_bytes);
  if (rc != VTC_OK) return rc;
  Carver carve(workspace);
  call->ws = IndexAnsLayout(carve, m, kmax);
  call->blocks = (int)ceil_div(call->streams, kWavesPerBlock);
  call->st = as_stream(stream);
  call->flags = reinterpret_cast<u64*>(status);
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
  AnsCall c;   // no packed bytes: 0 passes their check
  const int rc = open_call(who, b, m, kmax, rows_per_stream, 0, status,
                           workspace, workspace_bytes, stream, &c);
  if (rc != VTC_OK) return rc;
  ans_begin_kernel<<<1, 1, 0, c.st>>>(c.ws.bad, c.flags);
  ans_cum_kernel<<<m, kBlock, 0, c.st>>>(freq, kmax, c.ws);
  ans_encode_kernel<false><<<c.blocks, kBlock, 0, c.st>>>(
      indices, b, m, freq, kmax, rows_per_stream, c.streams, c.ws,
      stream_bytes, nullptr, nullptr, nullptr, 0, c.flags);
  ans_end_kernel<<<1, 1, 0, c.st>>>(c.ws.bad, c.flags);
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
  AnsCall c;
  const int rc = open_call(who, b, m, kmax, rows_per_stream, packed_bytes,
                           status, workspace, workspace_bytes, stream, &c);
  if (rc != VTC_OK) return rc;
  if (packed_bytes)
    VTC_HIP_CHECK(hipMemsetAsync(packed, 0, (size_t)packed_bytes, c.st));
  ans_begin_kernel<<<1, 1, 0, c.st>>>(c.ws.bad, c.flags);
  ans_cum_kernel<<<m, kBlock, 0, c.st>>>(freq, kmax, c.ws);
  ans_encode_kernel<true><<<c.blocks, kBlock, 0, c.st>>>(
      indices, b, m, freq, kmax, rows_per_stream, c.streams, c.ws, nullptr,
      stream_bytes, offsets, packed, packed_bytes, c.flags);
  ans_end_kernel<<<1, 1, 0, c.st>>>(c.ws.bad, c.flags);
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
  AnsCall c;
  const int rc = open_call(who, b, m, kmax, rows_per_stream, packed_bytes,
                           status, workspace, workspace_bytes, stream, &c);
  if (rc != VTC_OK) return rc;
  ans_begin_kernel<<<1, 1, 0, c.st>>>(c.ws.bad, c.flags);
  ans_cum_kernel<<<m, kBlock, 0, c.st>>>(freq, kmax, c.ws);
  ans_decode_kernel<<<c.blocks, kBlock, 0, c.st>>>(
      packed, packed_bytes, offsets, b, m, freq, kmax, rows_per_stream,
      c.streams, c.ws, indices, used_bytes, c.flags);
  ans_end_kernel<<<1, 1, 0, c.st>>>(c.ws.bad, c.flags);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}
