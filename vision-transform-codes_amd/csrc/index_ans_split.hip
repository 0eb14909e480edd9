// Range coding (rANS) of ONE index column of up to 131 072 symbols on the
// device (include/ext/vtc_index_ans_split.h): stream sizes, the packed streams and
// the way back.  DESIGN.md 4.21 states the code; the header is the contract.
//
// The stream format and its coder (one wave codes one stream, the words of a
// phase in lane order) are stated in ans_stream.h, shared with index_ans.hip
// (DESIGN.md 4.19).  This file states the model: every index i is coded as two
// symbols under the same lane state, hi = i >> 8 under freq_hi [H] and
// lo = i & 255 under row hi of freq_lo (H, 256), H = ceil(kmax / 256) <= 512.
// In step q lane l holds position 64 q + l, and the step's 64 indices are
// consecutive in memory.  256-thread blocks, 4 streams.
//
// Launches per call, all on the caller's stream:
//   1. ans_begin_kernel: status and the workspace's bad-table word
//   2. split_cum_kernel, one block per table row (the hi row, then the H lo
//      rows): exclusive integer scan of the row's frequencies into the
//      workspace, and the checks of the row
//   3. split_encode_kernel<stores> or split_decode_kernel
//   4. ans_end_kernel: status[1] and the bad-table word into status[2]
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
#include "../../include/ext/vtc_index_ans_split.h"
#include "ans_stream.h"

namespace vtc {
namespace {

constexpr int kMaxSymbols = VTC_INDEX_ANS_SPLIT_MAX_SYMBOLS;
constexpr int kLoBits = VTC_INDEX_ANS_SPLIT_LO_BITS;
constexpr int kLoSymbols = 1 << kLoBits;                // 256
constexpr int kMaxHi = kMaxSymbols / kLoSymbols;        // 512
constexpr int kBadHi = 1;        // status[2] of a bad freq_hi; 2 + h of a row

static_assert(kLoSymbols == kBlock, "split_cum_kernel: one thread per lo symbol");
static_assert(kMaxHi <= 2 * kBlock, "split_cum_kernel: two hi symbols a thread");

__host__ __device__ constexpr int hi_symbols(int kmax) {
  return (kmax + kLoSymbols - 1) >> kLoBits;
}

struct SplitLayout {
  uint16_t* cum_hi;   // [H] exclusive cumulative sums of freq_hi
  uint16_t* cum_lo;   // [H * 256] the same of every row of freq_lo
  int32_t* bad;       // [1] the bad-table word, INT_MAX when none
  SplitLayout() = default;
  SplitLayout(Carver& c, int kmax) {
    const int h = hi_symbols(kmax);
    cum_hi = c.take<uint16_t>((size_t)h);
    cum_lo = c.take<uint16_t>((size_t)h * kLoSymbols);
    bad = c.take<int32_t>(1);
  }
};

// ---- tables -------------------------------------------------------------------
// Block 0 scans freq_hi (H <= 512 symbols, at most two a thread), block 1 + h
// row h of freq_lo (256 symbols, one a thread), both with scan_row.  A lo row
// is also bad when it has a nonzero entry at or beyond kmax.  A row with
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
  if (tid == 0) past = 0;
  __syncthreads();
  if (!is_hi && freq[tid] != 0 && row * kLoSymbols + tid >= kmax)
    past = 1;   // a lo row has one symbol a thread; all store the same value
  const unsigned total = scan_row(freq, cum, length, part);   // barriers
  if (tid == kBlock - 1 && (total != kProbScale || past))
    atomicMin(ws.bad, is_hi ? kBadHi : kBadHi + 1 + row);
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
  const StreamSpan span = stream_span(s, b, rows, 1);
  EncodeSlot out = {nullptr, 0};
  if (kStore && !open_pack_slot(out, s, sizes_in, offsets, packed,
                                packed_bytes, lane, status))
    return;

  int t = (span.steps - 1) * 64 + lane;
  unsigned x = kLower;
  int cursor = out.room;   // pack: words still free in front; sizes: counts down
  bool strayed = false;
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
    encode_phase<kStore>(f_lo, now.c_lo, x, cursor, out.slot, out.room, lane,
                         strayed);
    encode_phase<kStore>(now.f_hi, now.c_hi, x, cursor, out.slot, out.room,
                         lane, strayed);
  }
  finish_encode<kStore>(x, cursor, strayed, uncodable, first, out.slot, s, lane,
                        sizes_out, status);
}

// ---- decoding -------------------------------------------------------------------
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
  const StreamSpan span = stream_span(s, b, rows, 1);
  unsigned x;
  // a slot holds at most 2^25 words that a stream can use: two per symbol
  const DecodeSlot in = open_decode_slot(decoding, s, offsets, packed,
                                         packed_bytes, 2 * kMaxStreamSymbols,
                                         lane, x);
  bool alive = in.opened;
  bool malformed = decoding && !in.opened;

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
      alive = refill(need, x, cursor, in.slot, in.room, lane);
      need = false;
      if (alive && active) {   // phase B: row hi was scanned and checked
        const int row = hi << kLoBits;
        const unsigned at = x & (kProbScale - 1);
        const int lo = symbol_of(ws.cum_lo + row, 0, kLoSymbols - 1, at);
        x = freq_lo[row + lo] * (x >> kProbBits) + at - ws.cum_lo[row + lo];
        need = x < kLower;
        symbol = row + lo;   // < kmax: the row is 0 from kmax on
      }
      if (alive) alive = refill(need, x, cursor, in.slot, in.room, lane);
      if (!alive) {   // out of words: the whole wave
        malformed = true;
        symbol = -1;
        cursor = before;
      }
    }
    if (active) indices[span.base + t] = symbol;
    t += 64;
  }
  finish_decode(alive, malformed, x, in.opened, cursor, s, lane, used_bytes,
                status);
}

// ---- host side ------------------------------------------------------------------
// What an entry point needs for its launches.
struct SplitCall {
  SplitLayout ws;
  int64_t streams;
  int blocks;
  hipStream_t st;
  u64* flags;
};

// The checks that the three calls share, in their order (shape, packed_bytes,
// workspace), then the carve.  VTC_OK, or the error with its text set.
int open_call(const char* who, int64_t b, int32_t kmax, int32_t rows,
              int64_t packed_bytes, int64_t* status, void* workspace,
              size_t workspace_bytes, void* stream, SplitCall* call) {
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
  int rc = check_streams(who, b, rows, &call->streams);
  if (rc != VTC_OK) return rc;
  VTC_REQUIRE(packed_bytes >= 0 && packed_bytes < (int64_t)1 << 59,
              "%s: bad size packed_bytes = %lld", who, (long long)packed_bytes);
  rc = check_workspace(who, vtc_index_ans_split_workspace_bytes(kmax),
                       workspace, workspace_bytes);
  if (rc != VTC_OK) return rc;
  Carver carve(workspace);
  call->ws = SplitLayout(carve, kmax);
  call->blocks = (int)ceil_div(call->streams, kWavesPerBlock);
  call->st = as_stream(stream);
  call->flags = reinterpret_cast<u64*>(status);
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
  SplitCall c;   // no packed bytes: 0 passes their check
  const int rc = open_call(who, b, kmax, rows_per_stream, 0, status, workspace,
                           workspace_bytes, stream, &c);
  if (rc != VTC_OK) return rc;
  ans_begin_kernel<<<1, 1, 0, c.st>>>(c.ws.bad, c.flags);
  split_cum_kernel<<<1 + hi_symbols(kmax), kBlock, 0, c.st>>>(freq_hi, freq_lo,
                                                              kmax, c.ws);
  split_encode_kernel<false><<<c.blocks, kBlock, 0, c.st>>>(
      indices, b, freq_hi, freq_lo, kmax, rows_per_stream, c.streams, c.ws,
      stream_bytes, nullptr, nullptr, nullptr, 0, c.flags);
  ans_end_kernel<<<1, 1, 0, c.st>>>(c.ws.bad, c.flags);
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
  SplitCall c;
  const int rc = open_call(who, b, kmax, rows_per_stream, packed_bytes, status,
                           workspace, workspace_bytes, stream, &c);
  if (rc != VTC_OK) return rc;
  if (packed_bytes)
    VTC_HIP_CHECK(hipMemsetAsync(packed, 0, (size_t)packed_bytes, c.st));
  ans_begin_kernel<<<1, 1, 0, c.st>>>(c.ws.bad, c.flags);
  split_cum_kernel<<<1 + hi_symbols(kmax), kBlock, 0, c.st>>>(freq_hi, freq_lo,
                                                              kmax, c.ws);
  split_encode_kernel<true><<<c.blocks, kBlock, 0, c.st>>>(
      indices, b, freq_hi, freq_lo, kmax, rows_per_stream, c.streams, c.ws,
      nullptr, stream_bytes, offsets, packed, packed_bytes, c.flags);
  ans_end_kernel<<<1, 1, 0, c.st>>>(c.ws.bad, c.flags);
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
  SplitCall c;
  const int rc = open_call(who, b, kmax, rows_per_stream, packed_bytes, status,
                           workspace, workspace_bytes, stream, &c);
  if (rc != VTC_OK) return rc;
  ans_begin_kernel<<<1, 1, 0, c.st>>>(c.ws.bad, c.flags);
  split_cum_kernel<<<1 + hi_symbols(kmax), kBlock, 0, c.st>>>(freq_hi, freq_lo,
                                                              kmax, c.ws);
  split_decode_kernel<<<c.blocks, kBlock, 0, c.st>>>(
      packed, packed_bytes, offsets, b, freq_hi, freq_lo, kmax,
      rows_per_stream, c.streams, c.ws, indices, used_bytes, c.flags);
  ans_end_kernel<<<1, 1, 0, c.st>>>(c.ws.bad, c.flags);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}
