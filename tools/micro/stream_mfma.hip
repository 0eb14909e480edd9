// How fast can a CU stream dictionary fragments from L2 into MFMA operands
// with the instruction mix of the fused FISTA kernel (csrc/fc_fused.hip), and
// does a second wave per SIMD help?
//
// One workgroup per CU.  Every wave walks its share of a 2 MiB L2-resident
// buffer ("hi" and "lo" fragment arrays, 1 KiB per wave-instruction) through a
// rolling register ring of RING fragment pairs; each pair feeds three
// 32x32x16 f16 MFMAs whose B operands come from LDS (two ds_read_b128 per
// pair, fetched one step ahead) -- exactly steps 1 / 3 of the kernel without
// its epilogue, barriers and exchanges.  Per "phase" a CU moves 256 KiB and
// issues 384 MFMAs (96 per SIMD x 32 cycles = 3072 cycles), whatever WAVES is.
//
// `stream_mfma shape` runs a second experiment instead (further down): the
// same mix on random operands with the wave's 32x32 tile built from 32x32x16
// or from 16x16x32 MFMAs, alternated, with the in-kernel clock of each.
//
//   hipcc --offload-arch=gfx950 -O3 tools/micro/stream_mfma.hip -o tools/micro/stream_mfma
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#define CHECK(x)                                                        \
  do {                                                                  \
    hipError_t e_ = (x);                                                \
    if (e_ != hipSuccess) {                                             \
      printf("%s: %s\n", #x, hipGetErrorString(e_));                    \
      return 1;                                                         \
    }                                                                   \
  } while (0)

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint4 load16(__amdgpu_buffer_rsrc_t rs, unsigned voff,
                                        unsigned soff) {
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0);
  return make_uint4(v[0], v[1], v[2], v[3]);
}

constexpr int kPairsPerPhase = 128;      // 128 pairs x 2 KiB = 256 KiB per CU

template <int WAVES, int RING, bool MFMA>
__global__ __launch_bounds__(64 * WAVES) void mix_kernel(
    const uint4* __restrict__ hi, const uint4* __restrict__ lo, int phases,
    int buffer_pairs, float* out, unsigned long long* cycles) {
  __shared__ __attribute__((aligned(16))) char ldsb[2 * 16896];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < 2 * 16896 / 4; i += 64 * WAVES)
    reinterpret_cast<float*>(ldsb)[i] = 0.001f * (float)(i & 255);
  __syncthreads();
  const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc(
      (void*)hi, 0, buffer_pairs * 1024, 0x00020000);
  const __amdgpu_buffer_rsrc_t rl = __builtin_amdgcn_make_buffer_rsrc(
      (void*)lo, 0, buffer_pairs * 1024, 0x00020000);
  const unsigned voff = (unsigned)lane * 16u;
  constexpr int PER_WAVE = kPairsPerPhase / WAVES;   // pairs per wave and phase
  const int rd = (lane & 31) * 528 + 16 * (lane >> 5);
  f32x16 acc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
  uint4 ring[2][RING];
  // pair j of this wave in phase p sits at fragment ((p % P) * 128 + wave *
  // PER_WAVE + j) of the buffer
  const int buffer_phases = buffer_pairs / kPairsPerPhase;
  auto frag_off = [&](int p, int j) -> unsigned {
    return (unsigned)(((p % buffer_phases) * kPairsPerPhase + wave * PER_WAVE +
                       j) * 1024);
  };
#pragma unroll
  for (int i = 0; i < RING; ++i) {
    ring[0][i] = load16(rh, voff, frag_off(0, i));
    ring[1][i] = load16(rl, voff, frag_off(0, i));
  }
  const unsigned long long t0 = __builtin_readcyclecounter();
  for (int p = 0; p < phases; ++p) {
    uint4 b_next[2];
    b_next[0] = *reinterpret_cast<const uint4*>(ldsb + rd);
    b_next[1] = *reinterpret_cast<const uint4*>(ldsb + 16896 + rd);
#pragma unroll
    for (int j = 0; j < PER_WAVE; ++j) {
      uint4 b[2] = {b_next[0], b_next[1]};
      if (j + 1 < PER_WAVE) {
        b_next[0] =
            *reinterpret_cast<const uint4*>(ldsb + rd + 32 * ((j + 1) & 15));
        b_next[1] = *reinterpret_cast<const uint4*>(ldsb + 16896 + rd +
                                                    32 * ((j + 1) & 15));
      }
      const uint4 ah = ring[0][j % RING], al = ring[1][j % RING];
      if (MFMA) {
        f32x16& a = acc[j & 1];
        a = __builtin_amdgcn_mfma_f32_32x32x16_f16(
            __builtin_bit_cast(f16x8, ah), __builtin_bit_cast(f16x8, b[0]), a,
            0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_32x32x16_f16(
            __builtin_bit_cast(f16x8, ah), __builtin_bit_cast(f16x8, b[1]), a,
            0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_32x32x16_f16(
            __builtin_bit_cast(f16x8, al), __builtin_bit_cast(f16x8, b[0]), a,
            0, 0, 0);
      } else {
        acc[j & 1][0] += __uint_as_float(ah.x ^ al.y ^ b[0].z ^ b[1].w);
      }
      const int jn = j + RING;
      const unsigned off = jn < PER_WAVE ? frag_off(p, jn)
                                         : frag_off(p + 1, jn - PER_WAVE);
      ring[0][j % RING] = load16(rh, voff, off);
      ring[1][j % RING] = load16(rl, voff, off);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  const unsigned long long t1 = __builtin_readcyclecounter();
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) sum += acc[t][e];
#pragma unroll
  for (int i = 0; i < RING; ++i) sum += __uint_as_float(ring[0][i].x ^ ring[1][i].y);
  out[blockIdx.x * blockDim.x + threadIdx.x] = sum;
  if (threadIdx.x == 0) cycles[blockIdx.x] = t1 - t0;
}

template <int WAVES, int RING, bool MFMA>
static int run(int cus, const uint4* hi, const uint4* lo, int buffer_pairs,
               float* out, unsigned long long* cyc) {
  const int phases = 4000;
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  hipLaunchKernelGGL((mix_kernel<WAVES, RING, MFMA>), dim3(cus), dim3(64 * WAVES),
                     0, 0, hi, lo, 50, buffer_pairs, out, cyc);
  CHECK(hipEventRecord(e0));
  hipLaunchKernelGGL((mix_kernel<WAVES, RING, MFMA>), dim3(cus), dim3(64 * WAVES),
                     0, 0, hi, lo, phases, buffer_pairs, out, cyc);
  CHECK(hipEventRecord(e1));
  CHECK(hipEventSynchronize(e1));
  float ms;
  CHECK(hipEventElapsedTime(&ms, e0, e1));
  std::vector<unsigned long long> h(cus);
  CHECK(hipMemcpy(h.data(), cyc, (size_t)cus * 8, hipMemcpyDeviceToHost));
  double mean = 0;
  for (auto c : h) mean += (double)c;
  mean /= cus;
  const double bytes = 256.0 * 1024 * phases;
  printf("%d waves/CU, ring %2d pairs (%3d KiB in flight per CU), %s: %6.0f "
         "cycles per 256 KiB phase = %5.1f B/clk/CU, %.0f MHz, %.2f ms\n",
         WAVES, RING, WAVES * RING * 2, MFMA ? "3 MFMA per pair" : "no MFMA    ",
         mean / phases, bytes / mean, mean / ms / 1e3, ms);
  return 0;
}

// ---------------------------------------------------------------------------
// `stream_mfma shape`: does the MFMA shape move the clock the chip holds?
//
// The same mix at 4 waves and a ring of 8 pairs, on random operands, with the
// 32x32 output tile of a wave computed either by 32x32x16 MFMAs (one pair =
// K 16, 3 MFMAs of 32 cycles) or by four 16x16x32 sub-tiles (two pairs = the
// two 16-row halves of K 32, 12 MFMAs of 16 cycles).  Both arms read the same
// bytes from L2 (one pair per 96 MFMA cycles) and the same bytes from LDS (two
// ds_read_b128 per pair, one step ahead), and hold 32 accumulator registers.
// Every launch stamps s_memtime and s_memrealtime (100 MHz) around its loop:
// their quotient is the clock the kernel ran at.

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <bool TILE16>
__global__ __launch_bounds__(256) void shape_kernel(
    const uint4* __restrict__ hi, const uint4* __restrict__ lo,
    const uint4* __restrict__ operands, int phases, int buffer_pairs, float* out,
    unsigned long long* cycles, unsigned long long* ticks) {
  constexpr int WAVES = 4, RING = 8;
  constexpr int IMG = 32 * 528;            // 32 patch rows of 256 f16 + 16 B pad
  __shared__ __attribute__((aligned(16))) char ldsb[2 * IMG];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < 2 * IMG / 16; i += 64 * WAVES)
    reinterpret_cast<uint4*>(ldsb)[i] = operands[i];
  __syncthreads();
  const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc(
      (void*)hi, 0, buffer_pairs * 1024, 0x00020000);
  const __amdgpu_buffer_rsrc_t rl = __builtin_amdgcn_make_buffer_rsrc(
      (void*)lo, 0, buffer_pairs * 1024, 0x00020000);
  const unsigned voff = (unsigned)lane * 16u;
  constexpr int PER_WAVE = kPairsPerPhase / WAVES;
  const int buffer_phases = buffer_pairs / kPairsPerPhase;
  auto frag_off = [&](int p, int j) -> unsigned {
    return (unsigned)(((p % buffer_phases) * kPairsPerPhase + wave * PER_WAVE +
                       j) * 1024);
  };
  auto refill = [&](uint4 (&ring)[2][RING], int p, int j) {
    const int jn = j + RING;
    const unsigned off = jn < PER_WAVE ? frag_off(p, jn)
                                       : frag_off(p + 1, jn - PER_WAVE);
    ring[0][j % RING] = load16(rh, voff, off);
    ring[1][j % RING] = load16(rl, voff, off);
  };
  uint4 ring[2][RING];
#pragma unroll
  for (int i = 0; i < RING; ++i) {
    ring[0][i] = load16(rh, voff, frag_off(0, i));
    ring[1][i] = load16(rl, voff, frag_off(0, i));
  }
  float sum = 0.f;
  unsigned long long t0, t1, r0, r1;
  if (!TILE16) {
    // B operand of k-step j: patch lane&31, K chunk lane>>5, 32 B per row
    const int rd = (lane & 31) * 528 + 16 * (lane >> 5);
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
    r0 = __builtin_amdgcn_s_memrealtime();
    t0 = __builtin_amdgcn_s_memtime();
    for (int p = 0; p < phases; ++p) {
      uint4 b_next[2];
      b_next[0] = *reinterpret_cast<const uint4*>(ldsb + rd);
      b_next[1] = *reinterpret_cast<const uint4*>(ldsb + IMG + rd);
#pragma unroll
      for (int j = 0; j < PER_WAVE; ++j) {
        uint4 b[2] = {b_next[0], b_next[1]};
        if (j + 1 < PER_WAVE) {
          b_next[0] =
              *reinterpret_cast<const uint4*>(ldsb + rd + 32 * ((j + 1) & 15));
          b_next[1] = *reinterpret_cast<const uint4*>(ldsb + IMG + rd +
                                                      32 * ((j + 1) & 15));
        }
        const uint4 ah = ring[0][j % RING], al = ring[1][j % RING];
        f32x16& a = acc[j & 1];
        a = __builtin_amdgcn_mfma_f32_32x32x16_f16(
            __builtin_bit_cast(f16x8, ah), __builtin_bit_cast(f16x8, b[0]), a,
            0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_32x32x16_f16(
            __builtin_bit_cast(f16x8, ah), __builtin_bit_cast(f16x8, b[1]), a,
            0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_32x32x16_f16(
            __builtin_bit_cast(f16x8, al), __builtin_bit_cast(f16x8, b[0]), a,
            0, 0, 0);
        refill(ring, p, j);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    t1 = __builtin_amdgcn_s_memtime();
    r1 = __builtin_amdgcn_s_memrealtime();
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) sum += acc[t][e];
  } else {
    // B operand of k-step ks (K 32) and patch half n: patch 16n + (lane&15),
    // K chunk q = lane>>4 at 256(q&1) + 128(q>>1) + 16ks of the row: the two
    // halves of a ds_read_b128 lane group sit a multiple of 256 B apart, so the
    // 16 rows of a group keep one 4-bank slot each (row stride 132 dwords)
    const int q = lane >> 4;
    const int rd = (lane & 15) * 528 + 256 * (q & 1) + 128 * (q >> 1);
    f32x4 acc[2][2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[t][m][n][e] = 0.f;
    r0 = __builtin_amdgcn_s_memrealtime();
    t0 = __builtin_amdgcn_s_memtime();
    for (int p = 0; p < phases; ++p) {
      uint4 b_next[2][2];
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        b_next[n][0] =
            *reinterpret_cast<const uint4*>(ldsb + rd + n * 16 * 528);
        b_next[n][1] =
            *reinterpret_cast<const uint4*>(ldsb + IMG + rd + n * 16 * 528);
      }
#pragma unroll
      for (int s = 0; s < PER_WAVE / 2; ++s) {
        uint4 b[2][2] = {{b_next[0][0], b_next[0][1]},
                         {b_next[1][0], b_next[1][1]}};
        // pair 2s + m holds the 16-row half m of this k-step; the six MFMAs of
        // a half alternate between its two accumulators
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          if (s + 1 < PER_WAVE / 2) {
            const int o = rd + m * 16 * 528 + 16 * ((s + 1) & 7);
            b_next[m][0] = *reinterpret_cast<const uint4*>(ldsb + o);
            b_next[m][1] = *reinterpret_cast<const uint4*>(ldsb + IMG + o);
          }
          const int j = 2 * s + m;
          const uint4 ah = ring[0][j % RING], al = ring[1][j % RING];
#pragma unroll
          for (int prod = 0; prod < 3; ++prod)
#pragma unroll
            for (int n = 0; n < 2; ++n) {
              f32x4& a = acc[s & 1][m][n];
              a = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                  __builtin_bit_cast(f16x8, prod == 2 ? al : ah),
                  __builtin_bit_cast(f16x8, b[n][prod == 1]), a, 0, 0, 0);
            }
          refill(ring, p, j);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    t1 = __builtin_amdgcn_s_memtime();
    r1 = __builtin_amdgcn_s_memrealtime();
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int e = 0; e < 4; ++e) sum += acc[t][m][n][e];
  }
#pragma unroll
  for (int i = 0; i < RING; ++i) sum += __uint_as_float(ring[0][i].x ^ ring[1][i].y);
  out[blockIdx.x * blockDim.x + threadIdx.x] = sum;
  if (threadIdx.x == 0) {
    cycles[blockIdx.x] = t1 - t0;
    ticks[blockIdx.x] = r1 - r0;
  }
}

// uniform f16 in (-scale, scale) from a 64-bit LCG: no constant, no zero runs
static void fill_random(std::vector<_Float16>& v, unsigned long long seed,
                        float scale) {
  unsigned long long s = seed;
  for (auto& x : v) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    x = (_Float16)(scale * ((float)(s >> 40) * (2.f / 16777216.f) - 1.f));
  }
}

struct ShapeResult {
  double ms_per_launch, cycles_per_phase, mhz;
};

template <bool TILE16>
static int shape_rep(int cus, const uint4* hi, const uint4* lo, const uint4* ops,
                     int buffer_pairs, float* out, unsigned long long* cyc,
                     unsigned long long* tck, ShapeResult* r) {
  const int phases = 4000, warm_launches = 220, timed_launches = 20;
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  // >= 2 s of back-to-back launches of this arm before anything is read
  for (int i = 0; i < warm_launches; ++i)
    hipLaunchKernelGGL((shape_kernel<TILE16>), dim3(cus), dim3(256), 0, 0, hi, lo,
                       ops, phases, buffer_pairs, out, cyc, tck);
  CHECK(hipEventRecord(e0));
  for (int i = 0; i < timed_launches; ++i)
    hipLaunchKernelGGL((shape_kernel<TILE16>), dim3(cus), dim3(256), 0, 0, hi, lo,
                       ops, phases, buffer_pairs, out, cyc, tck);
  CHECK(hipEventRecord(e1));
  CHECK(hipEventSynchronize(e1));
  float ms;
  CHECK(hipEventElapsedTime(&ms, e0, e1));
  std::vector<unsigned long long> hc(cus), ht(cus);
  CHECK(hipMemcpy(hc.data(), cyc, (size_t)cus * 8, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(ht.data(), tck, (size_t)cus * 8, hipMemcpyDeviceToHost));
  std::vector<double> c(cus), f(cus);
  for (int i = 0; i < cus; ++i) {
    c[i] = (double)hc[i];
    f[i] = 100.0 * (double)hc[i] / (double)ht[i];     // s_memrealtime: 100 MHz
  }
  std::sort(c.begin(), c.end());
  std::sort(f.begin(), f.end());
  r->ms_per_launch = ms / timed_launches;
  r->cycles_per_phase = c[cus / 2] / phases;
  r->mhz = f[cus / 2];
  CHECK(hipEventDestroy(e0));
  CHECK(hipEventDestroy(e1));
  return 0;
}

static int shape_main(int cus) {
  const int buffer_pairs = 1024, reps = 7;
  const size_t frag_elems = (size_t)buffer_pairs * 512, op_elems = 2 * 32 * 264;
  std::vector<_Float16> h_hi(frag_elems), h_lo(frag_elems), h_op(op_elems);
  // hi parts of order one, lo parts 2^-11 of them, as the operand split leaves
  fill_random(h_hi, 1, 1.f);
  fill_random(h_lo, 2, 1.f / 2048.f);
  fill_random(h_op, 3, 1.f);
  for (size_t i = op_elems / 2; i < op_elems; ++i) h_op[i] *= (_Float16)(1.f / 2048.f);
  uint4 *hi, *lo, *ops;
  float* out;
  unsigned long long *cyc, *tck;
  CHECK(hipMalloc(&hi, frag_elems * 2));
  CHECK(hipMalloc(&lo, frag_elems * 2));
  CHECK(hipMalloc(&ops, op_elems * 2));
  CHECK(hipMemcpy(hi, h_hi.data(), frag_elems * 2, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(lo, h_lo.data(), frag_elems * 2, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(ops, h_op.data(), op_elems * 2, hipMemcpyHostToDevice));
  CHECK(hipMalloc(&out, (size_t)cus * 256 * sizeof(float)));
  CHECK(hipMalloc(&cyc, (size_t)cus * 8));
  CHECK(hipMalloc(&tck, (size_t)cus * 8));
  printf("MFMA shape at one 32x32 tile per wave: 4 waves/CU, ring 8 pairs, f16, "
         "random operands, %d CUs\n"
         "each line: 220 warm launches (>= 2 s), then 20 timed; cycles and clock "
         "are medians over workgroups of the last launch\n", cus);
  ShapeResult r32[reps], r16[reps];
  for (int i = 0; i < reps; ++i) {
    if (shape_rep<false>(cus, hi, lo, ops, buffer_pairs, out, cyc, tck, &r32[i]))
      return 1;
    printf("rep %d  32x32x16: %7.3f ms/launch  %6.0f cycles/phase  %4.0f MHz\n", i,
           r32[i].ms_per_launch, r32[i].cycles_per_phase, r32[i].mhz);
    if (shape_rep<true>(cus, hi, lo, ops, buffer_pairs, out, cyc, tck, &r16[i]))
      return 1;
    printf("rep %d  16x16x32: %7.3f ms/launch  %6.0f cycles/phase  %4.0f MHz\n", i,
           r16[i].ms_per_launch, r16[i].cycles_per_phase, r16[i].mhz);
    fflush(stdout);
  }
  auto summary = [&](const char* name, ShapeResult* r, double* med) {
    std::vector<double> w(reps), c(reps), f(reps);
    for (int i = 0; i < reps; ++i) {
      w[i] = r[i].ms_per_launch;
      c[i] = r[i].cycles_per_phase;
      f[i] = r[i].mhz;
    }
    std::sort(w.begin(), w.end());
    std::sort(c.begin(), c.end());
    std::sort(f.begin(), f.end());
    *med = w[reps / 2];
    printf("%s: wall median %.3f ms (min %.3f, max %.3f, spread %.3f), "
           "cycles/phase median %.0f, clock median %.0f MHz\n", name, w[reps / 2],
           w[0], w[reps - 1], w[reps - 1] - w[0], c[reps / 2], f[reps / 2]);
    return w[reps - 1] - w[0];
  };
  double m32, m16;
  const double s32 = summary("32x32x16", r32, &m32);
  const double s16 = summary("16x16x32", r16, &m16);
  const double spread = s32 > s16 ? s32 : s16;
  printf("16x16x32 vs 32x32x16 by wall: %+.2f %% (median difference %.3f ms, "
         "larger min-max spread %.3f ms): %s\n", 100.0 * (m32 / m16 - 1.0),
         m32 - m16, spread, m32 - m16 > spread ? "GO" : "NO-GO");
  return 0;
}

int main(int argc, char** argv) {
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  if (argc > 1 && std::string(argv[1]) == "shape") return shape_main(cus);
  const int buffer_pairs = 1024;           // 1 MiB hi + 1 MiB lo: the 1024-atom
                                           // dictionary's two packings
  uint4 *hi, *lo;
  float* out;
  unsigned long long* cyc;
  CHECK(hipMalloc(&hi, (size_t)buffer_pairs * 1024));
  CHECK(hipMalloc(&lo, (size_t)buffer_pairs * 1024));
  CHECK(hipMemset(hi, 0x11, (size_t)buffer_pairs * 1024));
  CHECK(hipMemset(lo, 0x12, (size_t)buffer_pairs * 1024));
  CHECK(hipMalloc(&out, (size_t)cus * 512 * sizeof(float)));
  CHECK(hipMalloc(&cyc, (size_t)cus * 8));
  printf("fragment stream + MFMA mix of the fused FISTA kernel, %d CUs "
         "(pure MFMA time per phase: 3072 cycles)\n", cus);
  if (run<4, 8, true>(cus, hi, lo, buffer_pairs, out, cyc)) return 1;
  if (run<4, 16, true>(cus, hi, lo, buffer_pairs, out, cyc)) return 1;
  if (run<8, 4, true>(cus, hi, lo, buffer_pairs, out, cyc)) return 1;
  if (run<8, 8, true>(cus, hi, lo, buffer_pairs, out, cyc)) return 1;
  if (run<8, 16, true>(cus, hi, lo, buffer_pairs, out, cyc)) return 1;
  if (run<4, 8, false>(cus, hi, lo, buffer_pairs, out, cyc)) return 1;
  if (run<4, 16, false>(cus, hi, lo, buffer_pairs, out, cyc)) return 1;
  if (run<8, 4, false>(cus, hi, lo, buffer_pairs, out, cyc)) return 1;
  if (run<8, 8, false>(cus, hi, lo, buffer_pairs, out, cyc)) return 1;
  if (run<8, 16, false>(cus, hi, lo, buffer_pairs, out, cyc)) return 1;
  return 0;
}
