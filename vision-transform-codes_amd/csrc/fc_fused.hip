// Fused persistent FISTA kernel for 16x16 patches (n = 256) on gfx950.
//
// One workgroup (4 waves, one per SIMD) owns 32 patches and runs ALL the
// iterations of analysis_transforms/fully_connected/ista_fista.py:100-146 for
// them without touching HBM in between: the per-patch state (gradient
// evaluation point Y, previous codes C, residual R, the patch X) lives in
// VGPRs / LDS, only the dictionary is streamed (from L2) every iteration.
//
// Orientation.  Everything is computed transposed, patches on the MFMA column
// (= lane) index:
//     G^T[atoms x 32]  = D[atoms x 256]     . R^T[256 x 32]        ("step 1")
//     R^T[256 x 32]   += D^T[256 x atoms]   . Ynew^T[atoms x 32]   ("step 3")
// so that both products consume their right-hand operand with the reduction
// index on the accumulator ROW axis: the result of one product is, after the
// epilogue, the B operand of the next in the same lanes.
//
// Work split.  The atoms are walked in phases of 128 = 4 tiles of 32, one tile
// per wave.  In phase p wave w
//   step 1   G = D[tile 4p+w] R_k                     16 MFMA 32x32x16 (x NP)
//   epilogue C' = shrink(Y - eta G); Y' = C' + beta (C' - C)   (f32, exact op
//            order of the reference), Y' -> bf16 -> LDS exchange buffer
//   barrier
//   step 3   Racc[n-slice w] += D[phase p]^T[n-slice w] Y'[phase p]   16 MFMA
// and after the last phase the waves exchange R_{k+1} = Racc - X through LDS.
// The reference's two GEMMs per iteration become one sweep over D in which
// each dictionary tile is used for the gradient (step 1) and immediately for
// the next residual (step 3).
//
// Dictionary operands are pre-packed once per call into MFMA A-fragment order
// (pack_dictionary_kernel), so every fragment load is one fully coalesced
// 1 KiB global_load_dwordx4 per wave, straight to registers, prefetched one
// step (16 fragments) ahead through a register ring.
//
// Precision (NP): 1 = single bf16 product (fast mode); 2 = bf16 hi/lo split of
// both operands, three products hi*hi + hi*lo + lo*hi accumulated in f32
// (bf16x3, ~2^-16 relative per product: float32-level results on the bf16
// matrix pipe).  State, epilogue and accumulation are f32 in both.
//
// F16 (with NP = 2): the same three products on an f16 hi/lo split -- 11 + 11
// significand bits instead of 8 + 8, i.e. ~2^-21 per product at the same MFMA
// rate and the same bytes.  f16 has 5 exponent bits, so the kernel works in
// power-of-two scaled units: the dictionary is packed as sigma_D * D (one
// global sigma_D, max |D| in [256, 512)), and each patch carries its own
// sigma_Y = 2^(8 - e), e = exponent of max(||x||, ||y0||), so that the
// residual and the codes sit around 2^9 whatever the data's magnitude; the
// f32 state (Y, C, X) is kept in those units for the whole launch.  Scaling by
// a power of two commutes with every IEEE operation of the epilogue (no
// under/overflow at these magnitudes), so the iteration is the reference's
// own, bit for bit, given the products; codes are scaled back on the way out.
//
// MFMA tile.  The kernel exists twice: fused_fista_kernel on 32x32x16 MFMAs
// (described above) and fused_fista_kernel16, the same plan on 16x16x32 MFMAs
// with its own lane maps (comment there).  Cycles per phase are the same; under
// load the chip holds a higher clock on the 16x16x32 shape
// (profiles/fused_mfma_shape.txt).  default_tile16() picks per precision,
// VTC_FUSED_TILE=32|16 forces one.  The two differ in the last bits of the
// codes only: one MFMA accumulates over K = 32 instead of 16.
//
// Schedules.  fused_fista_kernel16 has three schedule bits (comment there;
// VTC_FUSED_SCHED=0..7 forces one, default_sched() picks per precision), none
// of which changes an operand, a product or a summation order: the epilogue of
// the middle phases spread over two segments, the residual exchange started
// under the iteration's last step 3, and the residual operands of step 1's
// first k-steps kept in registers for the NPH phases of an iteration instead
// of being read from LDS in each (profiles/fused_resident_operand.txt).  That
// kernel also has the variant (FISTA / ISTA) compiled in; the 32x32x16 kernel
// has one schedule and selects the variant at run time.
#include "fc_fused.h"
#include "fused_common.h"

#include <stdlib.h>
#include <mutex>
#include <vector>

namespace vtc {

struct FusedParams {
  const float* images;
  const float* init;   // may be null
  float* codes;
  const uint4* packA[2];  // [hi, lo]
  const uint4* packT[2];
  const float* betas;
  int64_t b;
  int s;
  int num_iters;
  int fista;              // 0: ISTA, the gradient is evaluated at the codes
  float eta, cutoff;      // used when eta_dev is null
  const float* eta_dev;   // device scalar 1/L (vtc_lambda_max out[1]) or null
  float lam;              // sparsity weight, cutoff = lam * *eta_dev
  const float* dscale;    // F16: {sigma_D, 1 / sigma_D} (dictionary_scale_kernel)
  unsigned long long* stamps;  // diagnostic build only: 8 cycle sums
};

// LDS plan (bytes), NPH phases, NP precision parts, CREG phases of C in VGPRs:
//   Cst : (NPH-CREG) x 16 KiB   previous codes, [phase][wave][group][lane] f32x4
//   Yx  : 2 x NP x 8704         Y' exchange, double buffered,
//                               [buf][part][patch][256 B + 16 B pad]
//   Rx  : NP x 16896            R exchange, [part][patch][512 B + 16 B pad]
// The 16-byte row pad makes the ds_read_b128 fragment reads of a 16-lane
// group (16 different patches, same column chunk) hit 16 different 4-bank
// slots, and keeps every address of the form lane_base + immediate.
constexpr int kYxRow = 272;
constexpr int kRxRow = 528;
constexpr int kYxPart = 32 * kYxRow;   // 8704
constexpr int kRxPart = 32 * kRxRow;   // 16896

template <int NPH, int NP>
struct FusedLds {
  static constexpr int CREG_WANT = (NP == 1) ? 1 : 3;
  static constexpr int CREG = CREG_WANT < NPH ? CREG_WANT : NPH;
  static constexpr int CL = NPH - CREG;
  static constexpr int cst_bytes = CL * 16384;
  static constexpr int yx_bytes = 2 * NP * kYxPart;
  static constexpr int rx_bytes = NP * kRxPart;
  static constexpr int stat_bytes = 2 * 4 * 32 * 4;   // F16: residual maxima, [call parity][wave][patch]
  static constexpr int total = cst_bytes + yx_bytes + rx_bytes + stat_bytes;
};

template <int NPH, int NP, int MODE, bool F16 = false, bool STAMP = false>
__global__ __launch_bounds__(256, 1) void fused_fista_kernel(FusedParams P) {
  static_assert(!F16 || NP == 2, "the f16 split exists as three products only");
  using L = FusedLds<NPH, NP>;
  constexpr int CREG = L::CREG;
  constexpr int CR = CREG > 0 ? CREG : 1;
  // fragments (k-steps) in flight; must divide 16.  bf16x3 with 16 spills and
  // measures slower (77.7 vs 74.8 ms): the phases are bandwidth-, not
  // latency-bound
  constexpr int RING = (NP == 1) ? 16 : 8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Cst = smem;
  char* Yx = smem + L::cst_bytes;
  char* Rx = Yx + L::yx_bytes;
  float* Stat = reinterpret_cast<float*>(Rx + L::rx_bytes);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int64_t patch = (int64_t)blockIdx.x * kFP + r;
  const bool live = patch < P.b;
  const int s = P.s;

  // Dictionary fragments through buffer loads: wave-uniform descriptor (base
  // already offset to this wave's share), one VGPR byte offset (lane * 16),
  // the fragment index as a scalar offset.
  const unsigned pack_bytes_total = (unsigned)s * kFN * 2u;
  const unsigned a_wave_off = (unsigned)w * (16u * 64u * 16u);
  const unsigned t_wave_off = (unsigned)(2 * w) * (8u * 64u * 16u);
  __amdgpu_buffer_rsrc_t rsA[NP], rsT[NP];
#pragma unroll
  for (int part = 0; part < NP; ++part) {
    rsA[part] = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const char*)P.packA[part] + a_wave_off), 0,
        (int)(pack_bytes_total - a_wave_off), 0x00020000);
    rsT[part] = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const char*)P.packT[part] + t_wave_off), 0,
        (int)(pack_bytes_total - t_wave_off), 0x00020000);
  }
  const unsigned frag_voff = (unsigned)lane * 16u;
  //   packA fragment (phase p, k-step i):      ((4p) * 16 + i) * 1024 bytes
  //   packT fragment (phase p, block nb, ks):  ((p * 8 + nb) * 8 + ks) * 1024
#define VTC_LOAD_A(part, p, i) \
  buffer_load16(rsA[part], frag_voff, (unsigned)(((4 * (p)) * 16 + (i)) * 1024))
#define VTC_LOAD_T(part, p, nb, ks) \
  buffer_load16(rsT[part], frag_voff,  \
                (unsigned)((((p) * 8 + (nb)) * 8 + (ks)) * 1024))

  // LDS lane bases
  const int yx_rd = r * kYxRow + 16 * h;            // + 32 ks
  const int yx_wr = r * kYxRow + 64 * w + 8 * h;    // + 16 g
  const int rx_rd = r * kRxRow + 16 * h;            // + 32 ks
  const int rx_wr = r * kRxRow + 128 * w + 8 * h;   // + 64 nb + 16 g
  const int cst_ln = w * 4096 + lane * 16;          // + pl*16384 + g*1024

  // ---- per-wave state --------------------------------------------------
  f32x16 Y[NPH];    // gradient evaluation point, this wave's tile per phase
  f32x16 Cr[CR];    // previous codes of the first CREG phases
  f32x16 Xr[2];     // the patches, this wave's two 32-pixel blocks
  f32x16 Racc[2];
  uint4 ring[NP][RING];

  // element e of a 32x32 accumulator: row (e&3) + 8(e>>2) + 4h, column r
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (live)
        v = *reinterpret_cast<const float4*>(
            P.images + patch * kFN + 64 * w + 32 * nb + 8 * g + 4 * h);
      Xr[nb][4 * g + 0] = v.x;
      Xr[nb][4 * g + 1] = v.y;
      Xr[nb][4 * g + 2] = v.z;
      Xr[nb][4 * g + 3] = v.w;
    }
  }
  const bool warm = (P.init != nullptr);
#pragma unroll
  for (int p = 0; p < NPH; ++p) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (warm && live)
        v = *reinterpret_cast<const float4*>(
            P.init + patch * s + kPhaseAtoms * p + 32 * w + 8 * g + 4 * h);
      Y[p][4 * g + 0] = v.x;
      Y[p][4 * g + 1] = v.y;
      Y[p][4 * g + 2] = v.z;
      Y[p][4 * g + 3] = v.w;
    }
  }
  // F16: the patch's power-of-two scale (header comment).  e = exponent of
  // max(||x||, ||y0||) over the whole patch: partial sums of squares per lane,
  // the two lane halves by a lane exchange, the four waves through LDS (the R
  // exchange area is not in use yet).
  float sigma_y = 1.f, inv_sigma_y = 1.f;   // per lane (= per patch)
  float sigma_d = 1.f, inv_sigma_d = 1.f;
  if (F16) {
    float sx = 0.f, sy = 0.f;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int e = 0; e < 16; ++e) sx += Xr[nb][e] * Xr[nb][e];
    if (warm) {
#pragma unroll
      for (int p = 0; p < NPH; ++p)
#pragma unroll
        for (int e = 0; e < 16; ++e) sy += Y[p][e] * Y[p][e];
    }
    sx += __shfl_xor(sx, 32, 64);
    sy += __shfl_xor(sy, 32, 64);
    float* red = reinterpret_cast<float*>(Rx);
    if (h == 0) {
      red[w * 64 + r] = sx;
      red[w * 64 + 32 + r] = sy;
    }
    __syncthreads();
    float tx = 0.f, ty = 0.f;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      tx += red[v * 64 + r];
      ty += red[v * 64 + 32 + r];
    }
    __syncthreads();
    const float m2 = fmaxf(tx, ty);
    int e2 = 0;
    if (m2 > 0.f && m2 < __builtin_inff()) e2 = ilogbf(m2) >> 1;
    e2 = e2 < -60 ? -60 : (e2 > 60 ? 60 : e2);
    sigma_y = ldexpf(1.f, 8 - e2);
    inv_sigma_y = ldexpf(1.f, e2 - 8);
    sigma_d = P.dscale[0];
    inv_sigma_d = P.dscale[1];
    const float sx_scale = sigma_d * sigma_y;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int e = 0; e < 16; ++e) Xr[nb][e] *= sx_scale;
#pragma unroll
    for (int p = 0; p < NPH; ++p)
#pragma unroll
      for (int e = 0; e < 16; ++e) Y[p][e] *= sigma_y;
  }
  // eta either came by value or sits in device memory (sync-free callers);
  // lambda * eta is then the same single f32 multiply the host would do
  float eta = P.eta, cutoff_l = P.cutoff;
  if (P.eta_dev) {
    eta = *P.eta_dev;
    cutoff_l = mul_rn(P.lam, eta);
  }
  if (F16) {
    // scaled units: eta_s * Gacc = sigma_Y * (eta * G) with Gacc = sigma_D
    // sigma_R G, sigma_R = 2 sigma_Y; the threshold scales with the codes
    // (per lane, i.e. per patch)
    eta = eta * (0.5f * inv_sigma_d);
    cutoff_l = cutoff_l * sigma_y;
  }
  // residual operand: Rs = (Racc - Xs) * r_scale = sigma_R * R with
  // sigma_R = 2 sigma_Y (||Rs|| starts in [2^12, 2^13))
  const float r_scale = F16 ? 2.f * inv_sigma_d : 1.f;
  int xr_calls = 0;
#pragma unroll
  for (int p = 0; p < NPH; ++p) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (p < CREG) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          Cr[p < CREG ? p : 0][4 * g + q] = Y[p][4 * g + q];
      } else {
        *reinterpret_cast<float4*>(Cst + cst_ln + (p - CREG) * 16384 +
                                   g * 1024) =
            make_float4(Y[p][4 * g + 0], Y[p][4 * g + 1], Y[p][4 * g + 2],
                        Y[p][4 * g + 3]);
      }
    }
  }
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int e = 0; e < 16; ++e) Racc[nb][e] = 0.f;

  // write the wave's tile of Y (as bf16 parts) into exchange buffer `buf`
  auto publish_y = [&](const f32x16& y, int buf) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float v4[4] = {y[4 * g], y[4 * g + 1], y[4 * g + 2], y[4 * g + 3]};
      uint2 hi, lo;
      split_packed<F16, 4, NP == 2>(v4, hi, lo);
      char* dst = Yx + buf * NP * kYxPart + yx_wr + 16 * g;
      *reinterpret_cast<uint2*>(dst) = hi;
      if (NP == 2) *reinterpret_cast<uint2*>(dst + kYxPart) = lo;
    }
  };

  // Per iteration the dictionary is consumed as a stream of 2*NPH segments of
  // 16 fragments; the epilogue of phase p is software-pipelined under step 1
  // of phase p+1, so the order is
  //   A(0) | A(1) T(0) | A(2) T(1) | ... | A(NPH-1) T(NPH-2) | T(NPH-1)
  // (A(p) = step-1 fragments of phase p, T(p) = its step-3 fragments).
  // Segment sigma: is it a T segment, and of which phase?
#define VTC_SEG_IS_T(sg) (((sg) >= 2 && ((sg) % 2) == 0) || (sg) == 2 * NPH - 1)
#define VTC_SEG_PHASE(sg)                                        \
  ((sg) == 0 ? 0                                                 \
             : (sg) == 2 * NPH - 1 ? NPH - 1                     \
                                   : ((sg) % 2 ? ((sg) + 1) / 2 : (sg) / 2 - 1))
#define VTC_LOAD_SEG(part, sg, i)                                          \
  (VTC_SEG_IS_T(sg) ? VTC_LOAD_T(part, VTC_SEG_PHASE(sg), (i) & 1, (i) >> 1) \
                    : VTC_LOAD_A(part, VTC_SEG_PHASE(sg), (i)))
  // refill of the ring slot consumed at (segment sg, position i): the
  // fragment RING positions further down the stream (wrapping to the next
  // iteration's first segment)
#define VTC_REFILL(sg, i)                                                   \
  {                                                                         \
    const int j_ = (i) + RING;                                              \
    const int sg_ = (j_ < 16) ? (sg) : (((sg) + 1) % (2 * NPH));            \
    const int i_ = (j_ < 16) ? j_ : j_ - 16;                                \
    _Pragma("unroll") for (int part = 0; part < NP; ++part)                 \
        ring[part][(i) % RING] = VTC_LOAD_SEG(part, sg_, i_);               \
  }

  // step 3 of phase p: Racc[nb] += D^T fragments x Y' fragments.
  // pipe: fragments come from the ring (stream segment sg); otherwise they
  // are loaded on the spot (warm-start prologue).
  // hipcc would sink every dictionary load down to its consumer (to shorten
  // live ranges), which serialises load -> wait -> MFMA; the sched_barrier
  // after each k-step pins the issue order written here.
  auto step3 = [&](int p, int buf, bool pipe, int sg, auto&& between) {
    uint4 yb_next[NP];
#pragma unroll
    for (int part = 0; part < NP; ++part)
      yb_next[part] = *reinterpret_cast<const uint4*>(
          Yx + (buf * NP + part) * kYxPart + yx_rd);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      uint4 yb[NP];
#pragma unroll
      for (int part = 0; part < NP; ++part) {
        yb[part] = yb_next[part];
        if (ks + 1 < 8)
          yb_next[part] = *reinterpret_cast<const uint4*>(
              Yx + (buf * NP + part) * kYxPart + yx_rd + 32 * (ks + 1));
      }
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const int i = 2 * ks + nb;          // position in the segment
        uint4 a[NP];
#pragma unroll
        for (int part = 0; part < NP; ++part)
          a[part] = pipe ? ring[part][i % RING] : VTC_LOAD_T(part, p, nb, ks);
        Racc[nb] = mfma16<F16>(a[0], yb[0], Racc[nb]);
        if constexpr (NP == 2) {
          Racc[nb] = mfma16<F16>(a[0], yb[1], Racc[nb]);
          Racc[nb] = mfma16<F16>(a[1], yb[0], Racc[nb]);
        }
        // (epilogue arithmetic of another phase, if any, before the refill:
        // see step 1)
        between(i);
        if (pipe) VTC_REFILL(sg, i)
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };
  auto nothing = [](int) {};

  // R_{k+1} = Racc - X  ->  bf16 parts -> LDS (read back as B fragments by
  // every wave during step 1 of the next iteration)
  auto exchange_r = [&]() {
    float v[2][16];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        v[nb][e] = sub_rn(Racc[nb][e], Xr[nb][e]);
        if (F16) v[nb][e] *= r_scale;
      }
    if (F16) {
      // f16 range guard.  With eta = 1/L the residual never grows past a small
      // multiple of ||x|| (2^9 .. 2^10 in these units), but a caller's own
      // stepsize may make the iteration diverge -- as it does in f32 in the
      // reference.  When a patch's residual has passed 2^11 all of its state
      // drops by a power of two (exact, so the iteration goes on bit for bit as
      // before, in smaller units; growth of up to 32x per iteration is
      // absorbed before f16 overflows): max over the patch through LDS, then a
      // wave-uniform branch that is not taken in a convergent run.
      float m = 0.f;
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int e = 0; e < 16; ++e) m = fmaxf(m, fabsf(v[nb][e]));
      m = fmaxf(m, __shfl_xor(m, 32, 64));
      // the decision uses the maxima all four waves left at the PREVIOUS call
      // (visible since that call's closing barrier): no barrier of its own
      float f = 1.f;
      if (xr_calls > 0) {
        const float* prev = Stat + ((xr_calls - 1) & 1) * 128;
        const float Mx = fmaxf(fmaxf(prev[r], prev[32 + r]),
                               fmaxf(prev[64 + r], prev[96 + r]));
        if (Mx > 2048.f && Mx < __builtin_inff())
          f = ldexpf(1.f, 9 - ilogbf(Mx));
      }
      if (h == 0) Stat[(xr_calls & 1) * 128 + w * 32 + r] = m * f;
      ++xr_calls;
      if (__any(f != 1.f)) {
#pragma unroll
        for (int p = 0; p < NPH; ++p)
#pragma unroll
          for (int e = 0; e < 16; ++e) Y[p][e] *= f;
#pragma unroll
        for (int p = 0; p < CR; ++p)
#pragma unroll
          for (int e = 0; e < 16; ++e) Cr[p][e] *= f;
#pragma unroll
        for (int pl = 0; pl < L::CL; ++pl)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            float4* c4 = reinterpret_cast<float4*>(Cst + cst_ln + pl * 16384 +
                                                   g * 1024);
            float4 c = *c4;
            c.x *= f; c.y *= f; c.z *= f; c.w *= f;
            *c4 = c;
          }
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            Xr[nb][e] *= f;
            v[nb][e] *= f;
          }
        cutoff_l *= f;
        inv_sigma_y *= 1.f / f;
      }
    }
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float v4[4] = {v[nb][4 * g], v[nb][4 * g + 1], v[nb][4 * g + 2],
                             v[nb][4 * g + 3]};
        uint2 hi, lo;
        split_packed<F16, 4, NP == 2>(v4, hi, lo);
        char* dst = Rx + rx_wr + 64 * nb + 16 * g;
        *reinterpret_cast<uint2*>(dst) = hi;
        if (NP == 2) *reinterpret_cast<uint2*>(dst + kRxPart) = lo;
      }
    }
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int e = 0; e < 16; ++e) Racc[nb][e] = 0.f;
    __syncthreads();
  };

  // ---- R_0 = Y_0 D - X ---------------------------------------------------
  if (warm) {
#pragma unroll
    for (int p = 0; p < NPH; ++p) {
      publish_y(Y[p], p & 1);
      __syncthreads();
      step3(p, p & 1, false, 0, nothing);
    }
  }
  exchange_r();

  // prime the ring with the first RING fragments of segment 0
#pragma unroll
  for (int i = 0; i < RING; ++i)
#pragma unroll
    for (int part = 0; part < NP; ++part)
      ring[part][i] = VTC_LOAD_SEG(part, 0, i);

  const bool fista = P.fista != 0;   // ISTA: every beta is 0
  unsigned long long acc_t[5] = {0, 0, 0, 0, 0};
  unsigned long long t0 = 0, t1 = 0;
#define VTC_STAMP(slot)                    \
  if (STAMP) {                             \
    t1 = stamp_now();                      \
    acc_t[slot] += t1 - t0;                \
    t0 = t1;                               \
  }
  if (STAMP) t0 = stamp_now();

  f32x16 Gb[2];     // gradient tiles of two consecutive phases
  float4 cold4;      // previous codes of the 4 elements being processed
  float cn4[4];

  // Proximal step + extrapolation for element e of phase p
  // (ista_fista.py:105-131); elements are visited in order 0..15, group
  // loads/stores of C and the bf16 publication of Y' happen at group edges.
  auto epilogue_elem = [&](int p, int e, const f32x16& Gp, float beta) {
    const int g = e >> 2, k = e & 3;
    if (MODE == 7) {         // diagnostic: step 1 with (almost) no epilogue work
      const float cn = Y[p][e] + Gp[e];
      Y[p][e] = cn;
      cn4[k] = cn;
      if (k == 3) {
        if (p < CREG) {
#pragma unroll
          for (int q = 0; q < 4; ++q) Cr[p < CREG ? p : 0][4 * g + q] = cn4[q];
        } else {
          *reinterpret_cast<float4*>(Cst + cst_ln + (p - CREG) * 16384 +
                                     g * 1024) =
              make_float4(cn4[0], cn4[1], cn4[2], cn4[3]);
        }
      }
      return;
    }
    if (k == 0) {
      if (p < CREG) {
        cold4 = make_float4(Cr[p < CREG ? p : 0][4 * g + 0],
                            Cr[p < CREG ? p : 0][4 * g + 1],
                            Cr[p < CREG ? p : 0][4 * g + 2],
                            Cr[p < CREG ? p : 0][4 * g + 3]);
      } else {
        cold4 = *reinterpret_cast<const float4*>(
            Cst + cst_ln + (p - CREG) * 16384 + g * 1024);
      }
    }
    const float co = (k == 0) ? cold4.x : (k == 1) ? cold4.y
                   : (k == 2) ? cold4.z : cold4.w;
    const float c = sub_rn(Y[p][e], mul_rn(eta, Gp[e]));
    const float cn = shrink_fast<MODE>(c, cutoff_l);
    // ISTA: y = codes (ista_fista.py:133), not codes + 0 * (codes - old):
    // a code that has overflowed to inf stays inf as it does there
    Y[p][e] = fista ? add_rn(cn, mul_rn(beta, sub_rn(cn, co))) : cn;
    cn4[k] = cn;
    if (k == 3) {
      if (p < CREG) {
#pragma unroll
        for (int q = 0; q < 4; ++q) Cr[p < CREG ? p : 0][4 * g + q] = cn4[q];
      } else {
        *reinterpret_cast<float4*>(Cst + cst_ln + (p - CREG) * 16384 +
                                   g * 1024) =
            make_float4(cn4[0], cn4[1], cn4[2], cn4[3]);
      }
      const float v4[4] = {Y[p][4 * g], Y[p][4 * g + 1], Y[p][4 * g + 2],
                           Y[p][4 * g + 3]};
      uint2 hi, lo;
      split_packed<F16, 4, NP == 2>(v4, hi, lo);
      char* dst = Yx + (p & 1) * NP * kYxPart + yx_wr + 16 * g;
      *reinterpret_cast<uint2*>(dst) = hi;
      if (NP == 2) *reinterpret_cast<uint2*>(dst + kYxPart) = lo;
    }
  };

  // step 1 of phase p (stream segment sg): Gb[p&1] = D[tile] R_k, with the
  // epilogue of phase p-1 interleaved element by element when `overlap`
  auto step1 = [&](int p, int sg, bool overlap, float beta) {
    f32x16& G = Gb[p & 1];
#pragma unroll
    for (int e = 0; e < 16; ++e) G[e] = 0.f;
    uint4 rb_next[NP];
#pragma unroll
    for (int part = 0; part < NP; ++part)
      rb_next[part] =
          *reinterpret_cast<const uint4*>(Rx + part * kRxPart + rx_rd);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      uint4 rb[NP];
#pragma unroll
      for (int part = 0; part < NP; ++part) {
        rb[part] = rb_next[part];
        if (i + 1 < 16)
          rb_next[part] = *reinterpret_cast<const uint4*>(
              Rx + part * kRxPart + rx_rd + 32 * (i + 1));
      }
      G = mfma16<F16>(ring[0][i % RING], rb[0], G);
      if constexpr (NP == 2) {
        G = mfma16<F16>(ring[0][i % RING], rb[1], G);
        G = mfma16<F16>(ring[1][i % RING], rb[0], G);
      }
      // epilogue arithmetic first, then the refill: a wave blocks at a
      // buffer load while the vector-memory path is busy, and in that order
      // its VALU work would wait behind the load instead of overlapping it
      if (overlap) {
        epilogue_elem(p - 1, i, Gb[(p - 1) & 1], beta);
        __builtin_amdgcn_sched_barrier(0);
      }
      VTC_REFILL(sg, i)
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  for (int it = 0; it < P.num_iters; ++it) {
    const float beta = fista ? P.betas[it] : 0.f;
    step1(0, 0, false, beta);
    VTC_STAMP(0)
#pragma unroll
    for (int p = 0; p < NPH; ++p) {
      if (p + 1 < NPH) {
        step1(p + 1, 2 * p + 1, true, beta);   // + epilogue of phase p
        VTC_STAMP(0)
      }
      // (the epilogue of the LAST phase has no step 1 to hide under: it rides
      // on step 3 of the phase before it -- its gradient tile is complete by
      // then, and it writes the exchange buffer step 3 is not reading)
      __syncthreads();
      VTC_STAMP(2)
      // ---- step 3: next residual, this wave's 64 pixels
      if (p + 2 == NPH) {
        step3(p, p & 1, true, 2 * p + 2, [&](int i) {
          epilogue_elem(NPH - 1, i, Gb[(NPH - 1) & 1], beta);
          __builtin_amdgcn_sched_barrier(0);
        });
      } else {
        step3(p, p & 1, true, (p + 1 < NPH) ? 2 * p + 2 : 2 * NPH - 1, nothing);
      }
      VTC_STAMP(3)
    }
    exchange_r();
    VTC_STAMP(4)
  }
  if (STAMP && lane == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) atomicAdd(P.stamps + k, acc_t[k]);
    atomicAdd(P.stamps + 7, 1ull);
  }
#undef VTC_STAMP

  // ---- codes out: the last C -----------------------------------------
#pragma unroll
  for (int p = 0; p < NPH; ++p) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float4 v;
      if (p < CREG) {
        v = make_float4(Cr[p < CREG ? p : 0][4 * g + 0],
                        Cr[p < CREG ? p : 0][4 * g + 1],
                        Cr[p < CREG ? p : 0][4 * g + 2],
                        Cr[p < CREG ? p : 0][4 * g + 3]);
      } else {
        v = *reinterpret_cast<const float4*>(Cst + cst_ln +
                                             (p - CREG) * 16384 + g * 1024);
      }
      if (F16) {
        v.x *= inv_sigma_y;
        v.y *= inv_sigma_y;
        v.z *= inv_sigma_y;
        v.w *= inv_sigma_y;
      }
      if (live)
        *reinterpret_cast<float4*>(P.codes + patch * s + kPhaseAtoms * p +
                                   32 * w + 8 * g + 4 * h) = v;
    }
  }
#undef VTC_LOAD_A
#undef VTC_LOAD_T
#undef VTC_LOAD_SEG
#undef VTC_REFILL
#undef VTC_SEG_IS_T
#undef VTC_SEG_PHASE
}

// ---------------------------------------------------------------------------
// The same kernel on v_mfma_f32_16x16x32: same phases, same 32-atom tile per
// wave in step 1 and 64-pixel slice per wave in step 3, same stream of 16
// one-KiB fragments per segment, same ring, same pipelined epilogue -- only
// the instruction and with it the lane maps change (the chip holds a higher
// clock on this shape: profiles/fused_mfma_shape.txt).
//
// Lane l = (c, q) = (l & 15, l >> 4).  A 32x32 tile is four 16x16 sub-tiles
// (m, n): rows 16m.., patches 16n..; element k of sub-tile (m, n) sits at row
// 16m + 4q + k, patch 16n + c.  A lane therefore owns TWO patches, c and
// 16 + c, and everything per patch is a pair indexed by n.  State tiles keep
// the f32x16 form, element 4g + k with group g = 2m + n, so that a group is
// still four consecutive atoms of one patch: one 16-byte C access, one 8-byte
// publication.
//
// Exchange images: rows per patch as before (272 B / 528 B).  A B operand is
// one ds_read_b128 of patch 16n + c, K chunk q of the k-step; the chunks of a
// k-step (64 B of a row) are stored in K order except that chunks 2j and 2j+1
// swap places in rows 4..11 of each half.  A ds_read_b128 lane group holds
// the rows {0-3, 12-15} of one chunk and the rows {4-11} of its neighbour:
// with the swap both sit at the same offset of their rows, so the 16 rows of
// a group keep one 4-bank slot each (row stride = 4 banks mod 64): no
// conflict.  The 8-byte publishing stores go out in groups of 16 consecutive
// lanes = 16 rows of one half at 2-bank slots 2 * row (+ 2 for the swap)
// mod 16: 2-way, as the 32x32x16 kernel's stores are.
//
// SCHED moves VALU work between stream segments; arithmetic, bytes and
// products are the same in every schedule, and so are the codes, bit for bit
// (profiles/fused_epilogue_spread.txt).
//   bit 0: the epilogue of a middle phase p (0 < p < NPH-1) runs half under
//          step 3(p-1) (groups 0, 1) and half under step 1(p+1) (groups 2, 3)
//          instead of wholly under step 1(p+1).  NPH = 2 has no middle phase.
//   bit 1: the iteration's last step 3 walks its fragments pixel-block-major
//          (blocks {0, 1} over the four k-steps, then {2, 3}), and the residual
//          exchange of blocks 0 and 1 runs in the MFMA gaps of the second half.
//   bit 2: the B operands of step 1's first kResidentKsteps k-steps (the
//          residual R_k: the same in all NPH phases of an iteration) are read
//          from the exchange image once per iteration and kept in registers;
//          the other k-steps keep their one-ahead ds_read_b128.
// FISTA compiles the variant in: the 32x32x16 kernel selects at run time.
//
// split_group: split_packed<F16, 4> with the lo part's subtraction written per
// element.  split_operand.h subtracts a pair at a time, which becomes
// v_pk_add_f32: 49 of them per iteration of the f16x3 kernel, each of which
// costs about three plain f32 instructions beside MFMAs
// (MI355X_MICROARCH.md).  Same conversions, same subtraction, same bits.
template <bool F16, bool LO>
__device__ __forceinline__ void split_group(const float (&v)[4], uint2& hi_out,
                                            uint2& lo_out) {
  if constexpr (F16) {
    typedef float pair_f32 __attribute__((ext_vector_type(2)));
    typedef _Float16 pair_f16 __attribute__((ext_vector_type(2)));
    unsigned hw[2], lw[2] = {0u, 0u};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const pair_f32 x = {v[2 * k], v[2 * k + 1]};
      const pair_f16 h = __builtin_convertvector(x, pair_f16);
      hw[k] = __builtin_bit_cast(unsigned, h);
      if (LO) {
        const float d0 = sub_rn(v[2 * k], (float)h[0]);
        const float d1 = sub_rn(v[2 * k + 1], (float)h[1]);
        const pair_f32 d = {d0, d1};
        lw[k] = __builtin_bit_cast(unsigned,
                                   __builtin_convertvector(d, pair_f16));
      }
    }
    hi_out = make_uint2(hw[0], hw[1]);
    if (LO) lo_out = make_uint2(lw[0], lw[1]);
  } else {
    split_packed<F16, 4, LO>(v, hi_out, lo_out);
  }
}
// kResidentKsteps: 2, 3 and 4 were built (-DVTC_FUSED_KRES) and measured, all
// without scratch; each step is faster than the one before it, 4 is what
// schedule 7 of f16x3 still holds in its 512 registers
// (profiles/fused_resident_operand.txt).
#ifndef VTC_FUSED_KRES
#define VTC_FUSED_KRES 4
#endif
constexpr int kResidentKsteps = VTC_FUSED_KRES;
template <int NPH, int NP, int MODE, bool F16 = false, bool STAMP = false,
          int SCHED = 0, bool FISTA = true>
__global__ __launch_bounds__(256, 1) void fused_fista_kernel16(FusedParams P) {
  static_assert(!F16 || NP == 2, "the f16 split exists as three products only");
  static_assert(SCHED >= 0 && SCHED < 8, "three schedule bits");
  constexpr bool SPREAD = (SCHED & 1) != 0 && NPH > 2;
  constexpr bool EARLY_R = (SCHED & 2) != 0;
  constexpr int KRES = (SCHED & 4) != 0 ? kResidentKsteps : 0;
  constexpr int KR = KRES > 0 ? KRES : 1;
  static_assert(KRES >= 0 && KRES < 8, "step 1 has eight k-steps");
  using L = FusedLds<NPH, NP>;
  constexpr int CREG = L::CREG;
  constexpr int CR = CREG > 0 ? CREG : 1;
  constexpr int RING = (NP == 1) ? 16 : 8;
  constexpr int NPROD = (NP == 2) ? 3 : 1;   // hi*hi, hi*lo, lo*hi
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Cst = smem;
  char* Yx = smem + L::cst_bytes;
  char* Rx = Yx + L::yx_bytes;
  float* Stat = reinterpret_cast<float*>(Rx + L::rx_bytes);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, q = lane >> 4;
  int64_t patch[2];
  bool live[2];
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    patch[n] = (int64_t)blockIdx.x * kFP + 16 * n + c;
    live[n] = patch[n] < P.b;
  }
  const int s = P.s;

  const unsigned pack_bytes_total = (unsigned)s * kFN * 2u;
  const unsigned a_wave_off = (unsigned)w * (16u * 64u * 16u);
  const unsigned t_wave_off = (unsigned)(4 * w) * (4u * 64u * 16u);
  __amdgpu_buffer_rsrc_t rsA[NP], rsT[NP];
#pragma unroll
  for (int part = 0; part < NP; ++part) {
    rsA[part] = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const char*)P.packA[part] + a_wave_off), 0,
        (int)(pack_bytes_total - a_wave_off), 0x00020000);
    rsT[part] = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const char*)P.packT[part] + t_wave_off), 0,
        (int)(pack_bytes_total - t_wave_off), 0x00020000);
  }
  const unsigned frag_voff = (unsigned)lane * 16u;
  //   packA fragment (phase p, position i = 2ks + m):  ((4p) * 16 + i) * 1024
  //   packT fragment (phase p, block nb, ks):  ((p * 16 + nb) * 4 + ks) * 1024
#define VTC_LOAD_A(part, p, i) \
  buffer_load16(rsA[part], frag_voff, (unsigned)(((4 * (p)) * 16 + (i)) * 1024))
#define VTC_LOAD_T(part, p, nb, ks) \
  buffer_load16(rsT[part], frag_voff,  \
                (unsigned)((((p) * 16 + (nb)) * 4 + (ks)) * 1024))

  // LDS lane bases (patch half n: + 16 rows)
  const int swap = ((c >> 2) ^ (c >> 3)) & 1;        // rows 4..11
  const int rd_chunk = 32 * (q >> 1) + 16 * ((q & 1) ^ swap);
  const int wr_chunk = 16 * ((q >> 1) ^ swap) + 8 * (q & 1);
  const int yx_rd = c * kYxRow + rd_chunk;            // + 64 ks
  const int yx_wr = c * kYxRow + 64 * w + wr_chunk;   // + 32 m
  const int rx_rd = c * kRxRow + rd_chunk;            // + 64 ks
  const int rx_wr = c * kRxRow + 128 * w + wr_chunk;  // + 32 nb
  const int cst_ln = w * 4096 + lane * 16;            // + pl*16384 + g*1024
  constexpr int kYxHalf = 16 * kYxRow, kRxHalf = 16 * kRxRow;

  // ---- per-wave state --------------------------------------------------
  f32x16 Y[NPH];      // element 4g + k: atom 16(g>>1) + 4q + k, patch half g&1
  f32x16 Cr[CR];
  f32x4 Xr[4][2];     // [16-pixel block][patch half]: pixel 16nb + 4q + k
  f32x4 Racc[4][2];
  uint4 ring[NP][RING];
  uint4 rres[KR][2][NP];   // KRES: B operands of step 1's first k-steps

#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (live[n])
        v = *reinterpret_cast<const float4*>(P.images + patch[n] * kFN + 64 * w +
                                             16 * nb + 4 * q);
      Xr[nb][n][0] = v.x;
      Xr[nb][n][1] = v.y;
      Xr[nb][n][2] = v.z;
      Xr[nb][n][3] = v.w;
    }
  }
  const bool warm = (P.init != nullptr);
#pragma unroll
  for (int p = 0; p < NPH; ++p) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (warm && live[g & 1])
        v = *reinterpret_cast<const float4*>(P.init + patch[g & 1] * s +
                                             kPhaseAtoms * p + 32 * w +
                                             16 * (g >> 1) + 4 * q);
      Y[p][4 * g + 0] = v.x;
      Y[p][4 * g + 1] = v.y;
      Y[p][4 * g + 2] = v.z;
      Y[p][4 * g + 3] = v.w;
    }
  }
  // F16: the power-of-two scale of each of the lane's two patches
  float sigma_y[2] = {1.f, 1.f}, inv_sigma_y[2] = {1.f, 1.f};
  float sigma_d = 1.f, inv_sigma_d = 1.f;
  if (F16) {
    float sx[2] = {0.f, 0.f}, sy[2] = {0.f, 0.f};
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int k = 0; k < 4; ++k) sx[n] += Xr[nb][n][k] * Xr[nb][n][k];
    if (warm) {
#pragma unroll
      for (int p = 0; p < NPH; ++p)
#pragma unroll
        for (int e = 0; e < 16; ++e) sy[(e >> 2) & 1] += Y[p][e] * Y[p][e];
    }
    float* red = reinterpret_cast<float*>(Rx);
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      sx[n] += __shfl_xor(sx[n], 16, 64);
      sx[n] += __shfl_xor(sx[n], 32, 64);
      sy[n] += __shfl_xor(sy[n], 16, 64);
      sy[n] += __shfl_xor(sy[n], 32, 64);
      if (q == 0) {
        red[w * 64 + 16 * n + c] = sx[n];
        red[w * 64 + 32 + 16 * n + c] = sy[n];
      }
    }
    __syncthreads();
    float m2[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      float tx = 0.f, ty = 0.f;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        tx += red[v * 64 + 16 * n + c];
        ty += red[v * 64 + 32 + 16 * n + c];
      }
      m2[n] = fmaxf(tx, ty);
    }
    __syncthreads();
    sigma_d = P.dscale[0];
    inv_sigma_d = P.dscale[1];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      int e2 = 0;
      if (m2[n] > 0.f && m2[n] < __builtin_inff()) e2 = ilogbf(m2[n]) >> 1;
      e2 = e2 < -60 ? -60 : (e2 > 60 ? 60 : e2);
      sigma_y[n] = ldexpf(1.f, 8 - e2);
      inv_sigma_y[n] = ldexpf(1.f, e2 - 8);
      const float sx_scale = sigma_d * sigma_y[n];
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int k = 0; k < 4; ++k) Xr[nb][n][k] *= sx_scale;
    }
#pragma unroll
    for (int p = 0; p < NPH; ++p)
#pragma unroll
      for (int e = 0; e < 16; ++e) Y[p][e] *= sigma_y[(e >> 2) & 1];
  }
  float eta = P.eta, cutoff = P.cutoff;
  if (P.eta_dev) {
    eta = *P.eta_dev;
    cutoff = mul_rn(P.lam, eta);
  }
  float cutoff_l[2] = {cutoff, cutoff};
  if (F16) {
    // scaled units, as in the 32x32x16 kernel; the threshold scales with the
    // codes, per patch
    eta = eta * (0.5f * inv_sigma_d);
    cutoff_l[0] = cutoff * sigma_y[0];
    cutoff_l[1] = cutoff * sigma_y[1];
  }
  const float r_scale = F16 ? 2.f * inv_sigma_d : 1.f;
  int xr_calls = 0;
#pragma unroll
  for (int p = 0; p < NPH; ++p) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (p < CREG) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          Cr[p < CREG ? p : 0][4 * g + k] = Y[p][4 * g + k];
      } else {
        *reinterpret_cast<float4*>(Cst + cst_ln + (p - CREG) * 16384 +
                                   g * 1024) =
            make_float4(Y[p][4 * g + 0], Y[p][4 * g + 1], Y[p][4 * g + 2],
                        Y[p][4 * g + 3]);
      }
    }
  }
#pragma unroll
  for (int nb = 0; nb < 4; ++nb)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int k = 0; k < 4; ++k) Racc[nb][n][k] = 0.f;

  // group g of a Y tile (as parts) into exchange buffer `buf`
  auto publish_group = [&](const f32x16& y, int g, int buf) {
    const float v4[4] = {y[4 * g], y[4 * g + 1], y[4 * g + 2], y[4 * g + 3]};
    uint2 hi, lo;
    split_group<F16, NP == 2>(v4, hi, lo);
    char* dst = Yx + buf * NP * kYxPart + yx_wr + 32 * (g >> 1) +
                kYxHalf * (g & 1);
    *reinterpret_cast<uint2*>(dst) = hi;
    if (NP == 2) *reinterpret_cast<uint2*>(dst + kYxPart) = lo;
  };

#define VTC_SEG_IS_T(sg) (((sg) >= 2 && ((sg) % 2) == 0) || (sg) == 2 * NPH - 1)
#define VTC_SEG_PHASE(sg)                                        \
  ((sg) == 0 ? 0                                                 \
             : (sg) == 2 * NPH - 1 ? NPH - 1                     \
                                   : ((sg) % 2 ? ((sg) + 1) / 2 : (sg) / 2 - 1))
  // position i of a T segment: k-step i >> 2, pixel block i & 3 -- except, with
  // EARLY_R, in the iteration's last segment, which is walked block-major:
  // k-step (i >> 1) & 3, pixel block 2 (i >> 3) + (i & 1)
#define VTC_SEG_BLOCK_MAJOR(sg) (EARLY_R && (sg) == 2 * NPH - 1)
#define VTC_T_NB(sg, i) \
  (VTC_SEG_BLOCK_MAJOR(sg) ? 2 * ((i) >> 3) + ((i) & 1) : (i) & 3)
#define VTC_T_KS(sg, i) (VTC_SEG_BLOCK_MAJOR(sg) ? ((i) >> 1) & 3 : (i) >> 2)
#define VTC_LOAD_SEG(part, sg, i)                                          \
  (VTC_SEG_IS_T(sg) ? VTC_LOAD_T(part, VTC_SEG_PHASE(sg), VTC_T_NB(sg, i), \
                                 VTC_T_KS(sg, i))                          \
                    : VTC_LOAD_A(part, VTC_SEG_PHASE(sg), (i)))
#define VTC_REFILL(sg, i)                                                   \
  {                                                                         \
    const int j_ = (i) + RING;                                              \
    const int sg_ = (j_ < 16) ? (sg) : (((sg) + 1) % (2 * NPH));            \
    const int i_ = (j_ < 16) ? j_ : j_ - 16;                                \
    _Pragma("unroll") for (int part = 0; part < NP; ++part)                 \
        ring[part][(i) % RING] = VTC_LOAD_SEG(part, sg_, i_);               \
  }
  // the NPROD * 2 MFMAs of one fragment: both patch halves, products outermost,
  // so that consecutive MFMAs write different accumulators
#define VTC_MFMA_PAIR(acc0, acc1, a, b)                                     \
  _Pragma("unroll") for (int prod = 0; prod < NPROD; ++prod) {              \
    acc0 = mfma_k32<F16>(a[prod == 2], b[0][prod == 1], acc0);              \
    acc1 = mfma_k32<F16>(a[prod == 2], b[1][prod == 1], acc1);              \
  }

  // step 3 of phase p: Racc[nb][n] += D^T fragments x Y' fragments; position
  // i = 4 ks + nb.  The B operands of k-step ks + 1 are fetched under the
  // first two positions of k-step ks, one patch half each.
  auto step3 = [&](int p, int buf, bool pipe, int sg, auto&& between) {
    uint4 yb[2][NP], yb_next[2][NP];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int part = 0; part < NP; ++part)
        yb_next[n][part] = *reinterpret_cast<const uint4*>(
            Yx + (buf * NP + part) * kYxPart + yx_rd + kYxHalf * n);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int ks = i >> 2, nb = i & 3;
      if (nb == 0) {
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int part = 0; part < NP; ++part) yb[n][part] = yb_next[n][part];
      }
      if (nb < 2 && ks + 1 < 4) {
#pragma unroll
        for (int part = 0; part < NP; ++part)
          yb_next[nb][part] = *reinterpret_cast<const uint4*>(
              Yx + (buf * NP + part) * kYxPart + yx_rd + kYxHalf * nb +
              64 * (ks + 1));
      }
      uint4 a[NP];
#pragma unroll
      for (int part = 0; part < NP; ++part)
        a[part] = pipe ? ring[part][i % RING] : VTC_LOAD_T(part, p, nb, ks);
      VTC_MFMA_PAIR(Racc[nb][0], Racc[nb][1], a, yb)
      between(i);
      if (pipe) VTC_REFILL(sg, i)
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  auto nothing = [](int) {};

  // R_{k+1} = Racc - X  ->  parts -> LDS
  auto exchange_r = [&]() {
    float v[4][2][4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          v[nb][n][k] = sub_rn(Racc[nb][n][k], Xr[nb][n][k]);
          if (F16) v[nb][n][k] *= r_scale;
        }
    if (F16) {
      // f16 range guard (see the 32x32x16 kernel), per patch: a lane decides
      // for each of its two patches on its own
      float f[2] = {1.f, 1.f};
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        float m = 0.f;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
          for (int k = 0; k < 4; ++k) m = fmaxf(m, fabsf(v[nb][n][k]));
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        const int row = 16 * n + c;
        if (xr_calls > 0) {
          const float* prev = Stat + ((xr_calls - 1) & 1) * 128;
          const float Mx = fmaxf(fmaxf(prev[row], prev[32 + row]),
                                 fmaxf(prev[64 + row], prev[96 + row]));
          if (Mx > 2048.f && Mx < __builtin_inff())
            f[n] = ldexpf(1.f, 9 - ilogbf(Mx));
        }
        if (q == 0) Stat[(xr_calls & 1) * 128 + w * 32 + row] = m * f[n];
      }
      ++xr_calls;
      if (__any(f[0] != 1.f || f[1] != 1.f)) {
#pragma unroll
        for (int p = 0; p < NPH; ++p)
#pragma unroll
          for (int e = 0; e < 16; ++e) Y[p][e] *= f[(e >> 2) & 1];
#pragma unroll
        for (int p = 0; p < CR; ++p)
#pragma unroll
          for (int e = 0; e < 16; ++e) Cr[p][e] *= f[(e >> 2) & 1];
#pragma unroll
        for (int pl = 0; pl < L::CL; ++pl)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            float4* c4 = reinterpret_cast<float4*>(Cst + cst_ln + pl * 16384 +
                                                   g * 1024);
            float4 cc = *c4;
            const float fg = f[g & 1];
            cc.x *= fg; cc.y *= fg; cc.z *= fg; cc.w *= fg;
            *c4 = cc;
          }
#pragma unroll
        for (int n = 0; n < 2; ++n) {
#pragma unroll
          for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              Xr[nb][n][k] *= f[n];
              v[nb][n][k] *= f[n];
            }
          cutoff_l[n] *= f[n];
          inv_sigma_y[n] *= 1.f / f[n];
        }
      }
    }
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const float v4[4] = {v[nb][n][0], v[nb][n][1], v[nb][n][2], v[nb][n][3]};
        uint2 hi, lo;
        split_group<F16, NP == 2>(v4, hi, lo);
        char* dst = Rx + rx_wr + 32 * nb + kRxHalf * n;
        *reinterpret_cast<uint2*>(dst) = hi;
        if (NP == 2) *reinterpret_cast<uint2*>(dst + kRxPart) = lo;
      }
    }
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int k = 0; k < 4; ++k) Racc[nb][n][k] = 0.f;
    __syncthreads();
  };

  // EARLY_R: exchange_r in pieces, the same operations on the same values.
  // The guard factor depends on the previous call's Stat row only, so it is
  // known before any block; a block is published as soon as its accumulators
  // are final (times the factor: times 1 where exchange_r skips the product);
  // the rescaling of the state and this call's maxima wait for the last block.
  float xf[2] = {1.f, 1.f}, xm[2] = {0.f, 0.f};
  auto exchange_guard = [&]() {
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      xf[n] = 1.f;
      xm[n] = 0.f;
      if (F16 && xr_calls > 0) {
        const int row = 16 * n + c;
        const float* prev = Stat + ((xr_calls - 1) & 1) * 128;
        const float Mx = fmaxf(fmaxf(prev[row], prev[32 + row]),
                               fmaxf(prev[64 + row], prev[96 + row]));
        if (Mx > 2048.f && Mx < __builtin_inff())
          xf[n] = ldexpf(1.f, 9 - ilogbf(Mx));
      }
    }
  };
  // in two stages, for one (block, patch half) under two positions: a the
  // values (xv), b their parts into LDS
  float xv[4];
  auto exchange_block_a = [&](int nb, int n) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      xv[k] = sub_rn(Racc[nb][n][k], Xr[nb][n][k]);
      if (F16) {
        xv[k] *= r_scale;
        xm[n] = fmaxf(xm[n], fabsf(xv[k]));
        xv[k] *= xf[n];
      }
      Racc[nb][n][k] = 0.f;
    }
  };
  auto exchange_block_b = [&](int nb, int n) {
    uint2 hi, lo;
    split_group<F16, NP == 2>(xv, hi, lo);
    char* dst = Rx + rx_wr + 32 * nb + kRxHalf * n;
    *reinterpret_cast<uint2*>(dst) = hi;
    if (NP == 2) *reinterpret_cast<uint2*>(dst + kRxPart) = lo;
  };
  auto exchange_block = [&](int nb, int n) {
    exchange_block_a(nb, n);
    exchange_block_b(nb, n);
  };
  // blocks nb0.. (the ones no MFMA gap took), then the state
  auto exchange_finish = [&](int nb0) {
#pragma unroll
    for (int nb = nb0; nb < 4; ++nb)
#pragma unroll
      for (int n = 0; n < 2; ++n) exchange_block(nb, n);
    if (F16) {
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        float m = xm[n];
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        if (q == 0) Stat[(xr_calls & 1) * 128 + w * 32 + 16 * n + c] = m * xf[n];
      }
      ++xr_calls;
      if (__any(xf[0] != 1.f || xf[1] != 1.f)) {
#pragma unroll
        for (int p = 0; p < NPH; ++p)
#pragma unroll
          for (int e = 0; e < 16; ++e) Y[p][e] *= xf[(e >> 2) & 1];
#pragma unroll
        for (int p = 0; p < CR; ++p)
#pragma unroll
          for (int e = 0; e < 16; ++e) Cr[p][e] *= xf[(e >> 2) & 1];
#pragma unroll
        for (int pl = 0; pl < L::CL; ++pl)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            float4* c4 = reinterpret_cast<float4*>(Cst + cst_ln + pl * 16384 +
                                                   g * 1024);
            float4 cc = *c4;
            const float fg = xf[g & 1];
            cc.x *= fg; cc.y *= fg; cc.z *= fg; cc.w *= fg;
            *c4 = cc;
          }
#pragma unroll
        for (int n = 0; n < 2; ++n) {
#pragma unroll
          for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int k = 0; k < 4; ++k) Xr[nb][n][k] *= xf[n];
          cutoff_l[n] *= xf[n];
          inv_sigma_y[n] *= 1.f / xf[n];
        }
      }
    }
    __syncthreads();
  };

  // EARLY_R: the iteration's last step 3, block-major: position i is k-step
  // (i >> 1) & 3 of pixel block 2 (i >> 3) + (i & 1), so that blocks 0 and 1
  // are final after position 7 (each accumulator still sums its k-steps in
  // ascending order) and their exchange rides on positions 8..15.  The B
  // operands are read twice, one patch half under each position of a k-step.
  auto step3_last = [&](int buf, int sg) {
    uint4 yb[2][NP], yb_next[2][NP];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int part = 0; part < NP; ++part)
        yb_next[n][part] = *reinterpret_cast<const uint4*>(
            Yx + (buf * NP + part) * kYxPart + yx_rd + kYxHalf * n);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int j = i & 1, nb = VTC_T_NB(sg, i);
      if (j == 0) {
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int part = 0; part < NP; ++part) yb[n][part] = yb_next[n][part];
      }
      if (i + 2 < 16) {
#pragma unroll
        for (int part = 0; part < NP; ++part)
          yb_next[j][part] = *reinterpret_cast<const uint4*>(
              Yx + (buf * NP + part) * kYxPart + yx_rd + kYxHalf * j +
              64 * VTC_T_KS(sg, i + 2));
      }
      uint4 a[NP];
#pragma unroll
      for (int part = 0; part < NP; ++part) a[part] = ring[part][i % RING];
      VTC_MFMA_PAIR(Racc[nb][0], Racc[nb][1], a, yb)
      if (i == 6) {
        exchange_guard();
        __builtin_amdgcn_sched_barrier(0);
      }
      if (i >= 8) {
        if (j == 0)
          exchange_block_a((i - 8) >> 2, ((i - 8) >> 1) & 1);
        else
          exchange_block_b((i - 8) >> 2, ((i - 8) >> 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
      }
      VTC_REFILL(sg, i)
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  // ---- R_0 = Y_0 D - X ---------------------------------------------------
  if (warm) {
#pragma unroll
    for (int p = 0; p < NPH; ++p) {
#pragma unroll
      for (int g = 0; g < 4; ++g) publish_group(Y[p], g, p & 1);
      __syncthreads();
      step3(p, p & 1, false, 0, nothing);
    }
  }
  exchange_r();

#pragma unroll
  for (int i = 0; i < RING; ++i)
#pragma unroll
    for (int part = 0; part < NP; ++part)
      ring[part][i] = VTC_LOAD_SEG(part, 0, i);

  // (the variant is compiled in: ISTA has no momentum arithmetic, FISTA no select)
  unsigned long long acc_t[5] = {0, 0, 0, 0, 0};
  unsigned long long t0 = 0, t1 = 0;
#define VTC_STAMP(slot)                    \
  if (STAMP) {                             \
    t1 = stamp_now();                      \
    acc_t[slot] += t1 - t0;                \
    t0 = t1;                               \
  }
  if (STAMP) t0 = stamp_now();

  f32x4 Gb[2][4];    // gradient tiles of two consecutive phases, [g = 2m + n]
  float4 cold4;
  float cn4[4];

  // Proximal step + extrapolation for element e = 4g + k of phase p
  auto epilogue_elem = [&](int p, int e, const f32x4 (&Gp)[4], float beta) {
    const int g = e >> 2, k = e & 3;
    if (MODE == 7) {         // diagnostic: step 1 with (almost) no epilogue work
      const float cn = Y[p][e] + Gp[g][k];
      Y[p][e] = cn;
      cn4[k] = cn;
      if (k == 3) {
        if (p < CREG) {
#pragma unroll
          for (int j = 0; j < 4; ++j) Cr[p < CREG ? p : 0][4 * g + j] = cn4[j];
        } else {
          *reinterpret_cast<float4*>(Cst + cst_ln + (p - CREG) * 16384 +
                                     g * 1024) =
              make_float4(cn4[0], cn4[1], cn4[2], cn4[3]);
        }
      }
      return;
    }
    if (k == 0) {
      if (p < CREG) {
        cold4 = make_float4(Cr[p < CREG ? p : 0][4 * g + 0],
                            Cr[p < CREG ? p : 0][4 * g + 1],
                            Cr[p < CREG ? p : 0][4 * g + 2],
                            Cr[p < CREG ? p : 0][4 * g + 3]);
      } else {
        cold4 = *reinterpret_cast<const float4*>(
            Cst + cst_ln + (p - CREG) * 16384 + g * 1024);
      }
    }
    const float co = (k == 0) ? cold4.x : (k == 1) ? cold4.y
                   : (k == 2) ? cold4.z : cold4.w;
    const float cv = sub_rn(Y[p][e], mul_rn(eta, Gp[g][k]));
    const float cn = shrink_fast<MODE>(cv, cutoff_l[g & 1]);
    // ISTA: y = codes (ista_fista.py:133), not codes + 0 * (codes - old):
    // a code that has overflowed to inf stays inf as it does there
    if constexpr (FISTA)
      Y[p][e] = add_rn(cn, mul_rn(beta, sub_rn(cn, co)));
    else
      Y[p][e] = cn;
    cn4[k] = cn;
    if (k == 3) {
      if (p < CREG) {
#pragma unroll
        for (int j = 0; j < 4; ++j) Cr[p < CREG ? p : 0][4 * g + j] = cn4[j];
      } else {
        *reinterpret_cast<float4*>(Cst + cst_ln + (p - CREG) * 16384 +
                                   g * 1024) =
            make_float4(cn4[0], cn4[1], cn4[2], cn4[3]);
      }
      publish_group(Y[p], g, p & 1);
    }
  };
  // SPREAD: epilogue_elem in two stages, the same operations on the same
  // values, for one element under two positions: a position then carries about
  // seven VALU instructions, which fit the issue gaps its MFMAs leave.
  // a: the proximal step (cn4[k]); b: extrapolation, C and the publication.
  auto epilogue_stage_a = [&](int p, int e, const f32x4 (&Gp)[4]) {
    const int g = e >> 2, k = e & 3;
    if (MODE == 7) {
      cn4[k] = Y[p][e] + Gp[g][k];
      return;
    }
    if (k == 0) {
      if (p < CREG) {
        cold4 = make_float4(Cr[p < CREG ? p : 0][4 * g + 0],
                            Cr[p < CREG ? p : 0][4 * g + 1],
                            Cr[p < CREG ? p : 0][4 * g + 2],
                            Cr[p < CREG ? p : 0][4 * g + 3]);
      } else {
        cold4 = *reinterpret_cast<const float4*>(
            Cst + cst_ln + (p - CREG) * 16384 + g * 1024);
      }
    }
    const float cv = sub_rn(Y[p][e], mul_rn(eta, Gp[g][k]));
    cn4[k] = shrink_fast<MODE>(cv, cutoff_l[g & 1]);
  };
  auto epilogue_stage_b = [&](int p, int e, float beta) {
    const int g = e >> 2, k = e & 3;
    const float cn = cn4[k];
    if (MODE == 7) {
      Y[p][e] = cn;
    } else {
      const float co = (k == 0) ? cold4.x : (k == 1) ? cold4.y
                     : (k == 2) ? cold4.z : cold4.w;
      if constexpr (FISTA)
        Y[p][e] = add_rn(cn, mul_rn(beta, sub_rn(cn, co)));
      else
        Y[p][e] = cn;
    }
    if (k == 3) {
      if (p < CREG) {
#pragma unroll
        for (int j = 0; j < 4; ++j) Cr[p < CREG ? p : 0][4 * g + j] = cn4[j];
      } else {
        *reinterpret_cast<float4*>(Cst + cst_ln + (p - CREG) * 16384 +
                                   g * 1024) =
            make_float4(cn4[0], cn4[1], cn4[2], cn4[3]);
      }
      if (MODE != 7) publish_group(Y[p], g, p & 1);
    }
  };
  // position i of a segment that carries half an epilogue: element
  // e0 + (i >> 1), stage a under the even position, stage b under the odd one
  auto epilogue_half = [&](int p, int e0, int i, const f32x4 (&Gp)[4],
                           float beta) {
    if ((i & 1) == 0)
      epilogue_stage_a(p, e0 + (i >> 1), Gp);
    else
      epilogue_stage_b(p, e0 + (i >> 1), beta);
  };

  // step 1 of phase p (stream segment sg): Gb[p&1] = D[tile] R_k; position
  // i = 2 ks + m.  The B operands of k-step ks + 1 are fetched under the two
  // positions of k-step ks, one patch half each.  overlap: 0 nothing, 1 the
  // epilogue of phase p - 1, 2 (SPREAD) its groups 2 and 3, half an element
  // under every position.
  auto step1 = [&](int p, int sg, int overlap, float beta) {
    f32x4 (&G)[4] = Gb[p & 1];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int k = 0; k < 4; ++k) G[g][k] = 0.f;
    uint4 rb[2][NP], rb_next[2][NP];
    if constexpr (KRES == 0) {
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int part = 0; part < NP; ++part)
          rb_next[n][part] = *reinterpret_cast<const uint4*>(
              Rx + part * kRxPart + rx_rd + kRxHalf * n);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int ks = i >> 1, m = i & 1;
      if (m == 0) {
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int part = 0; part < NP; ++part)
            rb[n][part] = ks < KRES ? rres[ks < KRES ? ks : 0][n][part]
                                    : rb_next[n][part];
      }
      // (the resident k-steps need no fetch: the first one under way is that
      // of k-step KRES, under the positions of k-step KRES - 1)
      if (ks + 1 < 8 && ks + 1 >= KRES) {
#pragma unroll
        for (int part = 0; part < NP; ++part)
          rb_next[m][part] = *reinterpret_cast<const uint4*>(
              Rx + part * kRxPart + rx_rd + kRxHalf * m + 64 * (ks + 1));
      }
      uint4 a[NP];
#pragma unroll
      for (int part = 0; part < NP; ++part) a[part] = ring[part][i % RING];
      VTC_MFMA_PAIR(G[2 * m], G[2 * m + 1], a, rb)
      if (overlap == 1) {
        epilogue_elem(p - 1, i, Gb[(p - 1) & 1], beta);
        __builtin_amdgcn_sched_barrier(0);
      } else if (overlap == 2) {
        epilogue_half(p - 1, 8, i, Gb[(p - 1) & 1], beta);
        __builtin_amdgcn_sched_barrier(0);
      }
      VTC_REFILL(sg, i)
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  for (int it = 0; it < P.num_iters; ++it) {
    float beta = 0.f;
    if constexpr (FISTA) beta = P.betas[it];
    // KRES: R_k is final and visible (the exchange's closing barrier is behind
    // us, the range guard's factor already in the published parts) and does
    // not change until this iteration's exchange, which follows every step 1
    if constexpr (KRES > 0) {
#pragma unroll
      for (int ks = 0; ks < KRES; ++ks)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int part = 0; part < NP; ++part)
            rres[ks][n][part] = *reinterpret_cast<const uint4*>(
                Rx + part * kRxPart + rx_rd + kRxHalf * n + 64 * ks);
    }
    step1(0, 0, 0, beta);
    VTC_STAMP(0)
#pragma unroll
    for (int p = 0; p < NPH; ++p) {
      if (p + 1 < NPH) {
        // + epilogue of phase p; SPREAD: of a middle phase the half that
        // step 3(p - 1) left
        step1(p + 1, 2 * p + 1, (SPREAD && p > 0) ? 2 : 1, beta);
        VTC_STAMP(0)
      }
      __syncthreads();
      VTC_STAMP(2)
      if (p + 2 == NPH) {
        step3(p, p & 1, true, 2 * p + 2, [&](int i) {
          epilogue_elem(NPH - 1, i, Gb[(NPH - 1) & 1], beta);
          __builtin_amdgcn_sched_barrier(0);
        });
      } else if (SPREAD && p + 2 < NPH) {
        // groups 0 and 1 of the middle phase p + 1: G(p + 1) is complete, and
        // the barrier above put the last readers of exchange buffer (p + 1) & 1
        // (step 3(p - 1)) behind us
        step3(p, p & 1, true, 2 * p + 2, [&](int i) {
          epilogue_half(p + 1, 0, i, Gb[(p + 1) & 1], beta);
          __builtin_amdgcn_sched_barrier(0);
        });
      } else if (EARLY_R && p + 1 == NPH) {
        step3_last(p & 1, 2 * NPH - 1);
      } else {
        step3(p, p & 1, true, (p + 1 < NPH) ? 2 * p + 2 : 2 * NPH - 1, nothing);
      }
      VTC_STAMP(3)
    }
    if (EARLY_R)
      exchange_finish(2);
    else
      exchange_r();
    VTC_STAMP(4)
  }
  if (STAMP && lane == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) atomicAdd(P.stamps + k, acc_t[k]);
    atomicAdd(P.stamps + 7, 1ull);
  }
#undef VTC_STAMP

  // ---- codes out: the last C -----------------------------------------
#pragma unroll
  for (int p = 0; p < NPH; ++p) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float4 v;
      if (p < CREG) {
        v = make_float4(Cr[p < CREG ? p : 0][4 * g + 0],
                        Cr[p < CREG ? p : 0][4 * g + 1],
                        Cr[p < CREG ? p : 0][4 * g + 2],
                        Cr[p < CREG ? p : 0][4 * g + 3]);
      } else {
        v = *reinterpret_cast<const float4*>(Cst + cst_ln +
                                             (p - CREG) * 16384 + g * 1024);
      }
      if (F16) {
        v.x *= inv_sigma_y[g & 1];
        v.y *= inv_sigma_y[g & 1];
        v.z *= inv_sigma_y[g & 1];
        v.w *= inv_sigma_y[g & 1];
      }
      if (live[g & 1])
        *reinterpret_cast<float4*>(P.codes + patch[g & 1] * s + kPhaseAtoms * p +
                                   32 * w + 16 * (g >> 1) + 4 * q) = v;
    }
  }
#undef VTC_LOAD_A
#undef VTC_LOAD_T
#undef VTC_LOAD_SEG
#undef VTC_REFILL
#undef VTC_MFMA_PAIR
#undef VTC_SEG_IS_T
#undef VTC_SEG_PHASE
#undef VTC_SEG_BLOCK_MAJOR
#undef VTC_T_NB
#undef VTC_T_KS
}

}  // namespace vtc

namespace vtc {

// -------------------------------------------------------------------- host
static int phases_for(int64_t s) { return (int)(s / kPhaseAtoms); }

bool fused_shape_supported(int64_t b, int64_t n, int64_t s, int precision) {
  if (n != kFN || b <= 0) return false;
  if (s % kPhaseAtoms != 0) return false;
  const int nph = phases_for(s);
  if (!(nph == 2 || nph == 4 || nph == 8)) return false;
  return precision == VTC_BF16 || precision == VTC_BF16X3 ||
         precision == VTC_F16X3;
}

// operand parts of a precision: bf16 packs hi only, the split modes hi and lo
static int fused_parts(int precision) { return precision == VTC_BF16 ? 1 : 2; }

// Scratch of the fused kernel: per part the dictionary packed for step 1 and
// for step 3, then {sigma_D, 1 / sigma_D} of the f16 split.
struct FusedLayout {
  unsigned short* packs[4] = {nullptr, nullptr, nullptr, nullptr};
  float* dscale;
  FusedLayout(Carver& ws, int64_t s, int parts) {
    for (int part = 0; part < parts; ++part) {
      packs[2 * part] = ws.take<unsigned short>((size_t)s * kFN);
      packs[2 * part + 1] = ws.take<unsigned short>((size_t)s * kFN);
    }
    dscale = ws.take<float>(2);
  }
};

size_t fused_workspace_bytes(int64_t b, int64_t n, int64_t s, int precision) {
  if (!fused_shape_supported(b, n, s, precision)) return 256;
  return measured_bytes<FusedLayout>(s, fused_parts(precision));
}

// Which MFMA tile a precision runs on by default
// (profiles/fused_mfma_shape.txt).  VTC_FUSED_TILE=32|16 forces
// one (a diagnostic switch, read on every call so that one process can run
// both).
static bool default_tile16(int precision) {
  // f16x3 and bf16: 16x16x32 is 6 % faster at the benchmark shape.  bf16x3 is
  // as well (6.7 %) but stays on 32x32x16: on the other tile one
  // hard-threshold case of the suite lands outside its gate (a flip in an
  // intermediate iterate moves the codes by 6e-4).
  return precision == VTC_F16X3 || precision == VTC_BF16;
}
static bool use_tile16(int precision) {
  const char* v = getenv("VTC_FUSED_TILE");
  if (v && v[0] == '1' && v[1] == '6' && v[2] == 0) return true;
  if (v && v[0] == '3' && v[1] == '2' && v[2] == 0) return false;
  return default_tile16(precision);
}

// Which schedule the 16x16x32 kernel runs by default: the spread epilogue for
// f16x3 and bf16 (0.9 % and 2.8 % faster per step at the benchmark shape,
// profiles/fused_epilogue_spread.txt) with the resident residual operand
// (another 1.1 % and 1.1 %, profiles/fused_resident_operand.txt); the early
// exchange is no gain and stays off, bf16x3 on this tile is a forced arm and
// was not measured.
template <int NP, bool F16>
constexpr int default_sched() {
  return (F16 || NP == 1) ? (1 | 4) : 0;
}
// VTC_FUSED_SCHED=0..7 forces a schedule: bit 0 spreads the epilogue of the
// middle phases, bit 1 starts the residual exchange under the iteration's last
// step 3, bit 2 keeps step 1's first residual operands in registers (a
// diagnostic switch, read on every call, as VTC_FUSED_TILE is).  The 32x32x16
// kernel has one schedule.
static int use_sched(int by_default) {
  const char* v = getenv("VTC_FUSED_SCHED");
  if (v && v[0] >= '0' && v[0] <= '7' && v[1] == 0) return v[0] - '0';
  return by_default;
}

// FISTA: the variant of the 16x16x32 kernel; the 32x32x16 kernel reads
// P.fista and has the one instantiation (FISTA = true here).
template <int NPH, int NP, int MODE, bool F16, bool STAMP, bool TILE16,
          int SCHED, bool FISTA>
static auto fused_kernel() {
  static_assert(TILE16 || (SCHED == 0 && FISTA),
                "schedules and variants exist on the 16x16x32 tile");
  if constexpr (TILE16)
    return fused_fista_kernel16<NPH, NP, MODE, F16, STAMP, SCHED, FISTA>;
  else
    return fused_fista_kernel<NPH, NP, MODE, F16, STAMP>;
}

template <int NPH, int NP, int MODE, bool F16, bool TILE16, int SCHED,
          bool FISTA>
static int launch_fused(const FusedParams& P, hipStream_t st) {
  using L = FusedLds<NPH, NP>;
  auto kernel = fused_kernel<NPH, NP, MODE, F16, false, TILE16, SCHED, FISTA>();
  static unsigned long long configured = 0;
  if (first_use_on_this_device(&configured)) {
    VTC_HIP_CHECK(hipFuncSetAttribute(
        reinterpret_cast<const void*>(kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize, L::total));
  }
  const unsigned grid = (unsigned)ceil_div(P.b, kFP);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), L::total, st, P);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

// Diagnostic: VTC_FUSED_STAMPS=1 runs the stamped instantiation (soft
// threshold, FISTA only) and prints per-segment cycle shares.  Its run time is
// not representative (the stamps fence the schedule); read the shares only.
template <int NPH, int NP, bool F16, bool TILE16, int SCHED>
static int launch_stamped(FusedParams P, hipStream_t st) {
  using L = FusedLds<NPH, NP>;
  static const bool no_epilogue = getenv("VTC_FUSED_NOEPI") != nullptr;
  auto kernel =
      no_epilogue
          ? fused_kernel<NPH, NP, 7, F16, true, TILE16, SCHED, true>()
          : fused_kernel<NPH, NP, VTC_SOFT, F16, true, TILE16, SCHED, true>();
  unsigned long long* dev = nullptr;
  VTC_HIP_CHECK(hipMalloc(&dev, 8 * sizeof(unsigned long long)));
  VTC_HIP_CHECK(hipMemsetAsync(dev, 0, 8 * sizeof(unsigned long long), st));
  VTC_HIP_CHECK(hipFuncSetAttribute(
      reinterpret_cast<const void*>(kernel),
      hipFuncAttributeMaxDynamicSharedMemorySize, L::total));
  P.stamps = dev;
  hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div(P.b, kFP)), dim3(256),
                     L::total, st, P);
  VTC_LAUNCH_CHECK();
  unsigned long long host[8];
  VTC_HIP_CHECK(hipMemcpyAsync(host, dev, sizeof(host), hipMemcpyDeviceToHost,
                               st));
  VTC_HIP_CHECK(hipStreamSynchronize(st));
  VTC_HIP_CHECK(hipFree(dev));
  const char* names[5] = {"step1+epi", "epi-alone", "barrier", "step3",
                          "exchange"};
  double total = 0;
  for (int k = 0; k < 5; ++k) total += (double)host[k];
  const double per = (double)host[7] * P.num_iters * NPH;
  for (int k = 0; k < 5; ++k)
    fprintf(stderr, "[vtc stamps] %-9s %5.1f%%  %8.0f cycles/phase/wave\n",
            names[k], 100.0 * host[k] / total, host[k] / per);
  return VTC_OK;
}

template <int NPH, int NP, bool F16, bool TILE16, int SCHED, bool FISTA>
static int dispatch_threshold(const FusedParams& P, int threshold,
                              hipStream_t st) {
  switch (threshold) {
    case VTC_SOFT:
      return launch_fused<NPH, NP, VTC_SOFT, F16, TILE16, SCHED, FISTA>(P, st);
    case VTC_SOFT_NONNEG:
      return launch_fused<NPH, NP, VTC_SOFT_NONNEG, F16, TILE16, SCHED, FISTA>(
          P, st);
    case VTC_HARD:
      return launch_fused<NPH, NP, VTC_HARD, F16, TILE16, SCHED, FISTA>(P, st);
    default:
      return launch_fused<NPH, NP, VTC_HARD_NONNEG, F16, TILE16, SCHED, FISTA>(
          P, st);
  }
}

template <int NPH, int NP, bool F16, bool TILE16, int SCHED>
static int dispatch_mode(const FusedParams& P, int threshold, hipStream_t st) {
  static const bool stamps = getenv("VTC_FUSED_STAMPS") != nullptr;
  // the stamped run is of the benchmark's shape; schedule 0 keeps the
  // instantiations it always had
  if constexpr (SCHED == 0 || (NPH == 8 && NP == 2)) {
    if (stamps && threshold == VTC_SOFT && NPH == 8 && NP == 2 &&
        (P.fista || !TILE16))
      return launch_stamped<NPH, NP, F16, TILE16, SCHED>(P, st);
  }
  if constexpr (TILE16) {
    if (!P.fista)
      return dispatch_threshold<NPH, NP, F16, TILE16, SCHED, false>(
          P, threshold, st);
  }
  return dispatch_threshold<NPH, NP, F16, TILE16, SCHED, true>(P, threshold,
                                                               st);
}

// The schedule of a call: one on the 32x32x16 tile; on the other the switch's
// or the default, without bit 0 where there is no middle phase (NPH = 2).
template <int NPH, int NP, bool F16, bool TILE16>
static int dispatch_sched(const FusedParams& P, int threshold,
                          hipStream_t st) {
  if constexpr (TILE16) {
    int sched = use_sched(default_sched<NP, F16>());
    if (NPH == 2) sched &= ~1;
    if constexpr (NPH > 2) {
      switch (sched) {
        case 1: return dispatch_mode<NPH, NP, F16, TILE16, 1>(P, threshold, st);
        case 3: return dispatch_mode<NPH, NP, F16, TILE16, 3>(P, threshold, st);
        case 5: return dispatch_mode<NPH, NP, F16, TILE16, 5>(P, threshold, st);
        case 7: return dispatch_mode<NPH, NP, F16, TILE16, 7>(P, threshold, st);
      }
    }
    switch (sched) {
      case 2: return dispatch_mode<NPH, NP, F16, TILE16, 2>(P, threshold, st);
      case 4: return dispatch_mode<NPH, NP, F16, TILE16, 4>(P, threshold, st);
      case 6: return dispatch_mode<NPH, NP, F16, TILE16, 6>(P, threshold, st);
    }
  }
  return dispatch_mode<NPH, NP, F16, TILE16, 0>(P, threshold, st);
}

template <int NP, bool F16, bool TILE16>
static int dispatch_phases(const FusedParams& P, int threshold,
                           hipStream_t st) {
  switch (phases_for(P.s)) {
    case 2: return dispatch_sched<2, NP, F16, TILE16>(P, threshold, st);
    case 4: return dispatch_sched<4, NP, F16, TILE16>(P, threshold, st);
    case 8: return dispatch_sched<8, NP, F16, TILE16>(P, threshold, st);
  }
  set_error("fused FISTA: unsupported atom count %d", P.s);
  return VTC_ERR_UNSUPPORTED;
}

// The FISTA momentum table beta_k = (t_k - 1) / t_{k+1} (ista_fista.py:123-127,
// float64 recurrence rounded to f32) does not depend on the call: one copy per
// device, placed by vtc_init() -- or by the first inference call on a device
// nobody prepared (one hipMalloc and a blocking 64 KiB copy, under a lock);
// afterwards a call only enqueues.
constexpr int kBetaTable = 16384;
const float* fista_beta_table_on_this_device() {
  static float* tables[64] = {nullptr};
  static std::mutex guard;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return nullptr;
  std::lock_guard<std::mutex> lock(guard);
  if (tables[dev]) return tables[dev];
  std::vector<float> host;
  fista_betas(kBetaTable, &host);
  float* table = nullptr;
  if (hipMalloc(&table, sizeof(float) * kBetaTable) != hipSuccess)
    return nullptr;
  if (hipMemcpy(table, host.data(), sizeof(float) * kBetaTable,
                hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(table);
    return nullptr;
  }
  tables[dev] = table;
  return table;
}

int fused_max_iters() { return kBetaTable; }

int run_fused(const float* images, const float* dictionary,
              const float* initial_codes, float* codes, int64_t b, int64_t n,
              int64_t s, float eta, const float* eta_dev,
              float sparsity_weight, int num_iters, int variant,
              int threshold, int precision, void* workspace,
              size_t workspace_bytes, int* iters_run, hipStream_t st) {
  if (!fused_shape_supported(b, n, s, precision)) {
    set_error("fused FISTA: unsupported shape");
    return VTC_ERR_UNSUPPORTED;
  }
  if (num_iters > kBetaTable) {
    set_error("fused FISTA: at most %d iterations per call", kBetaTable);
    return VTC_ERR_UNSUPPORTED;
  }
  if (!workspace ||
      workspace_bytes < fused_workspace_bytes(b, n, s, precision)) {
    set_error("fused FISTA: workspace too small");
    return VTC_ERR_WORKSPACE;
  }
  const float* betas_dev = fista_beta_table_on_this_device();
  if (!betas_dev) {
    set_error("fused FISTA: could not place the momentum table on the device");
    return VTC_ERR_HIP;
  }
  const int parts = fused_parts(precision);
  const bool f16 = (precision == VTC_F16X3);
  Carver ws(workspace);
  FusedParams P;
  const FusedLayout L(ws, s, parts);
  unsigned short* const* packs = L.packs;
  float* dscale = L.dscale;
  if (f16) {
    hipLaunchKernelGGL(dictionary_scale_kernel, dim3(1), dim3(1024), 0, st,
                       dictionary, (int64_t)s * kFN, dscale);
    VTC_LAUNCH_CHECK();
  }
  const bool tile16 = use_tile16(precision);
  auto pack = f16 ? (tile16 ? pack_dictionary_kernel<true, true>
                            : pack_dictionary_kernel<true, false>)
                  : (tile16 ? pack_dictionary_kernel<false, true>
                            : pack_dictionary_kernel<false, false>);
  hipLaunchKernelGGL(pack, dim3(256), dim3(256), 0, st, dictionary, (int)s,
                     packs[0], packs[1], packs[2], packs[3], dscale);
  VTC_LAUNCH_CHECK();
  P.images = images;
  P.init = initial_codes;
  P.codes = codes;
  for (int part = 0; part < 2; ++part) {
    P.packA[part] = reinterpret_cast<const uint4*>(packs[2 * (part % parts)]);
    P.packT[part] =
        reinterpret_cast<const uint4*>(packs[2 * (part % parts) + 1]);
  }
  P.betas = betas_dev;
  P.b = b;
  P.s = (int)s;
  P.num_iters = num_iters;
  P.fista = (variant == VTC_FISTA) ? 1 : 0;
  P.eta = eta;
  P.eta_dev = eta_dev;
  P.lam = sparsity_weight;
  // lambda * eta: the Python float rounded to f32, then one f32 multiply
  P.cutoff = sparsity_weight * eta;
  P.dscale = dscale;
  P.stamps = nullptr;
  int rc;
  if (tile16)
    rc = f16          ? dispatch_phases<2, true, true>(P, threshold, st)
         : parts == 2 ? dispatch_phases<2, false, true>(P, threshold, st)
                      : dispatch_phases<1, false, true>(P, threshold, st);
  else
    rc = f16          ? dispatch_phases<2, true, false>(P, threshold, st)
         : parts == 2 ? dispatch_phases<2, false, false>(P, threshold, st)
                      : dispatch_phases<1, false, false>(P, threshold, st);
  if (rc == VTC_OK && iters_run) *iters_run = num_iters;
  return rc;
}

}  // namespace vtc

extern "C" int vtc_init(void) {
  if (!vtc::fista_beta_table_on_this_device()) {
    vtc::set_error("vtc_init: could not place the momentum table on the device");
    return VTC_ERR_HIP;
  }
  return VTC_OK;
}
