// The dictionary gradient of the fully-connected update, G = C^T (C D - X), on
// the three-part bf16 contraction of gemm_b3.h (built without SLP
// vectorisation: packed f32 VALU beside MFMAs is slow, see the Makefile).
#include "gemm_b3.h"

namespace vtc {

template <bool A_KC, bool MINUS>
static int launch_gemm_b3(const GemmB3Args& g, bool two_sets, hipStream_t st) {
  const int64_t tiles_m = ceil_div(g.M, kB3BM), tiles_n = ceil_div(g.N, kB3BN);
  // the outer index of the block -> tile map is padded to a multiple of 8
  const int64_t blocks = g.slices > 1
                             ? ceil_div(g.slices, 8) * 8 * tiles_m * tiles_n
                             : ceil_div(tiles_m, 8) * 8 * tiles_n;
  if (blocks > 0x7fffffffLL) {
    set_error("gemm_b3: too many tiles");
    return VTC_ERR_INVALID_ARGUMENT;
  }
  if (two_sets)
    hipLaunchKernelGGL((gemm_b3_kernel<A_KC, MINUS, true>),
                       dim3((unsigned)blocks), dim3(256), 0, st, g);
  else
    hipLaunchKernelGGL((gemm_b3_kernel<A_KC, MINUS, false>),
                       dim3((unsigned)blocks), dim3(256), 0, st, g);
  VTC_LAUNCH_CHECK();
  return VTC_OK;
}

int launch_fc_gradient_b3(const float* images, const float* dictionary,
                          const float* codes, float* E, float* slabs,
                          int slices, int64_t b, int64_t n, int64_t s,
                          bool two_sets, hipStream_t st) {
  // E = C D - X      (M = b, N = n, K = s)
  GemmB3Args r{codes, dictionary, b, n, s, s, n, s, 1, E, images, n, 0};
  int rc = launch_gemm_b3<true, true>(r, two_sets, st);
  if (rc != VTC_OK) return rc;
  // slabs[z] = C^T E over slice z of the batch   (M = s, N = n, K = b)
  const int64_t chunk = ceil_div(ceil_div(b, slices), kGemmBK) * kGemmBK;
  GemmB3Args q{codes, E, s, n, b, s, n, chunk, slices, slabs, nullptr, n,
               s * n};
  return launch_gemm_b3<false, false>(q, two_sets, st);
}

}  // namespace vtc
