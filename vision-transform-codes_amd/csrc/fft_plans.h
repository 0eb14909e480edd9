// hipFFT, opened with dlopen at first use (patches.hip): the float64 real
// round trip shared by vtc_whiten_center_surround and vtc_img_filter_fd.  The
// rest of the library has no link dependency on hipFFT.
#pragma once

#include <hipfft/hipfft.h>

namespace vtc {

struct FftApi {
  hipfftResult (*plan_many)(hipfftHandle*, int, int*, int*, int, int, int*,
                            int, int, hipfftType, int);
  hipfftResult (*exec_d2z)(hipfftHandle, hipfftDoubleReal*,
                           hipfftDoubleComplex*);
  hipfftResult (*exec_z2d)(hipfftHandle, hipfftDoubleComplex*,
                           hipfftDoubleReal*);
  hipfftResult (*set_stream)(hipfftHandle, hipStream_t);
  bool ok;
};

const FftApi& fft_api();

// batched 2D D2Z / Z2D pair over contiguous (batch, h, w) planes
struct FftPlans {
  hipfftHandle forward, inverse;
};

// plans are cached per (device, stream, h, w, batch) and bound to `st` when
// they are made: execute through them on that stream only
int get_plans(hipStream_t st, int h, int w, int batch, FftPlans* out);

}  // namespace vtc
