// Version / error-string plumbing of libvtc_hip and the per-device CU count.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "common.h"

namespace vtc {
static thread_local char g_error[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
}

int compute_units() {
  constexpr int kMaxDevices = 64;
  static int cached[kMaxDevices] = {0};   // 0: not asked yet
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices)
    return 256;
  if (cached[dev] == 0)
    cached[dev] = (hipDeviceGetAttribute(
                       &n, hipDeviceAttributeMultiprocessorCount, dev) ==
                       hipSuccess && n > 0) ? n : 256;
  return cached[dev];
}
}  // namespace vtc

extern "C" const char* vtc_version(void) {
  return "vtc_hip 0.1 (gfx950)";
}
extern "C" const char* vtc_last_error(void) { return vtc::g_error; }
extern "C" int vtc_abi_version(void) { return VTC_ABI_VERSION; }
