// The launch sequence of the kernels that use dynamic LDS: opt the kernel in to its largest LDS size (once per
// instantiation), launch, check.  The kernel is a template ARGUMENT, so a site names its instantiation once and the opt-in
// always lands on the kernel that is launched.  Header-inline: a launch gains no call level (the one-item training step
// is bound by the host side of its ~2900 launches).
#pragma once
#include "avt_common.h"

namespace avt {

// `max_bytes` must be the same on every call for one kernel: the attribute is set on the first call only.
template <auto Kernel>
inline int allow_dynamic_lds(int max_bytes, const char* who) {
  static const hipError_t e =
      hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, max_bytes);
  if (e != hipSuccess) {
    set_error("%s: hipFuncSetAttribute(%d B LDS): %s", who, max_bytes, hipGetErrorString(e));
    return AVT_ERR_LAUNCH;
  }
  return AVT_OK;
}

// lds_max = the opt-in (the largest size any call may ask for), lds_bytes = this launch's size (<= lds_max)
template <auto Kernel, class... A>
inline int launch(const char* who, dim3 grid, dim3 block, int lds_max, int lds_bytes, hipStream_t st, const A&... args) {
  const int rc = allow_dynamic_lds<Kernel>(lds_max, who);
  if (rc != AVT_OK) return rc;
  hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, st, args...);
  return check_launch(who);
}

}  // namespace avt
