// ramx_tsd.hip -- tenth translation unit of libramx's device code: the target-site duplications of the extended copies
// (ramx_kernels_tsd.h) and its launcher.  Kept apart so that the translation units compile side by side.
#define RAMX_SECONDARY_TU 1
#include "ramx_kernels_tsd.h"

int ramx_tsd_launch(hipStream_t st, const TsdArgs &ta)
{
  if (ta.n <= 0) return RAMX_OK;
  hipLaunchKernelGGL(ramx_tsd_kernel, dim3(ta.Np / 64), dim3(64), 0, st, ta);
  return hipGetLastError() != hipSuccess ? RAMX_ERR_HIP : RAMX_OK;
}
