// ramx_copystats.hip -- seventh translation unit of libramx's device code: the per-copy statistics of an extension along a given
// consensus (ramx_kernels_copystats.h) and its launcher.  Kept apart so that the translation units compile side by side.
#define RAMX_SECONDARY_TU 1
#include "ramx_kernels_copystats.h"

int ramx_copystats_launch(hipStream_t st, int ntiles, const CopyStatsArgs &ca)
{
  if (ntiles <= 0) return RAMX_OK;
  hipLaunchKernelGGL(ramx_copystats_kernel, dim3(ntiles), dim3(64), 0, st, ca);
  return hipGetLastError() != hipSuccess ? RAMX_ERR_HIP : RAMX_OK;
}
