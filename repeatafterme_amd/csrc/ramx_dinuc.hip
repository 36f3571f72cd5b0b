// ramx_dinuc.hip -- translation unit of libramx's device code for the dinucleotide pileup of an extension along a given
// consensus (ramx_kernels_dinuc.h) and its launchers.  Kept apart so that the translation units compile side by side.
#define RAMX_SECONDARY_TU 1
#include "ramx_kernels_dinuc.h"

int ramx_dinuc_launch(hipStream_t st, int ntiles, const DinucArgs &da)
{
  if (ntiles <= 0) return RAMX_OK;
  hipLaunchKernelGGL(ramx_dinuc_kernel, dim3(ntiles), dim3(64), 0, st, da);
  return hipGetLastError() != hipSuccess ? RAMX_ERR_HIP : RAMX_OK;
}

int ramx_dinuc_launch_sum(hipStream_t st, int n_families, int maxrows, const DinucSumArgs &sa)
{
  if (n_families <= 0 || maxrows <= 0) return RAMX_OK;
  hipLaunchKernelGGL(ramx_dinuc_sum_kernel, dim3(n_families, (maxrows + 255) / 256), dim3(256), 0, st, sa);
  return hipGetLastError() != hipSuccess ? RAMX_ERR_HIP : RAMX_OK;
}
