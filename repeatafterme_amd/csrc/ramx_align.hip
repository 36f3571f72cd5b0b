// ramx_align.hip -- fifth translation unit of libramx's device code: the traceback replay of an extension along a given
// consensus (ramx_kernels_align.h) and its launchers.  Kept apart so that the translation units compile side by side.
#define RAMX_SECONDARY_TU 1
#include "ramx_kernels_align.h"

int ramx_align_launch_forward(hipStream_t st, int ntiles, const AlnArgs &aa)
{
  if (ntiles <= 0) return RAMX_OK;
  hipLaunchKernelGGL(ramx_align_forward_kernel, dim3(ntiles), dim3(64), 0, st, aa);
  return hipGetLastError() != hipSuccess ? RAMX_ERR_HIP : RAMX_OK;
}

int ramx_align_launch_walk(hipStream_t st, int ntiles, const AlnArgs &aa)
{
  if (ntiles <= 0) return RAMX_OK;
  hipLaunchKernelGGL(ramx_align_walk_kernel, dim3(ntiles), dim3(64), 0, st, aa);
  return hipGetLastError() != hipSuccess ? RAMX_ERR_HIP : RAMX_OK;
}

int ramx_align_launch_preset(hipStream_t st, int *col_idx, int *col_ins, size_t count)
{
  if (count == 0) return RAMX_OK;
  hipLaunchKernelGGL(ramx_align_preset_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, col_idx, col_ins, count);
  return hipGetLastError() != hipSuccess ? RAMX_ERR_HIP : RAMX_OK;
}
