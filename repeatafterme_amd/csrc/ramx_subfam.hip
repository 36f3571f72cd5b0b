// ramx_subfam.hip -- ninth translation unit of libramx's device code: the assignment of a family's copies to variant patterns
// and the per-group plane counts (ramx_kernels_subfam.h), and their launchers.  Kept apart so that the translation units compile
// side by side.
#define RAMX_SECONDARY_TU 1
#include "ramx_kernels_subfam.h"

int ramx_subfam_assign_launch(hipStream_t st, int nwaves, const SubfamArgs &sa)
{
  if (nwaves <= 0) return RAMX_OK;
  hipLaunchKernelGGL(ramx_subfam_assign_kernel, dim3(nwaves), dim3(64), 0, st, sa);
  return hipGetLastError() != hipSuccess ? RAMX_ERR_HIP : RAMX_OK;
}

int ramx_subfam_count_launch(hipStream_t st, int nwaves, const SubfamArgs &sa)
{
  if (nwaves <= 0) return RAMX_OK;
  hipLaunchKernelGGL(ramx_subfam_count_kernel, dim3(nwaves), dim3(64), 0, st, sa);
  return hipGetLastError() != hipSuccess ? RAMX_ERR_HIP : RAMX_OK;
}
