// ramx_linkage.hip -- eighth translation unit of libramx's device code: the bit planes of a replay along a given consensus and
// the Gram matrix of chosen planes (ramx_kernels_linkage.h), and their launchers.  Kept apart so that the translation units
// compile side by side.
#define RAMX_SECONDARY_TU 1
#include "ramx_kernels_linkage.h"

int ramx_planes_launch(hipStream_t st, int ntiles, const PlanesArgs &pa)
{
  if (ntiles <= 0) return RAMX_OK;
  hipLaunchKernelGGL(ramx_planes_kernel, dim3(ntiles), dim3(64), 0, st, pa);
  return hipGetLastError() != hipSuccess ? RAMX_ERR_HIP : RAMX_OK;
}

int ramx_plane_gram_launch(hipStream_t st, int nblocks, const GramArgs &ga)
{
  if (nblocks <= 0) return RAMX_OK;
  hipLaunchKernelGGL(ramx_plane_gram_kernel, dim3(nblocks), dim3(256), 0, st, ga);
  return hipGetLastError() != hipSuccess ? RAMX_ERR_HIP : RAMX_OK;
}
