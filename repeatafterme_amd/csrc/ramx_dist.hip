// ramx_dist.hip -- translation unit of libramx's device code for the pairwise divergence between copies: the transposition of
// the resident bit planes into per-copy bit streams and the pair matrix of those streams (ramx_kernels_dist.h), and their
// launchers.  Kept apart so that the translation units compile side by side.
#define RAMX_SECONDARY_TU 1
#include "ramx_kernels_dist.h"

int ramx_dist_transpose_launch(hipStream_t st, int nitems, const DistArgs &da)
{
  if (nitems <= 0) return RAMX_OK;
  hipLaunchKernelGGL(ramx_dist_transpose_kernel, dim3(nitems), dim3(64), 0, st, da);
  return hipGetLastError() != hipSuccess ? RAMX_ERR_HIP : RAMX_OK;
}

int ramx_dist_pairs_launch(hipStream_t st, int nblocks, const DistArgs &da)
{
  if (nblocks <= 0) return RAMX_OK;
  hipLaunchKernelGGL(ramx_dist_pairs_kernel, dim3(nblocks), dim3(256), 0, st, da);
  return hipGetLastError() != hipSuccess ? RAMX_ERR_HIP : RAMX_OK;
}
