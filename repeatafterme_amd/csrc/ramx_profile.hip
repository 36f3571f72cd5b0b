// ramx_profile.hip -- fourth translation unit of libramx's device code: the replay of an extension along a given consensus
// (ramx_kernels_profile.h) and its launcher.  Kept apart from ramx_device.hip so that the translation units compile side by side.
#define RAMX_SECONDARY_TU 1
#include "ramx_kernels_profile.h"

int ramx_profile_launch(hipStream_t st, bool resident, bool chain, int tiles, const ProfArgs &pa, int n_families, const ProfSumArgs &sa)
{
  if (tiles > 0)
  {
    if (resident)
    {
      switch (pa.k.W)
      {
        case 14: hipLaunchKernelGGL((ramx_profile_resident_kernel<14>), dim3(tiles), dim3(64), 0, st, pa); break;
        case 20: hipLaunchKernelGGL((ramx_profile_resident_kernel<20>), dim3(tiles), dim3(64), 0, st, pa); break;
        case 40: hipLaunchKernelGGL((ramx_profile_resident_kernel<40>), dim3(tiles), dim3(64), 0, st, pa); break;
        case 80: hipLaunchKernelGGL((ramx_profile_resident_kernel<80>), dim3(tiles), dim3(64), 0, st, pa); break;
        default: return RAMX_ERR_ARG;
      }
    }
    else if (chain) hipLaunchKernelGGL((ramx_profile_kernel<true>), dim3(tiles), dim3(64), 0, st, pa);
    else hipLaunchKernelGGL((ramx_profile_kernel<false>), dim3(tiles), dim3(64), 0, st, pa);
    if (hipGetLastError() != hipSuccess) return RAMX_ERR_HIP;
  }
  if (n_families > 0 && pa.slab_rows > 0)
  {
    hipLaunchKernelGGL(ramx_profile_sum_kernel, dim3(n_families, (pa.slab_rows + 255) / 256), dim3(256), 0, st, sa);
    if (hipGetLastError() != hipSuccess) return RAMX_ERR_HIP;
  }
  return RAMX_OK;
}
