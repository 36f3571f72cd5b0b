// ramx_period.hip -- eleventh translation unit of libramx's device code: the tandem periodicity of the extended copies
// (ramx_kernels_period.h) and its launchers.  Kept apart so that the translation units compile side by side.
#define RAMX_SECONDARY_TU 1
#include "ramx_kernels_period.h"

int ramx_period_squeeze_launch(hipStream_t st, const PeriodArgs &pa)
{
  if (pa.n <= 0) return RAMX_OK;
  hipLaunchKernelGGL(ramx_period_squeeze_kernel, dim3(pa.Np / 64), dim3(64), 0, st, pa);
  return hipGetLastError() != hipSuccess ? RAMX_ERR_HIP : RAMX_OK;
}

int ramx_period_scan_launch(hipStream_t st, const PeriodArgs &pa)
{
  if (pa.n <= 0) return RAMX_OK;
  // the longest stream of the group and its padding, bases and validity: at most 2 * (2048 + 3) * 8 bytes
  const size_t lds = (size_t)2 * (pa.SW + RAMX_PERIOD_PAD) * sizeof(unsigned long long);
  hipLaunchKernelGGL(ramx_period_scan_kernel, dim3(pa.n), dim3(RAMX_PERIOD_THREADS), lds, st, pa);
  return hipGetLastError() != hipSuccess ? RAMX_ERR_HIP : RAMX_OK;
}
