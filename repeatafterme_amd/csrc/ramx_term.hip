// ramx_term.hip -- twelfth translation unit of libramx's device code: the terminal repeats of the extended copies
// (ramx_kernels_term.h) and their launcher.  Kept apart so that the translation units compile side by side.
#define RAMX_SECONDARY_TU 1
#include "ramx_kernels_term.h"

int ramx_term_align_launch(hipStream_t st, const TermArgs &ta, int Tmax)
{
  if (ta.n <= 0) return RAMX_OK;
  if (Tmax > RAMX_TERM_TMAX) return RAMX_ERR_ARG;
  const dim3 grid((unsigned)((2 * (long long)ta.n + RAMX_TERM_WAVES - 1) / RAMX_TERM_WAVES)), block(64 * RAMX_TERM_WAVES);
  // columns per lane: the smallest of 1, 2, 4, 8, 16 with 64 C >= Tmax
  if (Tmax <= 64) hipLaunchKernelGGL(ramx_term_align_kernel<1>, grid, block, 0, st, ta);
  else if (Tmax <= 128) hipLaunchKernelGGL(ramx_term_align_kernel<2>, grid, block, 0, st, ta);
  else if (Tmax <= 256) hipLaunchKernelGGL(ramx_term_align_kernel<4>, grid, block, 0, st, ta);
  else if (Tmax <= 512) hipLaunchKernelGGL(ramx_term_align_kernel<8>, grid, block, 0, st, ta);
  else hipLaunchKernelGGL(ramx_term_align_kernel<16>, grid, block, 0, st, ta);
  return hipGetLastError() != hipSuccess ? RAMX_ERR_HIP : RAMX_OK;
}
