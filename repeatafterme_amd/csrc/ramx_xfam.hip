// ramx_xfam.hip -- fourteenth translation unit of libramx's device code: the alignment of two sequences of any two lengths for
// the cross-family overlap (ramx_kernels_xfam.h) and its launcher.  Kept apart so that the translation units compile side by side.
#define RAMX_SECONDARY_TU 1
#include "ramx_kernels_xfam.h"

int ramx_xfam_align_launch(hipStream_t st, XfamArgs xa, int C, int na_max)
{
  if (xa.n <= 0) return RAMX_OK;
  if (na_max < 1 || na_max > RAMX_XFAM_MAXLEN || (C != 4 && C != 8 && C != 16)) return RAMX_ERR_ARG;
  // a nibble a base, a multiple of 16 bytes a wave: at most 4 * 16,384 bytes
  xa.lds_stride = (((na_max + 1) / 2) + 15) & ~15;
  const size_t lds = (size_t)RAMX_XFAM_WAVES * xa.lds_stride;
  const dim3 grid((unsigned)((xa.n + RAMX_XFAM_WAVES - 1) / RAMX_XFAM_WAVES)), block(64 * RAMX_XFAM_WAVES);
  if (C == 4) hipLaunchKernelGGL(ramx_xfam_align_kernel<4>, grid, block, lds, st, xa);
  else if (C == 8) hipLaunchKernelGGL(ramx_xfam_align_kernel<8>, grid, block, lds, st, xa);
  else hipLaunchKernelGGL(ramx_xfam_align_kernel<16>, grid, block, lds, st, xa);
  return hipGetLastError() != hipSuccess ? RAMX_ERR_HIP : RAMX_OK;
}
