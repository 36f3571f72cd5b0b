// ramx_kernels_squeeze.h -- a word of a packed window (eight 4-bit classes) as two bits a base: shared by the kernels that
// compare bases as bit streams (ramx_kernels_tsd.h, ramx_kernels_period.h).
#pragma once

#include <hip/hip_runtime.h>

// eight 4-bit fields -> their low two bits, packed: field i to bits 2i, 2i + 1
__device__ __forceinline__ unsigned tsd_squeeze(unsigned x)
{
  x &= 0x33333333u;
  x = (x | (x >> 2)) & 0x0f0f0f0fu;
  x = (x | (x >> 4)) & 0x00ff00ffu;
  return (x | (x >> 8)) & 0xffffu;
}
