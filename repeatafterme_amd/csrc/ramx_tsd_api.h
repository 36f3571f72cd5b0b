// ramx_tsd_api.h -- host-side interface of the target-site-duplication kernel (ramx_tsd.hip), used by ramx_device.hip.
// Internal to libramx (not installed).
#pragma once

#include <hip/hip_runtime.h>

#include "ramx_kernels_common.h"

// The two outside windows of a site are flanks packed with W = 0 (ramx_pack_kernel / ramx_pack2_kernel): nibble t + 8 of a
// window is flank position t, and t runs from -slack up to kmax + slack - 1 <= 38: nibbles 1..46, six words.
#define RAMX_TSD_W 0
#define RAMX_TSD_KW 6

struct TsdArgs
{
  const unsigned *bases;        // [RAMX_TSD_KW][2 * Np]: the left windows of sites 0..Np-1, then their right windows
  const int *room;              // [Np]: min(hi + 1 - lo, 64): dl - dr may not exceed it (the two words may not cross)
  ramx_tsd *out;                // [n]
  int n, Np;                    // sites, sites padded to whole waves
  int slack, kmin, kmax, mm_div;
};

// one record per site (one lane each, Np / 64 waves)
int ramx_tsd_launch(hipStream_t st, const TsdArgs &ta);
