// ramx_align_api.h -- host-side interface of the traceback replay kernels (ramx_align.hip), used by ramx_device.hip.
// Internal to libramx (not installed).
#pragma once

#include <hip/hip_runtime.h>

#include "ramx_kernels_common.h"

struct AlnArgs
{
  KArgs k;                      // bases, bounds, S_in == S_out, Np, W, go, ge, tab (what run_band reads)
  const int2 *tile_fam;         // [tiles]: (family, flanks of the family in this tile); family < 0: the tile belongs to none
  const signed char *cons;      // [n_families][L]
  const int *rows;              // [n_families]
  unsigned *codes;              // [max rows][nd][gn]: decision codes of the group's flanks, eight cells per dword
  ramx_aln_end *ends;           // [Np]
  int *col_idx, *col_ins;       // NULL, or [max rows][Np], preset by the caller
  int L, nd, gn, tile0;         // nd = W / 4 + 1 dwords per flank-row; the group: flanks tile0 * 64 .. tile0 * 64 + gn - 1
};

// dwords of codes per flank and row
static inline int ramx_align_dwords(int W) { return W / 4 + 1; }

// col_idx = RAMX_ALN_NONE, col_ins = 0 everywhere; the forward replay of tiles tile0 .. tile0 + ntiles - 1 (one wave each); the
// walk back of their flanks
int ramx_align_launch_preset(hipStream_t st, int *col_idx, int *col_ins, size_t count);
int ramx_align_launch_forward(hipStream_t st, int ntiles, const AlnArgs &aa);
int ramx_align_launch_walk(hipStream_t st, int ntiles, const AlnArgs &aa);
