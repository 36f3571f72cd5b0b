// ramx_copystats_api.h -- host-side interface of the per-copy statistics kernel (ramx_copystats.hip), used by ramx_device.hip.
// Internal to libramx (not installed).
#pragma once

#include <hip/hip_runtime.h>

#include "ramx_kernels_common.h"

struct CopyStatsArgs
{
  const unsigned *bases;        // [KW][Np] packed windows (ramx_pack_kernel): nibble (t + W + 8) of a flank's window is position t
  const int2 *tile_fam;         // [tiles]: (family, flanks of the family in this tile); family < 0: the tile belongs to none
  const signed char *cons;      // [n_families][L]
  const int *rows;              // [n_families]
  const ramx_aln_end *ends;     // [Np], as the walk left them
  const int *col_idx, *col_ins; // [max rows][gn]: the GROUP's columns, flank tile0 * 64 + i at [r * gn + i]
  ramx_copy_stats *stats;       // [Np]: one record per flank of the whole set
  int L, Np, W, KW, gn, tile0;
  int reversed;                 // rows run against the reading order (the left extension): the next base of column r is column r - 1
};

// the records of the flanks of tiles tile0 .. tile0 + ntiles - 1 (one wave each) from the group's walked columns
int ramx_copystats_launch(hipStream_t st, int ntiles, const CopyStatsArgs &ca);
