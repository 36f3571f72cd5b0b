// ramx_dinuc_api.h -- host-side interface of the dinucleotide pileup kernels (ramx_dinuc.hip), used by ramx_device.hip.
// Internal to libramx (not installed).
#pragma once

#include <hip/hip_runtime.h>

#include "ramx_kernels_common.h"

struct DinucArgs
{
  const unsigned *bases;        // [KW][Np] packed windows (ramx_pack_kernel): nibble (t + W + 8) of a flank's window is position t
  const int2 *tile_fam;         // [tiles]: (family, flanks of the family in this tile); family < 0: the tile belongs to none
  const signed char *cons;      // [n_families][L]
  const int *rows;              // [n_families]
  const ramx_aln_end *ends;     // [Np], as the walk left them
  const int *col_idx, *col_ins; // [max rows][gn]: the GROUP's columns, flank tile0 * 64 + i at [r * gn + i]
  ramx_col_dinuc *slab;         // [tiles][slab_rows]: one record per (global tile, row)
  int L, Np, W, KW, gn, tile0, slab_rows;
};

struct DinucSumArgs
{
  const ramx_col_dinuc *slab;
  const int4 *fam;              // [n_families]: (first tile, tiles, rows, -)
  const signed char *cons;
  ramx_col_dinuc *di;           // [n_families][L]
  int L, slab_rows;
};

// the row-pair records of tiles tile0 .. tile0 + ntiles - 1 (one wave each) from the group's walked columns; the sum of every
// family's per-tile records (maxrows: the longest family's rows)
int ramx_dinuc_launch(hipStream_t st, int ntiles, const DinucArgs &da);
int ramx_dinuc_launch_sum(hipStream_t st, int n_families, int maxrows, const DinucSumArgs &sa);
