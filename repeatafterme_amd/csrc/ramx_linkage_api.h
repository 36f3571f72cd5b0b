// ramx_linkage_api.h -- host-side interface of the linkage kernels (ramx_linkage.hip), used by ramx_device.hip: the bit planes
// of a replay and the Gram matrix of chosen planes.  Internal to libramx (not installed).
#pragma once

#include <hip/hip_runtime.h>

#include "ramx_kernels_common.h"

#define RAMX_PLANE_CLASSES 8      // planes per row: A C G T N, deleted, covered, inserted before
#define RAMX_GRAM_BLOCK 64        // planes per side of a workgroup's block of the Gram matrix
#define RAMX_GRAM_CHUNK 32        // tiles (64-bit words of a plane) staged through LDS at a time

struct PlanesArgs
{
  const unsigned *bases;        // [KW][Np] packed windows (ramx_pack_kernel): nibble (t + W + 8) of a flank's window is position t
  const int2 *tile_fam;         // [tiles]: (family, flanks of the family in this tile); family < 0: the tile belongs to none
  const int4 *fam;              // [n_families]: (first tile, tiles, rows, 0)
  const long long *fam_base;    // [n_families]: where the family's planes begin in `planes`, in words
  const int *rows;              // [n_families]
  const ramx_aln_end *ends;     // [Np], as the walk left them
  const int *col_idx, *col_ins; // [max rows][gn]: the GROUP's columns, flank tile0 * 64 + i at [r * gn + i]
  unsigned long long *planes;   // family f, plane (row, cls), tile t of the family: [fam_base[f] + (row * 8 + cls) * tiles_f + t]
  int Np, W, KW, gn, tile0;
};

// the words of tiles tile0 .. tile0 + ntiles - 1 (one wave each) from the group's walked columns; `planes` was zeroed before
int ramx_planes_launch(hipStream_t st, int ntiles, const PlanesArgs &pa);

struct GramArgs
{
  const unsigned long long *planes;   // as PlanesArgs
  const int4 *block;                  // [workgroups]: (family, block row bi, block column bj >= bi, 0)
  const int4 *fam;                    // [n_families]: (first chosen plane in `at`, chosen planes P, tiles T, 0)
  const long long *at;                // [chosen planes]: where the plane's T words begin in `planes`
  const long long *co_at;             // [n_families]: where the family's [P][P] matrix begins in `co`
  int *co;
};

// one workgroup per entry of ga.block
int ramx_plane_gram_launch(hipStream_t st, int nblocks, const GramArgs &ga);
