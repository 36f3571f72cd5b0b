// ramx_dist_api.h -- host-side interface of the pairwise-divergence kernels (ramx_dist.hip), used by ramx_device.hip: the
// transposition of the resident bit planes into bit streams over the rows, one set per chosen copy, and the pair matrix of
// those streams.  Internal to libramx (not installed).
#pragma once

#include <hip/hip_runtime.h>

#include "ramx_kernels_common.h"
#include "ramx_linkage_api.h"
#include "ramx_dist.h"

#define RAMX_DIST_STREAMS 5       // per copy: called, lo (class bit 0), hi (class bit 1), deleted, covered
#define RAMX_DIST_BLOCK 64        // copies per side of a workgroup's block of the pair matrix
#define RAMX_DIST_CHUNK 8         // row words (64 rows each) of every stream staged through LDS at a time

struct DistFam
{
  long long plane_base;         // where the family's planes begin in `planes`, in words (PlanesArgs::fam_base)
  long long stream_base;        // where the family's streams begin in `streams`, in words
  long long out_base;           // where the family's [C][C] records begin in `out`, in records
  int T, rows, RW, C;           // tiles, rows, row words (rows + 63) / 64, chosen copies
};

struct DistArgs
{
  const unsigned long long *planes;   // as PlanesArgs
  const DistFam *fam;                 // [n_families]
  const int4 *item;                   // transposition, [waves]: (family, tile of the family, first entry in `slot`, row block)
  const int *slot;                    // [chosen tiles][64]: the slot (place in the family's list) of the tile's copy, or -1
  const int4 *block;                  // pairs, [workgroups]: (family, block row bi, block column bj >= bi, 0)
  unsigned long long *streams;        // family f, slot s, stream k, row word w: [stream_base + (s * 5 + k) * RW + w]
  ramx_copy_dist *out;
};

// one wave per entry of da.item
int ramx_dist_transpose_launch(hipStream_t st, int nitems, const DistArgs &da);
// one workgroup per entry of da.block
int ramx_dist_pairs_launch(hipStream_t st, int nblocks, const DistArgs &da);
