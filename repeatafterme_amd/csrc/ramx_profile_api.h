// ramx_profile_api.h -- host-side interface of the profile replay kernels (ramx_profile.hip), used by ramx_device.hip.
// Internal to libramx (not installed).
#pragma once

#include <hip/hip_runtime.h>

#include "ramx_kernels_common.h"

struct ProfArgs
{
  KArgs k;                      // bases, bounds, S_in == S_out, Np, W, go, ge, cap, tab (what run_band reads)
  const ramx_flank *flanks;     // [Np]: which end of the band is the far edge of a flank
  const int2 *tile_fam;         // [tiles]: (family, flanks of the family in this tile); family < 0: the tile belongs to none
  const signed char *cons;      // [n_families][L]
  const int *rows;              // [n_families]
  ramx_col_profile *slab;       // [tiles][slab_rows]: per-wave partial records
  int *last_uncapped;           // [Np]
  int *row_best, *row_best_idx; // NULL, or [slab_rows][Np]
  int L, slab_rows;             // slab_rows = max rows[f]
  int pack_ok, lean_p;          // the resident kernel's fast bands: as in PArgs (ramx_kernels_resident.h)
};

// ramx_profile_sum_kernel: per (family, column) the sum of the family's per-wave records
struct ProfSumArgs
{
  const ramx_col_profile *slab;
  const int4 *fam;              // [n_families]: (first tile, tiles, rows, 0)
  const signed char *cons;      // [n_families][L]: a family without flanks still reports its bases
  ramx_col_profile *cols;       // [n_families][L]
  int L, slab_rows;
};

// which band widths have a row-on-chip instantiation of the replay (no positive gap penalty, go + ge >= -32768 besides)
static inline bool ramx_profile_has_resident(int W) { return W == 14 || W == 20 || W == 40 || W == 80; }

// the replay of every tile (one wave each), then the per-(family, column) sum of the per-wave records; resident: the
// row-on-chip kernel of pa.k.W; otherwise the rows go through pa.k.S_in, chain: the full candidate recurrence (a positive gap
// penalty, or RAMX_FORCE_CHAIN)
int ramx_profile_launch(hipStream_t st, bool resident, bool chain, int tiles, const ProfArgs &pa, int n_families, const ProfSumArgs &sa);
