// ramx_subfam_api.h -- host-side interface of the subfamily kernels (ramx_subfam.hip), used by ramx_device.hip: every copy of a
// family assigned to the nearest variant pattern, and the counts of every listed plane within every group.  Both read the
// resident bit planes of ramx_dev_planes (ramx_linkage_api.h).  Internal to libramx (not installed).
#pragma once

#include <hip/hip_runtime.h>

#include "ramx_kernels_common.h"

#define RAMX_SUBFAM_K 8           // RAMX_SUBFAM_MAX of include/ramx.h: patterns of a family, one bit each in a pattern byte

struct SubfamFam
{
  int var0, V;                    // the family's variants in `var` / `pat`
  int at0, P;                     // the family's listed planes in `at`
  int T;                          // tiles of the family
  int flank0;                     // the family's first flank in `labels`
  long long mask0;                // the family's mask planes in `mask`: [K][T]
  long long cnt0;                 // the family's counts in `cnt`: [K][P + 1], column P the group's size
};

struct SubfamArgs
{
  const unsigned long long *planes;   // the resident planes, as PlanesArgs
  const SubfamFam *fam;               // [n_families]
  const long long *at;                // [listed planes]: where the plane's T words begin in `planes`
  const longlong2 *var;               // [variants]: (where the variant's words begin, where its row's cover plane's)
  const unsigned char *pat;           // [variants]: bit k is pat_k[v]
  const int2 *tile;                   // assign, [waves]: (family, tile of the family)
  const int2 *item;                   // count, [waves]: (family, listed plane p; p == P: the sizes)
  const int *count;                   // [n_families]: non-padding flanks of the family
  int *labels;                        // [n_padded]: read as the previous label, then written
  unsigned long long *mask;           // word t of mask plane k of family f: [mask0 + k * T + t]
  int *changed;                       // [waves of the assign launch]: lanes whose label differs from the previous one
  int *cnt;
  int K;
};

// one wave per entry of sa.tile
int ramx_subfam_assign_launch(hipStream_t st, int nwaves, const SubfamArgs &sa);
// one wave per entry of sa.item
int ramx_subfam_count_launch(hipStream_t st, int nwaves, const SubfamArgs &sa);
