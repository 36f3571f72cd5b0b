// ramx_xfam_api.h -- host-side interface of the cross-family alignment kernel (ramx_xfam.hip), used by ramx_device.hip.
// Internal to libramx (not installed).
#pragma once

#include <hip/hip_runtime.h>

#include "ramx_xfam.h"
#include "ramx_kernels_common.h"

#define RAMX_XFAM_WAVES 4       // waves of a workgroup, each with a pair of its own

// one pair of a group as the kernel reads it: where its two sequences lie in the group's codes, where its strip border lies in
// the group's border buffer (in records of 16 bytes; room for na of them), and which record of the group it writes
struct XfamPair
{
  long long a_off, b_off, border_off;
  int na, nb, inverted, out_index;      // 1 <= na, nb <= RAMX_XFAM_MAXLEN
};

struct XfamArgs
{
  const signed char *codes;     // the sequences the group uses, library codes
  const XfamPair *pairs;        // [n]: the pairs of this launch
  int4 *border;                 // the strip borders of the group
  ramx_term *out;               // the records of the group
  int n;
  int lds_stride;               // bytes of LDS a wave has for its A: >= ceil(na / 2) of every pair of the launch, a multiple of 16
  int match, mismatch, gap, min_score;
};

extern "C" int ramx_pair_check_params(const ramx_pair_params *pp);      // ramx_xfam.c

// columns a lane owns for a partner of nb bases: 4 up to 256 bases, 8 up to 512, 16 beyond (one strip wherever one strip will do)
static inline int ramx_xfam_cols(int nb) { return nb <= 256 ? 4 : nb <= 512 ? 8 : 16; }

// one wave per pair: pairs -> records, with C (4, 8 or 16) columns a lane; na_max is the longest A of the launch
int ramx_xfam_align_launch(hipStream_t st, XfamArgs xa, int C, int na_max);
