// ramx_term_api.h -- host-side interface of the terminal-repeat kernel (ramx_term.hip), used by ramx_device.hip.
// Internal to libramx (not installed).
#pragma once

#include <hip/hip_runtime.h>

#include "ramx_kernels_common.h"

#define RAMX_TERM_WAVES 4       // waves of a workgroup, each with its own (site, orientation)

struct TermArgs
{
  // the streams of ramx_period_squeeze_kernel over the 3 * Np windows of the group: window A of site s is stream s, B is Np + s,
  // C is 2 Np + s; offset j of a window at bits 2 (j % 32) of bases word j / 32, bit j % 32 of valid word j / 32
  const unsigned long long *bases;  // [3 Np][SW]
  const unsigned *valid;            // [3 Np][SW]
  const int *T;                     // [Np]: the sites' window lengths (0 for a padding lane)
  ramx_term *out;                   // [2 n]
  int n, Np, SW;                    // sites of the group, padded to whole tiles; words of a stream
  int match, mismatch, gap, min_score;
};

// one wave per (site, orientation): streams -> records.  Tmax is the longest window of the group: it chooses the specialisation
// (columns per lane 1, 2, 4, 8 or 16)
int ramx_term_align_launch(hipStream_t st, const TermArgs &ta, int Tmax);
