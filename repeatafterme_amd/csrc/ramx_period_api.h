// ramx_period_api.h -- host-side interface of the tandem-periodicity kernels (ramx_period.hip), used by ramx_device.hip.
// Internal to libramx (not installed).
#pragma once

#include <hip/hip_runtime.h>

#include "ramx_kernels_common.h"

// A segment is a flank packed with W = 0 (ramx_pack_kernel / ramx_pack2_kernel): nibble i of word k of its window is offset
// j = 8 (k - 1) + i of the segment (word 0 is the pad word in front), so block b of the contract is word b + 1.
#define RAMX_PERIOD_W 0
#define RAMX_PERIOD_THREADS 256
#define RAMX_PERIOD_PAD 3       // 64-bit words of zeros behind a staged stream: a funnel shift reads up to two words past its end

// words of a window that holds n bases, and 32-base words of a stream
static inline int period_window_words(int n) { return (n + 7) / 8 + 1; }
static inline int period_stream_words(int n) { return (n + 31) / 32; }

struct PeriodArgs
{
  const unsigned *win;            // [KW][Np] packed windows of the group's segments
  unsigned long long *bases;      // [Np][SW]: two bits a base, offset j at bits 2 (j % 32) of word j / 32
  unsigned *valid;                // [Np][SW]: bit j % 32 of word j / 32 set iff the class of offset j is below 4
  const int *len;                 // [Np]: the segments' lengths (0 for a padding lane)
  ramx_period *out;               // [n]
  int n, Np, KW, SW;              // segments of the group, padded to whole tiles; words of a window, words of a stream
  int pmax, mm, min_score;
};

// one wave per tile of 64 segments: windows -> streams
int ramx_period_squeeze_launch(hipStream_t st, const PeriodArgs &pa);
// one workgroup per segment: streams -> records
int ramx_period_scan_launch(hipStream_t st, const PeriodArgs &pa);
