// ramx_kernels_dinuc.h -- the dinucleotide pileup of an extension: what every flank puts into every PAIR of adjacent columns of a
// GIVEN consensus, counted from the columns the walk of ramx_kernels_align.h has just written (device code of libramx; included
// by ramx_dinuc.hip only)
//
// ramx_dinuc_kernel: one wave per tile of 64 flanks, one lane per flank, as ramx_pileup_kernel.  The lanes go down the rows
// together: lane i loads col_idx[r][i] and col_ins[r][i] (one 256-byte line per array and row), fetches the matched base from
// its packed window (matched positions only grow, so it holds one window word at a time) and carries what it put into the row
// before: a class, "deleted" or "not covered".  At row r it therefore knows the pair (r - 1, r) and the wave counts it: every
// counter is a ballot and a population count.  Lane k < 32 then holds the k-th 32-bit word of the record, and the wave writes
// the 128-byte record of (tile, r - 1) with one plain store: no atomics, and no order in which the result could depend on.  The
// record of the last row has no pair: next = -1 and zeros.
//
// ramx_dinuc_sum_kernel: per (family, column) the sum of the family's per-tile records, as ramx_pileup_sum_kernel.
#pragma once

#include "ramx_dinuc_api.h"

static_assert(sizeof(ramx_col_dinuc) == 128, "ramx_col_dinuc is 32 words");

#define RAMX_DINUC_DELETED 5      // what a lane put into a row: a class 0..4, or
#define RAMX_DINUC_OFF     6

__global__ __launch_bounds__(64) void ramx_dinuc_kernel(const DinucArgs da)
{
  const int lane = threadIdx.x, tile = da.tile0 + blockIdx.x;
  const int2 tf = da.tile_fam[tile];
  if (tf.x < 0) return;                               // uniform: a tile outside every family
  const int rows = da.rows[tf.x];
  if (rows <= 0) return;
  const signed char *cons = da.cons + (size_t)tf.x * da.L;
  const int n = tile * 64 + lane;
  const size_t Np = (size_t)da.Np, gn = (size_t)da.gn;
  const int *ci = da.col_idx + (size_t)blockIdx.x * 64 + lane, *cn = da.col_ins + (size_t)blockIdx.x * 64 + lane;
  const unsigned *win = da.bases + n;
  const int end_row = lane < tf.y ? da.ends[n].end_row : -1;   // padding flanks and flanks without an alignment: above every row
  const int toff = da.W + 8, KW = da.KW;
  int cw = -1;
  unsigned cword = 0;
  // class of flank position t, as the pileup's
  auto cls = [&](int t) {
    const int tp = t + toff, wi = tp >> 3;
    if (tp < 0 || wi >= KW) return 4;
    if (wi != cw) { cw = wi; cword = win[(size_t)wi * Np]; }
    const int c = (int)((cword >> (4 * (tp & 7))) & 15u);
    return c < 8 ? (c & 3) : 4;
  };
  ramx_col_dinuc *slab = da.slab + (size_t)tile * da.slab_rows;

  int prev = RAMX_DINUC_OFF;
  for (int r = 0; r < rows; r++)
  {
    const int idx = ci[(size_t)r * gn];
    const int ins = cn[(size_t)r * gn];
    const bool on = r <= end_row;
    int cur = RAMX_DINUC_OFF;
    if (on) cur = idx == RAMX_ALN_DELETED ? RAMX_DINUC_DELETED : (idx == RAMX_ALN_NONE ? 4 : cls(idx));
    if (r > 0)
    {
      // the pair (r - 1, r): a flank that covers r covers r - 1
      const bool gapped = on && (prev == RAMX_DINUC_DELETED || cur == RAMX_DINUC_DELETED);
      const bool matched = on && !gapped;
      const bool adjacent = matched && ins == 0;
      const int pair = adjacent ? 5 * prev + cur : -1;
      int v = 0;
      auto put = [&](int word, bool pred) {
        const int cnt = __popcll(__ballot(pred));
        if (lane == word) v = cnt;
      };
      if (lane == 0) v = cons[r - 1];
      if (lane == 1) v = cons[r];
      put(2, on);
      put(3, adjacent);
      put(4, matched && ins > 0);
      put(5, gapped);
#pragma unroll
      for (int k = 0; k < 25; k++) put(6 + k, pair == k);
      if (lane < 32) reinterpret_cast<int *>(slab + (r - 1))[lane] = v;
    }
    prev = cur;
  }
  if (lane < 32) reinterpret_cast<int *>(slab + (rows - 1))[lane] = lane == 0 ? cons[rows - 1] : (lane == 1 ? -1 : 0);
}

// per (family, column): the sum of the family's per-tile records
__global__ __launch_bounds__(256) void ramx_dinuc_sum_kernel(const DinucSumArgs sa)
{
  const int4 fd = sa.fam[blockIdx.x];
  const int r = blockIdx.y * 256 + threadIdx.x;
  if (r >= fd.z) return;
  int t[32];
#pragma unroll
  for (int i = 0; i < 32; i++) t[i] = 0;
  for (int k = 0; k < fd.y; k++)
  {
    const int4 *s = reinterpret_cast<const int4 *>(sa.slab + (size_t)(fd.x + k) * sa.slab_rows + r);
#pragma unroll
    for (int q = 0; q < 8; q++)
    {
      const int4 x = s[q];
      t[4 * q] += x.x; t[4 * q + 1] += x.y; t[4 * q + 2] += x.z; t[4 * q + 3] += x.w;
    }
  }
  const signed char *cons = sa.cons + (size_t)blockIdx.x * sa.L;
  t[0] = cons[r];
  t[1] = r + 1 < fd.z ? cons[r + 1] : -1;
  int4 *o = reinterpret_cast<int4 *>(sa.di + (size_t)blockIdx.x * sa.L + r);
#pragma unroll
  for (int q = 0; q < 8; q++) o[q] = make_int4(t[4 * q], t[4 * q + 1], t[4 * q + 2], t[4 * q + 3]);
}
