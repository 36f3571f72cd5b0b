// ramx_kernels_pileup.h -- the pileup of an extension: what every flank puts into every column of a GIVEN consensus, counted
// from the columns the walk of ramx_kernels_align.h has just written (device code of libramx; included by ramx_pileup.hip only)
//
// ramx_pileup_kernel: one wave per tile of 64 flanks, one lane per flank, as the replays.  The lanes go down the rows together:
// lane i loads col_idx[r][i] and col_ins[r][i] (one 256-byte line per array and row), keeps its own running position -- the
// consumed positions of a flank are contiguous from start_idx, so the run inserted before column r begins where the move of
// column r - 1 ended --, fetches the matched base and up to RAMX_PILEUP_INS inserted bases from its packed window (a lane's
// positions only grow, so it holds one window word at a time and loads every word once) and classes them.  Every counter is a
// ballot and a population count over the wave; ins_bases is the wave sum the profile uses.  Lane k < 32 then holds the k-th
// 32-bit word of the record, and the wave writes the 128-byte record of (tile, row) with one plain store: no atomics, and no
// order in which the result could depend on.
//
// ramx_pileup_sum_kernel: per (family, column) the sum of the family's per-tile records, as ramx_profile_sum_kernel.
#pragma once

#include "ramx_pileup_api.h"

static_assert(sizeof(ramx_col_pileup) == 128, "ramx_col_pileup is 32 words");

__global__ __launch_bounds__(64) void ramx_pileup_kernel(const PileArgs pa)
{
  const int lane = threadIdx.x, tile = pa.tile0 + blockIdx.x;
  const int2 tf = pa.tile_fam[tile];
  if (tf.x < 0) return;                               // uniform: a tile outside every family
  const int rows = pa.rows[tf.x];
  const signed char *cons = pa.cons + (size_t)tf.x * pa.L;
  const int n = tile * 64 + lane;
  const size_t Np = (size_t)pa.Np, gn = (size_t)pa.gn;
  const int *ci = pa.col_idx + (size_t)blockIdx.x * 64 + lane, *cn = pa.col_ins + (size_t)blockIdx.x * 64 + lane;
  const unsigned *win = pa.bases + n;
  const ramx_aln_end e = pa.ends[n];
  const int end_row = lane < tf.y ? e.end_row : -1;   // padding flanks and flanks without an alignment: above every row
  const int toff = pa.W + 8, KW = pa.KW;
  int pos = e.start_idx;
  int cw = -1;
  unsigned cword = 0;
  // class of flank position t: A C G T, lower case alike; 4 for N and for everything the pack kernel made N (outside the flank's
  // bounds, outside the library) or that lies outside the window
  auto cls = [&](int t) {
    const int tp = t + toff, wi = tp >> 3;
    if (tp < 0 || wi >= KW) return 4;
    if (wi != cw) { cw = wi; cword = win[(size_t)wi * Np]; }
    const int c = (int)((cword >> (4 * (tp & 7))) & 15u);
    return c < 8 ? (c & 3) : 4;
  };
  ramx_col_pileup *slab = pa.slab + (size_t)tile * pa.slab_rows;

  for (int r = 0; r < rows; r++)
  {
    const int idx = ci[(size_t)r * gn];
    int ins = cn[(size_t)r * gn];
    const bool on = r <= end_row;
    if (!on) ins = 0;
    int m = -1, s[RAMX_PILEUP_INS];
#pragma unroll
    for (int k = 0; k < RAMX_PILEUP_INS; k++) s[k] = -1;
    if (on)
    {
#pragma unroll
      for (int k = 0; k < RAMX_PILEUP_INS; k++)
        if (k < ins) s[k] = cls(pos + k);
      pos += ins;
      if (idx != RAMX_ALN_DELETED && idx != RAMX_ALN_NONE) { m = cls(idx); pos = idx + 1; }
    }
    int v = 0;
    auto put = [&](int word, bool pred) {
      const int cnt = __popcll(__ballot(pred));
      if (lane == word) v = cnt;
    };
    if (lane == 0) v = cons[r];
    put(1, on);
#pragma unroll
    for (int b = 0; b < 5; b++) put(2 + b, m == b);
    put(7, on && idx == RAMX_ALN_DELETED);
    put(8, ins > 0);
    put(9, ins > RAMX_PILEUP_INS);
    const long long nb = wave_sum_nonneg31(ins);
    if (lane == 10) v = (int)(unsigned)nb;
    if (lane == 11) v = (int)(nb >> 32);
#pragma unroll
    for (int k = 0; k < RAMX_PILEUP_INS; k++)
#pragma unroll
      for (int b = 0; b < 5; b++) put(12 + 5 * k + b, s[k] == b);
    if (lane < 32) reinterpret_cast<int *>(slab + r)[lane] = v;
  }
}

// per (family, column): the sum of the family's per-tile records
__global__ __launch_bounds__(256) void ramx_pileup_sum_kernel(const PileSumArgs sa)
{
  const int4 fd = sa.fam[blockIdx.x];
  const int r = blockIdx.y * 256 + threadIdx.x;
  if (r >= fd.z) return;
  int t[32];
#pragma unroll
  for (int i = 0; i < 32; i++) t[i] = 0;
  long long nb = 0;
  for (int k = 0; k < fd.y; k++)
  {
    const int4 *s = reinterpret_cast<const int4 *>(sa.slab + (size_t)(fd.x + k) * sa.slab_rows + r);
#pragma unroll
    for (int q = 0; q < 8; q++)
    {
      const int4 x = s[q];
      t[4 * q] += x.x; t[4 * q + 1] += x.y; t[4 * q + 2] += x.z; t[4 * q + 3] += x.w;
      if (q == 2) nb += ((long long)x.w << 32) | (unsigned)x.z;
    }
  }
  t[0] = sa.cons[(size_t)blockIdx.x * sa.L + r];
  t[10] = (int)(unsigned)nb; t[11] = (int)(nb >> 32);
  int4 *o = reinterpret_cast<int4 *>(sa.cols + (size_t)blockIdx.x * sa.L + r);
#pragma unroll
  for (int q = 0; q < 8; q++) o[q] = make_int4(t[4 * q], t[4 * q + 1], t[4 * q + 2], t[4 * q + 3]);
}
