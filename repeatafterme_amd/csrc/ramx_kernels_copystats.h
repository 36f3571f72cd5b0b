// ramx_kernels_copystats.h -- the per-copy statistics of an extension: how every flank's alignment to a GIVEN consensus divides
// into matches, transitions, transversions, deletions and insertions, counted from the columns the walk of ramx_kernels_align.h
// has just written (device code of libramx; included by ramx_copystats.hip only).  The pileup's transpose: ramx_pileup_kernel
// reduces the same columns over the flanks, this kernel over the rows.
//
// ramx_copystats_kernel: one wave per tile of 64 flanks, one lane per flank, as the pileup.  The lanes go down the rows
// together: lane i loads col_idx[r][i] and col_ins[r][i] (one 256-byte line per array and row) and fetches the matched base
// from its packed window (a lane's positions only grow, so it holds one window word at a time); inserted bases are counted, not
// read.  cons[r] and its two neighbours are the same for the whole wave: they sit in scalar registers and are shifted along, one
// load a row.  The eleven counters are registers of the lane, the loop ends at the wave's largest end_row, and each lane then
// writes its own 48-byte record once: no LDS, no atomics, no lane reads another's value, and no order the result could depend on.
#pragma once

#include "ramx_copystats_api.h"

static_assert(sizeof(ramx_copy_stats) == 48, "ramx_copy_stats is 12 words");

__global__ __launch_bounds__(64) void ramx_copystats_kernel(const CopyStatsArgs ca)
{
  const int lane = threadIdx.x, tile = ca.tile0 + blockIdx.x;
  const int2 tf = ca.tile_fam[tile];
  if (tf.x < 0) return;                               // uniform: a tile outside every family
  const int rows = ca.rows[tf.x];
  const signed char *cons = ca.cons + (size_t)tf.x * ca.L;
  const int n = tile * 64 + lane;
  const size_t Np = (size_t)ca.Np, gn = (size_t)ca.gn;
  const int *ci = ca.col_idx + (size_t)blockIdx.x * 64 + lane, *cn = ca.col_ins + (size_t)blockIdx.x * 64 + lane;
  const unsigned *win = ca.bases + n;
  const ramx_aln_end e = ca.ends[n];
  // padding flanks and flanks without an alignment: above every row
  const int end_row = lane < tf.y ? (e.end_row < rows ? e.end_row : rows - 1) : -1;
  const int toff = ca.W + 8, KW = ca.KW;
  const bool rev = ca.reversed != 0;
  int cw = -1;
  unsigned cword = 0;
  // class of flank position t, as the pileup's: A C G T, lower case alike; 4 for N and for everything the pack kernel made N
  // (outside the flank's bounds, outside the library) or that lies outside the window
  auto cls = [&](int t) {
    const int tp = t + toff, wi = tp >> 3;
    if (tp < 0 || wi >= KW) return 4;
    if (wi != cw) { cw = wi; cword = win[(size_t)wi * Np]; }
    const int c = (int)((cword >> (4 * (tp & 7))) & 15u);
    return c < 8 ? (c & 3) : 4;
  };
  // the consensus at r - 1, r, r + 1 (-1: no such column), wave-uniform
  auto cons_at = [&](int r) { return r < rows ? __builtin_amdgcn_readfirstlane((int)cons[r]) : -1; };
  int c_lo = -1, c_at = cons_at(0), c_hi = cons_at(1);

  int match = 0, ts = 0, tv = 0, n_match = 0, del = 0, del_open = 0, ins = 0, ins_open = 0, cpg_cols = 0, cpg_ts = 0;
  bool prev_del = false;
  for (int r = 0; r < rows; r++)
  {
    if (__ballot(r <= end_row) == 0) break;           // uniform: beyond the wave's largest end_row
    const int idx = ci[(size_t)r * gn];
    const int ni = cn[(size_t)r * gn];
    const int c_next = cons_at(r + 2);
    // column r lies in a CpG: it is the C and the next column in reading order is G, or the G and the previous one is C
    const int after = rev ? c_lo : c_hi, before = rev ? c_hi : c_lo;
    const bool cpg = (c_at == 1 && after == 2) || (c_at == 2 && before == 1);
    if (r <= end_row)
    {
      ins += ni;
      ins_open += ni > 0;
      if (idx == RAMX_ALN_DELETED)
      {
        del++;
        del_open += r == 0 || !prev_del || ni > 0;
        prev_del = true;
      }
      else
      {
        prev_del = false;
        if (idx != RAMX_ALN_NONE)
        {
          const int m = cls(idx);
          if (m == 4) n_match++;
          else
          {
            const bool is_ts = (m ^ c_at) == 2;
            if (m == c_at) match++;
            else if (is_ts) ts++;
            else tv++;
            if (cpg) { cpg_cols++; cpg_ts += is_ts; }
          }
        }
      }
    }
    c_lo = c_at; c_at = c_hi; c_hi = c_next;
  }
  int4 *o = reinterpret_cast<int4 *>(ca.stats + n);
  o[0] = make_int4(end_row + 1, match, ts, tv);
  o[1] = make_int4(n_match, del, del_open, ins);
  o[2] = make_int4(ins_open, cpg_cols, cpg_ts, end_row >= 0 ? e.score : 0);
}
