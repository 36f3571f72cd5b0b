// ramx_kernels_term.h -- terminal repeats of the extended copies (include/ramx.h, ramx_term): the gapped local alignment of a
// site's 5' window with its 3' window, direct and inverted (device code of libramx; included by ramx_term.hip only).
//
// The three windows of a site were packed as flanks and squeezed into streams by ramx_period_squeeze_kernel (two bits a base and
// a validity bit).  ramx_term_align_kernel<C>: one wave per (site, orientation), a systolic sweep of the T x T cells in registers.
//   Lane l owns the C columns j = l C + 1 .. (l + 1) C; at step t it computes row i = t - l + 1 of them, so the wave works on an
//   anti-diagonal of lane-wide blocks.  Row i - 1 of the lane's own columns -- H and the payload of every cell -- stays in VGPRs
//   (3 C of them); H and the payload of the lane's last column move one lane up per step (__shfl_up; the value received in the
//   step before is the diagonal of the lane's first column).  The row's base of A is read from a copy of the window in LDS, one
//   byte a base (a lane-dependent address, no bank conflict worth the name: consecutive lanes read consecutive bytes), the lane's
//   C bases of B sit in one register, and the agreement of the row's base with all of them is one xor.
//   The contract's "first of D, U, L" is folded into the compared key: 4 * value + (2, 1, 0), one max3.  The payload is two
//   words: i0 | j0 << 11, and matches | columns << 12.
//   Every lane keeps the best cell of its columns; rows ascend and columns ascend within a row, so a strict improvement keeps the
//   smallest i, then the smallest j.  At the end one 64-bit key (H, then the smaller i, then the smaller j) is reduced over the
//   wave as a maximum, and the lane that holds it writes the record with two 16-byte stores.  No atomics, no scratch, no barrier
//   in the loop, and no order of evaluation shows.
//   The specialisation on C (1, 2, 4, 8, 16) keeps the row arrays in registers; the host chooses it from the longest window of the
//   group.  A shorter window in the same launch uses fewer lanes and fewer steps: columns behind T hold "no base" and are never a
//   best cell, lanes whose first column lies behind T never compute.
#pragma once

#include "ramx_term_api.h"

static_assert(sizeof(ramx_term) == 32, "ramx_term is 8 words");
static_assert(RAMX_TERM_TMAX <= 1024, "16 columns a lane; i0 and j0 in 11 bits, matches in 12, columns in 12");

// sixteen bits -> the even bits of 32
__device__ __forceinline__ unsigned term_spread16(unsigned x)
{
  x &= 0xffffu;
  x = (x | (x << 8)) & 0x00ff00ffu;
  x = (x | (x << 4)) & 0x0f0f0f0fu;
  x = (x | (x << 2)) & 0x33333333u;
  return (x | (x << 1)) & 0x55555555u;
}

template <int C>
__global__ __launch_bounds__(64 * RAMX_TERM_WAVES) void ramx_term_align_kernel(const TermArgs ta)
{
  __shared__ unsigned char lds_a[RAMX_TERM_WAVES][RAMX_TERM_TMAX];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int pair = blockIdx.x * RAMX_TERM_WAVES + wave;
  const bool live = pair < 2 * ta.n;                                // (a wave behind the last pair only meets the barrier)
  const int site = live ? pair >> 1 : 0, inv = pair & 1;
  const int T = live ? ta.T[site] : 0;                              // <= 64 C: the host chose C from the longest window
  {
    const unsigned long long *ab = ta.bases + (size_t)site * ta.SW;
    const unsigned *av = ta.valid + (size_t)site * ta.SW;
    for (int o = lane; o < T; o += 64)                              // o / 32 < SW
    {
      const unsigned long long w = ab[o >> 5];
      const unsigned v = av[o >> 5];
      lds_a[wave][o] = ((v >> (o & 31)) & 1u) ? (unsigned char)((w >> (2 * (o & 31))) & 3u) : (unsigned char)4;
    }
  }
  __syncthreads();
  if (!live) return;
  // the lane's C bases of the partner window: C divides 32, so they lie in one word of the stream
  const int off0 = lane * C;
  unsigned bw = 0, bvs = 0;
  if ((off0 >> 5) < ta.SW)
  {
    const size_t at = ((size_t)(1 + inv) * ta.Np + site) * ta.SW + (off0 >> 5);
    bw = (unsigned)(ta.bases[at] >> (2 * (off0 & 31)));
    bvs = term_spread16((ta.valid[at] >> (off0 & 31)) & ((1u << C) - 1u));
  }
  const int match = ta.match, mismatch = ta.mismatch, gap = ta.gap;
  int H[C];
  unsigned P0[C], P1[C];
#pragma unroll
  for (int c = 0; c < C; c++) { H[c] = 0; P0[c] = (unsigned)(off0 + c + 1) << 11; P1[c] = 0; }       // row 0: (0, j, 0, 0)
  int dgH = 0, oH = 0, bH = 0, bi = 0, bj = 0;
  unsigned dgP0 = (unsigned)off0 << 11, dgP1 = 0, oP0 = 0, oP1 = 0, bP0 = 0, bP1 = 0;
  const int lanes_used = (T + C - 1) / C, steps = T + lanes_used - 1;
  const bool mine = off0 < T;
  for (int t = 0; t < steps; t++)
  {
    // row i of the last column of the lane below, computed in the step before
    int rH = __shfl_up(oH, 1);
    unsigned rP0 = __shfl_up(oP0, 1), rP1 = __shfl_up(oP1, 1);
    const int i = t - lane + 1;
    if (mine && i >= 1 && i <= T)
    {
      if (lane == 0) { rH = 0; rP0 = (unsigned)i; rP1 = 0; }        // the boundary cell (i, 0)
      const unsigned a = lds_a[wave][i - 1];
      unsigned eqm = 0;                                             // bit 2 c: the row's base agrees with column c
      if (a < 4) { const unsigned x = bw ^ (a * 0x55555555u); eqm = ~(x | (x >> 1)) & bvs; }
      int dH = dgH, lH = rH;
      unsigned dP0 = dgP0, dP1 = dgP1, lP0 = rP0, lP1 = rP1;
#pragma unroll
      for (int c = 0; c < C; c++)
      {
        const unsigned ag = (eqm >> (2 * c)) & 1u;
        const int kd = (dH + (ag ? match : -mismatch)) * 4 + 2, ku = (H[c] - gap) * 4 + 1, kl = (lH - gap) * 4;
        const int k = max(kd, max(ku, kl));
        int h = k >> 2;
        const int sel = k & 3;
        unsigned p0 = sel == 2 ? dP0 : sel == 1 ? P0[c] : lP0;
        unsigned p1 = (sel == 2 ? dP1 + ag : sel == 1 ? P1[c] : lP1) + (1u << 12);
        if (h <= 0) { h = 0; p0 = (unsigned)i | ((unsigned)(off0 + c + 1) << 11); p1 = 0; }
        dH = H[c]; dP0 = P0[c]; dP1 = P1[c];
        H[c] = h; P0[c] = p0; P1[c] = p1;
        lH = h; lP0 = p0; lP1 = p1;
        if (h > bH && off0 + c < T) { bH = h; bi = i; bj = off0 + c + 1; bP0 = p0; bP1 = p1; }
      }
      dgH = rH; dgP0 = rP0; dgP1 = rP1;                             // H[i][l C] is the diagonal of the next row's first column
      oH = lH; oP0 = lP0; oP1 = lP1;
    }
  }
  // the contract's order over the cells in one key: the larger H, then the smaller i, then the smaller j
  const unsigned long long key = ((unsigned long long)(unsigned)bH << 22) | ((unsigned long long)(2047 - bi) << 11) | (unsigned long long)(2047 - bj);
  unsigned long long top = key;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) { const unsigned long long o = __shfl_xor(top, s); top = o > top ? o : top; }
  int4 *rec = reinterpret_cast<int4 *>(ta.out + pair);
  if ((int)(top >> 22) < ta.min_score)                              // (min_score >= 1: no cell above 0 is never found)
  {
    if (lane == 0) { rec[0] = make_int4(0, 0, 0, 0); rec[1] = make_int4(0, 0, 0, T); }
    return;
  }
  if (key != top) return;                                           // the cells differ between lanes: one lane holds it
  rec[0] = make_int4(bH, (int)(bP0 & 2047u), bi - 1, (int)(bP0 >> 11));
  rec[1] = make_int4(bj - 1, (int)(bP1 & 4095u), (int)(bP1 >> 12), T);
}
