// ramx_kernels_linkage.h -- co-segregation of an extension's variants: the second-order sibling of the pileup and the per-copy
// statistics (device code of libramx; included by ramx_linkage.hip only).
//
// ramx_planes_kernel: one wave per tile of 64 flanks, one lane per flank, over the columns the walk of ramx_kernels_align.h has
// just written -- the addressing and the base classes of ramx_copystats_kernel.  Per row the wave takes eight ballots: "this
// lane's flank is matched to class A / C / G / T / N, is deleted, is covered, has bases inserted before the column".  A ballot is
// the tile's 64-bit word of a BIT PLANE over the family's flanks; lane c < 8 stores the word of class c.  The planes of a family
// are plane-major and contiguous along the family's tiles.  The buffer is zeroed before the first group, so the loop ends at the
// wave's largest end_row.  No LDS, no atomics.
//
// ramx_plane_gram_kernel: co[p][q] = sum over the tiles of popcount(plane_p & plane_q) for the chosen planes of a family.  One
// workgroup of 256 threads per 64 x 64 block of the upper triangle (block row <= block column); thread (ty, tx) of 16 x 16 owns
// the 4 x 4 entries (ty + 16 a, tx + 16 b).  The words of the block's 64 row planes and 64 column planes are staged through LDS
// 32 tiles at a time as [64][33]: the odd pitch (in 8-byte words) makes the 16 column planes a half-wave reads at one k fall
// into 16 different bank pairs, and the stores of 16 consecutive k of one plane likewise; the row-plane reads are broadcasts.
// The sums are int32 registers (a count is at most the family's flanks), every entry is written by exactly one thread -- the
// mirror entry by the same thread, and not at all inside a diagonal block, whose both halves are computed -- so there are no
// atomics and no order the result could depend on.
#pragma once

#include "ramx_linkage_api.h"

__global__ __launch_bounds__(64) void ramx_planes_kernel(const PlanesArgs pa)
{
  const int lane = threadIdx.x, tile = pa.tile0 + blockIdx.x;
  const int2 tf = pa.tile_fam[tile];
  if (tf.x < 0) return;                               // uniform: a tile outside every family
  const int rows = pa.rows[tf.x];
  const int4 fd = pa.fam[tf.x];                       // (first tile, tiles, rows, 0)
  const int n = tile * 64 + lane;
  const size_t Np = (size_t)pa.Np, gn = (size_t)pa.gn, nt = (size_t)fd.y;
  const int *ci = pa.col_idx + (size_t)blockIdx.x * 64 + lane, *cn = pa.col_ins + (size_t)blockIdx.x * 64 + lane;
  const unsigned *win = pa.bases + n;
  const ramx_aln_end e = pa.ends[n];
  // padding flanks and flanks without an alignment: above every row
  const int end_row = lane < tf.y ? (e.end_row < rows ? e.end_row : rows - 1) : -1;
  const int toff = pa.W + 8, KW = pa.KW;
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
  // lane c < 8 writes the word of class c of this tile, row after row
  unsigned long long *out = pa.planes + pa.fam_base[tf.x] + (size_t)(lane & 7) * nt + (size_t)(tile - fd.x);
  for (int r = 0; r < rows; r++)
  {
    const bool cover = r <= end_row;
    const unsigned long long b_cover = __ballot(cover);
    if (b_cover == 0) break;                          // uniform: beyond the wave's largest end_row
    const int idx = ci[(size_t)r * gn];
    const int ni = cn[(size_t)r * gn];
    int m = -1;                                       // 0..4: matched to that class; 5: deleted
    if (cover)
    {
      if (idx == RAMX_ALN_DELETED) m = 5;
      else if (idx != RAMX_ALN_NONE) m = cls(idx);
    }
    const unsigned long long b0 = __ballot(m == 0), b1 = __ballot(m == 1), b2 = __ballot(m == 2), b3 = __ballot(m == 3),
                             b4 = __ballot(m == 4), b5 = __ballot(m == 5), b7 = __ballot(cover && ni > 0);
    unsigned long long w = b0;
    w = lane == 1 ? b1 : w; w = lane == 2 ? b2 : w; w = lane == 3 ? b3 : w; w = lane == 4 ? b4 : w;
    w = lane == 5 ? b5 : w; w = lane == 6 ? b_cover : w; w = lane == 7 ? b7 : w;
    if (lane < RAMX_PLANE_CLASSES) out[(size_t)r * RAMX_PLANE_CLASSES * nt] = w;
  }
}

#define RAMX_GRAM_PITCH (RAMX_GRAM_CHUNK + 1)

__global__ __launch_bounds__(256) void ramx_plane_gram_kernel(const GramArgs ga)
{
  __shared__ unsigned long long sa[RAMX_GRAM_BLOCK * RAMX_GRAM_PITCH], sb[RAMX_GRAM_BLOCK * RAMX_GRAM_PITCH];
  const int4 blk = ga.block[blockIdx.x];              // (family, bi, bj, 0)
  const int4 fd = ga.fam[blk.x];                      // (first chosen plane, P, T, 0)
  const int P = fd.y, T = fd.z;
  const int p0 = blk.y * RAMX_GRAM_BLOCK, q0 = blk.z * RAMX_GRAM_BLOCK;
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const long long *at = ga.at + fd.x;
  // staging: thread -> word k = tid % 32 of planes tid / 32 + 8 i: 32 consecutive threads read 256 contiguous bytes of a plane
  const int lk = tid & (RAMX_GRAM_CHUNK - 1), lp = tid >> 5;
  long long src_a[8], src_b[8];                       // -1: no such plane (behind P): zeros
  #pragma unroll
  for (int i = 0; i < 8; i++)
  {
    const int pl = lp + 8 * i;
    src_a[i] = p0 + pl < P ? at[p0 + pl] : -1;
    src_b[i] = q0 + pl < P ? at[q0 + pl] : -1;
  }
  int acc[4][4];
  #pragma unroll
  for (int a = 0; a < 4; a++)
    #pragma unroll
    for (int b = 0; b < 4; b++) acc[a][b] = 0;

  for (int k0 = 0; k0 < T; k0 += RAMX_GRAM_CHUNK)
  {
    const bool in = k0 + lk < T;
    #pragma unroll
    for (int i = 0; i < 8; i++)
    {
      const int pl = lp + 8 * i;
      sa[pl * RAMX_GRAM_PITCH + lk] = in && src_a[i] >= 0 ? ga.planes[src_a[i] + k0 + lk] : 0ull;
      sb[pl * RAMX_GRAM_PITCH + lk] = in && src_b[i] >= 0 ? ga.planes[src_b[i] + k0 + lk] : 0ull;
    }
    __syncthreads();
    #pragma unroll 4
    for (int k = 0; k < RAMX_GRAM_CHUNK; k++)
    {
      unsigned long long va[4], vb[4];
      #pragma unroll
      for (int a = 0; a < 4; a++) va[a] = sa[(ty + 16 * a) * RAMX_GRAM_PITCH + k];
      #pragma unroll
      for (int b = 0; b < 4; b++) vb[b] = sb[(tx + 16 * b) * RAMX_GRAM_PITCH + k];
      #pragma unroll
      for (int a = 0; a < 4; a++)
        #pragma unroll
        for (int b = 0; b < 4; b++) acc[a][b] += __popcll(va[a] & vb[b]);
    }
    __syncthreads();
  }
  int *co = ga.co + ga.co_at[blk.x];
  #pragma unroll
  for (int a = 0; a < 4; a++)
    #pragma unroll
    for (int b = 0; b < 4; b++)
    {
      const int p = p0 + ty + 16 * a, q = q0 + tx + 16 * b;
      if (p >= P || q >= P) continue;
      co[(size_t)p * P + q] = acc[a][b];
      if (blk.y != blk.z) co[(size_t)q * P + p] = acc[a][b];
    }
}
