// ramx_kernels_dist.h -- pairwise divergence between the copies of an extension: the transpose of the plane Gram's view, copy
// against copy over the rows where the Gram counts column against column over the copies (device code of libramx; included by
// ramx_dist.hip only).
//
// ramx_dist_transpose_kernel: the resident planes (ramx_kernels_linkage.h) hold one 64-bit word per tile, row and class, a bit
// vector over the tile's 64 copies.  One wave per tile that holds a chosen copy and per block of 64 rows: lane l reads the words
// of row r0 + l (classes 0..3, 5, 6) and forms five words -- called = A|C|G|T, lo = C|T (bit 0 of the base class), hi = G|T
// (bit 1), deleted, covered.  64 ballots of bit c of such a word hand lane c the word of ITS copy over the 64 rows, and a lane
// whose copy is chosen stores it into the copy's stream.  Rows >= rows[f] read as 0, and so does what the planes kernel never
// wrote (its buffer is zeroed).  Every row word of every chosen copy is written by exactly one lane, so the stream buffer needs
// no clearing.  No LDS, no atomics.
//
// ramx_dist_pairs_kernel: the blocking of ramx_plane_gram_kernel.  One workgroup of 256 threads per 64 x 64 block of the upper
// triangle; thread (ty, tx) of 16 x 16 owns the 4 x 4 pairs (ty + 16 a, tx + 16 b), six int32 sums each.  The five streams of
// the block's 64 row copies and 64 column copies are staged through LDS RAMX_DIST_CHUNK row words at a time as [64][5 * 8 + 1]:
// the odd pitch (in 8-byte words) makes the 16 column copies a wave reads at one (stream, word) fall into 16 different bank
// pairs; the row-copy reads are broadcasts.  Per word a pair costs a handful of ANDs and XORs and six 64-bit popcounts.  Every
// entry is written by exactly one thread -- the mirror entry by the same thread, and not at all inside a diagonal block, whose
// both halves are computed -- so there are no atomics and no order the result could depend on.
#pragma once

#include "ramx_dist_api.h"

__global__ __launch_bounds__(64) void ramx_dist_transpose_kernel(const DistArgs da)
{
  const int lane = threadIdx.x;
  const int4 it = da.item[blockIdx.x];                // (family, tile, first slot entry, row block)
  const DistFam fd = da.fam[it.x];
  const int row = it.w * 64 + lane;
  unsigned long long w[RAMX_DIST_STREAMS] = { 0, 0, 0, 0, 0 };
  if (row < fd.rows)
  {
    const size_t T = (size_t)fd.T;
    const unsigned long long *p = da.planes + fd.plane_base + (size_t)row * RAMX_PLANE_CLASSES * T + (size_t)it.y;
    const unsigned long long p0 = p[0], p1 = p[T], p2 = p[2 * T], p3 = p[3 * T];
    w[0] = p0 | p1 | p2 | p3; w[1] = p1 | p3; w[2] = p2 | p3; w[3] = p[5 * T]; w[4] = p[6 * T];
  }
  const int slot = da.slot[it.z + lane];
  unsigned long long *out = da.streams + fd.stream_base + (size_t)(slot < 0 ? 0 : slot) * RAMX_DIST_STREAMS * fd.RW + it.w;
  #pragma unroll
  for (int k = 0; k < RAMX_DIST_STREAMS; k++)
  {
    unsigned long long mine = 0;
    #pragma unroll 8
    for (int c = 0; c < 64; c++)
    {
      const unsigned long long b = __ballot((w[k] >> c) & 1ull);   // bit l: row r0 + l of copy c
      mine = lane == c ? b : mine;
    }
    if (slot >= 0) out[(size_t)k * fd.RW] = mine;
  }
}

#define RAMX_DIST_ROW (RAMX_DIST_STREAMS * RAMX_DIST_CHUNK)       // staged words of one copy
#define RAMX_DIST_PITCH (RAMX_DIST_ROW + 1)

__global__ __launch_bounds__(256) void ramx_dist_pairs_kernel(const DistArgs da)
{
  __shared__ unsigned long long sa[RAMX_DIST_BLOCK * RAMX_DIST_PITCH], sb[RAMX_DIST_BLOCK * RAMX_DIST_PITCH];
  const int4 blk = da.block[blockIdx.x];              // (family, bi, bj, 0)
  const DistFam fd = da.fam[blk.x];
  const int C = fd.C, RW = fd.RW;
  const int a0 = blk.y * RAMX_DIST_BLOCK, b0 = blk.z * RAMX_DIST_BLOCK;
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const unsigned long long *st = da.streams + fd.stream_base;
  int acc[4][4][6];
  #pragma unroll
  for (int a = 0; a < 4; a++)
    #pragma unroll
    for (int b = 0; b < 4; b++)
      #pragma unroll
      for (int i = 0; i < 6; i++) acc[a][b][i] = 0;

  for (int k0 = 0; k0 < RW; k0 += RAMX_DIST_CHUNK)
  {
    // staging: entry e -> copy e / 40, stream (e % 40) / 8, word e % 8: eight consecutive threads read 64 contiguous bytes
    #pragma unroll
    for (int i = 0; i < RAMX_DIST_BLOCK * RAMX_DIST_ROW / 256; i++)
    {
      const int e = tid + 256 * i, cp = e / RAMX_DIST_ROW, rem = e - cp * RAMX_DIST_ROW, s = rem / RAMX_DIST_CHUNK, k = rem - s * RAMX_DIST_CHUNK;
      const bool in = k0 + k < RW;
      sa[cp * RAMX_DIST_PITCH + rem] = in && a0 + cp < C ? st[((size_t)(a0 + cp) * RAMX_DIST_STREAMS + s) * RW + k0 + k] : 0ull;
      sb[cp * RAMX_DIST_PITCH + rem] = in && b0 + cp < C ? st[((size_t)(b0 + cp) * RAMX_DIST_STREAMS + s) * RW + k0 + k] : 0ull;
    }
    __syncthreads();
    const int kn = RW - k0 < RAMX_DIST_CHUNK ? RW - k0 : RAMX_DIST_CHUNK;
    for (int k = 0; k < kn; k++)
    {
      unsigned long long vb[4][RAMX_DIST_STREAMS];
      #pragma unroll
      for (int b = 0; b < 4; b++)
        #pragma unroll
        for (int s = 0; s < RAMX_DIST_STREAMS; s++) vb[b][s] = sb[(tx + 16 * b) * RAMX_DIST_PITCH + s * RAMX_DIST_CHUNK + k];
      #pragma unroll
      for (int a = 0; a < 4; a++)
      {
        unsigned long long va[RAMX_DIST_STREAMS];
        #pragma unroll
        for (int s = 0; s < RAMX_DIST_STREAMS; s++) va[s] = sa[(ty + 16 * a) * RAMX_DIST_PITCH + s * RAMX_DIST_CHUNK + k];
        #pragma unroll
        for (int b = 0; b < 4; b++)
        {
          const unsigned long long v = va[0] & vb[b][0], x = va[1] ^ vb[b][1], y = va[2] ^ vb[b][2], c = va[4] & vb[b][4];
          acc[a][b][0] += __popcll(c);                               // cover
          acc[a][b][1] += __popcll(v);                               // sites
          acc[a][b][2] += __popcll(v & y & ~x);                      // ts: same bit 0, other bit 1
          acc[a][b][3] += __popcll(v & x);                           // tv: other bit 0
          acc[a][b][4] += __popcll((va[3] ^ vb[b][3]) & c);          // del_one
          acc[a][b][5] += __popcll(va[3] & vb[b][3]);                // del_both
        }
      }
    }
    __syncthreads();
  }
  ramx_copy_dist *out = da.out + fd.out_base;
  #pragma unroll
  for (int a = 0; a < 4; a++)
    #pragma unroll
    for (int b = 0; b < 4; b++)
    {
      const int p = a0 + ty + 16 * a, q = b0 + tx + 16 * b;
      if (p >= C || q >= C) continue;
      ramx_copy_dist r;
      r.cover = acc[a][b][0]; r.sites = acc[a][b][1]; r.ts = acc[a][b][2]; r.tv = acc[a][b][3];
      r.del_one = acc[a][b][4]; r.del_both = acc[a][b][5];
      out[(size_t)p * C + q] = r;
      if (blk.y != blk.z) out[(size_t)q * C + p] = r;
    }
}
