// ramx_kernels_subfam.h -- an extension's copies split into subfamilies (device code of libramx; included by ramx_subfam.hip
// only).  Both kernels read the bit planes that ramx_planes_kernel left resident and small uploaded lists; neither repeats a
// forward pass or a walk.
//
// ramx_subfam_assign_kernel: one wave per tile of 64 flanks, one lane per flank.  The family's variants go by in blocks of 64:
// lane j loads, for variant v0 + j, the tile's word of its plane, the word of its row's cover plane and its pattern byte (bit k:
// pat_k[v]) -- one independent load chain per lane, 64 in flight.  The wave then walks the block with a uniform index, every
// step a broadcast of one word pair and one byte; lane i tests its own bit and keeps the K <= 8 distances in registers,
// d_k += c & (x ^ pat_k).  At the end: argmin with ties to the lowest k, one label store per lane, the group masks
// ballot(label == k) as the tile's words of K mask planes (lane k stores plane k), and the number of lanes whose label differs
// from the one in `labels` before.  No LDS, no atomics, nothing order-dependent.
//
// ramx_subfam_count_kernel: one wave per listed plane of a family (and one more for the sizes: the all-ones plane).  Lanes stride
// the family's tiles with K int32 sums of popcount(plane[t] & mask_k[t]); a butterfly over the wave; lane k stores sum k.
#pragma once

#include "ramx_subfam_api.h"

// lane j's 64-bit word for the whole wave; j is uniform, so this is two readlanes and no LDS traffic
static __device__ __forceinline__ unsigned long long lane_word(unsigned long long w, int j)
{
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)w, j), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(w >> 32), j);
  return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(64) void ramx_subfam_assign_kernel(const SubfamArgs sa)
{
  const int lane = threadIdx.x;
  const int2 tl = sa.tile[blockIdx.x];                // (family, tile of the family)
  const SubfamFam fd = sa.fam[tl.x];
  const int V = fd.V, K = sa.K;
  const size_t t = (size_t)tl.y;
  int d[RAMX_SUBFAM_K];
  #pragma unroll
  for (int k = 0; k < RAMX_SUBFAM_K; k++) d[k] = 0;
  for (int v0 = 0; v0 < V; v0 += 64)
  {
    unsigned long long x = 0, c = 0;
    unsigned pb = 0;
    if (v0 + lane < V)
    {
      const longlong2 vr = sa.var[fd.var0 + v0 + lane];
      x = sa.planes[vr.x + t]; c = sa.planes[vr.y + t];
      pb = sa.pat[fd.var0 + v0 + lane];
    }
    const int nb = V - v0 < 64 ? V - v0 : 64;
    for (int j = 0; j < nb; j++)                      // uniform: every shuffle below is a broadcast
    {
      const unsigned long long xx = lane_word(x, j), cc = lane_word(c, j);
      const unsigned pp = (unsigned)__builtin_amdgcn_readlane((int)pb, j);
      const unsigned mx = (unsigned)(xx >> lane) & 1u, mc = (unsigned)(cc >> lane) & 1u;
      #pragma unroll
      for (int k = 0; k < RAMX_SUBFAM_K; k++) d[k] += (int)(mc & (mx ^ ((pp >> k) & 1u)));
    }
  }
  int best = 0, bd = d[0];
  #pragma unroll
  for (int k = 1; k < RAMX_SUBFAM_K; k++)
    if (k < K && d[k] < bd) { bd = d[k]; best = k; }  // strictly below: ties to the lowest k
  const int left = sa.count[tl.x] - 64 * tl.y;        // flanks of the family in this tile: the rest is padding
  const int label = lane < left ? best : -1;
  int *lab = sa.labels + fd.flank0 + 64 * (size_t)tl.y + lane;
  const int prev = *lab;
  *lab = label;
  const unsigned long long chg = __ballot(label != prev);
  if (lane == 0) sa.changed[blockIdx.x] = __popcll(chg);
  unsigned long long w = 0;
  #pragma unroll
  for (int k = 0; k < RAMX_SUBFAM_K; k++)
  {
    const unsigned long long m = __ballot(label == k);
    w = lane == k ? m : w;
  }
  if (lane < K) sa.mask[fd.mask0 + (size_t)lane * fd.T + t] = w;
}

__global__ __launch_bounds__(64) void ramx_subfam_count_kernel(const SubfamArgs sa)
{
  const int lane = threadIdx.x;
  const int2 it = sa.item[blockIdx.x];                // (family, listed plane; P: the sizes)
  const SubfamFam fd = sa.fam[it.x];
  const int K = sa.K, T = fd.T;
  const bool sizes = it.y >= fd.P;
  const unsigned long long *pl = sizes ? sa.planes : sa.planes + sa.at[fd.at0 + it.y];
  const unsigned long long *mk = sa.mask + fd.mask0;
  int acc[RAMX_SUBFAM_K];
  #pragma unroll
  for (int k = 0; k < RAMX_SUBFAM_K; k++) acc[k] = 0;
  for (int t = lane; t < T; t += 64)
  {
    const unsigned long long w = sizes ? ~0ull : pl[t];
    #pragma unroll
    for (int k = 0; k < RAMX_SUBFAM_K; k++)
      if (k < K) acc[k] += __popcll(w & mk[(size_t)k * T + t]);
  }
  int mine = 0;
  #pragma unroll
  for (int k = 0; k < RAMX_SUBFAM_K; k++)
  {
    int s = acc[k];
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    mine = lane == k ? s : mine;
  }
  if (lane < K) sa.cnt[fd.cnt0 + (size_t)lane * (fd.P + 1) + it.y] = mine;
}
