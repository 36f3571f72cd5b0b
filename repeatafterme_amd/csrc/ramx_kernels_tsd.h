// ramx_kernels_tsd.h -- target-site duplications of the extended copies (include/ramx.h, ramx_tsd): for every site the best
// direct repeat between the word that ends in front of the element and the word that begins behind it, over every shift pair
// (dl, dr) within the slack and every length k (device code of libramx; included by ramx_tsd.hip only).
//
// ramx_tsd_kernel: one lane per site, 64 sites a wave.  The two outside windows of a site were packed as flanks (W = 0, six
// words of eight 4-bit classes, transposed: a wave reads 256 contiguous bytes per word): the left one runs DOWN the library from
// lo - 1, the right one up from hi + 1, both from t = -slack to kmax + slack - 1.  A lane squeezes its twelve words once into two
// streams of 48 positions, two bits a base and a validity bit beside it, the left stream reversed so that both run up the
// library.  A 32-base word at any shift is then a funnel shift of a stream by a wave-uniform amount: for (dl, dr) the left word
// ENDS at lo + dl - 1 and the right word BEGINS at hi + 1 + dr, so the candidate of length k compares the top k bases of the one
// with the bottom k of the other -- the left word moved down by 32 - k bases (from the longest k downwards: one base a step), a
// xor folded to a bit per base, the validity masks, a popcount.
// The loops over (dl, dr, k) are the same for every lane; the best candidate is the maximum of ONE 25-bit key that orders the
// candidates as the contract does, so no order of evaluation shows.  Everything is registers indexed at compile time: no LDS, no
// scratch, no atomics, and no lane reads another's value.
#pragma once

#include "ramx_tsd_api.h"
#include "ramx_kernels_squeeze.h"       // tsd_squeeze

static_assert(sizeof(ramx_tsd) == 16, "ramx_tsd is 4 words");

// eight 2-bit fields in reverse order
__device__ __forceinline__ unsigned tsd_reverse(unsigned x)
{
  const unsigned r = __brev(x) >> 16;
  return ((r & 0x5555u) << 1) | ((r >> 1) & 0x5555u);
}

__global__ __launch_bounds__(64) void ramx_tsd_kernel(const TsdArgs ta)
{
  const int site = blockIdx.x * 64 + threadIdx.x;               // < Np: the windows of the padding sites are all N
  const size_t stride = 2 * (size_t)ta.Np;
  const unsigned *wl = ta.bases + site, *wr = ta.bases + ta.Np + site;
  // stream position y of the right stream is nibble y (t = y - 8); of the left stream nibble 47 - y (t = 39 - y): library
  // position lo - 40 + y.  lo / hi hold positions 0..31, *_top positions 32..47; v*: bit 2y set iff the class is below 4
  unsigned long long r_lo = 0, r_top = 0, vr_lo = 0, vr_top = 0, l_lo = 0, l_top = 0, vl_lo = 0, vl_top = 0;
#pragma unroll
  for (int k = 0; k < RAMX_TSD_KW; k++)
  {
    const unsigned a = wr[(size_t)k * stride], b = wl[(size_t)k * stride];
    const unsigned long long rb = tsd_squeeze(a), rv = tsd_squeeze(~a >> 3) & 0x5555u;
    const unsigned long long lb = tsd_reverse(tsd_squeeze(b)), lv = tsd_reverse(tsd_squeeze(~b >> 3) & 0x5555u);
    if (k < 4) { r_lo |= rb << (16 * k); vr_lo |= rv << (16 * k); }
    else { r_top |= rb << (16 * (k - 4)); vr_top |= rv << (16 * (k - 4)); }
    if (k >= 2) { l_lo |= lb << (16 * (5 - k)); vl_lo |= lv << (16 * (5 - k)); }
    else { l_top |= lb << (16 * (1 - k)); vl_top |= lv << (16 * (1 - k)); }
  }
  const int room = site < ta.n ? ta.room[site] : 0;
  const int S = ta.slack, kmin = ta.kmin, kmax = ta.kmax, mm_div = ta.mm_div;
  const unsigned long long even = 0x5555555555555555ull;
  const int s_max = 2 * (32 - kmax), allowed_max = mm_div ? kmax / mm_div : 0, left_max = mm_div ? kmax % mm_div : (1 << 30);
  unsigned best = 0;
  for (int dl = -S; dl <= S; dl++)
  {
    // 32 bases that end at lo + dl - 1: stream positions 8 + dl .. 39 + dl
    const int ol = 2 * (8 + dl);                                // 2 .. 30
    const unsigned long long lw = (l_lo >> ol) | (l_top << (64 - ol)), lvw = (vl_lo >> ol) | (vl_top << (64 - ol));
    for (int dr = -S; dr <= S; dr++)
    {
      // 32 bases that begin at hi + 1 + dr
      const int orr = 2 * (8 + dr);
      const unsigned long long rw = (r_lo >> orr) | (r_top << (64 - orr)), rvw = (vr_lo >> orr) | (vr_top << (64 - orr));
      const bool apart = dl - dr <= room;                        // (i): the left word ends before the right one begins
      const int off = (dl < 0 ? -dl : dl) + (dr < 0 ? -dr : dr);
      // from the longest word down: the left word of length k - 1 is that of length k moved down one base, so the only shifts by
      // a variable amount are these three, once per shift pair
      unsigned long long a = lw >> s_max, va = lvw >> s_max, m = even >> s_max, top = 1ull << (2 * kmax - 2);
      int allowed = allowed_max, left = left_max;                // (iii): k / mm_div, and k % mm_div to count it down
      for (int k = kmax; k >= kmin; k--)
      {
        const unsigned long long x = a ^ rw;
        // bit 2j: base j of the two words does not agree
        const unsigned long long bad = (((x | (x >> 1)) & even) | ~(va & rvw)) & m;
        const int mm = __popcll(bad);
        const bool ends = (bad & (top | 1ull)) == 0;              // (ii)
        // the contract's order in one key: q = 2 (k - 2 mm) - off, then the smaller |dl| + |dr|, the larger k, the smaller dl, the
        // smaller dr; everything but mm is the same for the whole wave
        const unsigned ukey = ((unsigned)(2 * k - off + 16) << 18) | ((unsigned)(14 - off) << 14) | ((unsigned)k << 8) | ((unsigned)(7 - dl) << 4) | (unsigned)(7 - dr);
        const unsigned key = ukey - ((unsigned)mm << 20);
        if (apart && ends && mm <= allowed && key > best) best = key;
        a >>= 2; va >>= 2; m >>= 2; top >>= 2;
        if (left == 0) { allowed--; left = mm_div - 1; } else left--;
      }
    }
  }
  if (site >= ta.n) return;
  int4 rec = make_int4(0, 0, 0, 0);
  if (best)
  {
    const int q = (int)(best >> 18) - 16, off = 14 - (int)((best >> 14) & 15u), k = (int)((best >> 8) & 63u);
    rec = make_int4(k, (2 * k - off - q) / 4, 7 - (int)((best >> 4) & 15u), 7 - (int)(best & 15u));
  }
  *reinterpret_cast<int4 *>(ta.out + site) = rec;
}
