// ramx_kernels_xfam.h -- cross-family overlap of the extended consensi (include/ramx_xfam.h): the gapped local alignment of two
// sequences of any two lengths up to RAMX_XFAM_MAXLEN (device code of libramx; included by ramx_xfam.hip only).
//
// ramx_xfam_align_kernel<C>: one wave per pair, RAMX_XFAM_WAVES waves a workgroup, each wave on a pair of its own.  It is the sweep
// of ramx_term_align_kernel<C> (ramx_kernels_term.h) extended to any rectangle: B' is cut into strips of S = 64 C columns, and
// within a strip lane l owns the C columns j = strip + l C + 1 .. strip + (l + 1) C; at step t it computes row i = t - l + 1 of
// them.  Row i - 1 of the lane's own columns -- H and the two payload words of every cell -- stays in VGPRs, the row's last cell
// moves one lane up per step, the row's base of A comes from LDS, the lane's C bases of B' sit in one register and the agreement
// of the row's base with all of them is one xor.  "First of D, U, L" is folded into the compared key 4 * value + (2, 1, 0).
//   A in LDS: one nibble a base (the class 0..4), so the four waves of a workgroup take 64 KiB at na = 32,767 and two workgroups
//   fit the 160 KiB of a CU; the launch asks for what its longest A needs.
//   Payload: i0 | j0 << 16 and matches | columns << 16: i0, j0 and matches are at most 32,767, columns at most 65,534.
//   The strip border: the last column of a strip -- H and the two payload words of every row -- goes to a buffer of the pair's own
//   in global memory, one 16-byte vector store by lane 63 per step, and lane 0 of the next strip takes it as its left and diagonal
//   neighbour.  ONE buffer per wave, in this order: at every step t that is a multiple of 64 the wave reads rows t .. t + 63 (a lane
//   each; lane 0 needs row t' at step t', and picks it from the holder's register with a readlane), and lane 63 rewrites row t - 63
//   at step t.  So row r is read at step 64 floor(r / 64) <= r and rewritten at step r + 63 of the same strip: the read comes at
//   least 63 steps earlier in the program order of the one wave that does both, and its value has arrived (it is used in the step
//   that loads it) before the store is issued.  Between two strips the wave waits for its stores (s_waitcnt vmcnt(0)): the last
//   rows of a strip are read back at once when na is small.  The loads are relaxed agent-scope loads, which are served by the L2
//   and not by the CU's vector cache, so a line cached in an earlier strip is never read; the stores are plain and write through
//   to that L2.  Nothing else reads or writes the buffer: no barrier, no atomic read-modify-write and no fence in the loop.
//   Best cell: within a strip rows ascend and columns ascend within a row, so a strict improvement keeps the strip's smallest i,
//   then its smallest j.  Strips break that order -- a later strip may reach the same H in an earlier row -- so the strip's best
//   replaces the lane's only by the explicit key (larger H, then smaller i; on equal i the earlier strip has the smaller j), and
//   the wave reduces one 64-bit key (H, 32767 - i, 32767 - j) as a maximum.  The lane that holds it writes the record with two
//   16-byte stores.  No scratch, and no order of evaluation shows.
//   A shorter last strip uses fewer lanes and fewer steps; columns behind nb hold "no base" and are never a best cell.
// The roles of A and B are never swapped: the tie rules (first of D, U, L; smallest i before smallest j) are not symmetric.
#pragma once

#include "ramx_xfam_api.h"

static_assert(sizeof(ramx_term) == 32, "ramx_term is 8 words");
static_assert(RAMX_XFAM_MAXLEN <= 32767, "i0, j0 and matches in 15 bits, columns <= 2 * 32767 in 16; the reduced key has 15 bits for i and j");
static_assert(15 * RAMX_XFAM_MAXLEN < (1 << 19), "the largest H (match 15) in the 64-bit key and, times 4, in an int");
static_assert(sizeof(XfamPair) == 40, "three offsets and four ints");

__device__ __forceinline__ unsigned xfam_class(signed char c) { return c >= 0 && c <= 7 ? (unsigned)c & 3u : 4u; }

template <int C>
__global__ __launch_bounds__(64 * RAMX_XFAM_WAVES) void ramx_xfam_align_kernel(const XfamArgs xa)
{
  extern __shared__ unsigned char xfam_lds[];
  constexpr int S = 64 * C;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int slot = blockIdx.x * RAMX_XFAM_WAVES + wave;
  const bool live = slot < xa.n;                                    // (a wave behind the last pair only meets the barrier)
  XfamPair p;
  if (live) p = xa.pairs[slot]; else { p.a_off = p.b_off = p.border_off = 0; p.na = p.nb = p.inverted = p.out_index = 0; }
  const int na = p.na, nb = p.nb;
  unsigned char *const la = xfam_lds + (size_t)wave * xa.lds_stride;
  {
    const signed char *a = xa.codes + p.a_off;
    for (int o = lane; 2 * o < na; o += 64)                         // o < ceil(na / 2) <= lds_stride
    {
      const unsigned c0 = xfam_class(a[2 * o]), c1 = 2 * o + 1 < na ? xfam_class(a[2 * o + 1]) : 4u;
      la[o] = (unsigned char)(c0 | (c1 << 4));
    }
  }
  __syncthreads();
  if (!live) return;
  const signed char *const b = xa.codes + p.b_off;
  unsigned long long *const border = reinterpret_cast<unsigned long long *>(xa.border + p.border_off);   // [na][2]
  const int match = xa.match, mismatch = xa.mismatch, gap = xa.gap;
  int bH = 0, bi = 0, bj = 0;
  unsigned bP0 = 0, bP1 = 0;
  for (int strip = 0; strip < nb; strip += S)
  {
    const bool first = strip == 0, last = strip + S >= nb;
    const int off0 = strip + lane * C;                              // the lane's columns are j = off0 + 1 .. off0 + C
    const int cols = last ? nb - strip : S, lanes_used = (cols + C - 1) / C, steps = na + lanes_used - 1;
    const bool mine = off0 < nb;
    // the lane's C bases of B': two bits a base and, spread to the even bits, whether there is a base
    unsigned bw = 0, bvs = 0;
#pragma unroll
    for (int c = 0; c < C; c++)
      if (off0 + c < nb)
      {
        unsigned x = xfam_class(p.inverted ? b[nb - 1 - (off0 + c)] : b[off0 + c]);
        if (x < 4) { if (p.inverted) x = 3 - x; bw |= x << (2 * c); bvs |= 1u << (2 * c); }
      }
    int H[C];
    unsigned P0[C], P1[C];
#pragma unroll
    for (int c = 0; c < C; c++) { H[c] = 0; P0[c] = (unsigned)(off0 + c + 1) << 16; P1[c] = 0; }       // row 0: (0, j, 0, 0)
    int dgH = 0, oH = 0, sH = 0, si = 0, sj = 0;
    unsigned dgP0 = (unsigned)off0 << 16, dgP1 = 0, oP0 = 0, oP1 = 0, sP0 = 0, sP1 = 0;
    // (lane 0: the cell (0, strip) of the boundary row is the diagonal of its first row in every strip)
    unsigned long long q0 = 0, q1 = 0;                              // row t0 + lane of the border, t0 = t & ~63
    if (!first) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the border the strip before wrote has left the wave
    for (int t = 0; t < steps; t++)
    {
      if (!first && (t & 63) == 0)
      {
        const int r = t + lane;
        q0 = q1 = 0;
        if (r < na)
        {
          q0 = __hip_atomic_load(border + 2 * (size_t)r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          q1 = __hip_atomic_load(border + 2 * (size_t)r + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      // row i of the last column of the lane below, computed in the step before
      int rH = __shfl_up(oH, 1);
      unsigned rP0 = __shfl_up(oP0, 1), rP1 = __shfl_up(oP1, 1);
      // lane 0's left neighbour of row t + 1: the boundary cell, or the border's row t, held by lane t % 64
      const int k = t & 63;
      const int qH = __builtin_amdgcn_readlane((int)(unsigned)q0, k);
      const unsigned qP0 = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(q0 >> 32), k);
      const unsigned qP1 = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)q1, k);
      const int i = t - lane + 1;
      if (mine && i >= 1 && i <= na)
      {
        if (lane == 0)
        {
          if (first) { rH = 0; rP0 = (unsigned)i; rP1 = 0; }        // the boundary cell (i, 0)
          else { rH = qH; rP0 = qP0; rP1 = qP1; }
        }
        const unsigned a = (la[(i - 1) >> 1] >> (4 * ((i - 1) & 1))) & 15u;
        unsigned eqm = 0;                                           // bit 2 c: the row's base agrees with column c
        if (a < 4) { const unsigned x = bw ^ (a * 0x55555555u); eqm = ~(x | (x >> 1)) & bvs; }
        int dH = dgH, lH = rH;
        unsigned dP0 = dgP0, dP1 = dgP1, lP0 = rP0, lP1 = rP1;
#pragma unroll
        for (int c = 0; c < C; c++)
        {
          const unsigned ag = (eqm >> (2 * c)) & 1u;
          const int kd = (dH + (ag ? match : -mismatch)) * 4 + 2, ku = (H[c] - gap) * 4 + 1, kl = (lH - gap) * 4;
          const int kk = max(kd, max(ku, kl));
          int h = kk >> 2;
          const int sel = kk & 3;
          unsigned p0 = sel == 2 ? dP0 : sel == 1 ? P0[c] : lP0;
          unsigned p1 = (sel == 2 ? dP1 + ag : sel == 1 ? P1[c] : lP1) + (1u << 16);
          if (h <= 0) { h = 0; p0 = (unsigned)i | ((unsigned)(off0 + c + 1) << 16); p1 = 0; }
          dH = H[c]; dP0 = P0[c]; dP1 = P1[c];
          H[c] = h; P0[c] = p0; P1[c] = p1;
          lH = h; lP0 = p0; lP1 = p1;
          if (h > sH && off0 + c < nb) { sH = h; si = i; sj = off0 + c + 1; sP0 = p0; sP1 = p1; }
        }
        dgH = rH; dgP0 = rP0; dgP1 = rP1;                           // H[i][off0] is the diagonal of the next row's first column
        oH = lH; oP0 = lP0; oP1 = lP1;
        // the strip's last column, row i: lane 63 of a full strip (i - 1 < na: inside the pair's border)
        if (!last && lane == 63)
          *reinterpret_cast<ulonglong2 *>(border + 2 * (size_t)(i - 1)) =
              make_ulonglong2((unsigned long long)(unsigned)lH | ((unsigned long long)lP0 << 32), (unsigned long long)lP1);
      }
    }
    // the lane's best over the strips so far: the larger H, then the smaller i (on equal i the earlier strip has the smaller j)
    if (sH > bH || (sH == bH && sH > 0 && si < bi)) { bH = sH; bi = si; bj = sj; bP0 = sP0; bP1 = sP1; }
  }
  // the contract's order over the cells in one key: the larger H, then the smaller i, then the smaller j
  const unsigned long long key = ((unsigned long long)(unsigned)bH << 30) | ((unsigned long long)(32767 - bi) << 15) | (unsigned long long)(32767 - bj);
  unsigned long long top = key;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) { const unsigned long long o = __shfl_xor(top, s); top = o > top ? o : top; }
  const int T = na < nb ? na : nb;
  int4 *rec = reinterpret_cast<int4 *>(xa.out + p.out_index);
  if ((int)(top >> 30) < xa.min_score)                              // (min_score >= 1: no cell above 0 is never found)
  {
    if (lane == 0) { rec[0] = make_int4(0, 0, 0, 0); rec[1] = make_int4(0, 0, 0, T); }
    return;
  }
  if (key != top) return;                                           // the cells differ between lanes: one lane holds it
  rec[0] = make_int4(bH, (int)(bP0 & 0xffffu), bi - 1, (int)(bP0 >> 16));
  rec[1] = make_int4(bj - 1, (int)(bP1 & 0xffffu), (int)(bP1 >> 16), T);
}
