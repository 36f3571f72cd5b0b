// ramx_kernels_profile.h -- the support profile of an extension: every flank's band replayed along a GIVEN consensus
// (device code of libramx; included by ramx_profile.hip only)
//
// Once the consensus is known no flank depends on another: a wave (one tile of 64 flanks, one lane per flank) walks its rows on
// its own -- no vote, no barrier between workgroups, no backup row.  Step r computes row r under the winner cons[r] and, from
// it, the best cell of the four candidate rows r + 1 (the losing candidates' cells are never kept).  Two kernels, one workgroup
// of one wave per tile each, the same recurrence as the extension loop's kernels in both:
//   ramx_profile_resident_kernel<W>  W = 14 / 20 / 40 / 80, no positive gap penalty: the row stays on chip as in the persistent
//                                    and family kernels (m in registers, e - m as int16 in LDS; prk_band / prk_band_fast of
//                                    ramx_kernels_resident.h, the LEAN band included);
//   ramx_profile_kernel<CHAIN>       every other band width and gap sign: run_band (ramx_kernels_common.h) on the tile's slice of
//                                    a global buffer that only this wave touches (in place, as in ramx_family_stream_kernel).
//
// Reduction: the 64 lanes' values are summed in the wave (DPP, ballots for the counts) and written as one 48-byte record per
// (tile, column) with three plain 16-byte stores -- a per-wave partial slab.  ramx_profile_sum_kernel adds the slabs of a
// family's tiles per column.  Integers: exact in any order.
#pragma once

#include "ramx_profile_api.h"
#include "ramx_kernels_resident.h"

// the record of column r of this wave: three plain 16-byte stores: total[0..1], total[2..3], (base, n_capped, n_new_high,
// n_out_of_seq)
__device__ __forceinline__ void prof_store_record(ramx_col_profile *rec, const int lane, const long long (&tot)[4], const int besta,
                                                  const int n_cap, const int n_new, const int n_out)
{
  if (lane < 3)
  {
    int4 v;
    if (lane == 0) v = make_int4((int)(unsigned)tot[0], (int)(tot[0] >> 32), (int)(unsigned)tot[1], (int)(tot[1] >> 32));
    else if (lane == 1) v = make_int4((int)(unsigned)tot[2], (int)(tot[2] >> 32), (int)(unsigned)tot[3], (int)(tot[3] >> 32));
    else v = make_int4(besta, n_cap, n_new, n_out);
    reinterpret_cast<int4 *>(rec)[lane] = v;
  }
}

// contributions to column `col` (ram_extend.c:1042-1062) from the candidates' best cells and the record after the row before;
// capped count under that column's base `next`
__device__ __forceinline__ void prof_contrib(const bool active, const int high, const int cap, const int next, const int col,
                                             const LaneDP &D, long long (&tot)[4], int &n_cap, int &last_unc)
{
  const int capv = high + cap;
  bool capped = false;
  int v[4];
#pragma unroll
  for (int c = 0; c < 4; c++)
  {
    const int b = D.bestA[c] < 0 ? 0 : D.bestA[c];
    const bool cp = b < capv;
    v[c] = active ? (cp ? capv : b) : 0;          // never negative: a capped flank contributes capv > b >= 0
    if (c == next) capped = cp;
  }
  capped = capped && active;
#pragma unroll
  for (int c = 0; c < 4; c++) tot[c] = wave_sum_nonneg31(v[c]);
  n_cap = __popcll(__ballot(capped));
  if (active && !capped) last_unc = col;
}

template <bool CHAIN>
__global__ __launch_bounds__(64) void ramx_profile_kernel(const ProfArgs pa)
{
  __shared__ __attribute__((aligned(16))) int s_tab[TAB_ROWS * TAB_STRIDE];
  const int lane = threadIdx.x, tile = blockIdx.x;
  const int2 tf = pa.tile_fam[tile];
  if (tf.x < 0) return;                               // uniform: a tile outside every family
  const KArgs &a = pa.k;
  const int W = a.W, B = 2 * W + 1, Q = W + 1;
  const int n = tile * 64 + lane;
  const bool active = lane < tf.y;                    // padding flanks contribute to nothing and are counted nowhere
  const int rows = pa.rows[tf.x];
  const signed char *cons = pa.cons + (size_t)tf.x * pa.L;
  const int4 *Sin = a.S_in + (size_t)tile * Q * 64 + lane;
  int4 *Sout = a.S_out + (size_t)tile * Q * 64 + lane;
  const int2 bd = a.bounds[n];
  const ramx_flank fl = pa.flanks[n];
  // ram_extend.c:1135-1137 looks at band cell 0 in a left extension and at cell 2W in a right one; ramx_resolve_flanks gives a
  // right extension step +1 on the forward strand and step -1 (complemented) on the reverse strand
  const bool far_is_last = (fl.step > 0) != (fl.compl_ != 0);
  ramx_col_profile *slab = pa.slab + (size_t)tile * pa.slab_rows;

  for (int i = lane; i < TAB_ROWS * TAB_STRIDE; i += 64)
  {
    const int row = i / TAB_STRIDE, col = i % TAB_STRIDE;
    s_tab[i] = (row < RAMX_NCLASS && col < 4) ? a.tab[row][col] : 0;
  }
  int prev_high = 0, last_unc = -1;
  long long tot[4] = { 0, 0, 0, 0 };                  // column r's totals and capped count, taken at step r - 1
  int n_cap = 0;
  for (int r = -1; r < rows; r++)
  {
    const unsigned *bp = a.bases + (size_t)((r + 8) >> 3) * a.Np + n;
    int4 buf[PF], far[PF];
    if (r >= 0)
    {
#pragma unroll
      for (int i = 0; i < PF; i++) buf[i] = ld_stream(Sin + (size_t)(i < Q ? i : Q - 1) * 64);
#pragma unroll
      for (int i = 0; i < PF; i++) far[i] = ld_stream(Sin + (size_t)(i + PF < Q ? i + PF : Q - 1) * 64);
    }
    const unsigned w0 = bp[0], w1 = bp[(size_t)a.Np], w2 = bp[2 * (size_t)a.Np];
    const int besta = r >= 0 ? (cons[r] & 3) : 0;
    __syncthreads();                                  // the band of the row before has done its lookups
    if (lane < RAMX_NCLASS) s_tab[lane * TAB_STRIDE + 4] = a.tab[lane][besta];
    __syncthreads();
    const int jlo = bd.x - r, jhi = bd.y - r;
    const int e1_prev = r >= 0 ? buf[0].w : 0;                    // e of row r-1, cell 1: the deletion term of row r's cell 0
    LaneDP D;
    D.eC = NEG; D.mPrev = NEG - 1000000; D.bestF = NEG; D.jbest = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) { D.eA[c] = NEG; D.bestA[c] = NEG; }
    int high = 0, pos = 0;
    if (r < 0)
      run_band<true, true, CHAIN>(a, r, s_tab, Sin, Sout, bp, jlo, jhi, D, high, pos, buf, far, w0, w1, w2);
    else
    {
      const bool all_in = __all(!active || ((jlo <= 0) && (jhi >= B)));
      if (all_in) run_band<false, false, CHAIN>(a, r, s_tab, Sin, Sout, bp, jlo, jhi, D, high, pos, buf, far, w0, w1, w2);
      else run_band<false, true, CHAIN>(a, r, s_tab, Sin, Sout, bp, jlo, jhi, D, high, pos, buf, far, w0, w1, w2);
    }
    if (r >= 0)
    {
      // the kept row: record setters (ram_extend.c:1140-1150; run_band raised `high` iff the row's best beat it) and the gap
      // state of the far edge cell (:1135-1137), derived as band_step derives it: cell 0 has no insertion, so its gap is the
      // deletion from e of the row before's cell 1; cell 2W has no deletion, so its gap is e of this row's cell 2W-1; an
      // out-of-bounds cell holds the fill value of bnw_extend.c:990-1002
      const bool new_high = active && high > prev_high;
      int gap;
      if (far_is_last)
        gap = (jlo <= 2 * W && 2 * W <= jhi) ? imax(Sout[(size_t)(W - 1) * 64].w, NEG) : SENT;
      else
        gap = (jlo <= 0 && 0 <= jhi) ? imax(NEG, e1_prev) : ((r < W) ? a.go + (r + 1) * a.ge : SENT);
      const bool out = active && gap < -279000;
      const int n_new = __popcll(__ballot(new_high)), n_out = __popcll(__ballot(out));
      if (pa.row_best != nullptr)
      {
        pa.row_best[(size_t)r * a.Np + n] = D.bestF;
        pa.row_best_idx[(size_t)r * a.Np + n] = r + D.jbest - W;
      }
      prof_store_record(slab + r, lane, tot, besta, n_cap, n_new, n_out);
    }
    prev_high = high;
    if (r + 1 < rows) prof_contrib(active, high, a.cap, cons[r + 1] & 3, r + 1, D, tot, n_cap, last_unc);
  }
  pa.last_uncapped[n] = active ? last_unc : -1;
}

// The same replay with the row on chip.  One wave per workgroup, so the tables and the d-row in LDS are the wave's own and the
// block barriers below cost nothing; W = 80 runs one wave per SIMD (the row takes the accumulation registers too), the narrower
// bands two, as in the persistent and family kernels.
//
// LEAN (prk_band_fast) skips the candidate rows and the best cell's index.  The loop may do so when a flank can contribute
// nothing but max(0, high + cap); the replay also has to know WHETHER the flank is capped, so its test is strict:
// prevBest + 2P < max(0, high + cap) gives, for high + cap > 0, every candidate's best < high + cap (capped, contributes
// high + cap) and, for high + cap <= 0, every candidate's best < 0 (contributes 0, not capped) -- exactly what prof_contrib
// makes of the untouched D.bestA = NEG.  prevBest + P <= high: no record in this row.  Not with row_best asked for (no index).
template <int W>
__global__ __launch_bounds__(64, (W > 40 ? 1 : 2)) void ramx_profile_resident_kernel(const ProfArgs pa)
{
  constexpr int B = 2 * W + 1, NW = (B + 8) / 8 + 2, BLOCK = 64, RS = 2 * BLOCK;
  struct Smem     // tables first (16-bit ds offsets), see the persistent kernel
  {
    FastTabs ft;
    int tab4[4][TAB_ROWS * TAB_STRIDE];
    short d[((B + 1) / 2) * RS];
  };
  __shared__ __attribute__((aligned(16))) Smem sm;
  short *sD = sm.d;
  const int lane = threadIdx.x, tile = blockIdx.x;
  const int2 tf = pa.tile_fam[tile];
  if (tf.x < 0) return;                               // uniform: a tile outside every family
  const KArgs &a = pa.k;
  const int n = tile * 64 + lane;
  const bool active = lane < tf.y;
  const int rows = pa.rows[tf.x];
  const signed char *cons = pa.cons + (size_t)tf.x * pa.L;
  const int2 bd = a.bounds[n];
  const ramx_flank fl = pa.flanks[n];
  const bool far_is_last = (fl.step > 0) != (fl.compl_ != 0);       // see ramx_profile_kernel
  ramx_col_profile *slab = pa.slab + (size_t)tile * pa.slab_rows;
  short *myD = sD + 2 * lane;

  for (int i = lane; i < 4 * TAB_ROWS * TAB_STRIDE; i += BLOCK)
  {
    const int bt = i / (TAB_ROWS * TAB_STRIDE), e = i % (TAB_ROWS * TAB_STRIDE), row = e / TAB_STRIDE, col = e % TAB_STRIDE;
    int v = 0;
    if (row < RAMX_NCLASS) v = (col < 4) ? a.tab[row][col] : (col == 4 ? a.tab[row][bt] : 0);
    sm.tab4[bt][e] = v;
  }
  fast_tabs_init<BLOCK>(sm.ft, a.tab);
  __syncthreads();

  int M[B];
#pragma unroll
  for (int j = 0; j < B; j++) M[j] = 0;
  int high = 0, last_unc = -1, n_cap = 0;
  int prevBest = 0x3fffffff;                          // best cell of the previous row (LEAN test)
  long long tot[4] = { 0, 0, 0, 0 };                  // column r's totals and capped count, taken at step r - 1
  for (int r = -1; r < rows; r++)
  {
    unsigned w[NW];
    {
      const unsigned *bp = a.bases + (size_t)((r + 8) >> 3) * a.Np + n;
#pragma unroll
      for (int k = 0; k < NW; k++) w[k] = bp[(size_t)k * a.Np];
    }
    const int besta = r >= 0 ? (cons[r] & 3) : 0;
    const int *s_tab = sm.tab4[besta];
    if (r >= 0 && pa.pack_ok)
    {
      __syncthreads();                                // the band of the row before has done its lookups
      fast_tabs_winner(sm.ft, s_tab, lane);
      __syncthreads();
    }
    const int jlo = bd.x - r, jhi = bd.y - r;
    const int e1_prev = M[1] + (int)myD[1];           // e of row r-1, cell 1: the deletion term of row r's cell 0
    LaneDP D;
    D.eC = NEG; D.mPrev = NEG - 1000000; D.bestF = NEG; D.jbest = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) { D.eA[c] = NEG; D.bestA[c] = NEG; }
    if (r < 0)
      prk_band<W, true, BLOCK, true>(a.go, a.ge, s_tab, sm.ft, sD, r, w, jlo, jhi, M, D);
    else
    {
      const bool all_in = pa.pack_ok && __all(!active || ((jlo <= 0) && (jhi >= B)));
      const int capfloor = (high + a.cap) > 0 ? (high + a.cap) : 0;
      const bool lean = pa.lean_p >= 0 && pa.row_best == nullptr &&
                        __all(!active || ((prevBest + 2 * pa.lean_p < capfloor) && (prevBest + pa.lean_p <= high)));
      if (all_in)
      {
        if (lean) prk_band_fast<W, BLOCK, false, true>(a.go, a.ge, sm.ft, sD, r, 0, w, M, D);
        else prk_band<W, false, BLOCK>(a.go, a.ge, s_tab, sm.ft, sD, r, w, jlo, jhi, M, D);
      }
      else if (pa.pack_ok > 1 && r >= W && __all(!active || (jlo <= 0)))
      {
        if (lean) prk_band_fast<W, BLOCK, true, true>(a.go, a.ge, sm.ft, sD, r, jhi, w, M, D);
        else prk_band_fast<W, BLOCK, true>(a.go, a.ge, sm.ft, sD, r, jhi, w, M, D);
      }
      else prk_band<W, true, BLOCK>(a.go, a.ge, s_tab, sm.ft, sD, r, w, jlo, jhi, M, D);
      prevBest = D.bestF;
      // the kept row: record setters and the gap state of the far edge cell, as in ramx_profile_kernel; e = m + d
      const bool new_high = active && D.bestF > high;
      if (D.bestF > high) high = D.bestF;             // ram_extend.c:1140-1150
      int gap;
      if (far_is_last)
        gap = (jlo <= 2 * W && 2 * W <= jhi) ? imax(M[B - 2] + (int)myD[(W - 1) * RS + 1], NEG) : SENT;
      else
        gap = (jlo <= 0 && 0 <= jhi) ? imax(NEG, e1_prev) : ((r < W) ? a.go + (r + 1) * a.ge : SENT);
      const bool out = active && gap < -279000;
      const int n_new = __popcll(__ballot(new_high)), n_out = __popcll(__ballot(out));
      if (pa.row_best != nullptr)
      {
        // a row that lies behind the flank's last base altogether (every fill is the sentinel from row W on, bnw_extend.c:990-1002):
        // the reference's best cell is the row's first, holding the sentinel.  prk_band_fast ranks such cells below every score
        // by their keys and keeps no value for them (its bestF is then INT_MIN >> 4, its jbest 15), so the row is answered here
        const bool behind = r >= W && jhi < 0;
        pa.row_best[(size_t)r * a.Np + n] = behind ? SENT : D.bestF;
        pa.row_best_idx[(size_t)r * a.Np + n] = behind ? r - W : r + D.jbest - W;
      }
      prof_store_record(slab + r, lane, tot, besta, n_cap, n_new, n_out);
    }
    if (r + 1 < rows) prof_contrib(active, high, a.cap, cons[r + 1] & 3, r + 1, D, tot, n_cap, last_unc);
  }
  pa.last_uncapped[n] = active ? last_unc : -1;
}

// per (family, column): the sum of the family's per-wave records
__global__ __launch_bounds__(256) void ramx_profile_sum_kernel(const ProfSumArgs sa)
{
  const int4 fd = sa.fam[blockIdx.x];
  const int r = blockIdx.y * 256 + threadIdx.x;
  if (r >= fd.z) return;
  long long t[4] = { 0, 0, 0, 0 };
  int nc = 0, nn = 0, no = 0;
  for (int k = 0; k < fd.y; k++)
  {
    const int4 *s = reinterpret_cast<const int4 *>(sa.slab + (size_t)(fd.x + k) * sa.slab_rows + r);
    const int4 x = s[0], y = s[1], z = s[2];
    t[0] += ((long long)x.y << 32) | (unsigned)x.x; t[1] += ((long long)x.w << 32) | (unsigned)x.z;
    t[2] += ((long long)y.y << 32) | (unsigned)y.x; t[3] += ((long long)y.w << 32) | (unsigned)y.z;
    nc += z.y; nn += z.z; no += z.w;
  }
  ramx_col_profile o;
  o.total[0] = t[0]; o.total[1] = t[1]; o.total[2] = t[2]; o.total[3] = t[3];
  o.base = sa.cons[(size_t)blockIdx.x * sa.L + r] & 3; o.n_capped = nc; o.n_new_high = nn; o.n_out_of_seq = no;
  sa.cols[(size_t)blockIdx.x * sa.L + r] = o;
}
