// ramx_kernels_align.h -- per-copy alignments of an extension: every flank's band replayed along a GIVEN consensus with the
// decisions of every cell kept, then walked back from the flank's end cell
// (device code of libramx; included by ramx_align.hip only)
//
// Forward (ramx_align_forward_kernel): the layout of ramx_profile_kernel -- one wave per tile of 64 flanks, one lane per flank,
// free-running, the row streamed through the wave's own slice of a global row buffer, any band width and gap sign -- but only
// the kept row: aln_run_band is run_band (ramx_kernels_common.h) without the virtual last step, with band_step left as it is;
// nothing reads the four candidate rows' best cells, so their arithmetic and table lookups are dropped by the compiler, and
// the comparisons are taken from the same sub / gap / ins / del values band_step forms.  Per cell three comparisons of the
// reference are kept, 4 bits a cell, eight cells a dword, [row][dword][flank] so that a wave's stores are coalesced:
//   bit 0  gap > sub          the state the cell's score is in (bnw_extend.c:1015; the substitution wins ties)
//   bit 1  gap > sub + go     a gap continued from this cell extends rather than opens (:896-904, :976-984; opening wins ties)
//   bit 2  ins > del          the cell's gap state came from the insertion (:1007; the deletion wins ties)
//   8      the cell lies outside the flank (it holds a fill value, :990-1002); padding lanes store 8 in every cell
// The flank's end cell is the best cell of the first row whose best beats every earlier row's and 0 (ram_extend.c:1140-1150):
// what aln_run_band keeps as (high, pos), as run_band does, and the row at which it was raised last.
//
// Walk (ramx_align_walk_kernel): one lane per flank, back from the end cell through the flank's own codes.
#pragma once

#include "ramx_align_api.h"

// The whole band of one flank (one lane) for row r, as run_band: streams S(r-1) in, S(r) out, and stores the row's decision
// codes: acode points at this lane's entry of the row's first dword, astride is the distance between dwords; a padding lane
// (apad) stores 8 in every cell.  The boundary row (INIT) stores no codes.
template <bool INIT, bool OOB>
__device__ __forceinline__ void aln_run_band(const KArgs &a, const int r, const int *s_tab, const int4 *Sin, int4 *Sout,
                                             const unsigned *bp, const int jlo, const int jhi, LaneDP &D, int &high, int &pos,
                                             int4 (&buf)[PF], int4 (&far)[PF], unsigned w0, unsigned w1, unsigned w2,
                                             unsigned *acode, const size_t astride, const bool apad)
{
  const int W = a.W, Q = W + 1, go = a.go, ge = a.ge;
  const int edgeF = (r < W) ? go + (r + 1) * ge : SENT;        // OOB fill of row r, cells j < W (bnw_extend.c:990-1002)
  const int ph4 = 4 * ((r + 8) & 7);
  const size_t wstride = (size_t)a.Np;
  unsigned acc = 0;
  auto make_u = [&](int j) {
    StepU u;
    u.j = j; u.first = (j == 0); u.hi = 2147483647;
    u.vF = OOB ? ((j < W) ? edgeF : SENT) : 0;
    u.vC = 0;
    return u;
  };
  auto fetch_slot = [&](int q, unsigned bc0, unsigned bc1, StepT &t0, StepT &t1) {
    const int j0 = 2 * q, j1 = 2 * q + 1;
    t0 = fetch_step<OOB>(s_tab, bc0, (j0 >= jlo) && (j0 <= jhi), j0 == 0);
    t1 = fetch_step<OOB>(s_tab, bc1, (j1 >= jlo) && (j1 <= jhi), false);
  };
  // one cell: its code from the values band_step is about to combine (D.eC is still e of cell j - 1: the insertion term)
  auto cell = [&](int j, const StepT &t, int Pm, int PeNext, int &m, int &e) {
    if (!INIT)
    {
      const int sub = Pm + t.sF, gap = imax(D.eC, PeNext);
      unsigned c = (gap > sub ? 1u : 0u) | (gap > sub + go ? 2u : 0u) | ((j > 0 && D.eC > PeNext) ? 4u : 0u);
      if (OOB) c = t.inb ? c : 8u;
      acc |= c << (4 * (j & 7));
    }
    band_step<INIT, true, OOB, false>(go, ge, W, make_u(j), t, Pm, PeNext, D, m, e);
  };
  auto regular_slot = [&](int q, int4 cur, int4 nxt, const StepT &t0, const StepT &t1) {
    int m0, e0, m1, e1;
    cell(2 * q, t0, cur.x, cur.w, m0, e0);
    cell(2 * q + 1, t1, cur.z, nxt.y, m1, e1);
    st_stream(Sout + (size_t)q * 64, make_int4(m0, e0, m1, e1));
    if (!INIT && (q & 3) == 3) { acode[(size_t)(q >> 2) * astride] = apad ? 0x88888888u : acc; acc = 0; }
  };
  auto final_slot = [&](int4 cur, const StepT &t0) {
    int m0, e0;
    cell(2 * W, t0, cur.x, NEG, m0, e0);                        // cell 2W has no deletion predecessor (bnw_extend.c:892)
    if (!INIT)
    {
      high = cur.z; pos = cur.w;
      if (D.bestF > high) { high = D.bestF; pos = r + D.jbest - W; }   // ram_extend.c:1140-1150
      acode[(size_t)(W >> 2) * astride] = apad ? 0x88888888u : acc;
    }
    st_stream(Sout + (size_t)W * 64, make_int4(m0, e0, high, pos));
  };
  auto nib = [](unsigned A0, unsigned A1, int k) { return ((k < 8 ? A0 : A1) >> (4 * (k & 7))) & 15u; };

  const int G = W >> 3;
  int q0 = 0;
  unsigned A0 = __builtin_amdgcn_alignbit(w1, w0, ph4);
  unsigned A1 = __builtin_amdgcn_alignbit(w2, w1, ph4);
  StepT t0, t1;
  fetch_slot(0, nib(A0, A1, 0), nib(A0, A1, 1), t0, t1);
  for (int g = 0; g < G; g++, q0 += 8)
  {
    const unsigned *bq = bp + (size_t)(2 * g + 3) * wstride;
    const unsigned w3 = bq[0], w4 = bq[wstride];               // next group's words, consumed at the END of this group
#pragma unroll
    for (int i = 0; i < PF; i++)
    {
      const int q = q0 + i;
      int4 cur = make_int4(0, 0, 0, 0), nxt = cur;
      if (!INIT)
      {
        cur = buf[i];
        nxt = buf[(i + 1) % PF];
        buf[i] = far[i];
        const int qn = q + 2 * PF;
        far[i] = ld_stream(Sin + (size_t)(qn < Q ? qn : Q - 1) * 64);
      }
      StepT n0, n1;                                            // lookups of the NEXT slot, issued before this one's math
      if (i + 1 < PF) fetch_slot(q + 1, nib(A0, A1, 2 * i + 2), nib(A0, A1, 2 * i + 3), n0, n1);
      else
      {
        A0 = __builtin_amdgcn_alignbit(w3, w2, ph4);
        A1 = __builtin_amdgcn_alignbit(w4, w3, ph4);
        fetch_slot(q + 1, nib(A0, A1, 0), nib(A0, A1, 1), n0, n1);
      }
      regular_slot(q, cur, nxt, t0, t1);
      t0 = n0; t1 = n1;
    }
    w0 = w2; w1 = w3; w2 = w4;
  }
#pragma unroll
  for (int i = 0; i < PF; i++)
  {
    const int q = q0 + i;
    if (q <= W)
    {
      int4 cur = make_int4(0, 0, 0, 0), nxt = cur;
      if (!INIT) { cur = buf[i]; nxt = buf[(i + 1) % PF]; }
      if (q < W)
      {
        StepT n0, n1;
        fetch_slot(q + 1, nib(A0, A1, (2 * i + 2) & 15), nib(A0, A1, (2 * i + 3) & 15), n0, n1);
        regular_slot(q, cur, nxt, t0, t1);
        t0 = n0; t1 = n1;
      }
      else
        final_slot(cur, t0);
    }
  }
}

__global__ __launch_bounds__(64) void ramx_align_forward_kernel(const AlnArgs aa)
{
  __shared__ __attribute__((aligned(16))) int s_tab[TAB_ROWS * TAB_STRIDE];
  const int lane = threadIdx.x, tile = aa.tile0 + blockIdx.x;
  const int2 tf = aa.tile_fam[tile];
  if (tf.x < 0) return;                               // uniform: a tile outside every family
  const KArgs &a = aa.k;
  const int W = a.W, B = 2 * W + 1, Q = W + 1;
  const int n = tile * 64 + lane;
  const bool active = lane < tf.y;
  const int rows = aa.rows[tf.x];
  const signed char *cons = aa.cons + (size_t)tf.x * aa.L;
  const int4 *Sin = a.S_in + (size_t)tile * Q * 64 + lane;
  int4 *Sout = a.S_out + (size_t)tile * Q * 64 + lane;
  const int2 bd = a.bounds[n];
  unsigned *codes = aa.codes + (size_t)blockIdx.x * 64 + lane;
  const size_t astride = (size_t)aa.gn;

  for (int i = lane; i < TAB_ROWS * TAB_STRIDE; i += 64)
  {
    const int row = i / TAB_STRIDE, col = i % TAB_STRIDE;
    s_tab[i] = (row < RAMX_NCLASS && col < 4) ? a.tab[row][col] : 0;
  }
  int prev_high = 0, end_row = -1, end_idx = -1;
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
    LaneDP D;
    D.eC = NEG; D.mPrev = NEG - 1000000; D.bestF = NEG; D.jbest = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) { D.eA[c] = NEG; D.bestA[c] = NEG; }
    int high = 0, pos = 0;
    unsigned *rc = codes + (size_t)(r < 0 ? 0 : r) * aa.nd * astride;
    if (r < 0)
      aln_run_band<true, true>(a, r, s_tab, Sin, Sout, bp, jlo, jhi, D, high, pos, buf, far, w0, w1, w2, rc, astride, !active);
    else
    {
      const bool all_in = __all(!active || ((jlo <= 0) && (jhi >= B)));
      if (all_in) aln_run_band<false, false>(a, r, s_tab, Sin, Sout, bp, jlo, jhi, D, high, pos, buf, far, w0, w1, w2, rc, astride, !active);
      else aln_run_band<false, true>(a, r, s_tab, Sin, Sout, bp, jlo, jhi, D, high, pos, buf, far, w0, w1, w2, rc, astride, !active);
      if (high > prev_high) { end_row = r; end_idx = pos; }       // aln_run_band raised `high` iff the row's best beat it
      prev_high = high;
    }
  }
  ramx_aln_end e;
  e.end_row = active ? end_row : -1; e.end_idx = active ? end_idx : -1; e.score = active ? prev_high : 0;
  e.start_idx = 0; e.tail_ins = 0;
  aa.ends[n] = e;
}

// One lane per flank: back from the end cell.  In the substitution state column r is matched to the cell's base and the walk
// goes up; in the gap state bit 2 says insertion (left) or deletion (up and right), and bit 1 of the cell gone to says whether
// the gap goes on there.  It ends at the boundary row (whose offset o >= 0 is a leading insertion of o bases) or at a cell
// outside the flank, which holds the matrix-edge fill: the columns still to come are deletions.  col_ins[r] counts the bases
// inserted between the moves of column r - 1 and of column r; the walk meets them after column r's move.
__global__ __launch_bounds__(64) void ramx_align_walk_kernel(const AlnArgs aa)
{
  const int lane = threadIdx.x, tile = aa.tile0 + blockIdx.x;
  const int2 tf = aa.tile_fam[tile];
  if (tf.x < 0 || lane >= tf.y) return;
  const int n = tile * 64 + lane;
  const int W = aa.k.W, B = 2 * W + 1, nd = aa.nd;
  const size_t Np = (size_t)aa.k.Np, gn = (size_t)aa.gn;
  const unsigned *codes = aa.codes + (size_t)blockIdx.x * 64 + lane;
  ramx_aln_end e = aa.ends[n];
  if (e.end_row < 0) return;
  auto code_at = [&](int r, int j) { return (codes[((size_t)r * nd + (j >> 3)) * gn] >> (4 * (j & 7))) & 15u; };
  int r = e.end_row, j = e.end_idx - r + W;
  int cur = -1, ins = 0, start = e.end_idx + 1;       // cur: the column whose move came last; -1: none yet (insertions are the tail)
  auto flush = [&]() {
    if (cur < 0) e.tail_ins = ins;
    else if (aa.col_ins != nullptr) aa.col_ins[(size_t)cur * Np + n] = ins;
  };
  bool gap = (j >= 0 && j < B) ? (code_at(r, j) & 1u) != 0 : false;
  // every move lowers r or j, and j stays inside the band: at most end_row + 1 + 2W + ... moves; the guard ends a walk whose
  // codes do not hold together instead of letting it leave the buffer
  for (int guard = 0; guard < 2 * (e.end_row + 1) + B + 1; guard++)
  {
    if (j < 0 || j >= B) break;
    if (r < 0)
    {
      const int o = j - W;
      ins += o > 0 ? o : 0;                           // the first o bases: a leading insertion
      start = o < 0 ? o : 0;
      break;
    }
    const unsigned c = code_at(r, j);
    if (c & 8u)
    {
      flush();
      if (aa.col_idx != nullptr)
        for (int k = 0; k <= r; k++) { aa.col_idx[(size_t)k * Np + n] = RAMX_ALN_DELETED; aa.col_ins[(size_t)k * Np + n] = 0; }
      cur = -2;                                       // flushed
      start = j - W + r + 1;
      break;
    }
    if (!gap)
    {
      flush();
      if (aa.col_idx != nullptr) aa.col_idx[(size_t)r * Np + n] = j - W + r;
      cur = r; ins = 0; start = j - W + r;
      r--;
      gap = r >= 0 && (code_at(r, j) & 1u) != 0;
    }
    else if (c & 4u)
    {
      ins++; start = j - W + r;
      j--;
      gap = j >= 0 && (code_at(r, j) & 2u) != 0;
    }
    else
    {
      flush();
      if (aa.col_idx != nullptr) aa.col_idx[(size_t)r * Np + n] = RAMX_ALN_DELETED;
      cur = r; ins = 0;
      r--; j++;
      gap = r >= 0 && j < B && (code_at(r, j) & 2u) != 0;
    }
  }
  if (cur != -2) flush();
  e.start_idx = start;
  aa.ends[n] = e;
}

// what the walk does not reach: no column
__global__ void ramx_align_preset_kernel(int *col_idx, int *col_ins, size_t count)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) { col_idx[i] = RAMX_ALN_NONE; col_ins[i] = 0; }
}
