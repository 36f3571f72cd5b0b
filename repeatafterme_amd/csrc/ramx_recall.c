/* ramx_recall.c -- re-call of a consensus from its pileup (include/ramx.h: ramx_recall_consensus), and the CpG-aware re-call
 * from its pileup and dinucleotide pileup (ramx_recall_cpg).  Plain host C: one pass over the columns, a few comparisons each;
 * the CpG-aware one adds a pass over the pairs of adjacent columns.
 *
 * ramx_recall_cpg's second pass cannot conflict with itself: a pair is tested only if the plain call of its 5' column is a
 * pyrimidine (C, T) and that of its 3' column a purine (G, A).  A column that is the 3' column of one tested pair is a purine
 * and so cannot be the 5' column of another; tested pairs are disjoint, and every column is rewritten at most once.  The two
 * passes therefore run as one loop: a pair is looked at as soon as both its rows are called. */
#include "ramx.h"

/* the lowest code holding the largest of v[0..3] */
static int plurality(const int32_t *v)
{
  int best = 0;
  for (int b = 1; b < 4; b++)
    if (v[b] > v[best]) best = b;
  return best;
}

int32_t ramx_recall_consensus(const int8_t *cons, int32_t rows, const ramx_col_pileup *cols, int32_t L, int8_t *out)
{
  int32_t n = 0;
  for (int32_t r = 0; r < rows && n < L; r++)
  {
    const ramx_col_pileup *c = &cols[r];
    const int64_t cover = c->cover;
    if (cover == 0) { out[n++] = cons[r]; continue; }
    for (int k = 0; k < RAMX_PILEUP_INS && n < L; k++)
    {
      const int32_t *s = c->ins[k];
      const int64_t nk = (int64_t)s[0] + s[1] + s[2] + s[3] + s[4];
      if (!(2 * nk > cover) || !(s[0] > 0 || s[1] > 0 || s[2] > 0 || s[3] > 0)) break;
      out[n++] = (int8_t)plurality(s);
    }
    if (n >= L) break;
    if (2 * (int64_t)c->del > cover) continue;
    const int best = plurality(c->match);
    const int cur = cons[r];
    const int keep = (c->match[best] == 0) || (cur >= 0 && cur < 4 && c->match[cur] == c->match[best]);
    out[n++] = (int8_t)(keep ? cur : best);
  }
  return n;
}

/* S_CG > S_plain for the pair whose 5' / 3' columns are called (a, b); D[x][y] = di[x][y], or di[y][x] when transposed */
static int cpg_wins(const int32_t (*di)[5], int transposed, int a, int b, const int32_t *matrix, int32_t cpg_ts)
{
  enum { A = 0, C = 1, G = 2, T = 3 };
  int64_t s_plain = 0, s_cg = 0;
  for (int x = 0; x < 4; x++)
    for (int y = 0; y < 4; y++)
    {
      const int64_t d = transposed ? di[y][x] : di[x][y];
      const int64_t mc = x == T ? cpg_ts : matrix[C * 100 + x], mg = y == A ? cpg_ts : matrix[G * 100 + y];
      s_plain += d * ((int64_t)matrix[a * 100 + x] + matrix[b * 100 + y]);
      s_cg += d * (mc + mg);
    }
  return s_cg > s_plain;
}

int32_t ramx_recall_cpg(const int8_t *cons, int32_t rows, const ramx_col_pileup *cols, const ramx_col_dinuc *di,
                        int32_t rows_reversed, const int32_t *matrix, int32_t cpg_ts, int32_t L, int8_t *out, int32_t *n_cpg)
{
  enum { A = 0, C = 1, G = 2, T = 3 };
  int32_t n = 0, cg = 0;
  int32_t prev_at = -1;       /* where the base of row r - 1 landed in the output; -1: dropped, or there is no such row */
  for (int32_t r = 0; r < rows && n < L; r++)
  {
    /* pass 1: the rule of ramx_recall_consensus; at: where the row's base lands, before: inserted columns emitted before it */
    const ramx_col_pileup *c = &cols[r];
    const int64_t cover = c->cover;
    int32_t at = -1, before = 0;
    if (cover == 0) { at = n; out[n++] = cons[r]; }
    else
    {
      for (int k = 0; k < RAMX_PILEUP_INS && n < L; k++)
      {
        const int32_t *s = c->ins[k];
        const int64_t nk = (int64_t)s[0] + s[1] + s[2] + s[3] + s[4];
        if (!(2 * nk > cover) || !(s[0] > 0 || s[1] > 0 || s[2] > 0 || s[3] > 0)) break;
        out[n++] = (int8_t)plurality(s);
        before++;
      }
      if (n >= L) break;
      if (!(2 * (int64_t)c->del > cover))
      {
        const int best = plurality(c->match);
        const int cur = cons[r];
        const int keep = (c->match[best] == 0) || (cur >= 0 && cur < 4 && c->match[cur] == c->match[best]);
        at = n;
        out[n++] = (int8_t)(keep ? cur : best);
      }
    }
    /* pass 2 on the pair (r - 1, r), as soon as pass 1 has called both: it writes C over a pyrimidine and G over a purine only, so
     * whether the next pair is tested reads the same from out as from the plain calls, and a tested pair holds its plain calls
     * still (tested pairs are disjoint) */
    if (prev_at >= 0 && at >= 0 && before == 0)
    {
      const int32_t p5 = rows_reversed ? at : prev_at, p3 = rows_reversed ? prev_at : at;
      const int a = out[p5], b = out[p3];
      if ((a == C || a == T) && (b == G || b == A) &&
          ((a == C && b == G) || cpg_wins(di[r - 1].di, rows_reversed != 0, a, b, matrix, cpg_ts)))
      { out[p5] = C; out[p3] = G; cg++; }
    }
    prev_at = at;
  }
  if (n_cpg) *n_cpg = cg;
  return n;
}
