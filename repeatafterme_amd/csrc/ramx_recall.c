/* ramx_recall.c -- re-call of a consensus from its pileup (include/ramx.h: ramx_recall_consensus).  Plain host C: one pass
 * over the columns, a few comparisons each. */
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
