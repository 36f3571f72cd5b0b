/* ramx_period.c -- the host side of the tandem periodicity (include/ramx.h, ramx_period): the contract on an array of codes, the
 * segments of a core list, and what a family's records say together.  Plain host C, usable without a device. */
#include <stdlib.h>
#include <string.h>

#include "ramx_internal.h"

int ramx_period_check_params(const ramx_period_params *pp)
{
  if (!pp) { ramx_set_error("ramx_period_params missing"); return RAMX_ERR_ARG; }
  if (pp->pmax < 1 || pp->pmax > RAMX_PERIOD_PMAX || pp->mm < 1 || pp->mm > 15 || pp->min_score < 1)
  {
    ramx_set_error("ramx_period_params: pmax %d (1..%d), mm %d (1..15), min_score %d (>= 1)", pp->pmax, RAMX_PERIOD_PMAX, pp->mm,
                   pp->min_score);
    return RAMX_ERR_ARG;
  }
  return RAMX_OK;
}

int ramx_period_sequence(const int8_t *codes, int32_t n, const ramx_period_params *pp, ramx_period *out)
{
  int rc;
  if ((rc = ramx_period_check_params(pp)) != RAMX_OK) return rc;
  if (n < 0 || (n && !codes) || !out) { ramx_set_error("ramx_period_sequence: bad argument"); return RAMX_ERR_ARG; }
  if (n > RAMX_PERIOD_LEN_MAX) { ramx_set_error("ramx_period_sequence: %d bases, at most %d", n, RAMX_PERIOD_LEN_MAX); return RAMX_ERR_UNSUPPORTED; }
  memset(out, 0, sizeof(*out));
  if (n < 2) return RAMX_OK;
  int8_t *x = (int8_t *)malloc((size_t)n);
  for (int32_t j = 0; j < n; j++) x[j] = (int8_t)(codes[j] >= 0 && codes[j] <= 7 ? codes[j] & 3 : 4);
  const int32_t pm = pp->pmax < n - 1 ? pp->pmax : n - 1;
  ramx_period best;
  memset(&best, 0, sizeof(best));
  for (int32_t p = 1; p <= pm; p++)
  {
    /* the one-pass scan of the contract: begin anew where the running sum is <= 0, record on strict improvement (so the earliest
     * end wins, and among its starts the latest; the smallest p wins across periods) */
    int32_t run = 0, run_b0 = 0, run_a = 0, run_d = 0;
    const int32_t pairs = n - p;
    for (int32_t b = 0; 8 * b < pairs; b++)
    {
      int32_t a = 0, dd = 0;
      const int32_t j1 = 8 * b + 8 < pairs ? 8 * b + 8 : pairs;
      for (int32_t j = 8 * b; j < j1; j++)
        if (x[j] < 4 && x[j + p] < 4) { if (x[j] == x[j + p]) a++; else dd++; }
      const int32_t s = a - pp->mm * dd;
      if (run <= 0) { run = s; run_b0 = b; run_a = a; run_d = dd; }
      else { run += s; run_a += a; run_d += dd; }
      if (run > best.score)
      {
        best.period = p; best.score = run; best.start = 8 * run_b0;
        best.end = 8 * b + 7 < pairs - 1 ? 8 * b + 7 : pairs - 1;
        best.agree = run_a; best.disagree = run_d;
      }
    }
  }
  free(x);
  if (best.score >= pp->min_score) *out = best;
  return RAMX_OK;
}

int32_t ramx_period_segments(const ramx_flat_cores *c, int32_t which, ramx_period_seg *out)
{
  if (!c || c->n < 0 || (c->n && !out) || which < 0 || which > 2) { ramx_set_error("ramx_period_segments: bad argument"); return RAMX_ERR_ARG; }
  for (int32_t n = 0; n < c->n; n++)
  {
    /* ram_extend.c:721-727: a reverse-strand core's left edge is its upper end in the library */
    const int64_t lp = c->left_pos[n], rp = c->right_pos[n], ll = c->left_len[n], rl = c->right_len[n];
    if (which == 0) { out[n].lo = c->orient[n] ? lp + 1 : lp - ll; out[n].hi = c->orient[n] ? lp + ll : lp - 1; }
    else if (which == 1) { out[n].lo = c->orient[n] ? rp - rl : rp + 1; out[n].hi = c->orient[n] ? rp - 1 : rp + rl; }
    else { out[n].lo = c->orient[n] ? rp - rl : lp - ll; out[n].hi = c->orient[n] ? lp + ll : rp + rl; }
  }
  return c->n;
}

int ramx_period_summary(const ramx_period *rec, const ramx_period_seg *segs, int32_t n, const ramx_period_params *pp, ramx_period_hist *out)
{
  int rc;
  if ((rc = ramx_period_check_params(pp)) != RAMX_OK) return rc;
  if (n < 0 || (n && (!rec || !segs)) || !out) { ramx_set_error("ramx_period_summary: bad argument"); return RAMX_ERR_ARG; }
  for (int32_t i = 0; i < n; i++)
    if (rec[i].period < 0 || rec[i].period > RAMX_PERIOD_PMAX)
    { ramx_set_error("ramx_period_summary: record %d has period = %d", i, rec[i].period); return RAMX_ERR_ARG; }
  memset(out, 0, sizeof(*out));
  out->n = n;
  int32_t *hist = (int32_t *)calloc(RAMX_PERIOD_PMAX + 1, sizeof(int32_t));
  for (int32_t i = 0; i < n; i++)
  {
    const int32_t p = rec[i].period;
    if (p == 0) continue;
    out->n_tract++;
    if (p == 1) out->n_mono++; else if (p <= 6) out->n_simple++; else out->n_tandem++;
    if (rec[i].start == 0) out->at_lo++;
    if ((int64_t)rec[i].end == segs[i].hi + 1 - segs[i].lo - p - 1) out->at_hi++;
    hist[p]++;
  }
  /* the most frequent period, ties to the smaller one */
  for (int32_t p = 1; p <= RAMX_PERIOD_PMAX; p++)
    if (hist[p] > out->mode_count) { out->mode = p; out->mode_count = hist[p]; }
  free(hist);
  return RAMX_OK;
}
