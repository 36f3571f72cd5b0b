/* ramx_tsd.c -- the host side of the target-site duplications (include/ramx.h, ramx_tsd): the sites of a core list, what a
 * family's records say together, and the termini of the extended consensus.  Plain host C, usable without a device. */
#include <math.h>
#include <string.h>

#include "ramx_internal.h"

int ramx_tsd_check_params(const ramx_tsd_params *tp)
{
  if (!tp) { ramx_set_error("ramx_tsd_params missing"); return RAMX_ERR_ARG; }
  if (tp->slack < 0 || tp->slack > 7 || tp->kmin < 1 || tp->kmin > 32 || tp->kmax < tp->kmin || tp->kmax > 32 ||
      (tp->mm_div != 0 && tp->mm_div < 4))
  {
    ramx_set_error("ramx_tsd_params: slack %d (0..7), kmin %d (1..32), kmax %d (kmin..32), mm_div %d (0 or >= 4)", tp->slack, tp->kmin,
                   tp->kmax, tp->mm_div);
    return RAMX_ERR_ARG;
  }
  return RAMX_OK;
}

int32_t ramx_tsd_sites(const ramx_flat_cores *c, ramx_tsd_site *out)
{
  if (!c || c->n < 0 || (c->n && !out)) { ramx_set_error("ramx_tsd_sites: bad argument"); return RAMX_ERR_ARG; }
  for (int32_t n = 0; n < c->n; n++)
  {
    /* ram_extend.c:721-727: a reverse-strand core's left edge is its upper end in the library */
    if (c->orient[n]) { out[n].lo = c->right_pos[n] - c->right_len[n]; out[n].hi = c->left_pos[n] + c->left_len[n]; }
    else { out[n].lo = c->left_pos[n] - c->left_len[n]; out[n].hi = c->right_pos[n] + c->right_len[n]; }
    out[n].seq_lo = c->lower[n];
    out[n].seq_hi = c->upper[n];
  }
  return c->n;
}

int ramx_tsd_summary(const ramx_tsd *records, int32_t n, const ramx_tsd_params *tp, ramx_tsd_hist *out)
{
  int rc;
  if ((rc = ramx_tsd_check_params(tp)) != RAMX_OK) return rc;
  if (n < 0 || (n && !records) || !out) { ramx_set_error("ramx_tsd_summary: bad argument"); return RAMX_ERR_ARG; }
  for (int32_t i = 0; i < n; i++)
    if (records[i].k < 0 || records[i].k > 32) { ramx_set_error("ramx_tsd_summary: record %d has k = %d", i, records[i].k); return RAMX_ERR_ARG; }
  memset(out, 0, sizeof(*out));
  for (int32_t i = 0; i < n; i++) out->hist[records[i].k]++;
  for (int k = 1; k <= 32; k++)
    if (out->hist[k] > 0 && out->hist[k] >= out->mode_count) { out->mode = k; out->mode_count = out->hist[k]; }
  /* a random pair of words of length k agrees in all but j <= m(k) places with probability sum_j C(k, j) 3^j / 4^k; a copy has
   * (2 slack + 1)^2 shift pairs to show one at (the union bound, capped at 1) */
  const double pairs = (double)(2 * tp->slack + 1) * (double)(2 * tp->slack + 1);
  for (int k = 1; k <= 32; k++)
  {
    const int m = tp->mm_div ? k / tp->mm_div : 0;
    double term = 1.0, sum = 0.0;                       /* C(k, j) 3^j */
    for (int j = 0; j <= m; j++)
    {
      sum += term;
      term = term * 3.0 * (double)(k - j) / (double)(j + 1);
    }
    const double pr = pairs * ldexp(sum, -2 * k);
    out->null[k] = (double)n * (pr < 1.0 ? pr : 1.0);
  }
  return RAMX_OK;
}

int ramx_termini(const int8_t *cons_left, int32_t ret_left, const int8_t *cons_right, int32_t ret_right, int32_t T,
                 char *five, char *three, int32_t *tir_len)
{
  static const char base[4] = { 'A', 'C', 'G', 'T' };
  if (T < 0 || ret_left < 0 || ret_right < 0 || (ret_left && !cons_left) || (ret_right && !cons_right) || !five || !three || !tir_len)
  { ramx_set_error("ramx_termini: bad argument"); return RAMX_ERR_ARG; }
  const int32_t n5 = T < ret_left ? T : ret_left, n3 = T < ret_right ? T : ret_right;
  /* the left rows run outward from the core: the extended consensus begins with the last of them */
  for (int32_t j = 0; j < n5; j++) five[j] = base[cons_left[ret_left - 1 - j] & 3];
  five[n5] = 0;
  for (int32_t j = 0; j < n3; j++) three[j] = base[cons_right[ret_right - n3 + j] & 3];
  three[n3] = 0;
  int32_t lim = ret_left < ret_right ? ret_left : ret_right, t = 0;
  if (lim > 32) lim = 32;
  while (t < lim && cons_left[ret_left - 1 - t] == 3 - cons_right[ret_right - 1 - t]) t++;
  *tir_len = t;
  return RAMX_OK;
}
