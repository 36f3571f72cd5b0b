/* ramx_stats.c -- divergence of a copy and of a family from the per-copy statistics of an extension (include/ramx.h,
 * ramx_copy_stats): plain host C, usable without a device. */
#include <math.h>

#include "ramx.h"

double ramx_copy_kimura(const ramx_copy_stats *s)
{
  if (!s) return -1.0;
  const double sites = (double)s->match + (double)s->ts + (double)s->tv;
  if (sites <= 0) return -1.0;
  const double p = (double)s->ts / sites, q = (double)s->tv / sites;
  const double a = 1.0 - 2.0 * p - q, b = 1.0 - 2.0 * q;
  if (a <= 0 || b <= 0) return -1.0;
  return -0.5 * log(a * sqrt(b)) * 100.0 + 0.0;        /* + 0.0: no divergence is 0, not -0 */
}

double ramx_family_divergence(const ramx_copy_stats *stats, int32_t n, int32_t min_sites, int32_t *n_used)
{
  const long long need = min_sites > 1 ? min_sites : 1;
  double sum = 0;
  int32_t used = 0;
  for (int32_t i = 0; stats && i < n; i++)
  {
    if ((long long)stats[i].match + stats[i].ts + stats[i].tv < need) continue;
    const double k = ramx_copy_kimura(&stats[i]);
    if (k < 0) continue;
    sum += k;
    used++;
  }
  if (n_used) *n_used = used;
  return used > 0 ? sum / used : 0.0;
}
