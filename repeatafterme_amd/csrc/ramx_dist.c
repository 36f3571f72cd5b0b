/* ramx_dist.c -- which copies of an extension to compare, the Kimura distance of a pair and the summary of a pair matrix
 * (include/ramx_dist.h): plain host C, usable without a device. */
#include <math.h>
#include <stddef.h>

#include "ramx_dist.h"

/* columns of copy i along a consensus of `rows` rows; 0 without an alignment */
static int32_t copy_cols(const ramx_aln_end *e, int32_t rows)
{
  if (e->end_row < 0 || rows <= 0) return 0;
  return (e->end_row < rows - 1 ? e->end_row : rows - 1) + 1;
}

int32_t ramx_select_copies(const ramx_aln_end *ends, int32_t n, int32_t rows, int32_t min_cols, int32_t max_copies, int32_t *out)
{
  if (!ends || !out || n <= 0) return 0;
  if (max_copies > RAMX_DIST_MAX_COPIES) max_copies = RAMX_DIST_MAX_COPIES;
  if (max_copies <= 0) return 0;
  const int32_t need = min_cols > 1 ? min_cols : 1;
  int32_t qualify = 0;
  for (int32_t i = 0; i < n; i++) qualify += copy_cols(&ends[i], rows) >= need;
  int32_t cut = need, above = 0;
  if (qualify > max_copies)
  {
    /* the largest column count t with at least max_copies copies of >= t columns: the count falls as t grows */
    int32_t lo = need, hi = rows;
    while (lo < hi)
    {
      const int32_t mid = lo + (hi - lo + 1) / 2;
      int32_t c = 0;
      for (int32_t i = 0; i < n; i++) c += copy_cols(&ends[i], rows) >= mid;
      if (c >= max_copies) lo = mid; else hi = mid - 1;
    }
    cut = lo;
    for (int32_t i = 0; i < n; i++) above += copy_cols(&ends[i], rows) > cut;
  }
  /* everything above the cut, and of those at the cut the lowest indices until the list is full */
  int32_t k = 0, at_cut = qualify > max_copies ? max_copies - above : n;
  for (int32_t i = 0; i < n; i++)
  {
    const int32_t c = copy_cols(&ends[i], rows);
    if (c < cut) continue;
    if (qualify > max_copies && c == cut) { if (at_cut <= 0) continue; at_cut--; }
    out[k++] = i;
  }
  return k;
}

double ramx_dist_kimura(const ramx_copy_dist *d)
{
  if (!d) return -1.0;
  const double sites = (double)d->sites;
  if (sites <= 0) return -1.0;
  const double p = (double)d->ts / sites, q = (double)d->tv / sites;
  const double a = 1.0 - 2.0 * p - q, b = 1.0 - 2.0 * q;
  if (a <= 0 || b <= 0) return -1.0;
  return -0.5 * log(a * sqrt(b)) * 100.0 + 0.0;        /* + 0.0: no divergence is 0, not -0 */
}

/* the Kimura value of a used pair, -1 otherwise */
static double used_kimura(const ramx_copy_dist *d, int32_t min_sites)
{
  if (d->sites < (min_sites > 1 ? min_sites : 1)) return -1.0;
  return ramx_dist_kimura(d);
}

int ramx_dist_summary(const ramx_copy_dist *m, int32_t n, int32_t min_sites, ramx_dist_family *out)
{
  if (!out || n < 0 || (n > 0 && !m)) return RAMX_ERR_ARG;
  out->n = n; out->pairs = (int32_t)((int64_t)n * (n - 1) / 2); out->used = 0; out->medoid = -1;
  out->mean = 0.0; out->medoid_mean = 0.0;
  double sum = 0.0;
  for (int32_t a = 0; a < n; a++)
  {
    /* the pairs that contain a, read from the upper triangle, in the order of the other copy */
    double sa = 0.0;
    int32_t na = 0;
    for (int32_t b = 0; b < n; b++)
    {
      if (b == a) continue;
      const double k = used_kimura(a < b ? &m[(size_t)a * n + b] : &m[(size_t)b * n + a], min_sites);
      if (k < 0) continue;
      sa += k; na++;
      if (a < b) { sum += k; out->used++; }
    }
    if (na > 0 && (out->medoid < 0 || sa / na < out->medoid_mean)) { out->medoid = a; out->medoid_mean = sa / na; }
  }
  if (out->used > 0) out->mean = sum / out->used;
  return RAMX_OK;
}
