/* ramx_linkage.c -- co-segregation of an extension's variants, the host side (include/ramx.h, ramx_select_planes,
 * ramx_link_pairs and ramx_link_components): which bit planes to ask the device for, the pair statistic on their Gram matrix,
 * and the linked variants as the initial patterns of a split into subfamilies.  Plain host C, usable without a device.
 *
 * The statistic is a one-sided hypergeometric test per pair, and every pair of variants on different rows is tested: there is
 * NO multiple-testing correction here.  The caller sets the threshold with the number of pairs in mind. */
#include <math.h>
#include <stdlib.h>

#include "ramx.h"

struct cand { int32_t row, cls, count; };

static int by_count(const void *a, const void *b)
{
  const struct cand *x = (const struct cand *)a, *y = (const struct cand *)b;
  if (x->count != y->count) return x->count > y->count ? -1 : 1;
  if (x->row != y->row) return x->row < y->row ? -1 : 1;
  return (x->cls > y->cls) - (x->cls < y->cls);
}

static int by_place(const void *a, const void *b)
{
  const struct cand *x = (const struct cand *)a, *y = (const struct cand *)b;
  if (x->row != y->row) return x->row < y->row ? -1 : 1;
  return (x->cls > y->cls) - (x->cls < y->cls);
}

int32_t ramx_select_planes(const int8_t *cons, int32_t rows, const ramx_col_pileup *cols, int32_t min_count, int32_t min_permille,
                           int32_t max_variants, ramx_plane *out)
{
  if (!cons || !cols || !out || rows <= 0 || max_variants <= 0) return 0;
  struct cand *c = (struct cand *)malloc(sizeof(struct cand) * (size_t)rows * 6);
  if (!c) return 0;
  size_t n = 0;
  for (int32_t r = 0; r < rows; r++)
  {
    const ramx_col_pileup *col = &cols[r];
    for (int32_t cls = 0; cls < 8; cls++)
    {
      int32_t count;
      if (cls < 4) { if (cls == cons[r]) continue; count = col->match[cls]; }
      else if (cls == 5) count = col->del;
      else if (cls == 7) count = col->ins_open;
      else continue;                                  /* class N and the cover are never candidates */
      if (count >= min_count && 1000LL * count >= (long long)min_permille * col->cover) { c[n].row = r; c[n].cls = cls; c[n].count = count; n++; }
    }
  }
  if (n > (size_t)max_variants)
  {
    qsort(c, n, sizeof(*c), by_count);
    n = (size_t)max_variants;
    qsort(c, n, sizeof(*c), by_place);
  }
  /* the variants in (row, cls) order, the cover plane of their row between the classes below and above it */
  int32_t m = 0;
  for (size_t i = 0; i < n; i++)
  {
    const int first_of_row = i == 0 || c[i - 1].row != c[i].row;
    const int cover_due = c[i].cls > RAMX_PLANE_COVER && (first_of_row || c[i - 1].cls < RAMX_PLANE_COVER);
    if (cover_due) { out[m].row = c[i].row; out[m].cls = RAMX_PLANE_COVER; m++; }
    out[m].row = c[i].row; out[m].cls = c[i].cls; m++;
    const int last_of_row = i + 1 == n || c[i + 1].row != c[i].row;
    if (last_of_row && c[i].cls < RAMX_PLANE_COVER) { out[m].row = c[i].row; out[m].cls = RAMX_PLANE_COVER; m++; }
  }
  free(c);
  return m;
}

static double lchoose(int32_t n, int32_t k) { return lgamma((double)n + 1.0) - lgamma((double)k + 1.0) - lgamma((double)(n - k) + 1.0); }

/* -log10 P(X >= k), X hypergeometric: n copies, n_p of them marked, n_q drawn */
static double upper_tail_mlog10(int32_t n, int32_t n_p, int32_t n_q, int32_t k)
{
  if (n <= 0 || k <= 0) return 0.0;
  const int32_t lo = n_q - (n - n_p) > 0 ? n_q - (n - n_p) : 0, hi = n_p < n_q ? n_p : n_q;
  if (k <= lo) return 0.0;                            /* the whole support: P = 1 */
  if (k > hi) return INFINITY;                        /* no such table (not from a Gram matrix of planes) */
  const double denom = lchoose(n, n_q);
  double top = -INFINITY;
  for (int32_t x = k; x <= hi; x++)
  {
    const double t = lchoose(n_p, x) + lchoose(n - n_p, n_q - x) - denom;
    if (t > top) top = t;
  }
  double sum = 0.0;
  for (int32_t x = k; x <= hi; x++) sum += exp(lchoose(n_p, x) + lchoose(n - n_p, n_q - x) - denom - top);
  const double v = -(top + log(sum)) / log(10.0);
  return v > 0.0 ? v : 0.0;
}

int32_t ramx_link_pairs(const ramx_plane *planes, int32_t P, const int32_t *co, double min_mlog10p, ramx_link *out, int32_t cap)
{
  if (!planes || !co || P <= 0) return 0;
  /* the cover plane of every plane's row, -1 if the list has none */
  int32_t *cover = (int32_t *)malloc(sizeof(int32_t) * (size_t)P);
  if (!cover) return 0;
  for (int32_t i = 0; i < P; i++)
  {
    cover[i] = -1;
    for (int32_t j = i; j >= 0 && planes[j].row == planes[i].row; j--) if (planes[j].cls == RAMX_PLANE_COVER) cover[i] = j;
    for (int32_t j = i + 1; j < P && planes[j].row == planes[i].row; j++) if (planes[j].cls == RAMX_PLANE_COVER) cover[i] = j;
  }
  int32_t found = 0;
  for (int32_t p = 0; p < P; p++)
  {
    if (planes[p].cls == RAMX_PLANE_COVER || cover[p] < 0) continue;
    for (int32_t q = p + 1; q < P; q++)
    {
      if (planes[q].cls == RAMX_PLANE_COVER || cover[q] < 0 || planes[q].row == planes[p].row) continue;
      const size_t cp = (size_t)cover[p], cq = (size_t)cover[q], sp = (size_t)p, sq = (size_t)q, S = (size_t)P;
      ramx_link l;
      l.p = p; l.q = q;
      l.n = co[cp * S + cq]; l.n_p = co[sp * S + cq]; l.n_q = co[sq * S + cp]; l.n_pq = co[sp * S + sq];
      l.expected = l.n > 0 ? (double)l.n_p * (double)l.n_q / (double)l.n : 0.0;
      l.mlog10p = upper_tail_mlog10(l.n, l.n_p, l.n_q, l.n_pq);
      if (!(l.mlog10p >= min_mlog10p)) continue;
      if (out && found < cap) out[found] = l;
      found++;
    }
  }
  free(cover);
  return found;
}

struct comp { int32_t size, low; };

static int by_size(const void *a, const void *b)
{
  const struct comp *x = (const struct comp *)a, *y = (const struct comp *)b;
  if (x->size != y->size) return x->size > y->size ? -1 : 1;
  return (x->low > y->low) - (x->low < y->low);
}

static int32_t root_of(int32_t *up, int32_t i)
{
  while (up[i] != i) { up[i] = up[up[i]]; i = up[i]; }
  return i;
}

int32_t ramx_link_components(const ramx_plane *planes, int32_t P, const ramx_link *links, int32_t n_links, int32_t K,
                             uint8_t *init, int32_t *component)
{
  if (K < 1 || K > RAMX_SUBFAM_MAX || P < 0 || n_links < 0 || (P && !planes) || (n_links && !links)) return 0;
  /* variant number of every listed plane (-1: a cover plane); the smaller root wins a union, so a root is its lowest member */
  int32_t *vnum = (int32_t *)malloc(sizeof(int32_t) * (size_t)(P + 1) * 3);
  struct comp *c = (struct comp *)malloc(sizeof(struct comp) * (size_t)(P + 1));
  if (!vnum || !c) { free(vnum); free(c); return 0; }
  int32_t *up = vnum + (P + 1), *size = up + (P + 1), V = 0, nc = 0, Kp = 0;
  for (int32_t i = 0; i < P; i++) vnum[i] = planes[i].cls == RAMX_PLANE_COVER ? -1 : V++;
  for (int32_t v = 0; v < V; v++) { up[v] = v; size[v] = 0; }
  for (int32_t l = 0; l < n_links; l++)
  {
    if (links[l].p < 0 || links[l].p >= P || links[l].q < 0 || links[l].q >= P || vnum[links[l].p] < 0 || vnum[links[l].q] < 0) goto done;
    const int32_t a = root_of(up, vnum[links[l].p]), b = root_of(up, vnum[links[l].q]);
    if (a != b) up[a > b ? a : b] = a < b ? a : b;
  }
  for (int32_t v = 0; v < V; v++) size[root_of(up, v)]++;
  for (int32_t v = 0; v < V; v++) if (up[v] == v && size[v] >= 2) { c[nc].size = size[v]; c[nc].low = v; nc++; }
  qsort(c, (size_t)nc, sizeof(*c), by_size);
  if (nc > K - 1) nc = K - 1;
  Kp = nc + 1;
  for (int32_t v = 0; v < V; v++)
  {
    int32_t k = 0;
    for (int32_t j = 0; j < nc; j++) if (c[j].low == root_of(up, v)) k = j + 1;
    if (component) component[v] = k;
    if (init) for (int32_t j = 0; j < Kp; j++) init[(size_t)v * Kp + j] = j > 0 && j == k;
  }
done:
  free(vnum); free(c);
  return Kp;
}
