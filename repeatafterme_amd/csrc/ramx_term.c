/* ramx_term.c -- the host side of the terminal repeats (include/ramx.h, ramx_term): the contract on two arrays of codes and what
 * a family's records say together.  Plain host C, usable without a device. */
#include <stdlib.h>
#include <string.h>

#include "ramx_internal.h"

int ramx_term_check_params(const ramx_term_params *tp)
{
  if (!tp) { ramx_set_error("ramx_term_params missing"); return RAMX_ERR_ARG; }
  if (tp->tmax < 1 || tp->tmax > RAMX_TERM_TMAX || tp->match < 1 || tp->match > 15 || tp->mismatch < 1 || tp->mismatch > 15 ||
      tp->gap < 1 || tp->gap > 31 || tp->min_score < 1 || tp->slack < 0 || tp->slack > 15 || tp->reserved[0] || tp->reserved[1])
  {
    ramx_set_error("ramx_term_params: tmax %d (1..%d), match %d (1..15), mismatch %d (1..15), gap %d (1..31), min_score %d (>= 1), "
                   "slack %d (0..15), reserved %d %d (0)", tp->tmax, RAMX_TERM_TMAX, tp->match, tp->mismatch, tp->gap, tp->min_score,
                   tp->slack, tp->reserved[0], tp->reserved[1]);
    return RAMX_ERR_ARG;
  }
  return RAMX_OK;
}

struct term_cell { int32_t h, i0, j0, matches, columns; };

int ramx_term_pair(const int8_t *a, int32_t na, const int8_t *b, int32_t nb, const ramx_term_params *tp, ramx_term *out)
{
  int rc;
  if ((rc = ramx_term_check_params(tp)) != RAMX_OK) return rc;
  if (na < 0 || nb < 0 || (na && !a) || (nb && !b) || !out) { ramx_set_error("ramx_term_pair: bad argument"); return RAMX_ERR_ARG; }
  if (na > 65536 || nb > 65536) { ramx_set_error("ramx_term_pair: %d and %d bases, at most 65536", na, nb); return RAMX_ERR_UNSUPPORTED; }
  memset(out, 0, sizeof(*out));
  out->T = na < nb ? na : nb;
  if (out->T == 0) return RAMX_OK;
  /* row i - 1 of the cells in place: cell j is overwritten by row i once its value has moved on as the diagonal of cell j + 1 */
  struct term_cell *row = (struct term_cell *)malloc(sizeof(struct term_cell) * ((size_t)nb + 1));
  for (int32_t j = 0; j <= nb; j++) { row[j].h = 0; row[j].i0 = 0; row[j].j0 = j; row[j].matches = row[j].columns = 0; }
  struct term_cell best = { 0, 0, 0, 0, 0 };
  int32_t best_i = 0, best_j = 0;
  for (int32_t i = 1; i <= na; i++)
  {
    const int ca = a[i - 1] >= 0 && a[i - 1] <= 7 ? a[i - 1] & 3 : 4;
    struct term_cell diag = row[0];
    row[0].i0 = i;                                                          /* the boundary cell (i, 0) */
    for (int32_t j = 1; j <= nb; j++)
    {
      const int cb = b[j - 1] >= 0 && b[j - 1] <= 7 ? b[j - 1] & 3 : 4;
      const int agree = ca < 4 && ca == cb;
      const struct term_cell up = row[j], left = row[j - 1];
      const int32_t D = diag.h + (agree ? tp->match : -tp->mismatch), U = up.h - tp->gap, L = left.h - tp->gap;
      int32_t h = D > U ? D : U;
      if (L > h) h = L;
      struct term_cell c;
      if (h <= 0) { c.h = 0; c.i0 = i; c.j0 = j; c.matches = c.columns = 0; }
      else
      {
        /* the first of D, U, L that holds the value */
        c = D == h ? diag : U == h ? up : left;
        c.h = h; c.columns++;
        if (D == h && agree) c.matches++;
      }
      diag = up;
      row[j] = c;
      /* rows ascend and columns ascend within a row: a strict improvement keeps the smallest i, then the smallest j */
      if (c.h > best.h) { best = c; best_i = i; best_j = j; }
    }
  }
  free(row);
  if (best.h >= tp->min_score)
  {
    out->score = best.h; out->a_start = best.i0; out->a_end = best_i - 1; out->b_start = best.j0; out->b_end = best_j - 1;
    out->matches = best.matches; out->columns = best.columns;
  }
  return RAMX_OK;
}

static int cmp_i32(const void *x, const void *y)
{
  const int32_t a = *(const int32_t *)x, b = *(const int32_t *)y;
  return a < b ? -1 : a > b;
}

int ramx_term_summary(const ramx_term *rec, int32_t n, const ramx_term_params *tp, ramx_term_family *out)
{
  int rc;
  if ((rc = ramx_term_check_params(tp)) != RAMX_OK) return rc;
  if (n < 0 || (n && !rec) || !out) { ramx_set_error("ramx_term_summary: bad argument"); return RAMX_ERR_ARG; }
  memset(out, 0, sizeof(*out));
  out->n = n;
  int32_t *len = (int32_t *)malloc(sizeof(int32_t) * 2 * (size_t)(n ? n : 1)), *dlen = len, *ilen = len + n;
  for (int32_t s = 0; s < n; s++)
  {
    const ramx_term *d = &rec[2 * (size_t)s], *v = d + 1;
    if (d->score > 0)
    {
      out->n_direct++;
      if (d->a_start <= tp->slack && d->b_end >= d->T - 1 - tp->slack)
      {
        dlen[out->direct_anchored++] = d->a_end - d->a_start + 1;
        out->direct_matches += d->matches; out->direct_columns += d->columns;
      }
    }
    if (v->score > 0)
    {
      out->n_inverted++;
      if (v->a_start <= tp->slack && v->b_start <= tp->slack)
      {
        ilen[out->inverted_anchored++] = v->a_end - v->a_start + 1;
        out->inverted_matches += v->matches; out->inverted_columns += v->columns;
      }
    }
  }
  /* the lower median: element (k - 1) / 2 of the k sorted lengths */
  if (out->direct_anchored) { qsort(dlen, (size_t)out->direct_anchored, sizeof(int32_t), cmp_i32); out->direct_median = dlen[(out->direct_anchored - 1) / 2]; }
  if (out->inverted_anchored) { qsort(ilen, (size_t)out->inverted_anchored, sizeof(int32_t), cmp_i32); out->inverted_median = ilen[(out->inverted_anchored - 1) / 2]; }
  free(len);
  if (2 * (int64_t)out->direct_anchored > n && out->direct_anchored >= out->inverted_anchored) out->verdict = 1;
  else if (2 * (int64_t)out->inverted_anchored > n && out->inverted_anchored > out->direct_anchored) out->verdict = 2;
  return RAMX_OK;
}
