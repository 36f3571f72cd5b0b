/* ramx_xfam.c -- the host side of the cross-family overlap (include/ramx_xfam.h): the record of one pair through the cells of
 * ramx_term_pair, the candidates by shared K-mers, and the groups of linked families.  Plain host C, usable without a device. */
#include <stdlib.h>
#include <string.h>

#include "ramx_xfam.h"
#include "ramx_internal.h"

int ramx_pair_check_params(const ramx_pair_params *pp)
{
  if (!pp) { ramx_set_error("ramx_pair_params missing"); return RAMX_ERR_ARG; }
  if (pp->match < 1 || pp->match > 15 || pp->mismatch < 1 || pp->mismatch > 15 || pp->gap < 1 || pp->gap > 31 || pp->min_score < 1)
  {
    ramx_set_error("ramx_pair_params: match %d (1..15), mismatch %d (1..15), gap %d (1..31), min_score %d (>= 1)", pp->match,
                   pp->mismatch, pp->gap, pp->min_score);
    return RAMX_ERR_ARG;
  }
  return RAMX_OK;
}

static inline int xfam_class(int8_t c) { return c >= 0 && c <= 7 ? c & 3 : 4; }

int ramx_seq_pair_host(const int8_t *a, int32_t na, const int8_t *b, int32_t nb, int32_t inverted, const ramx_pair_params *pp,
                       ramx_term *out)
{
  int rc;
  if ((rc = ramx_pair_check_params(pp)) != RAMX_OK) return rc;
  if (na < 0 || nb < 0 || (na && !a) || (nb && !b) || !out || inverted < 0 || inverted > 1)
  { ramx_set_error("ramx_seq_pair_host: bad argument"); return RAMX_ERR_ARG; }
  if (na > RAMX_XFAM_MAXLEN || nb > RAMX_XFAM_MAXLEN)
  { ramx_set_error("ramx_seq_pair_host: %d and %d bases, at most %d", na, nb, RAMX_XFAM_MAXLEN); return RAMX_ERR_UNSUPPORTED; }
  memset(out, 0, sizeof(*out));
  if (na == 0 || nb == 0) return RAMX_OK;
  /* the cells are those of the terminal repeats; tmax and slack play no part in a pair */
  const ramx_term_params tp = { 1, pp->match, pp->mismatch, pp->gap, pp->min_score, 0, { 0, 0 } };
  if (!inverted) return ramx_term_pair(a, na, b, nb, &tp, out);
  int8_t *br = (int8_t *)malloc((size_t)nb);
  if (!br) { ramx_set_error("ramx_seq_pair_host: out of memory"); return RAMX_ERR_ARG; }
  for (int32_t j = 0; j < nb; j++) { const int c = xfam_class(b[nb - 1 - j]); br[j] = (int8_t)(c < 4 ? 3 - c : 99); }
  rc = ramx_term_pair(a, na, br, nb, &tp, out);
  free(br);
  return rc;
}

/* ---- candidates ---- */
static int cmp_u32(const void *x, const void *y)
{
  const uint32_t a = *(const uint32_t *)x, b = *(const uint32_t *)y;
  return a < b ? -1 : a > b;
}

/* the K-mers of s[0..n) without a class-4 base, as 2 K bits (first base highest), sorted and unique; rc: those of the reversed
 * and complemented sequence.  Returns their number; km has room for n. */
static int64_t kmer_set(const int8_t *s, int64_t n, int K, int rc, uint32_t *km)
{
  const uint32_t mask = K == 16 ? 0xffffffffu : ((1u << (2 * K)) - 1u);
  uint32_t w = 0;
  int64_t m = 0;
  int run = 0;
  for (int64_t t = 0; t < n; t++)
  {
    const int c0 = xfam_class(rc ? s[n - 1 - t] : s[t]);
    if (c0 >= 4) { run = 0; w = 0; continue; }
    w = ((w << 2) | (uint32_t)(rc ? 3 - c0 : c0)) & mask;
    if (++run >= K) km[m++] = w;
  }
  if (m > 1)
  {
    qsort(km, (size_t)m, sizeof(uint32_t), cmp_u32);
    int64_t u = 1;
    for (int64_t t = 1; t < m; t++) if (km[t] != km[u - 1]) km[u++] = km[t];
    m = u;
  }
  return m;
}

static int sets_meet(const uint32_t *x, int64_t nx, const uint32_t *y, int64_t ny)
{
  int64_t i = 0, j = 0;
  while (i < nx && j < ny)
  {
    if (x[i] == y[j]) return 1;
    if (x[i] < y[j]) i++; else j++;
  }
  return 0;
}

int64_t ramx_xfam_candidates(const int8_t *codes, const int64_t *seq_off, int32_t n_seqs, const int32_t *owner, int32_t K,
                             int32_t within, ramx_seq_pair *pairs, int64_t cap)
{
  if (n_seqs < 0 || cap < 0 || !seq_off || (n_seqs && !owner) || (cap && !pairs) || !(K == 0 || (K >= 8 && K <= 16)))
  { ramx_set_error("ramx_xfam_candidates: bad argument (K %d: 0 or 8..16)", K); return RAMX_ERR_ARG; }
  for (int32_t s = 0; s < n_seqs; s++)
    if (seq_off[s] < 0 || seq_off[s + 1] < seq_off[s] || (seq_off[s + 1] > seq_off[s] && !codes))
    { ramx_set_error("ramx_xfam_candidates: seq_off decreases at sequence %d, or codes missing", s); return RAMX_ERR_ARG; }
  /* the K-mer sets of every sequence, read forward and on the other strand: set s at at[s] .. at[s] + cnt[s] */
  uint32_t *km = NULL;
  int64_t *at = NULL, *cnt = NULL;
  if (K && n_seqs)
  {
    const int64_t total = seq_off[n_seqs] - seq_off[0];
    km = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)(2 * total + 1));
    at = (int64_t *)malloc(sizeof(int64_t) * 2 * (size_t)n_seqs);
    cnt = (int64_t *)malloc(sizeof(int64_t) * 2 * (size_t)n_seqs);
    if (!km || !at || !cnt) { free(km); free(at); free(cnt); ramx_set_error("ramx_xfam_candidates: out of memory"); return RAMX_ERR_ARG; }
    int64_t used = 0;
    for (int32_t s = 0; s < n_seqs; s++)
      for (int rc = 0; rc < 2; rc++)
      {
        const int64_t n = seq_off[s + 1] - seq_off[s];
        at[2 * s + rc] = used;
        cnt[2 * s + rc] = kmer_set(codes + seq_off[s], n, K, rc, km + used);
        used += n;                                              /* (room for n, whatever the count) */
      }
  }
  int64_t count = 0;
  for (int32_t a = 0; a < n_seqs; a++)
    for (int32_t b = a + 1; b < n_seqs; b++)
    {
      if ((!within && owner[a] == owner[b]) || seq_off[a + 1] == seq_off[a] || seq_off[b + 1] == seq_off[b]) continue;
      for (int inv = 0; inv < 2; inv++)
      {
        if (K && !sets_meet(km + at[2 * a], cnt[2 * a], km + at[2 * b + inv], cnt[2 * b + inv])) continue;
        if (count < cap) { pairs[count].a = a; pairs[count].b = b; pairs[count].inverted = inv; pairs[count].reserved = 0; }
        count++;
      }
    }
  free(km); free(at); free(cnt);
  return count;
}

/* ---- groups ---- */
static int32_t root_of(int32_t *up, int32_t f)
{
  while (up[f] != f) { up[f] = up[up[f]]; f = up[f]; }
  return f;
}

int ramx_xfam_groups(const ramx_seq_pair *pairs, const ramx_term *rec, int32_t n_pairs, const int32_t *owner, int32_t n_families,
                     const ramx_xfam_link_params *lp, int32_t *counts, int32_t *group)
{
  if (!lp || lp->min_columns < 0 || lp->min_permille < 0 || lp->min_permille > 1000 || n_pairs < 0 || n_families < 0 ||
      (n_pairs && (!pairs || !rec || !owner || !counts)) || (n_families && !group))
  { ramx_set_error("ramx_xfam_groups: bad argument (min_columns >= 0, min_permille 0..1000)"); return RAMX_ERR_ARG; }
  for (int32_t p = 0; p < n_pairs; p++)
  {
    if (pairs[p].a < 0 || pairs[p].b < 0) { ramx_set_error("ramx_xfam_groups: pair %d: negative sequence index", p); return RAMX_ERR_ARG; }
    const int32_t fa = owner[pairs[p].a], fb = owner[pairs[p].b];
    if (fa < 0 || fa >= n_families || fb < 0 || fb >= n_families)
    { ramx_set_error("ramx_xfam_groups: pair %d: owners %d and %d outside 0..%d", p, fa, fb, n_families - 1); return RAMX_ERR_ARG; }
  }
  /* union-find whose root is always the smallest index of its set */
  for (int32_t f = 0; f < n_families; f++) group[f] = f;
  for (int32_t p = 0; p < n_pairs; p++)
  {
    const ramx_term *r = &rec[p];
    counts[p] = r->score > 0 && r->columns >= lp->min_columns && 1000 * (int64_t)r->matches >= (int64_t)lp->min_permille * r->columns;
    if (!counts[p]) continue;
    const int32_t ra = root_of(group, owner[pairs[p].a]), rb = root_of(group, owner[pairs[p].b]);
    if (ra < rb) group[rb] = ra; else if (rb < ra) group[ra] = rb;
  }
  for (int32_t f = 0; f < n_families; f++) group[f] = root_of(group, f);
  return RAMX_OK;
}
