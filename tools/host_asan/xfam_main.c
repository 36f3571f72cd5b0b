/* ramx_seq_pair_host, ramx_xfam_candidates and ramx_xfam_groups (csrc/ramx_xfam.c and the cells of csrc/ramx_term.c, both
 * compiled into this program) on random inputs against a brute force of the contract's own words: the full matrix of cells with
 * its payload, every pair of offsets base by base, and labels relaxed until nothing changes.  Buffers have exactly the
 * promised size.  CPU only. */
#include <assert.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ramx_xfam.h"

void ramx_set_error(const char *fmt, ...) { (void)fmt; }

#include "ramx_term.c"
#include "ramx_xfam.c"

static unsigned long long g_state = 88172645463325252ULL;
static unsigned rnd(unsigned n) { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return (unsigned)((g_state >> 11) % n); }

static int cls(int8_t c) { return c >= 0 && c <= 7 ? c & 3 : 4; }
/* class of B'[j] */
static int cls_b(const int8_t *b, int nb, int j, int inv) { const int c = cls(inv ? b[nb - 1 - j] : b[j]); return inv && c < 4 ? 3 - c : c; }

struct cell { int h, i0, j0, m, c; };

static void brute_pair(const int8_t *a, int na, const int8_t *b, int nb, int inv, const ramx_pair_params *pp, ramx_term *out)
{
  memset(out, 0, sizeof(*out));
  if (!na || !nb) return;
  out->T = na < nb ? na : nb;
  struct cell *M = (struct cell *)malloc(sizeof(struct cell) * (size_t)(na + 1) * (size_t)(nb + 1));
#define AT(i, j) M[(size_t)(i) * (size_t)(nb + 1) + (size_t)(j)]
  int bh = 0, bi = 0, bj = 0;
  for (int i = 0; i <= na; i++)
    for (int j = 0; j <= nb; j++)
    {
      struct cell x = { 0, i, j, 0, 0 };
      if (i && j)
      {
        const int ca = cls(a[i - 1]), cb = cls_b(b, nb, j - 1, inv), agree = ca < 4 && ca == cb;
        const int D = AT(i - 1, j - 1).h + (agree ? pp->match : -pp->mismatch), U = AT(i - 1, j).h - pp->gap, L = AT(i, j - 1).h - pp->gap;
        int h = D > U ? D : U;
        if (L > h) h = L;
        if (h > 0)
        {
          x = D == h ? AT(i - 1, j - 1) : U == h ? AT(i - 1, j) : AT(i, j - 1);
          x.h = h; x.c++;
          if (D == h && agree) x.m++;
        }
      }
      AT(i, j) = x;
      if (x.h > bh) { bh = x.h; bi = i; bj = j; }
    }
  if (bh >= pp->min_score)
  {
    const struct cell x = AT(bi, bj);
    out->score = bh; out->a_start = x.i0; out->a_end = bi - 1; out->b_start = x.j0; out->b_end = bj - 1; out->matches = x.m; out->columns = x.c;
  }
#undef AT
  free(M);
}

static int brute_share(const int8_t *a, int na, const int8_t *b, int nb, int K, int inv)
{
  for (int oa = 0; oa + K <= na; oa++)
    for (int ob = 0; ob + K <= nb; ob++)
    {
      int t = 0;
      for (; t < K; t++)
      {
        const int x = cls(a[oa + t]), y = cls(inv ? b[ob + K - 1 - t] : b[ob + t]);
        if (x >= 4 || y >= 4 || x != (inv ? 3 - y : y)) break;
      }
      if (t == K) return 1;
    }
  return 0;
}

static int8_t *random_seq(int n)
{
  int8_t *s = (int8_t *)malloc((size_t)(n ? n : 1));
  static const int8_t odd[6] = { 8, 99, -1, 14, -128, 127 };
  for (int i = 0; i < n; i++) s[i] = rnd(25) ? (int8_t)rnd(8) : odd[rnd(6)];
  return s;
}

int main(void)
{
  /* ---- the pair ---- */
  for (int trial = 0; trial < 300; trial++)
  {
    const int na = (int)rnd(trial % 10 ? 40 : 300), nb = (int)rnd(trial % 7 ? 40 : 300), inv = (int)rnd(2);
    int8_t *a = random_seq(na), *b = random_seq(nb);
    if (na > 12 && nb > 12 && rnd(2))                          /* something in common, on either strand */
      for (int t = 0; t < 10; t++) { const int8_t c = (int8_t)rnd(4); a[2 + t] = c; if (inv) b[nb - 3 - t] = (int8_t)(3 - c); else b[1 + t] = c; }
    const ramx_pair_params pp = { 1 + (int)rnd(15), 1 + (int)rnd(15), 1 + (int)rnd(31), 1 + (int)rnd(30) };
    ramx_term *got = (ramx_term *)malloc(sizeof(ramx_term)), want;
    assert(ramx_seq_pair_host(na ? a : NULL, na, nb ? b : NULL, nb, inv, &pp, got) == RAMX_OK);
    brute_pair(a, na, b, nb, inv, &pp, &want);
    assert(memcmp(got, &want, sizeof(want)) == 0);
    free(got); free(a); free(b);
  }
  {
    const ramx_pair_params pp = { 2, 3, 5, 80 }, bad = { 2, 3, 32, 80 };
    int8_t *big = random_seq(RAMX_XFAM_MAXLEN + 1);
    ramx_term r;
    assert(ramx_seq_pair_host(big, RAMX_XFAM_MAXLEN + 1, big, 4, 0, &pp, &r) == RAMX_ERR_UNSUPPORTED);
    assert(ramx_seq_pair_host(big, 4, big, 4, 2, &pp, &r) == RAMX_ERR_ARG && ramx_seq_pair_host(big, 4, big, 4, 0, &bad, &r) == RAMX_ERR_ARG);
    assert(ramx_seq_pair_host(big, RAMX_XFAM_MAXLEN, big + 1, 300, 1, &pp, &r) == RAMX_OK && r.T == 300);
    free(big);
  }

  /* ---- the candidates ---- */
  for (int trial = 0; trial < 300; trial++)
  {
    const int n = (int)rnd(6), K = trial % 5 == 0 ? 0 : 8 + (int)rnd(3), within = (int)rnd(2);
    int64_t *off = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n + 1));
    int32_t *owner = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n ? n : 1));
    off[0] = 0;
    for (int s = 0; s < n; s++) { off[s + 1] = off[s] + (rnd(6) ? (int)rnd(50) : 0); owner[s] = (int32_t)rnd(3); }
    int8_t *codes = random_seq((int)off[n]);
    int8_t motif[10];
    for (int t = 0; t < 10; t++) motif[t] = (int8_t)rnd(4);
    for (int s = 0; s < n; s++)
      if (off[s + 1] - off[s] > 14 && rnd(3))
      {
        const int at = (int)rnd((unsigned)(off[s + 1] - off[s] - 10)), rc = (int)rnd(2);
        for (int t = 0; t < 10; t++) codes[off[s] + at + t] = rc ? (int8_t)(3 - motif[9 - t]) : motif[t];
      }
    ramx_seq_pair *want = (ramx_seq_pair *)malloc(sizeof(ramx_seq_pair) * (size_t)(n * n + 1));
    int64_t nw = 0;
    for (int a = 0; a < n; a++)
      for (int b = a + 1; b < n; b++)
        for (int inv = 0; inv < 2; inv++)
        {
          const int na = (int)(off[a + 1] - off[a]), nb = (int)(off[b + 1] - off[b]);
          if ((!within && owner[a] == owner[b]) || !na || !nb) continue;
          if (K && !brute_share(codes + off[a], na, codes + off[b], nb, K, inv)) continue;
          want[nw].a = a; want[nw].b = b; want[nw].inverted = inv; want[nw].reserved = 0; nw++;
        }
    assert(ramx_xfam_candidates(codes, off, n, owner, K, within, NULL, 0) == nw);
    const int64_t cap = nw ? (int64_t)rnd((unsigned)nw + 1) : 0;
    for (int pass = 0; pass < 2; pass++)
    {
      const int64_t room = pass ? nw : cap;
      ramx_seq_pair *got = (ramx_seq_pair *)malloc(sizeof(ramx_seq_pair) * (size_t)(room ? room : 1));
      assert(ramx_xfam_candidates(codes, off, n, owner, K, within, room ? got : NULL, room) == nw);
      assert(memcmp(got, want, sizeof(ramx_seq_pair) * (size_t)room) == 0);
      free(got);
    }
    assert(ramx_xfam_candidates(codes, off, n, owner, 7, within, NULL, 0) == RAMX_ERR_ARG);
    assert(ramx_xfam_candidates(codes, off, n, owner, 17, within, NULL, 0) == RAMX_ERR_ARG);
    free(want); free(codes); free(off); free(owner);
  }

  /* ---- the groups ---- */
  for (int trial = 0; trial < 300; trial++)
  {
    const int F = 1 + (int)rnd(8), S = 1 + (int)rnd(12), P = (int)rnd(20);
    int32_t *owner = (int32_t *)malloc(sizeof(int32_t) * (size_t)S);
    for (int s = 0; s < S; s++) owner[s] = (int32_t)rnd((unsigned)F);
    ramx_seq_pair *pairs = (ramx_seq_pair *)malloc(sizeof(ramx_seq_pair) * (size_t)(P ? P : 1));
    ramx_term *rec = (ramx_term *)calloc((size_t)(P ? P : 1), sizeof(ramx_term));
    const ramx_xfam_link_params lp = { (int32_t)rnd(100), (int32_t)rnd(1001) };
    for (int p = 0; p < P; p++)
    {
      pairs[p].a = (int32_t)rnd((unsigned)S); pairs[p].b = (int32_t)rnd((unsigned)S); pairs[p].inverted = (int32_t)rnd(2); pairs[p].reserved = 0;
      rec[p].score = rnd(4) ? 1 + (int32_t)rnd(500) : 0;
      rec[p].columns = (int32_t)rnd(200); rec[p].matches = rec[p].columns ? (int32_t)rnd((unsigned)rec[p].columns + 1) : 0;
    }
    int32_t *counts = (int32_t *)malloc(sizeof(int32_t) * (size_t)(P ? P : 1)), *group = (int32_t *)malloc(sizeof(int32_t) * (size_t)F);
    assert(ramx_xfam_groups(P ? pairs : NULL, P ? rec : NULL, P, owner, F, &lp, P ? counts : NULL, group) == RAMX_OK);
    int32_t *lab = (int32_t *)malloc(sizeof(int32_t) * (size_t)F);
    for (int f = 0; f < F; f++) lab[f] = f;
    for (int changed = 1; changed;)
    {
      changed = 0;
      for (int p = 0; p < P; p++)
      {
        const int c = rec[p].score > 0 && rec[p].columns >= lp.min_columns && 1000LL * rec[p].matches >= (long long)lp.min_permille * rec[p].columns;
        assert(counts[p] == c);
        if (!c) continue;
        int32_t *x = &lab[owner[pairs[p].a]], *y = &lab[owner[pairs[p].b]];
        if (*x < *y) { *y = *x; changed = 1; } else if (*y < *x) { *x = *y; changed = 1; }
      }
    }
    assert(memcmp(lab, group, sizeof(int32_t) * (size_t)F) == 0);
    free(lab); free(counts); free(group); free(rec); free(pairs); free(owner);
  }
  printf("xfam_main: ok\n");
  return 0;
}
