/* The pure host steps of the subfamily sink (static in ramx_extend.c) under ASan + UBSan on hand-made tables, no device call:
 * the gather before and the scatter after a per-K call against a brute-force statement of "the lists of the families that have
 * K, one after the other"; the distances against their definition by enumeration; the kept groups as families of their own.
 * Every source array is exactly as long as what it holds, and so is every table a step writes to.  Built and run by
 * tools/host_asan/run.sh. */
#include "../../repeatafterme_amd/csrc/ramx_extend.c"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); return 1; } } while (0)
#define KM RAMX_SUBFAM_MAX
enum { NBMAX = 5 };

static void *exact(size_t bytes) { void *p = malloc(bytes ? bytes : 1); memset(p, 0x5a, bytes ? bytes : 1); return p; }
static uint32_t lcg_state = 12345;
static uint32_t lcg(void) { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state >> 8; }

/* a list as ramx_select_planes gives it, `rows` rows from `row0` on: the cover behind, between and before its row's variants */
static int32_t make_list(ramx_plane *out, int32_t row0, int32_t rows)
{
  static const int8_t shapes[3][5] = { { 1, 6, -1 }, { 2, 5, 6, 7, -1 }, { 6, 7, -1 } };
  int32_t P = 0;
  for (int32_t r = 0; r < rows; r++)
    for (int j = 0; shapes[r % 3][j] >= 0; j++, P++)
      if (out) { memset(&out[P], 0, sizeof(ramx_plane)); out[P].row = row0 + r; out[P].cls = shapes[r % 3][j]; }
  return P;
}
static int32_t variants_in(const ramx_plane *pl, int32_t P) { int32_t V = 0; for (int32_t i = 0; i < P; i++) V += pl[i].cls != RAMX_PLANE_COVER; return V; }

/* nb families with rows[b] rows in their lists, K[b] patterns, count[b] flanks and on[b]: the work struct up to the tables, the
 * lists and the initial patterns filled; its arrays are separate exact blocks, released by free_case */
struct a_case { struct subfam_work w; int nb; int32_t first[NBMAX], count[NBMAX], npad, var_total; };
static void make_case(struct a_case *c, int nb, const int32_t *rows, const int32_t *K, const int32_t *count, const int32_t *on)
{
  struct subfam_work *w = &c->w;
  memset(c, 0, sizeof(*c));
  c->nb = nb;
  w->h.pfirst = (int32_t *)exact(sizeof(int32_t) * nb); w->h.pcount = (int32_t *)exact(sizeof(int32_t) * nb);
  w->on = (int32_t *)exact(sizeof(int32_t) * nb); w->Kb = (int32_t *)exact(sizeof(int32_t) * nb);
  w->vfirst = (int32_t *)exact(sizeof(int32_t) * nb); w->vcount = (int32_t *)exact(sizeof(int32_t) * nb);
  w->iters = (int32_t *)exact(sizeof(int32_t) * nb); w->conv = (int32_t *)exact(sizeof(int32_t) * nb);
  w->qfirst = (int32_t *)exact(sizeof(int32_t) * nb); w->qcount = (int32_t *)exact(sizeof(int32_t) * nb);
  for (int b = 0; b < nb; b++)
  {
    w->h.pfirst[b] = w->h.planes_total; w->h.pcount[b] = make_list(NULL, 0, rows[b]);
    w->h.planes_total += w->h.pcount[b];
    c->first[b] = c->npad; c->count[b] = count[b]; c->npad += (count[b] + 63) & ~63;
    w->on[b] = on[b]; w->Kb[b] = K[b];
  }
  w->h.planes = (ramx_plane *)exact(sizeof(ramx_plane) * (size_t)w->h.planes_total);
  for (int b = 0; b < nb; b++)
  {
    make_list(w->h.planes + w->h.pfirst[b], 10 * b, rows[b]);
    w->vfirst[b] = c->var_total; w->vcount[b] = variants_in(w->h.planes + w->h.pfirst[b], w->h.pcount[b]);
    c->var_total += w->vcount[b];
  }
  /* the initial patterns: family b's [V][K] at KM * vfirst[b], the table no longer than its last block */
  size_t ilen = 0;
  for (int b = 0; b < nb; b++) if ((size_t)KM * w->vfirst[b] + (size_t)K[b] * w->vcount[b] > ilen) ilen = (size_t)KM * w->vfirst[b] + (size_t)K[b] * w->vcount[b];
  w->init = (uint8_t *)exact(ilen);
  for (int b = 0; b < nb; b++)
    for (int32_t i = 0; i < K[b] * w->vcount[b]; i++) w->init[(size_t)KM * w->vfirst[b] + i] = (uint8_t)(1 + 40 * b + i);
}
static void free_case(struct a_case *c)
{
  struct subfam_work *w = &c->w;
  free(w->h.pfirst); free(w->h.pcount); free(w->h.planes); free(w->on); free(w->Kb); free(w->vfirst); free(w->vcount); free(w->iters);
  free(w->conv); free(w->qfirst); free(w->qcount); free(w->init);
}

/* one per-K call of a case: gather into lists exactly as long as the call's, a made-up answer, scatter into tables no longer than
 * the last block in them; both against the brute-force statement */
static int gather_scatter(struct a_case *c, int K)
{
  struct subfam_work *w = &c->w;
  const int nb = c->nb;
  int32_t sumP = 0, sumV = 0, members = 0;
  for (int b = 0; b < nb; b++) if (w->on[b] && w->Kb[b] == K) { sumP += w->h.pcount[b]; sumV += w->vcount[b]; members++; }
  w->qplanes = (ramx_plane *)exact(sizeof(ramx_plane) * (size_t)sumP);
  w->init1 = (uint8_t *)exact((size_t)K * sumV);
  CHECK(subfam_gather(w, nb, K) == members);
  int32_t at = 0, vat = 0;
  for (int b = 0; b < nb; b++)
  {
    const int in = w->on[b] && w->Kb[b] == K;
    CHECK(w->qfirst[b] == at && w->qcount[b] == (in ? w->h.pcount[b] : 0));
    if (!in) continue;
    CHECK(memcmp(w->qplanes + at, w->h.planes + w->h.pfirst[b], sizeof(ramx_plane) * (size_t)w->h.pcount[b]) == 0);
    for (int32_t i = 0; i < K * w->vcount[b]; i++) CHECK(w->init1[(size_t)K * vat + i] == (uint8_t)(1 + 40 * b + i));
    at += w->h.pcount[b]; vat += w->vcount[b];
  }
  /* what the call would return: the labels of every padded flank, the others in the call's own packing */
  w->lab1 = (int32_t *)exact(sizeof(int32_t) * (size_t)c->npad); w->pats1 = (uint8_t *)exact((size_t)K * sumV);
  w->cnt1 = (int32_t *)exact(sizeof(int32_t) * (size_t)K * sumP); w->size1 = (int32_t *)exact(sizeof(int32_t) * (size_t)K * nb);
  w->it1 = (int32_t *)exact(sizeof(int32_t) * nb); w->cv1 = (int32_t *)exact(sizeof(int32_t) * nb);
  for (int32_t i = 0; i < c->npad; i++) w->lab1[i] = 1000 + i;
  for (int32_t i = 0; i < K * sumV; i++) w->pats1[i] = (uint8_t)(3 + i);
  for (int32_t i = 0; i < K * sumP; i++) w->cnt1[i] = 2000 + i;
  for (int32_t i = 0; i < K * nb; i++) w->size1[i] = 3000 + i;
  for (int b = 0; b < nb; b++) { w->it1[b] = 50 + b; w->cv1[b] = 60 + b; w->iters[b] = -1; w->conv[b] = -1; }
  size_t plen = 0, clen = 0, slen = 0;
  for (int b = 0; b < nb; b++)
  {
    const size_t Kb = (size_t)w->Kb[b];
    if ((size_t)KM * w->vfirst[b] + Kb * w->vcount[b] > plen) plen = (size_t)KM * w->vfirst[b] + Kb * w->vcount[b];
    if ((size_t)KM * w->h.pfirst[b] + Kb * w->h.pcount[b] > clen) clen = (size_t)KM * w->h.pfirst[b] + Kb * w->h.pcount[b];
    slen = (size_t)KM * b + Kb;
  }
  w->labels = (int32_t *)exact(sizeof(int32_t) * (size_t)c->npad); w->pats = (uint8_t *)exact(plen);
  w->cnt = (int32_t *)exact(sizeof(int32_t) * clen); w->size = (int32_t *)exact(sizeof(int32_t) * slen);
  for (int32_t i = 0; i < c->npad; i++) w->labels[i] = -7;
  memset(w->pats, 0xee, plen ? plen : 1);
  for (size_t i = 0; i < clen; i++) w->cnt[i] = -7;
  for (size_t i = 0; i < slen; i++) w->size[i] = -7;
  subfam_scatter(w, c->first, c->count, nb, K);
  at = 0; vat = 0;
  for (int b = 0; b < nb; b++)
  {
    const int in = w->on[b] && w->Kb[b] == K;
    const int32_t Kb = w->Kb[b];
    CHECK(w->iters[b] == (in ? 50 + b : -1) && w->conv[b] == (in ? 60 + b : -1));
    for (int32_t f = 0; f < ((c->count[b] + 63) & ~63); f++) CHECK(w->labels[c->first[b] + f] == (in && f < c->count[b] ? 1000 + c->first[b] + f : -7));
    for (int32_t i = 0; i < Kb * w->vcount[b]; i++) CHECK(w->pats[(size_t)KM * w->vfirst[b] + i] == (in ? (uint8_t)(3 + K * vat + i) : 0xee));
    for (int32_t i = 0; i < Kb * w->h.pcount[b]; i++) CHECK(w->cnt[(size_t)KM * w->h.pfirst[b] + i] == (in ? 2000 + K * at + i : -7));
    for (int32_t i = 0; i < Kb; i++) CHECK(w->size[(size_t)KM * b + i] == (in ? 3000 + K * b + i : -7));
    if (in) { at += w->h.pcount[b]; vat += w->vcount[b]; }
  }
  free(w->qplanes); free(w->init1); free(w->lab1); free(w->pats1); free(w->cnt1); free(w->size1); free(w->it1); free(w->cv1);
  free(w->labels); free(w->pats); free(w->cnt); free(w->size);
  return 0;
}

static int bit_of(const uint64_t *words, int32_t f) { return (int)((words[f / 64] >> (f % 64)) & 1); }

/* the distances of two families (the first of `count` flanks and `rows` rows, the second of 70 and 4) with one between them that
 * does not take part, against the enumeration of include/ramx.h */
static int distances(int32_t count, int32_t rows, int32_t K0)
{
  const int32_t rowss[3] = { rows, 2, 4 }, Ks[3] = { K0, 2, 3 }, counts[3] = { count, 5, 70 }, ons[3] = { 1, 0, 1 };
  struct a_case c;
  make_case(&c, 3, rowss, Ks, counts, ons);
  struct subfam_work *w = &c.w;
  w->h.bfirst = (int64_t *)exact(sizeof(int64_t) * 3);
  int64_t words = 0;
  for (int b = 0; b < 3; b++) { w->h.bfirst[b] = words; words += (int64_t)w->h.pcount[b] * ((counts[b] + 63) / 64); }
  w->h.bits = (uint64_t *)exact(sizeof(uint64_t) * (size_t)words);
  for (int64_t i = 0; i < words; i++) w->h.bits[i] = ((uint64_t)lcg() << 40) ^ ((uint64_t)lcg() << 20) ^ lcg();
  /* the patterns take the place of the initial ones: bits */
  w->pats = w->init;
  for (int b = 0; b < 3; b++) for (int32_t i = 0; i < Ks[b] * w->vcount[b]; i++) w->pats[(size_t)KM * w->vfirst[b] + i] = (uint8_t)(lcg() & 1);
  /* the distance table ends with the last family's [count][K] */
  const size_t dlen = (size_t)KM * c.first[2] + (size_t)counts[2] * Ks[2];
  w->dist = (int32_t *)calloc(dlen, sizeof(int32_t));
  subfam_distances(w, c.first, c.count, 3);
  for (int b = 0; b < 3; b++)
  {
    const ramx_plane *pp = w->h.planes + w->h.pfirst[b];
    const int32_t P = w->h.pcount[b], T = (counts[b] + 63) / 64;
    for (int32_t f = 0; f < counts[b]; f++)
      for (int k = 0; k < Ks[b]; k++)
      {
        int32_t want = 0, vn = 0;
        for (int32_t i = 0; i < P && ons[b]; i++)
        {
          if (pp[i].cls == RAMX_PLANE_COVER) continue;
          int32_t cov = -1;
          for (int32_t j = 0; j < P; j++) if (pp[j].row == pp[i].row && pp[j].cls == RAMX_PLANE_COVER) cov = j;
          CHECK(cov >= 0);
          want += bit_of(w->h.bits + w->h.bfirst[b] + (size_t)cov * T, f) & (bit_of(w->h.bits + w->h.bfirst[b] + (size_t)i * T, f) ^ w->pats[(size_t)KM * w->vfirst[b] + (size_t)vn * Ks[b] + k]);
          vn++;
        }
        CHECK(w->dist[(size_t)KM * c.first[b] + (size_t)f * Ks[b] + k] == want);
      }
  }
  free(w->h.bfirst); free(w->h.bits); free(w->dist);
  free_case(&c);
  return 0;
}

/* the kept groups of three families: 130 flanks in groups of 65, 5 and 60, one without a kept column, 7 flanks in one group */
static int kept_groups(int32_t min_members, int want_ng)
{
  enum { L = 12 };
  const int32_t rowss[3] = { 2, 0, 1 }, Ks[3] = { 3, 1, 1 }, counts[3] = { 130, 9, 7 }, ons[3] = { 1, 0, 1 }, rets[3] = { 10, 0, L };
  struct a_case c;
  make_case(&c, 3, rowss, Ks, counts, ons);
  struct subfam_work *w = &c.w;
  ramx_params p;
  struct sink_view v;
  memset(&p, 0, sizeof(p)); memset(&v, 0, sizeof(v));
  p.L = L;
  ramx_flank *fl = (ramx_flank *)exact(sizeof(ramx_flank) * (size_t)c.npad);
  int8_t *cons = (int8_t *)exact(3 * L);
  for (int32_t i = 0; i < c.npad; i++) { fl[i] = empty_flank(); fl[i].start = 5000 + i; }
  for (int i = 0; i < 3 * L; i++) cons[i] = (int8_t)(1 + i % 4);
  v.p = &p; v.nb = 3; v.fl = fl; v.npad = c.npad; v.first = c.first; v.count = c.count; v.cons = cons; v.ret = rets;
  w->labels = (int32_t *)exact(sizeof(int32_t) * (size_t)c.npad);
  w->size = (int32_t *)calloc((size_t)KM * 2 + 1, sizeof(int32_t));
  for (int32_t i = 0; i < c.npad; i++) w->labels[i] = -1;
  for (int32_t f = 0; f < 130; f++) w->labels[f] = f % 2 == 0 ? 0 : f < 10 ? 1 : 2;          /* 65, 5, 60 */
  for (int32_t f = 0; f < 9; f++) w->labels[c.first[1] + f] = 0;
  for (int32_t f = 0; f < 7; f++) w->labels[c.first[2] + f] = 0;
  w->size[0] = 65; w->size[1] = 5; w->size[2] = 60; w->size[KM] = 9; w->size[2 * KM] = 7;
  g_subfam_members = min_members;
  subfam_kept_groups(&v, w);
  CHECK(w->ng == want_ng);
  if (want_ng == 3)
  {
    /* the middle group of the first family is dropped, the second family has none */
    CHECK(w->gpad == 128 + 64 + 64);
    CHECK(w->gof[0] == 0 && w->gof[1] == 0 && w->gof[2] == 2 && w->ggroup[0] == 0 && w->ggroup[1] == 2 && w->ggroup[2] == 0);
    CHECK(w->gfirst[0] == 0 && w->gfirst[1] == 128 && w->gfirst[2] == 192 && w->gcount[0] == 65 && w->gcount[1] == 60 && w->gcount[2] == 7);
    CHECK(w->grows[0] == 10 && w->grows[1] == 10 && w->grows[2] == L);
    for (int g = 0; g < 3; g++)
    {
      const int b = w->gof[g];
      int32_t at = w->gfirst[g];
      for (int r = 0; r < L; r++) CHECK(w->gcons[g * L + r] == (r < rets[b] ? cons[b * L + r] : 0));
      for (int32_t f = 0; f < counts[b]; f++) if (w->labels[c.first[b] + f] == w->ggroup[g]) CHECK(w->gfl[at++].start == 5000 + c.first[b] + f);
      CHECK(at == w->gfirst[g] + w->gcount[g]);
      for (; at < (g < 2 ? w->gfirst[g + 1] : w->gpad); at++) CHECK(w->gfl[at].t_lo > w->gfl[at].t_hi && w->gfl[at].start == 0);
    }
  }
  else
    CHECK(w->gpad == 0 && w->gfl != NULL && w->groups != NULL);
  free(fl); free(cons);
  /* the work's own release takes what the step allocated: the tables of this program are its own */
  free(w->labels); free(w->size);
  free_case(&c);
  memset(&w->h, 0, sizeof(w->h));
  w->on = w->labels = w->cnt = w->size = w->dist = NULL; w->init = NULL; w->qplanes = NULL;
  free_subfam_work(w);
  return 0;
}

int main(void)
{
  struct a_case c;
  /* two families that share K = 3 with one without a flank between them, one with another K, one that shares K but does not take part */
  { const int32_t rows[5] = { 3, 0, 5, 4, 2 }, K[5] = { 3, 1, 3, 2, 3 }, count[5] = { 70, 0, 50, 40, 64 }, on[5] = { 1, 0, 1, 1, 0 };
    make_case(&c, 5, rows, K, count, on);
    for (int k = 1; k <= 4; k++) if (gather_scatter(&c, k)) return 1;          /* K = 4: no family has it */
    free_case(&c); }
  /* no family, and one: with K = 1, with RAMX_SUBFAM_MAX, and without a plane */
  make_case(&c, 0, NULL, NULL, NULL, NULL);
  if (gather_scatter(&c, 1)) return 1;
  free_case(&c);
  for (int t = 0; t < 3; t++)
  {
    const int32_t rows = t == 2 ? 0 : 4, K = t == 1 ? KM : 1, count = 65, on = 1;
    make_case(&c, 1, &rows, &K, &count, &on);
    if (gather_scatter(&c, K) || gather_scatter(&c, K == 1 ? 2 : 1)) return 1;
    free_case(&c);
  }
  printf("subfam gather / scatter: ok\n");
  static const int32_t counts[] = { 1, 63, 64, 65, 130 };
  for (size_t k = 0; k < sizeof(counts) / sizeof(counts[0]); k++)
    if (distances(counts[k], 5, 3) || distances(counts[k], 0, 1) || distances(counts[k], 3, KM)) return 1;      /* rows = 0: P = 0 */
  printf("subfam distances: ok\n");
  if (kept_groups(6, 3) || kept_groups(1000, 0)) return 1;
  printf("subfam kept groups: ok\n");
  return 0;
}
