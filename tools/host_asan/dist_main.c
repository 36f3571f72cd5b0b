/* ramx_select_copies, ramx_dist_kimura and ramx_dist_summary (csrc/ramx_dist.c, compiled into this program) at their corners:
 * selection ties and the cut at max_copies in buffers of exactly the promised size, the clamps, the summary on empty, single and
 * undefined inputs and a medoid tie, and the edges of the Kimura formula.  CPU only. */
#include <assert.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ramx_dist.c"

static ramx_aln_end end_at(int32_t end_row) { ramx_aln_end e = { end_row, 0, 0, 0, 0 }; return e; }

int main(void)
{
  /* nothing to select from: nothing is read, nothing is written */
  int32_t *none = (int32_t *)malloc(1);
  assert(ramx_select_copies(NULL, 0, 10, 1, 256, none) == 0);
  ramx_aln_end one = end_at(4);
  assert(ramx_select_copies(&one, 1, 10, 1, 0, none) == 0 && ramx_select_copies(&one, 1, 10, 1, -5, none) == 0);
  assert(ramx_select_copies(&one, 1, 0, 0, 256, none) == 0);                 /* rows = 0: no columns */
  free(none);

  /* ties and the cut: end rows 9 9 4 -1 9 4 20 along 10 rows -> columns 10 10 5 0 10 5 10 */
  const int32_t er[7] = { 9, 9, 4, -1, 9, 4, 20 };
  ramx_aln_end *e7 = (ramx_aln_end *)malloc(sizeof(ramx_aln_end) * 7);
  for (int i = 0; i < 7; i++) e7[i] = end_at(er[i]);
  for (int cap = 1; cap <= 7; cap++)
  {
    int32_t *out = (int32_t *)malloc(sizeof(int32_t) * (size_t)cap);      /* room for min(n, max_copies) */
    const int32_t k = ramx_select_copies(e7, 7, 10, 0, cap, out);
    const int32_t want[6] = { 0, 1, 4, 6, 2, 5 };                          /* by columns, ties to the lower index */
    assert(k == (cap < 6 ? cap : 6));
    for (int i = 1; i < k; i++) assert(out[i] > out[i - 1]);
    for (int i = 0; i < k; i++)
    {
      int found = 0;
      for (int j = 0; j < k; j++) found |= out[j] == want[i];
      assert(found);
    }
    free(out);
  }
  int32_t out7[7];
  assert(ramx_select_copies(e7, 7, 10, 6, 256, out7) == 4 && out7[0] == 0 && out7[3] == 6);      /* min_cols between the two lengths */
  assert(ramx_select_copies(e7, 7, 10, 11, 256, out7) == 0);                                       /* above every copy */
  assert(ramx_select_copies(e7, 7, 10, -3, 1 << 30, out7) == 6);                                   /* both clamps */
  free(e7);

  /* more copies than the limit, all of one length: the first RAMX_DIST_MAX_COPIES */
  const int32_t many = RAMX_DIST_MAX_COPIES + 100;
  ramx_aln_end *em = (ramx_aln_end *)malloc(sizeof(ramx_aln_end) * (size_t)many);
  int32_t *om = (int32_t *)malloc(sizeof(int32_t) * RAMX_DIST_MAX_COPIES);
  for (int i = 0; i < many; i++) em[i] = end_at(7);
  assert(ramx_select_copies(em, many, 8, 1, many, om) == RAMX_DIST_MAX_COPIES && om[0] == 0 && om[RAMX_DIST_MAX_COPIES - 1] == RAMX_DIST_MAX_COPIES - 1);
  free(em); free(om);

  /* Kimura: identical, undefined at a = 0 and at b = 0, no site, and a value by hand */
  ramx_copy_dist r = { 100, 100, 0, 0, 0, 0 };
  assert(ramx_dist_kimura(&r) == 0.0 && !signbit(ramx_dist_kimura(&r)));
  r.ts = 50; assert(ramx_dist_kimura(&r) == -1.0);
  r.ts = 0; r.tv = 50; assert(ramx_dist_kimura(&r) == -1.0);
  r.sites = 0; r.tv = 0; assert(ramx_dist_kimura(&r) == -1.0);
  assert(ramx_dist_kimura(NULL) == -1.0);
  r = (ramx_copy_dist){ 100, 100, 10, 5, 0, 0 };
  assert(fabs(ramx_dist_kimura(&r) - (-0.5 * log(0.75 * sqrt(0.9)) * 100.0)) < 1e-12);

  /* the summary: empty, single, two, all undefined, a medoid tie */
  ramx_dist_family s;
  assert(ramx_dist_summary(NULL, 0, 1, &s) == RAMX_OK && s.n == 0 && s.pairs == 0 && s.used == 0 && s.medoid == -1 && s.mean == 0.0);
  assert(ramx_dist_summary(NULL, 1, 1, &s) == RAMX_ERR_ARG && ramx_dist_summary(NULL, -1, 1, &s) == RAMX_ERR_ARG);
  ramx_copy_dist *m1 = (ramx_copy_dist *)calloc(1, sizeof(ramx_copy_dist));
  assert(ramx_dist_summary(m1, 1, 1, &s) == RAMX_OK && s.n == 1 && s.pairs == 0 && s.medoid == -1);
  assert(ramx_dist_summary(m1, 1, 1, NULL) == RAMX_ERR_ARG);
  free(m1);
  ramx_copy_dist *m3 = (ramx_copy_dist *)calloc(9, sizeof(ramx_copy_dist));
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) m3[a * 3 + b] = (ramx_copy_dist){ 100, 100, a == b ? 0 : 50, 0, 0, 0 };      /* every pair undefined */
  assert(ramx_dist_summary(m3, 3, 1, &s) == RAMX_OK && s.pairs == 3 && s.used == 0 && s.medoid == -1 && s.mean == 0.0 && s.medoid_mean == 0.0);
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) m3[a * 3 + b].ts = a == b ? 0 : 10;                                            /* all equal: the lowest wins */
  assert(ramx_dist_summary(m3, 3, 1, &s) == RAMX_OK && s.used == 3 && s.medoid == 0 && fabs(s.mean - s.medoid_mean) < 1e-12 && s.mean > 0);
  assert(ramx_dist_summary(m3, 3, 101, &s) == RAMX_OK && s.used == 0 && s.medoid == -1);                       /* too few sites */
  m3[0 * 3 + 1].ts = m3[1 * 3 + 0].ts = 20;                                                                     /* 0-1 far: copy 2 is the medoid */
  assert(ramx_dist_summary(m3, 3, 0, &s) == RAMX_OK && s.used == 3 && s.medoid == 2);
  assert(ramx_dist_summary(m3, 2, 1, &s) == RAMX_OK && s.pairs == 1);       /* reads [2][2] of the same buffer */
  free(m3);
  printf("dist_main: ok\n");
  return 0;
}
