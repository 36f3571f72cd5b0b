/* ramx_select_planes, ramx_link_pairs and ramx_link_components (csrc/ramx_linkage.c, compiled into this program) at the corners
 * of their layouts: rows = 0, columns without cover, max_variants = 1, cap = 0, and 2048 planes; no plane, no link, every link of
 * the 2048-plane list, K = 1 and 8.  CPU only. */
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ramx_linkage.c"

int main(void)
{
  /* rows = 0: nothing is read, nothing is written */
  ramx_plane none[2];
  int8_t c0 = 0;
  ramx_col_pileup col0;
  memset(&col0, 0, sizeof(col0));
  assert(ramx_select_planes(&c0, 0, &col0, 4, 100, 1024, none) == 0);
  assert(ramx_select_planes(NULL, 0, NULL, 4, 100, 1024, none) == 0);

  /* columns without cover: no count reaches min_count >= 1; with min_count = 0 every candidate qualifies (0 >= 0) and the cap holds */
  enum { R = 1024 };
  int8_t *cons = (int8_t *)malloc(R);
  ramx_col_pileup *cols = (ramx_col_pileup *)calloc(R, sizeof(*cols));
  for (int r = 0; r < R; r++) cons[r] = (int8_t)(r & 3);
  ramx_plane *out = (ramx_plane *)malloc(sizeof(ramx_plane) * 2 * 1024);
  assert(ramx_select_planes(cons, R, cols, 1, 0, 1024, out) == 0);
  { const int32_t all0 = ramx_select_planes(cons, R, cols, 0, 0, 1024, out); assert(all0 > 1024 && all0 <= 2048); }

  /* every row has five variants (three bases, the deletion, the insertion): 5120 candidates */
  for (int r = 0; r < R; r++)
  {
    cols[r].base = cons[r]; cols[r].cover = 100;
    for (int b = 0; b < 4; b++) cols[r].match[b] = b == cons[r] ? 40 : 10 + (r % 7);
    cols[r].del = 12; cols[r].ins_open = 11;
  }
  /* max_variants = 1: room for exactly two planes, the variant and its row's cover */
  ramx_plane *two = (ramx_plane *)malloc(sizeof(ramx_plane) * 2);
  assert(ramx_select_planes(cons, R, cols, 4, 100, 1, two) == 2);
  assert(two[0].row == two[1].row && two[0].cls != RAMX_PLANE_COVER && two[1].cls == RAMX_PLANE_COVER);
  free(two);
  assert(ramx_select_planes(cons, R, cols, 4, 100, 0, out) == 0);
  /* the cap: 1024 variants on at most 1024 rows: at most 2048 planes, sorted */
  const int32_t P = ramx_select_planes(cons, R, cols, 4, 100, 1024, out);
  assert(P > 1024 && P <= 2048);
  for (int i = 1; i < P; i++) assert(out[i].row > out[i - 1].row || (out[i].row == out[i - 1].row && out[i].cls > out[i - 1].cls));

  /* P = 2048 in the pair statistic: 1024 rows of (variant, cover), a Gram matrix of 16 MB */
  enum { P2 = RAMX_LINKAGE_MAX_PLANES };
  ramx_plane *pl = (ramx_plane *)malloc(sizeof(ramx_plane) * P2);
  int32_t *co = (int32_t *)malloc(sizeof(int32_t) * (size_t)P2 * P2);
  for (int i = 0; i < P2; i++) { pl[i].row = i / 2; pl[i].cls = i % 2 ? RAMX_PLANE_COVER : (i / 2 + 1) % 4; }
  for (int i = 0; i < P2; i++)
    for (int j = 0; j < P2; j++) co[(size_t)i * P2 + j] = (i % 2 && j % 2) ? 300 : (i % 2 || j % 2) ? 30 : ((i / 2 + j / 2) % 5 ? 3 : 30);
  const int32_t tested = ramx_link_pairs(pl, P2, co, 0.0, NULL, 0);          /* cap = 0, out = NULL: only counted */
  assert(tested == 1024 * 1023 / 2);
  ramx_link one[1];
  const int32_t linked = ramx_link_pairs(pl, P2, co, 3.0, one, 0);           /* cap = 0 with a buffer: nothing is written */
  assert(linked > 0 && linked < tested);
  ramx_link *ln = (ramx_link *)malloc(sizeof(ramx_link) * (size_t)linked);
  assert(ramx_link_pairs(pl, P2, co, 3.0, ln, linked) == linked);
  for (int i = 0; i < linked; i++) assert(ln[i].n == 300 && ln[i].n_pq == 30 && ln[i].mlog10p >= 3.0 && ln[i].p < ln[i].q);
  assert(ramx_link_pairs(pl, 0, co, 0.0, ln, linked) == 0 && ramx_link_pairs(NULL, 5, co, 0.0, ln, linked) == 0);
  /* the components of those links: 1024 variants, init sized for exactly V * K' bytes */
  {
    int32_t *comp = (int32_t *)malloc(sizeof(int32_t) * 1024);
    for (int K = 1; K <= RAMX_SUBFAM_MAX; K += 7)
    {
      const int32_t Kp = ramx_link_components(pl, P2, ln, linked, K, NULL, comp);
      assert(Kp >= 1 && Kp <= K);
      uint8_t *init = (uint8_t *)malloc((size_t)1024 * (size_t)Kp);
      assert(ramx_link_components(pl, P2, ln, linked, K, init, comp) == Kp);
      for (int v = 0; v < 1024; v++)
      {
        assert(comp[v] >= 0 && comp[v] < Kp && init[(size_t)v * Kp] == 0);
        for (int k = 1; k < Kp; k++) assert(init[(size_t)v * Kp + k] == (comp[v] == k));
      }
      free(init);
    }
    uint8_t b1[1];
    assert(ramx_link_components(pl, P2, NULL, 0, 4, NULL, comp) == 1 && comp[1023] == 0);
    assert(ramx_link_components(NULL, 0, NULL, 0, 4, b1, NULL) == 1);
    assert(ramx_link_components(pl, P2, ln, linked, 0, NULL, NULL) == 0 && ramx_link_components(pl, P2, ln, linked, 9, NULL, NULL) == 0);
    ramx_link bad = ln[0];
    bad.q = 1;                                                               /* a cover plane is no variant */
    assert(ramx_link_components(pl, P2, &bad, 1, 4, NULL, comp) == 0);
    bad.q = P2;
    assert(ramx_link_components(pl, P2, &bad, 1, 4, NULL, comp) == 0);
    free(comp);
  }
  /* a list without cover planes tests nothing; empty tables score 0 */
  for (int i = 0; i < 8; i++) { pl[i].row = i; pl[i].cls = 5; }
  assert(ramx_link_pairs(pl, 8, co, 0.0, ln, linked) == 0);
  assert(upper_tail_mlog10(0, 0, 0, 0) == 0.0 && upper_tail_mlog10(10, 3, 3, 0) == 0.0 && upper_tail_mlog10(10, 10, 4, 4) == 0.0);

  free(ln); free(co); free(pl); free(out); free(cols); free(cons);
  printf("linkage_main: ok (%d planes selected at the cap, %d of %d pairs linked)\n", (int)P, (int)linked, (int)tested);
  return 0;
}
