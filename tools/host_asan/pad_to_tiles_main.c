/* Host-side memory safety of pad_to_tiles and of the one-family view the sinks are fed from (both static in ramx_extend.c) under
 * ASan + UBSan: every length around the tile edges, the source arrays exactly as long as what they hold; the padded tail, the
 * zero tail of the consensus block and the clamped ret.  Built and run by tools/host_asan/run.sh. */
#include "../../repeatafterme_amd/csrc/ramx_extend.c"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); return 1; } } while (0)

int main(void)
{
  static const int sizes[] = { 0, 1, 63, 64, 65, 70, 128, 129 };
  ramx_flank zero;
  memset(&zero, 0, sizeof(zero));
  zero.t_lo = 1; zero.step = 1;
  for (size_t k = 0; k < sizeof(sizes) / sizeof(sizes[0]); k++)
  {
    const int nx = sizes[k];
    ramx_flank *fl = nx ? (ramx_flank *)malloc(sizeof(ramx_flank) * (size_t)nx) : NULL;
    for (int i = 0; i < nx; i++) { memset(&fl[i], 0, sizeof(ramx_flank)); fl[i].start = 1000 + i; fl[i].t_lo = -i; fl[i].t_hi = i; fl[i].step = (i & 1) ? 1 : -1; }
    int npad = -1;
    ramx_flank *pf = pad_to_tiles(fl, nx, &npad);
    CHECK(pf != NULL && npad == (nx + 63) / 64 * 64);
    CHECK(nx == 0 || memcmp(pf, fl, sizeof(ramx_flank) * (size_t)nx) == 0);
    for (int i = nx; i < npad; i++) CHECK(memcmp(&pf[i], &zero, sizeof(zero)) == 0);
    free(pf); free(fl);
  }
  printf("pad_to_tiles: ok\n");

  /* the view of one family that the sinks are fed from: built and freed, never handed to a device call */
  enum { L = 30 };
  static const int nxs[] = { 0, 1, 64, 70 }, rowss[] = { 0, 1, L }, rets[] = { -1, 0, 1 };
  ramx_params p;
  memset(&p, 0, sizeof(p));
  p.L = L;
  for (size_t k = 0; k < sizeof(nxs) / sizeof(nxs[0]); k++)
    for (size_t j = 0; j < sizeof(rowss) / sizeof(rowss[0]); j++)
      for (size_t q = 0; q < sizeof(rets) / sizeof(rets[0]); q++)
      {
        const int nx = nxs[k], rows = rowss[j], ret = rets[q] > rows ? rows : rets[q];
        /* the callers' arrays are exactly as long as what they hold: nx flanks, rows bases */
        ramx_flank *fl = nx ? (ramx_flank *)malloc(sizeof(ramx_flank) * (size_t)nx) : NULL;
        int32_t *map = nx ? (int32_t *)malloc(sizeof(int32_t) * (size_t)nx) : NULL;
        int8_t *cons = rows ? (int8_t *)malloc((size_t)rows) : NULL;
        for (int i = 0; i < nx; i++) { memset(&fl[i], 0, sizeof(ramx_flank)); fl[i].start = 1000 + i; fl[i].t_hi = i; fl[i].step = 1; map[i] = 2 * i; }
        for (int r = 0; r < rows; r++) cons[r] = (int8_t)(1 + r % 3);
        struct sink_view v;
        one_family_view(&v, NULL, 1, &p, 7, fl, map, nx, cons, rows, ret);
        CHECK(v.nb == 1 && v.direction == 1 && v.p == &p && v.lib_at == NULL && v.map == map);
        CHECK(v.fidx[0] == 7 && v.first[0] == 0 && v.count[0] == nx && v.npad == (nx + 63) / 64 * 64);
        CHECK(v.rows_executed[0] == rows && v.ret[0] == (ret > 0 ? ret : 0));
        CHECK(nx == 0 || memcmp(v.fl, fl, sizeof(ramx_flank) * (size_t)nx) == 0);
        for (int i = nx; i < v.npad; i++) CHECK(memcmp(&v.fl[i], &zero, sizeof(zero)) == 0);
        CHECK(rows == 0 || memcmp(v.cons, cons, (size_t)rows) == 0);
        for (int r = rows; r < L; r++) CHECK(v.cons[r] == 0);
        ramx_flank *own = own_flanks(&v, 0);
        CHECK(own != NULL && (nx == 0 || memcmp(own, fl, sizeof(ramx_flank) * (size_t)nx) == 0));
        free(own);
        free_one_family_view(&v);
        free(fl); free(map); free(cons);
      }
  printf("one_family_view: ok\n");
  return 0;
}
