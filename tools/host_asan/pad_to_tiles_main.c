/* Host-side memory safety of pad_to_tiles (static in ramx_extend.c) under ASan + UBSan: every length around the tile edges, the
 * source array exactly nx flanks long.  Built and run by tools/host_asan/run.sh. */
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
  return 0;
}
