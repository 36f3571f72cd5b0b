/* ramx_recall_cpg of ramx_recall.c under AddressSanitizer + UBSan on random records: rows and L from 0, counts up to 2 * 10^9 in
 * every seventh trial (the sums are int64), both reading orders, n_cpg given and NULL.  The length must be the plain re-call's
 * and never exceed L.  ramx_recall.c is compiled into the program.  Built and run by tools/host_asan/run.sh. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ramx.h"

int main(void)
{
  srand(7);
  int32_t *m = (int32_t *)calloc(100 * 100, sizeof(int32_t));
  for (int i = 0; i < 100 * 100; i++) m[i] = rand() % 40 - 20;
  long total = 0;
  for (int t = 0; t < 20000; t++)
  {
    const int rows = rand() % 30, L = rand() % 40;
    int8_t *cons = (int8_t *)malloc(rows ? rows : 1), *out = (int8_t *)malloc(L ? L : 1), *plain = (int8_t *)malloc(L ? L : 1);
    ramx_col_pileup *c = (ramx_col_pileup *)calloc(rows ? rows : 1, sizeof(*c));
    ramx_col_dinuc *d = (ramx_col_dinuc *)calloc(rows ? rows : 1, sizeof(*d));
    for (int r = 0; r < rows; r++)
    {
      cons[r] = (int8_t)(rand() & 3);
      c[r].cover = rand() % 12;
      c[r].del = rand() % (c[r].cover + 1);
      for (int b = 0; b < 5; b++)
      {
        c[r].match[b] = rand() % 6;
        for (int k = 0; k < RAMX_PILEUP_INS; k++) c[r].ins[k][b] = rand() % 4;
      }
      for (int x = 0; x < 5; x++)
        for (int y = 0; y < 5; y++) d[r].di[x][y] = rand() % (t % 7 ? 9 : 2000000000);
    }
    int32_t ncpg = 0;
    const int32_t n = ramx_recall_cpg(cons, rows, c, d, t & 1, m, rand() % 30 - 15, L, out, t % 3 ? &ncpg : NULL);
    const int32_t n2 = ramx_recall_consensus(cons, rows, c, L, plain);
    if (n != n2 || n > L || ncpg < 0 || 2 * ncpg > n) { printf("recall_cpg: trial %d: length %d against %d, L %d, n_cpg %d\n", t, n, n2, L, ncpg); return 1; }
    total += n + ncpg;
    free(cons); free(out); free(plain); free(c); free(d);
  }
  free(m);
  printf("recall_cpg: 20000 random records, lengths equal the plain re-call's (checksum %ld)\n", total);
  return 0;
}
