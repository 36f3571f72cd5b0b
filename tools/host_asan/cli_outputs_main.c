/* The formatting layer of the command line (csrc/ramx_cli_outputs.c, compiled into this program; the rest comes from libramx.so)
 * without a device: hand-made records go to the seven sinks for two families and both directions, then the writers and the two
 * post-passes run, and a handful of lines of every file are compared with literals.  The library is 300 bases ACGTACGT... in three
 * records (the second with a genomic offset), the cores are a "+" one, a "-" one that is not extendable to the left, and a "+"
 * one; the right direction has three columns and two flanks, the left one n_flanks = 0 (alignment, copies, subfamilies) or
 * rows = 0 (the others); the second family names no file at all.  CPU only; leaks count. */
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "ramx_cli_outputs.c"

static char g_dir[64];
static const char *path_of(const char *name)
{
  char *p = (char *)malloc(strlen(g_dir) + strlen(name) + 2);
  sprintf(p, "%s/%s", g_dir, name);
  return p;
}

/* line `at` (0-based) of the file begins with `want`; at < 0 counts from the end */
static void expect_line(const char *path, int at, const char *want)
{
  FILE *fp = fopen(path, "r");
  assert(fp);
  char *lines[256], buf[4096];
  int n = 0;
  while (fgets(buf, sizeof(buf), fp) && n < 256) { buf[strcspn(buf, "\n")] = 0; lines[n++] = strdup(buf); }
  fclose(fp);
  const int k = at < 0 ? n + at : at;
  if (k < 0 || k >= n || strncmp(lines[k], want, strlen(want)) != 0)
  {
    fprintf(stderr, "%s line %d: got \"%s\", want \"%s\"\n", path, at, k >= 0 && k < n ? lines[k] : "(none)", want);
    exit(1);
  }
  for (int i = 0; i < n; i++) free(lines[i]);
}

static int give_tsd(void *ctx, const ramx_tsd_params *tp, ramx_tsd *rec)
{
  /* two families of three cores each */
  const ramx_tsd three[3] = { { 4, 0, 0, 0 }, { 0, 0, 0, 0 }, { 5, 1, -1, 1 } };
  memcpy(rec, three, sizeof(three)); memcpy(rec + 3, three, sizeof(three));
  return 0;
}
static int give_period(void *ctx, int part, const ramx_period_params *pp, ramx_period *rec, ramx_period_seg *segs)
{
  for (int i = 0; i < 6; i++) { segs[i].lo = 35; segs[i].hi = part == 0 ? 39 : 56; }
  if (part == 1) { rec[0] = rec[3] = (ramx_period){ 2, 20, 1, 8, 10, 0, { 0, 0 } }; segs[0].lo = segs[3].lo = 50; }
  return 0;
}
static int give_term(void *ctx, const ramx_term_params *tp, ramx_term *rec)
{
  /* the first core of either family carries a direct repeat of six bases at both termini */
  memset(rec, 0, 12 * sizeof(ramx_term));
  for (int i = 0; i < 12; i++) rec[i].T = 11;
  rec[0] = rec[6] = (ramx_term){ 12, 0, 5, 5, 10, 6, 6, 11 };
  return 0;
}
static const struct outputs_post_fns k_give = { give_tsd, give_period, give_term };

int main(void)
{
  strcpy(g_dir, "/tmp/ramx_cli_outputs_XXXXXX");
  assert(mkdtemp(g_dir));

  enum { LEN = 300, L = 10 };
  char seq[LEN];
  for (int i = 0; i < LEN; i++) seq[i] = (char)(i % 4);
  char *ids[3] = { "s0", "s1", "s2" };
  uint64_t bounds[3] = { 100, 200, 300 }, offs[3] = { 0, 1000, 0 };
  struct sequenceLibrary lib;
  memset(&lib, 0, sizeof(lib));
  lib.sequence = seq; lib.identifiers = ids; lib.boundaries = bounds; lib.offsets = offs; lib.length = LEN; lib.count = 3;
  struct coreAlignment c[3];
  memset(c, 0, sizeof(c));
  c[0].next = &c[1]; c[1].next = &c[2];
  c[0].seqIdx = 0; c[0].leftSeqPos = 40; c[0].rightSeqPos = 49; c[0].leftExtendable = c[0].rightExtendable = 1;
  c[0].upperSeqBound = 99; c[0].leftExtensionLen = 5; c[0].rightExtensionLen = 7; c[0].score = 30;
  c[1].seqIdx = 1; c[1].orient = 1; c[1].leftSeqPos = 159; c[1].rightSeqPos = 150; c[1].rightExtendable = 1;
  c[1].lowerSeqBound = 100; c[1].upperSeqBound = 199; c[1].rightExtensionLen = 4; c[1].score = 12;
  c[2].seqIdx = 2; c[2].leftSeqPos = 240; c[2].rightSeqPos = 249; c[2].leftExtendable = c[2].rightExtendable = 1;
  c[2].lowerSeqBound = 200; c[2].upperSeqBound = 299; c[2].leftExtensionLen = 3;
  char master[2 * L + 2];
  memset(master, 0, sizeof(master));
  master[L - 2] = 3; master[L - 1] = 0; master[L] = RAMX_SYM_N; master[L + 1] = 0; master[L + 2] = 1; master[L + 3] = 2;

  struct cli_opts o;
  memset(&o, 0, sizeof(o));
  o.flanking = 2; o.L = L; o.minimprovement = 27; o.refine = DEF_REFINE; o.linkcount = DEF_LINKCOUNT; o.linkfrac = DEF_LINKFRAC;
  o.linkscore = DEF_LINKSCORE; o.subfamk = 2; o.subfammin = 1; o.subfamiter = DEF_SUBFAMITER; o.periodwhole = 1;
  o.tsd = (ramx_tsd_params){ 3, 4, 20, 10 };
  o.period = (ramx_period_params){ 1024, 3, 16, 0 };
  o.term = (ramx_term_params){ 512, 2, 3, 5, 40, 3, { 0, 0 } };
  o.distmin = 2; o.distmax = DEF_DISTMAX;

  struct family_outputs fams[2];
  memset(fams, 0, sizeof(fams));
  for (int r = 0; r < N_OUTPUTS; r++) fams[0].paths[r] = path_of(k_outputs[r].flag + 1);
  fams[0].lib = fams[1].lib = &lib;
  outputs_begin(&o, fams, 2);

  /* the records of the right direction: three columns A C G, the flanks of cores 0 and 1 */
  const int8_t cons3[3] = { 0, 1, 2 }, refined3[3] = { 0, 1, 1 }, cons_left[2] = { 3, 0 };
  const int32_t core_index[2] = { 0, 1 };
  const ramx_flank flanks[2] = { { 50, 0, 40, 1, 0, { 0 } }, { 149, 0, 40, -1, 1, { 0 } } };
  const ramx_aln_end ends[2] = { { 2, 2, 30, 0, 0 }, { 1, 1, 12, 0, 0 } };
  const int32_t col_idx[6] = { 0, 0, 1, RAMX_ALN_DELETED, 2, RAMX_ALN_NONE }, col_ins[6] = { 0, 0, 0, 1, 0, 0 };
  ramx_col_profile prof[3];
  memset(prof, 0, sizeof(prof));
  prof[0].total[0] = 100; prof[0].total[1] = 2; prof[0].total[2] = 3; prof[0].total[3] = 1; prof[0].n_capped = 1; prof[0].n_new_high = 2;
  prof[1].base = 1; prof[1].total[1] = 50; prof[2].base = 2; prof[2].total[2] = 60;
  ramx_col_pileup pile[3];
  memset(pile, 0, sizeof(pile));
  for (int r = 0; r < 3; r++) { pile[r].base = cons3[r]; pile[r].cover = 2; pile[r].match[cons3[r]] = 2; }
  ramx_col_dinuc di[3];
  memset(di, 0, sizeof(di));
  for (int r = 0; r < 3; r++) { di[r].base = cons3[r]; di[r].next = r < 2 ? cons3[r + 1] : -1; di[r].both = di[r].adjacent = r < 2 ? 2 : 0; }
  di[0].di[0][1] = 2;
  ramx_copy_stats st[2];
  memset(st, 0, sizeof(st));
  st[0].cols = 3; st[0].match = 3; st[0].score = 30; st[1].cols = 2; st[1].match = 1; st[1].del = 1; st[1].del_open = 1; st[1].ins = 1; st[1].ins_open = 1; st[1].score = 12;
  const ramx_plane planes[4] = { { 0, 1 }, { 0, RAMX_PLANE_COVER }, { 2, 5 }, { 2, RAMX_PLANE_COVER } };
  const int32_t co[16] = { 20, 20, 20, 20,  20, 40, 20, 40,  20, 20, 20, 20,  20, 40, 20, 40 };
  const int32_t labels[2] = { 0, 1 }, size2[2] = { 1, 1 }, dist[4] = { 0, 2, 2, 0 }, size1[1] = { 0 };
  const uint8_t patterns[4] = { 0, 1, 0, 1 };
  const ramx_subfam_group group1 = { 1, 1, 3, 1, 1, cons3, pile }, group_empty = { 0, 0, 0, 1, 1, NULL, NULL };

  /* both flanks selected to the right, one pair: three columns covered by both, two sites, one of them a transition, one
   * column deleted in one of them; to the left the same two cores in the other order, one site */
  const int32_t sel2[2] = { 0, 1 }, core_left[2] = { 1, 0 };
  const ramx_copy_dist pair_r = { 3, 2, 1, 0, 1, 0 }, self_r = { 3, 3, 0, 0, 0, 0 }, pair_l = { 2, 1, 0, 0, 0, 0 }, self_l = { 2, 2, 0, 0, 0, 0 };
  const ramx_copy_dist dist_r[4] = { self_r, pair_r, pair_r, self_r }, dist_l[4] = { self_l, pair_l, pair_l, self_l };

  for (int f = 0; f < 2; f++)
    for (int d = 1; d >= 0; d--)
    {
      const ramx_dist ds = { d, f, d ? 3 : 2, 2, 2, d ? cons3 : cons_left, d ? core_index : core_left, ends, sel2, d ? dist_r : dist_l };
      dist_sink(&ds, fams);
      const ramx_profile pr = { d, f, d ? 3 : 0, d ? 2 : 0, d ? 2 : 0, prof, core_index, NULL };
      profile_sink(&pr, fams);
      const ramx_alignment al = { d, f, d ? 3 : 2, d ? 2 : 0, 2, d ? cons3 : cons_left, flanks, core_index, ends, d ? col_idx : NULL, d ? col_ins : NULL };
      aln_sink(&al, fams);
      const ramx_refinement rf = { d, f, d ? 3 : 0, d ? 3 : 0, d ? 2 : 1, 1, d ? 2 : 0, 0, cons3, pile, refined3, pile };
      refine_sink(&rf, fams);
      const ramx_copies cp = { d, f, d ? 3 : 2, d ? 2 : 0, d ? cons3 : cons_left, flanks, core_index, ends, st };
      copies_sink(&cp, fams);
      const ramx_cpg_refinement cr = { d, f, d ? 3 : 0, d ? 3 : 0, d ? 2 : 1, 1, d ? 2 : 0, d ? 1 : 0, cons3, cons3, pile, di };
      cpg_sink(&cr, fams);
      const ramx_linkage lk = { d, f, d ? 3 : 0, d ? 4 : 0, cons3, pile, planes, co };
      linkage_sink(&lk, fams);
      const ramx_subfamilies sf = { d, f, d ? 3 : 2, d ? 2 : 0, d ? 4 : 0, d ? 2 : 0, d ? 2 : 1, d ? 2 : 1, 1, 1, d ? cons3 : cons_left, flanks, core_index,
                                    planes, labels, patterns, NULL, d ? size2 : size1, dist, d ? &group1 : &group_empty };
      subfam_sink(&sf, fams);
    }
  for (int f = 0; f < 2; f++) outputs_family_done(&fams[f], c, master, 3, 2);
  outputs_post(&o, fams, 2, &k_give, NULL);
  assert(fams[0].n_cores == 3 && fams[1].n_cores == 3);
  outputs_end(fams, 2);

  const char *const *p = fams[0].paths;
  expect_line(p[OUT_PROFILE], 0, "dir\trow\tbase\ttotal_A");
  expect_line(p[OUT_PROFILE], 1, "right\t0\tA\t100\t2\t3\t1\t100\t97\t2\t1\t2\t0\t1\t1");
  expect_line(p[OUT_PROFILE], -1, "right\t2\tG\t0\t0\t60\t0\t60\t60\t2\t2\t0\t0\t0\t0");
  expect_line(p[OUT_ALN], 0, ">right-extension 3 bp");
  expect_line(p[OUT_ALN], 2, ">s0:34-59_+  dir=right,end_row=2,start=0,end=2,score=30");
  expect_line(p[OUT_ALN], 3, "GTA");
  expect_line(p[OUT_ALN], 4, ">s1:1045-1062_-  dir=right,end_row=1,start=0,end=1,score=12");
  expect_line(p[OUT_ALN], 5, "Gt--");
  expect_line(p[OUT_ALN], 6, ">left-extension 2 bp");
  expect_line(p[OUT_ALN], -1, "AT");
  expect_line(p[OUT_PILEUP], 1, "right\t0\tA\t2\t2\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0");
  expect_line(p[OUT_PILEUP], 4, "right-refined\t0\tA\t2");
  expect_line(p[OUT_PILEUP], -1, "right-refined\t2\tG\t2");
  expect_line(p[OUT_REFINED], 0, ">right-extension-refined 3 bp replays=2 converged=1");
  expect_line(p[OUT_REFINED], 1, "ACC");
  expect_line(p[OUT_REFINED], 2, ">left-extension-refined 0 bp replays=1 converged=1");
  expect_line(p[OUT_COPIES], 1, "right\ts0:34-59_+\t2\t0\t2\t30\t3\t3\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0.0000");
  expect_line(p[OUT_COPIES], 2, "right\ts1:1045-1062_-\t1\t0\t1\t12\t2\t1\t0\t0\t0\t1\t1\t1\t1\t0\t0\t");
  expect_line(p[OUT_COPIES], 3, "#right\tcopies=2\tused=");
  expect_line(p[OUT_COPIES], -1, "#left\tcopies=0\tused=0\tkimura=");
  expect_line(p[OUT_CPG], 0, ">right-extension-cpg 3 bp replays=2 converged=1 cpg=1");
  expect_line(p[OUT_CPG], 1, "ACG");
  expect_line(p[OUT_CPG], 2, ">left-extension-cpg 0 bp replays=1 converged=1 cpg=0");
  expect_line(p[OUT_DINUC], 0, "dir\trow\tbase\tnext\tboth\tadjacent\tsplit\tgapped\tAA\tAC\tAG");
  expect_line(p[OUT_DINUC], 1, "right\t0\tA\tC\t2\t2\t0\t0\t0\t2\t0");
  expect_line(p[OUT_DINUC], -1, "right\t2\tG\t-\t0\t0\t0\t0\t0");
  expect_line(p[OUT_LINKAGE], 1, "right\t0\tC\t20\t2\tdel\t20\t40\t20\t20\t20\t10.0000\t11.1394");
  expect_line(p[OUT_LINKAGE], 2, "#right\tvariants=2\tpairs=1\tlinked=1");
  expect_line(p[OUT_LINKAGE], -1, "#left\tvariants=0\tpairs=0\tlinked=0");
  expect_line(p[OUT_SUBFAM], 2, "group\tright\t0\t1\t2\t1\t-\tNA\tNA\tNA\t-");
  expect_line(p[OUT_SUBFAM], 3, "copy\tright\ts0:34-59_+\t0\t0\t2");
  expect_line(p[OUT_SUBFAM], 4, "group\tright\t1\t1\t2\t1\t0:C,2:del\t3\t1\t1\tACG");
  expect_line(p[OUT_SUBFAM], 5, "copy\tright\ts1:1045-1062_-\t1\t2\t0");
  expect_line(p[OUT_SUBFAM], -1, "group\tleft\t0\t0\t1\t1\t-\t0\t1\t1\t-");
  expect_line(p[OUT_TSD], 0, "#tsd\tslack=3\tkmin=4\tkmax=20\tmm_div=10");
  expect_line(p[OUT_TSD], 1, "#rows\tleft_rows=2\tright_rows=3");
  expect_line(p[OUT_TSD], 6, "0\ts0\t36\t57\t+\t5\t7\t4\t0\t0\t0\tTACG\tCGTA");
  expect_line(p[OUT_TSD], 7, "1\ts1\t1047\t1060\t-\t*\t4\t0\t0\t0\t0\t-\t-");
  expect_line(p[OUT_TSD], 8, "2\ts2\t38\t50\t+\t3\t0\t5\t1\t-1\t1\tTACGT\tTACGT");
  expect_line(p[OUT_PERIOD], 0, "#period\tpmax=1024\tmm=3\tmin_score=16");
  expect_line(p[OUT_PERIOD], 8, "0\ts0\t36\t57\t+\tleft\t5\t0\t0.00\t0\t0\t0\t0\t0\t-");
  expect_line(p[OUT_PERIOD], 9, "0\ts0\t36\t57\t+\tright\t7\t2\t5.00\t20\t52\t61\t10\t0\tTA");
  expect_line(p[OUT_PERIOD], -1, "2\ts2\t38\t50\t+\twhole\t22\t0\t0.00");
  expect_line(p[OUT_DIST], 0, "dir\tcopy_a\tcopy_b\tcover\tsites\tts\ttv\tdel_one\tdel_both\tkimura");
  expect_line(p[OUT_DIST], 1, "right\ts0:34-59_+\ts1:1045-1062_-\t3\t2\t1\t0\t1\t0\tNA");
  expect_line(p[OUT_DIST], 2, "#right\tcopies=2\tselected=2\tpairs=1\tused=0\tkimura=0.0000\tmedoid=NA\tmedoid_kimura=NA");
  expect_line(p[OUT_DIST], 3, "left\ts1:1045-1062_-\ts0:34-59_+\t2\t1\t0\t0\t0\t0\t0.0000");
  expect_line(p[OUT_DIST], 4, "#left\tcopies=2\tselected=2\tpairs=1\tused=0\t");
  expect_line(p[OUT_DIST], 5, "both\ts0:34-59_+\ts1:1045-1062_-\t5\t3\t1\t0\t1\t0\t");
  expect_line(p[OUT_DIST], -1, "#both\tcopies=2\tselected=2\tpairs=1\tused=1\tkimura=");

  /* the family without a path wrote nothing and kept nothing */
  int files = 0;
  for (int r = 0; r < N_OUTPUTS; r++) { files += access(p[r], F_OK) == 0; unlink(p[r]); free((char *)p[r]); }
  assert(files == N_OUTPUTS && rmdir(g_dir) == 0);
  printf("cli_outputs_main: ok (%d files of one family, none of the other)\n", files);
  return 0;
}
