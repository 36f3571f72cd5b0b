/*
 * ramx_cli_outputs.c -- the analysis outputs of the RAMExtend command line (no counterpart in the reference): one table row per
 * output file (k_outputs, at the end), one sink and one writer per kind of record, one view of a core for all of them, and the
 * four calls the two drivers of ramx_cli.c make: outputs_begin, outputs_family_done, outputs_post, outputs_end.
 */
#include <ctype.h>
#include <stdlib.h>
#include <string.h>

#include "ramx_cli_outputs.h"

FILE *open_or_die(const char *path, const char *mode, const char *word)
{
  FILE *fp = fopen(path, mode);
  if (!fp) { fprintf(stderr, mode[0] == 'a' ? "Could not append to the %s file %s\n" : "Could not create the %s file %s\n", word, path); exit(1); }
  return fp;
}

/* a family's file of table row r, NULL if it is not wanted */
static FILE *row_open(const struct family_outputs *fo, int r, const char *mode)
{
  return fo->paths[r] ? open_or_die(fo->paths[r], mode, k_outputs[r].word) : NULL;
}

/* ------------------------------------------------------------------ a core as every output places it */
static void core_view_of(struct core_view *v, const struct coreAlignment *s, const struct sequenceLibrary *lib)
{
  const int si = s->seqIdx;
  v->s = s;
  v->ident = lib->identifiers[si];
  v->lo = si > 0 ? lib->boundaries[si - 1] : 0;
  v->hi = lib->boundaries[si];
  v->off = (lib->offsets != NULL && lib->offsets[si] > 0) ? lib->offsets[si] : 0;
  v->orient = s->orient ? '-' : '+';
  v->e_lo = s->orient ? (int64_t)s->rightSeqPos - s->rightExtensionLen : (int64_t)s->leftSeqPos - s->leftExtensionLen;
  v->e_hi = s->orient ? (int64_t)s->leftSeqPos + s->leftExtensionLen : (int64_t)s->rightSeqPos + s->rightExtensionLen;
  if (s->leftExtendable) snprintf(v->left, sizeof(v->left), "%d", s->leftExtensionLen); else strcpy(v->left, "*");
  if (s->rightExtendable) snprintf(v->right, sizeof(v->right), "%d", s->rightExtensionLen); else strcpy(v->right, "*");
}

/* the one list-to-array loop */
static struct core_view *core_views(const struct coreAlignment *cores, const struct sequenceLibrary *lib, int *n)
{
  int cnt = 0;
  for (const struct coreAlignment *s = cores; s != NULL; s = s->next) cnt++;
  struct core_view *v = (struct core_view *)malloc(sizeof(*v) * (size_t)(cnt ? cnt : 1));
  cnt = 0;
  for (const struct coreAlignment *s = cores; s != NULL; s = s->next) core_view_of(&v[cnt++], s, lib);
  *n = cnt;
  return v;
}

void core_fa_range(const struct core_view *v, int flanking, uint64_t *from, uint64_t *to)
{
  *from = (uint64_t)v->e_lo; *to = (uint64_t)v->e_hi;
  if (flanking > 0)
  {
    if (v->lo == 0 && (uint64_t)flanking > *from) *from = 1;   /* sic: ram_extend.c:729-730 */
    else *from -= (uint64_t)flanking;
    if (*to + (uint64_t)flanking > v->hi) *to = v->hi;
    else *to += (uint64_t)flanking;
  }
}

void core_fa_id(char *buf, size_t n, const struct core_view *v, int flanking)
{
  uint64_t from, to;
  core_fa_range(v, flanking, &from, &to);
  snprintf(buf, n, "%s:%ld-%ld_%c", v->ident, (long)(v->off + from - v->lo + 1), (long)(v->off + to - v->lo + 1), v->orient);
}

void outputs_family_cores(struct family_outputs *fo, const struct coreAlignment *cores)
{
  if (!fo->cores) fo->cores = core_views(cores, fo->lib, &fo->n_cores);
}

/* the -outfa id of the core a sink's record names */
static const char *record_id(char *buf, size_t n, const struct family_outputs *fo, int core, const char *what)
{
  if (core < 0 || core >= fo->n_cores) { fprintf(stderr, "RAMExtend(ramx): %s record of an unknown core %d\n", what, core); exit(1); }
  core_fa_id(buf, n, &fo->cores[core], fo->o->flanking);
  return buf;
}

static const char *const k_dir[3] = { "left", "right", "whole" };          /* a direction, or a part of -outperiod */
static const char *const k_var_name[8] = { "A", "C", "G", "T", "N", "del", "cover", "ins" };

/* a direction's consensus as text in reading order: the left rows run outward from the core (room for one more character) */
static char *reading_order(const int8_t *cons, int n, int d)
{
  char *seq = (char *)malloc((size_t)n + 2);
  for (int r = 0; r < n; r++) seq[r] = code_to_char(cons[d ? r : n - 1 - r]);
  seq[n] = 0;
  return seq;
}

/* a refined consensus of both directions, kept until the FASTA is written: -outrefined and -outcpg */
static void keep_fasta(struct kept_fasta *k, int d, const int8_t *cons, int n, int replays, int converged, int n_cpg)
{
  k->have[d] = 1; k->rows[d] = n; k->replays[d] = replays; k->converged[d] = converged; k->n_cpg[d] = n_cpg;
  k->seq[d] = reading_order(cons, n, d);
}
static void kept_fasta_write(FILE *fp, struct kept_fasta *k, const char *kind, int with_cpg)
{
  for (int d = 1; d >= 0; d--)
  {
    if (!k->have[d]) continue;
    fprintf(fp, ">%s-extension-%s %d bp replays=%d converged=%d", k_dir[d], kind, k->rows[d], k->replays[d], k->converged[d]);
    if (with_cpg) fprintf(fp, " cpg=%d", k->n_cpg[d]);
    fprintf(fp, "\n%s\n", k->seq[d]);
    free(k->seq[d]);
    k->seq[d] = NULL; k->have[d] = 0;
  }
}

/*
 * -outprofile <file>: the per-column support profile of both extensions (include/ramx.h, ramx_set_profile_sink) as a TSV, the
 * right direction's rows first.  score is the reference's curr_extension_score (ram_extend.c:1064-1086), new_max its
 * MINIMPROVEMENT rule (:1194-1201), kept says whether the column is part of the returned extension.
 */
static void profile_start(FILE *fp)
{
  fputs("dir\trow\tbase\ttotal_A\ttotal_C\ttotal_G\ttotal_T\tscore\tmargin\tn_flanks\tn_uncapped\tn_new_high\tn_out_of_seq\tnew_max\tkept\n", fp);
}
static void profile_sink(const ramx_profile *pr, void *user)
{
  const struct family_outputs *fo = &((const struct family_outputs *)user)[pr->family];
  FILE *fp = row_open(fo, OUT_PROFILE, "a");
  if (!fp) return;
  long long max_ext = 0;
  int max_row = -1;
  for (int r = 0; r < pr->n_cols; r++)
  {
    const ramx_col_profile *c = &pr->cols[r];
    long long score = 0, other = 0;
    int have_other = 0;
    for (int a = 0; a < 4; a++)
    {
      if (c->total[a] > score) score = c->total[a];
      if (a != c->base && (!have_other || c->total[a] > other)) { other = c->total[a]; have_other = 1; }
    }
    const int new_max = score >= max_ext + (long long)abs(max_row - r) * fo->o->minimprovement;
    if (new_max) { max_row = r; max_ext = score; }
    fprintf(fp, "%s\t%d\t%c\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%d\t%d\t%d\t%d\t%d\t%d\n", pr->direction ? "right" : "left", r,
            code_to_char(c->base), (long long)c->total[0], (long long)c->total[1], (long long)c->total[2], (long long)c->total[3],
            score, (long long)c->total[c->base] - other, pr->n_flanks, pr->n_flanks - c->n_capped, c->n_new_high, c->n_out_of_seq,
            new_max, r < pr->ret ? 1 : 0);
  }
  fclose(fp);
}

/*
 * -outaln <file>: every extendable core's alignment to the kept consensus of both extensions (include/ramx.h,
 * ramx_set_align_sink) as A2M text, the right block first.  A block: ">right-extension <ret> bp" and the kept consensus, then
 * one record per extendable core in flank order, named as -outfa names the core (up to the two spaces) followed by
 * "  dir=,end_row=,start=,end=,score=".  A body holds exactly ret column characters -- an upper-case base, or '-' for a deleted
 * column and for the columns above end_row -- and lower-case inserted bases where they fall; nothing is wrapped.  The left block
 * reads as the sequence does: rows reversed, and every insertion run with them.  The names need both directions' lengths, so
 * the sink keeps the bodies and the file is written with the other results.
 */
static void reverse_chars(char *s, size_t n)
{
  for (size_t i = 0; i + 1 < n - i; i++) { const char t = s[i]; s[i] = s[n - 1 - i]; s[n - 1 - i] = t; }
}

/* what -outaln and -outcopies keep of every flank: its core and where its path ends */
static void keep_flanks(struct flank_block *b, int n_flanks, const int32_t *core_index, const ramx_aln_end *ends)
{
  b->have = 1; b->n = n_flanks;
  b->rec = (struct flank_rec *)calloc((size_t)(n_flanks > 0 ? n_flanks : 1), sizeof(struct flank_rec));
  for (int i = 0; i < n_flanks; i++)
  {
    const ramx_aln_end *e = &ends[i];
    struct flank_rec *rc = &b->rec[i];
    rc->core = core_index[i]; rc->end_row = e->end_row; rc->start = e->start_idx; rc->end = e->end_idx; rc->score = e->score;
  }
}

static void aln_sink(const ramx_alignment *al, void *user)
{
  struct family_outputs *fo = &((struct family_outputs *)user)[al->family];
  if (!fo->paths[OUT_ALN]) return;
  struct flank_block *b = &fo->aln[al->direction ? 1 : 0];
  const int rows = al->rows;
  keep_flanks(b, al->n_flanks, al->core_index, al->ends);
  b->ret = rows;
  b->cons = reading_order(al->cons, rows, al->direction ? 1 : 0);
  const uint64_t lib_len = fo->lib->length;
  for (int i = 0; i < al->n_flanks; i++)
  {
    const ramx_aln_end *e = &al->ends[i];
    const ramx_flank *f = &al->flanks[i];
    const long consumed = e->end_row >= 0 ? (long)e->end_idx - e->start_idx + 1 : 0;
    char *body = (char *)malloc((size_t)rows + (size_t)(consumed > 0 ? consumed : 0) + 1);
    size_t k = 0;
    long t = e->start_idx;
#define ALN_BASE(upper) do { \
      const int64_t at_ = f->start + (int64_t)f->step * t; \
      int code_ = (at_ >= 0 && (uint64_t)at_ < lib_len) ? ramx_lib_code(fo->lib, (uint64_t)at_) : RAMX_SYM_N; \
      if (f->compl_) code_ = code_compl(code_); \
      const char ch_ = code_to_char(code_); \
      body[k++] = (char)((upper) ? toupper((unsigned char)ch_) : tolower((unsigned char)ch_)); \
      t++; } while (0)
    for (int r = 0; r < rows; r++)
    {
      if (r > e->end_row) { body[k++] = '-'; continue; }
      const int idx = al->col_idx[(size_t)r * al->stride + i];
      for (int q = al->col_ins[(size_t)r * al->stride + i]; q > 0 && t <= e->end_idx; q--) ALN_BASE(0);
      if (idx == RAMX_ALN_DELETED || idx == RAMX_ALN_NONE) body[k++] = '-';
      else { t = idx; ALN_BASE(1); }
      if (r == e->end_row) for (int q = e->tail_ins; q > 0 && t <= e->end_idx; q--) ALN_BASE(0);
    }
#undef ALN_BASE
    body[k] = 0;
    if (!al->direction) reverse_chars(body, k);
    b->rec[i].body = body;
  }
}

/* after both directions: the file, then the buffers are released */
static void aln_write(FILE *fp, struct family_outputs *fo)
{
  for (int dir = 1; dir >= 0; dir--)
  {
    struct flank_block *b = &fo->aln[dir];
    if (!b->have) continue;
    fprintf(fp, ">%s-extension %d bp\n%s\n", k_dir[dir], b->ret, b->cons);
    for (int i = 0; i < b->n; i++)
    {
      const struct flank_rec *rc = &b->rec[i];
      char id[1024];
      fprintf(fp, ">%s  dir=%s,end_row=%d,start=%d,end=%d,score=%d\n%s\n", record_id(id, sizeof(id), fo, rc->core, "alignment"), k_dir[dir],
              rc->end_row, rc->start, rc->end, rc->score, rc->body);
      free(rc->body);
    }
    free(b->rec); free(b->cons);
    memset(b, 0, sizeof(*b));
  }
}

/*
 * -outpileup <file>: the pileup of both extensions' kept consensus (include/ramx.h, ramx_col_pileup, ramx_set_refine_sink) as a
 * TSV, one line per kept column, the right direction first.  -outrefined <file>: the kept consensus refined over at most
 * -refine <n> replays (default 10) as FASTA, ">right-extension-refined <n> bp replays=<k> converged=<0|1>" and the left one,
 * which reads as -cons writes it; nothing is wrapped.  With both files the pileup of a refined consensus that differs from the
 * kept one follows the kept one's block as right-refined / left-refined lines.
 */
static void pileup_start(FILE *fp)
{
  fputs("dir\trow\tbase\tcover\tA\tC\tG\tT\tN\tdel\tins_open\tins_long\tins_bases"
        "\ti0_A\ti0_C\ti0_G\ti0_T\ti0_N\ti1_A\ti1_C\ti1_G\ti1_T\ti1_N\ti2_A\ti2_C\ti2_G\ti2_T\ti2_N\ti3_A\ti3_C\ti3_G\ti3_T\ti3_N\n", fp);
}
static void pileup_block(FILE *fp, const char *tag, const ramx_col_pileup *cols, int rows)
{
  for (int r = 0; r < rows; r++)
  {
    const ramx_col_pileup *c = &cols[r];
    fprintf(fp, "%s\t%d\t%c\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%lld", tag, r, code_to_char(c->base), c->cover, c->match[0], c->match[1],
            c->match[2], c->match[3], c->match[4], c->del, c->ins_open, c->ins_long, (long long)c->ins_bases);
    for (int k = 0; k < RAMX_PILEUP_INS; k++)
      for (int b = 0; b < 5; b++) fprintf(fp, "\t%d", c->ins[k][b]);
    fputc('\n', fp);
  }
}
static void refine_sink(const ramx_refinement *rf, void *user)
{
  struct family_outputs *fo = &((struct family_outputs *)user)[rf->family];
  const int d = rf->direction ? 1 : 0;
  FILE *fp = row_open(fo, OUT_PILEUP, "a");
  if (fp)
  {
    pileup_block(fp, d ? "right" : "left", rf->cols, rf->rows);
    if (fo->paths[OUT_REFINED] && rf->replays > 1) pileup_block(fp, d ? "right-refined" : "left-refined", rf->refined_cols, rf->refined_rows);
    fclose(fp);
  }
  if (fo->paths[OUT_REFINED]) keep_fasta(&fo->refined, d, rf->refined_cons, rf->refined_rows, rf->replays, rf->converged, 0);
}
static void refined_write(FILE *fp, struct family_outputs *fo) { kept_fasta_write(fp, &fo->refined, "refined", 0); }

/*
 * -outcpg <file>: the kept consensus refined over at most -refine <n> replays with the CpG-aware re-call (include/ramx.h,
 * ramx_recall_cpg, ramx_set_cpg_sink; -cpgscore <n> is its cpg_ts, default 0) as FASTA, ">right-extension-cpg <n> bp replays=<k>
 * converged=<0|1> cpg=<pairs called CG>" and the left one, which reads as -cons writes it.  -outdinuc <file>: the dinucleotide
 * pileup of that result (ramx_col_dinuc) as a TSV, one line per column of the result, the right direction first; the rows are
 * the device's (a left extension's run outward from the core), xy counts class x in row and class y in row + 1.
 */
static void dinuc_start(FILE *fp)
{
  fputs("dir\trow\tbase\tnext\tboth\tadjacent\tsplit\tgapped", fp);
  for (int x = 0; x < 5; x++)
    for (int y = 0; y < 5; y++) fprintf(fp, "\t%c%c", "ACGTN"[x], "ACGTN"[y]);
  fputc('\n', fp);
}
static void cpg_sink(const ramx_cpg_refinement *cr, void *user)
{
  struct family_outputs *fo = &((struct family_outputs *)user)[cr->family];
  const int d = cr->direction ? 1 : 0, n = cr->refined_rows;
  FILE *fp = row_open(fo, OUT_DINUC, "a");
  if (fp)
  {
    for (int r = 0; r < n; r++)
    {
      const ramx_col_dinuc *c = &cr->refined_di[r];
      fprintf(fp, "%s\t%d\t%c\t%c\t%d\t%d\t%d\t%d", k_dir[d], r, code_to_char(c->base), c->next < 0 ? '-' : code_to_char(c->next),
              c->both, c->adjacent, c->split, c->gapped);
      for (int x = 0; x < 5; x++)
        for (int y = 0; y < 5; y++) fprintf(fp, "\t%d", c->di[x][y]);
      fputc('\n', fp);
    }
    fclose(fp);
  }
  if (fo->paths[OUT_CPG]) keep_fasta(&fo->cpg, d, cr->refined_cons, n, cr->replays, cr->converged, cr->n_cpg);
}
static void cpg_write(FILE *fp, struct family_outputs *fo) { kept_fasta_write(fp, &fo->cpg, "cpg", 1); }

/*
 * -outcopies <file>: every extendable core's divergence from the kept consensus of both extensions (include/ramx.h,
 * ramx_copy_stats, ramx_set_copies_sink) as a TSV, the right block first: one line per extendable core in flank order, named as
 * -outaln names it, then one summary line "#<dir> copies= used= kimura=" with the family's mean Kimura divergence over the
 * copies that have one (min_sites = 1).  The names need both directions' lengths, so the sink keeps the records and the file
 * is written with the other results.
 */
static void copies_sink(const ramx_copies *cp, void *user)
{
  struct family_outputs *fo = &((struct family_outputs *)user)[cp->family];
  if (!fo->paths[OUT_COPIES]) return;
  struct flank_block *b = &fo->copies[cp->direction ? 1 : 0];
  keep_flanks(b, cp->n_flanks, cp->core_index, cp->ends);
  for (int i = 0; i < cp->n_flanks; i++) b->rec[i].st = cp->stats[i];
}

/* after both directions: the file, then the buffers are released */
static void copies_write(FILE *fp, struct family_outputs *fo)
{
  fputs("dir\tcopy\tend_row\tstart\tend\tscore\tcols\tmatch\tts\ttv\tn\tdel\tdel_open\tins\tins_open\tcpg_cols\tcpg_ts\tkimura\n", fp);
  for (int dir = 1; dir >= 0; dir--)
  {
    struct flank_block *b = &fo->copies[dir];
    if (!b->have) continue;
    const char *tag = k_dir[dir];
    ramx_copy_stats *all = (ramx_copy_stats *)malloc(sizeof(ramx_copy_stats) * (size_t)(b->n > 0 ? b->n : 1));
    for (int i = 0; i < b->n; i++)
    {
      const struct flank_rec *rc = &b->rec[i];
      const ramx_copy_stats *t = &rc->st;
      char id[1024];
      fprintf(fp, "%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t", tag, record_id(id, sizeof(id), fo, rc->core, "copy"), rc->end_row,
              rc->start, rc->end, t->score, t->cols, t->match, t->ts, t->tv, t->n_match, t->del, t->del_open, t->ins, t->ins_open, t->cpg_cols, t->cpg_ts);
      const double k = ramx_copy_kimura(t);
      if (k < 0) fputs("NA\n", fp);
      else fprintf(fp, "%.4f\n", k);
      all[i] = *t;
    }
    int32_t used = 0;
    const double div = ramx_family_divergence(all, b->n, 1, &used);
    fprintf(fp, "#%s\tcopies=%d\tused=%d\tkimura=%.4f\n", tag, b->n, (int)used, div);
    free(all); free(b->rec);
    memset(b, 0, sizeof(*b));
  }
}

/*
 * -outlinkage <file>: the co-segregation of the variants of both extensions (include/ramx.h, ramx_set_linkage_sink,
 * ramx_link_pairs) as a TSV, the right block first: one line per pair of variants on different columns whose -log10 p reaches
 * -linkscore, in (p, q) order, then one summary line "#<dir> variants= pairs= linked=": the variants selected, the pairs tested
 * and the pairs written.
 */
static void linkage_sink(const ramx_linkage *lk, void *user)
{
  struct family_outputs *fo = &((struct family_outputs *)user)[lk->family];
  if (!fo->paths[OUT_LINKAGE]) return;
  struct linkage_block *b = &fo->linkage[lk->direction ? 1 : 0];
  const size_t P = (size_t)lk->n_planes;
  b->have = 1; b->P = lk->n_planes;
  b->planes = (ramx_plane *)malloc(sizeof(ramx_plane) * (P ? P : 1));
  b->co = (int32_t *)malloc(sizeof(int32_t) * (P ? P * P : 1));
  if (P) { memcpy(b->planes, lk->planes, sizeof(ramx_plane) * P); memcpy(b->co, lk->co, sizeof(int32_t) * P * P); }
}

/* after both directions: the file, then the buffers are released */
static void linkage_write(FILE *fp, struct family_outputs *fo)
{
  fputs("dir\trow_a\tvar_a\tcount_a\trow_b\tvar_b\tcount_b\tn\tn_a\tn_b\tn_ab\texpected\tmlog10p\n", fp);
  for (int dir = 1; dir >= 0; dir--)
  {
    struct linkage_block *b = &fo->linkage[dir];
    if (!b->have) continue;
    const char *tag = k_dir[dir];
    const int32_t P = b->P;
    /* the pairs tested: every pair scores at least 0 */
    const int32_t tested = ramx_link_pairs(b->planes, P, b->co, 0.0, NULL, 0);
    ramx_link *ln = (ramx_link *)malloc(sizeof(ramx_link) * (size_t)(tested > 0 ? tested : 1));
    const int32_t linked = ramx_link_pairs(b->planes, P, b->co, (double)fo->o->linkscore, ln, tested);
    int variants = 0;
    for (int32_t i = 0; i < P; i++) variants += b->planes[i].cls != RAMX_PLANE_COVER;
    for (int32_t i = 0; i < linked; i++)
    {
      const ramx_link *l = &ln[i];
      const ramx_plane *a = &b->planes[l->p], *c = &b->planes[l->q];
      fprintf(fp, "%s\t%d\t%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%.4f\t%.4f\n", tag, a->row, k_var_name[a->cls & 7],
              b->co[(size_t)l->p * P + l->p], c->row, k_var_name[c->cls & 7], b->co[(size_t)l->q * P + l->q], l->n, l->n_p, l->n_q, l->n_pq,
              l->expected, l->mlog10p);
    }
    fprintf(fp, "#%s\tvariants=%d\tpairs=%d\tlinked=%d\n", tag, variants, (int)tested, (int)linked);
    free(ln); free(b->planes); free(b->co);
    memset(b, 0, sizeof(*b));
  }
}

/*
 * -outsubfam <file>: the copies of both extensions split into subfamilies (include/ramx.h, ramx_set_subfam_sink) as a TSV, the
 * right block first.  Per group a line "group": direction, group, size, the assignments made and whether they converged, the
 * group's pattern as a list of row:variant ("-": none), and -- for a group of at least -subfammin copies -- the length of its
 * refined consensus, the replays, whether those converged, and the consensus in reading order (else NA NA NA -).  After it one
 * line "copy" per copy of the group in flank order: the -outfa record name, its label and its distance to every pattern.  The
 * names need both directions' lengths, so the sink keeps the records and the file is written with the other results.
 */
static void subfam_sink(const ramx_subfamilies *sf, void *user)
{
  struct family_outputs *fo = &((struct family_outputs *)user)[sf->family];
  if (!fo->paths[OUT_SUBFAM]) return;
  struct subfam_block *b = &fo->subfam[sf->direction ? 1 : 0];
  const size_t n = (size_t)(sf->n_flanks > 0 ? sf->n_flanks : 1), K = (size_t)sf->K;
  b->have = 1; b->n = sf->n_flanks; b->K = sf->K; b->iterations = sf->iterations; b->converged = sf->converged;
  b->core = (int32_t *)malloc(sizeof(int32_t) * n); b->labels = (int32_t *)malloc(sizeof(int32_t) * n);
  b->dist = (int32_t *)malloc(sizeof(int32_t) * n * K); b->size = (int32_t *)malloc(sizeof(int32_t) * K);
  b->pattern = (char **)calloc(K, sizeof(char *)); b->cons = (char **)calloc(K, sizeof(char *));
  b->rows = (int *)calloc(K * 3, sizeof(int)); b->replays = b->rows + K; b->conv = b->replays + K;
  memcpy(b->core, sf->core_index, sizeof(int32_t) * (size_t)sf->n_flanks);
  memcpy(b->labels, sf->labels, sizeof(int32_t) * (size_t)sf->n_flanks);
  memcpy(b->dist, sf->dist, sizeof(int32_t) * (size_t)sf->n_flanks * K);
  memcpy(b->size, sf->size, sizeof(int32_t) * K);
  for (int k = 0; k < sf->K; k++)
  {
    char *txt = (char *)malloc((size_t)sf->n_variants * 24 + 2), *w = txt;
    int v = 0;
    for (int i = 0; i < sf->n_planes; i++)
    {
      if (sf->planes[i].cls == RAMX_PLANE_COVER) continue;
      if (sf->patterns[(size_t)v * K + (size_t)k]) w += sprintf(w, "%s%d:%s", w == txt ? "" : ",", sf->planes[i].row, k_var_name[sf->planes[i].cls & 7]);
      v++;
    }
    if (w == txt) *w++ = '-';
    *w = 0;
    b->pattern[k] = txt;
  }
  for (int g = 0; g < sf->n_groups; g++)
  {
    const ramx_subfam_group *gr = &sf->groups[g];
    char *seq = reading_order(gr->refined_cons, gr->refined_rows, sf->direction ? 1 : 0);
    if (gr->refined_rows == 0) strcpy(seq, "-");
    b->cons[gr->group] = seq; b->rows[gr->group] = gr->refined_rows; b->replays[gr->group] = gr->replays; b->conv[gr->group] = gr->converged;
  }
}

/* after both directions: the file, then the buffers are released */
static void subfam_write(FILE *fp, struct family_outputs *fo)
{
  fputs("#group\tdir\tgroup\tsize\titerations\tconverged\tpattern\trefined_bp\treplays\trefined_converged\tconsensus\n"
        "#copy\tdir\tcopy\tlabel\tdistances\n", fp);
  for (int dir = 1; dir >= 0; dir--)
  {
    struct subfam_block *b = &fo->subfam[dir];
    if (!b->have) continue;
    const char *tag = k_dir[dir];
    for (int k = 0; k < b->K; k++)
    {
      fprintf(fp, "group\t%s\t%d\t%d\t%d\t%d\t%s\t", tag, k, b->size[k], b->iterations, b->converged, b->pattern[k]);
      if (b->cons[k]) fprintf(fp, "%d\t%d\t%d\t%s\n", b->rows[k], b->replays[k], b->conv[k], b->cons[k]);
      else fputs("NA\tNA\tNA\t-\n", fp);
      for (int i = 0; i < b->n; i++)
      {
        if (b->labels[i] != k) continue;
        char id[1024];
        fprintf(fp, "copy\t%s\t%s\t%d", tag, record_id(id, sizeof(id), fo, b->core[i], "subfamily"), b->labels[i]);
        for (int j = 0; j < b->K; j++) fprintf(fp, "\t%d", b->dist[(size_t)i * b->K + j]);
        fputc('\n', fp);
      }
      free(b->pattern[k]); free(b->cons[k]);
    }
    free(b->core); free(b->labels); free(b->dist); free(b->size); free(b->pattern); free(b->cons); free(b->rows);
    memset(b, 0, sizeof(*b));
  }
}

/* ------------------------------------------------------------------ the sinks */
/*
 * -outdist <file>: the pairwise divergence between the selected copies of both extensions (include/ramx_dist.h,
 * ramx_set_dist_sink; -distmin <cols> and -distmax <copies> are its selection) as a TSV, the right block first: one line per
 * pair a < b of selected copies in flank order, named as -outcopies names them, with the pair's record and its Kimura distance
 * (NA: undefined), then one summary line "#<dir> copies= selected= pairs= used= kimura= medoid= medoid_kimura=" (ramx_dist_summary
 * with min_sites = -distmin; medoid NA when no pair is used).  If both directions ran, a third block "both" follows: the cores
 * selected in both directions, in the right block's order, every record the field-wise sum of the two directions' records.
 * The names need both directions' lengths, so the sink keeps the records and the file is written with the other results.
 */
static void dist_sink(const ramx_dist *ds, void *user)
{
  struct family_outputs *fo = &((struct family_outputs *)user)[ds->family];
  if (!fo->paths[OUT_DIST]) return;
  struct dist_block *b = &fo->dist[ds->direction ? 1 : 0];
  const size_t n = (size_t)ds->n_flanks, C = (size_t)ds->n_copies;
  b->have = 1; b->n = ds->n_flanks; b->C = ds->n_copies;
  b->core = (int32_t *)malloc(sizeof(int32_t) * (n ? n : 1));
  b->sel = (int32_t *)malloc(sizeof(int32_t) * (C ? C : 1));
  b->m = (ramx_copy_dist *)malloc(sizeof(ramx_copy_dist) * (C ? C * C : 1));
  if (n) memcpy(b->core, ds->core_index, sizeof(int32_t) * n);
  if (C) { memcpy(b->sel, ds->copies, sizeof(int32_t) * C); memcpy(b->m, ds->dist, sizeof(ramx_copy_dist) * C * C); }
}

/* one block: core[a] is the core of the a-th copy of the [C][C] matrix m */
static void dist_block_write(FILE *fp, struct family_outputs *fo, const char *tag, int copies, const int32_t *core, int32_t C, const ramx_copy_dist *m)
{
  char ida[1024], idb[1024];
  for (int32_t a = 0; a < C; a++)
  {
    record_id(ida, sizeof(ida), fo, core[a], "dist");
    for (int32_t b = a + 1; b < C; b++)
    {
      const ramx_copy_dist *r = &m[(size_t)a * C + b];
      fprintf(fp, "%s\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t", tag, ida, record_id(idb, sizeof(idb), fo, core[b], "dist"), r->cover, r->sites,
              r->ts, r->tv, r->del_one, r->del_both);
      const double k = ramx_dist_kimura(r);
      if (k < 0) fputs("NA\n", fp);
      else fprintf(fp, "%.4f\n", k);
    }
  }
  ramx_dist_family s;
  if (ramx_dist_summary(m, C, fo->o->distmin, &s) != RAMX_OK) { fprintf(stderr, "RAMExtend(ramx): pairwise distances: bad matrix\n"); exit(1); }
  fprintf(fp, "#%s\tcopies=%d\tselected=%d\tpairs=%d\tused=%d\tkimura=%.4f\t", tag, copies, (int)C, (int)s.pairs, (int)s.used, s.mean);
  if (s.medoid < 0) fputs("medoid=NA\tmedoid_kimura=NA\n", fp);
  else fprintf(fp, "medoid=%s\tmedoid_kimura=%.4f\n", record_id(ida, sizeof(ida), fo, core[s.medoid], "dist"), s.medoid_mean);
}

/* after both directions: the file, then the buffers are released */
static void dist_write(FILE *fp, struct family_outputs *fo)
{
  fputs("dir\tcopy_a\tcopy_b\tcover\tsites\tts\ttv\tdel_one\tdel_both\tkimura\n", fp);
  for (int dir = 1; dir >= 0; dir--)
  {
    struct dist_block *b = &fo->dist[dir];
    if (!b->have) continue;
    int32_t *core = (int32_t *)malloc(sizeof(int32_t) * (size_t)(b->C > 0 ? b->C : 1));
    for (int32_t a = 0; a < b->C; a++) core[a] = b->core[b->sel[a]];
    dist_block_write(fp, fo, k_dir[dir], b->n, core, b->C, b->m);
    free(core);
  }
  struct dist_block *r = &fo->dist[1], *l = &fo->dist[0];
  if (r->have && l->have)
  {
    /* where a core stands in the left block's selection and whether it is a flank there at all */
    const size_t nc = (size_t)(fo->n_cores > 0 ? fo->n_cores : 1);
    int32_t *at = (int32_t *)malloc(sizeof(int32_t) * nc), *core = (int32_t *)malloc(sizeof(int32_t) * (size_t)(r->C > 0 ? r->C : 1));
    int32_t *ra = (int32_t *)malloc(sizeof(int32_t) * (size_t)(r->C > 0 ? r->C : 1)), *la = (int32_t *)malloc(sizeof(int32_t) * (size_t)(r->C > 0 ? r->C : 1));
    char *in_left = (char *)calloc(nc, 1);
    for (size_t c = 0; c < nc; c++) at[c] = -1;
    for (int i = 0; i < l->n; i++) if (l->core[i] >= 0 && l->core[i] < fo->n_cores) in_left[l->core[i]] = 1;
    for (int32_t a = 0; a < l->C; a++) { const int32_t c = l->core[l->sel[a]]; if (c >= 0 && c < fo->n_cores) at[c] = a; }
    int both = 0;
    for (int i = 0; i < r->n; i++) both += r->core[i] >= 0 && r->core[i] < fo->n_cores && in_left[r->core[i]];
    int32_t C = 0;
    for (int32_t a = 0; a < r->C; a++)
    {
      const int32_t c = r->core[r->sel[a]];
      if (c < 0 || c >= fo->n_cores || at[c] < 0) continue;
      core[C] = c; ra[C] = a; la[C] = at[c]; C++;
    }
    ramx_copy_dist *m = (ramx_copy_dist *)malloc(sizeof(ramx_copy_dist) * (size_t)(C > 0 ? (size_t)C * C : 1));
    for (int32_t a = 0; a < C; a++)
      for (int32_t b = 0; b < C; b++)
      {
        const ramx_copy_dist *x = &r->m[(size_t)ra[a] * r->C + ra[b]], *y = &l->m[(size_t)la[a] * l->C + la[b]];
        ramx_copy_dist *z = &m[(size_t)a * C + b];
        z->cover = x->cover + y->cover; z->sites = x->sites + y->sites; z->ts = x->ts + y->ts; z->tv = x->tv + y->tv;
        z->del_one = x->del_one + y->del_one; z->del_both = x->del_both + y->del_both;
      }
    dist_block_write(fp, fo, "both", both, core, C, m);
    free(at); free(core); free(ra); free(la); free(in_left); free(m);
  }
  for (int dir = 0; dir < 2; dir++)
  {
    struct dist_block *b = &fo->dist[dir];
    free(b->core); free(b->sel); free(b->m);
    memset(b, 0, sizeof(*b));
  }
}

static int any_wants(const struct family_outputs *fams, int F, int row)
{
  for (int i = 0; fams != NULL && i < F; i++)
    if (fams[i].paths[row]) return 1;
  return 0;
}

/* Every sink that a family has a file for gets `fams` as its user, in the order of the table; fams = NULL takes all of them away
 * again (outputs_end, with the options' defaults).  -outpileup and -outrefined share the refine sink -- without a refined
 * consensus to write it makes one replay, the pileup of the kept consensus -- and -outcpg and -outdinuc the CpG sink. */
static void install_sinks(const struct cli_opts *o, struct family_outputs *fams, int F)
{
#define WANTED(row) (fams == NULL || any_wants(fams, F, row))
  const int max_variants = 1024;
  if (WANTED(OUT_PROFILE)) ramx_set_profile_sink(fams ? profile_sink : NULL, fams);
  if (WANTED(OUT_ALN)) ramx_set_align_sink(fams ? aln_sink : NULL, fams);
  if (WANTED(OUT_PILEUP) || WANTED(OUT_REFINED)) ramx_set_refine_sink(fams ? refine_sink : NULL, fams, any_wants(fams, F, OUT_REFINED) ? o->refine : 1);
  if (WANTED(OUT_COPIES)) ramx_set_copies_sink(fams ? copies_sink : NULL, fams);
  if (WANTED(OUT_CPG) || WANTED(OUT_DINUC)) ramx_set_cpg_sink(fams ? cpg_sink : NULL, fams, o->refine, o->cpgscore);
  if (WANTED(OUT_LINKAGE)) ramx_set_linkage_sink(fams ? linkage_sink : NULL, fams, o->linkcount, o->linkfrac, max_variants);
  if (WANTED(OUT_SUBFAM))
    ramx_set_subfam_sink(fams ? subfam_sink : NULL, fams, o->linkcount, o->linkfrac, max_variants, (double)o->linkscore, o->subfamk, o->subfamiter,
                         o->subfammin, o->refine);
  if (WANTED(OUT_DIST)) ramx_set_dist_sink(fams ? dist_sink : NULL, fams, o->distmin, o->distmax);
#undef WANTED
}

/*
 * -outtsd <file>: the target-site duplication of every extended copy (include/ramx.h, ramx_tsd) as a TSV.  "#" lines carry the
 * parameters, the kept columns of both directions, the two termini of the extended consensus with the length of their inverted
 * repeat, the histogram of the lengths found, and the modal length with its count and the count expected by chance.  Then one
 * line per core in list order: named and placed as -outtsv places it, the record, and the two words as the library has them on
 * its forward strand ("N" for a position outside the core's bounds, "-" without a duplication).  Unlike the files above this
 * one is no sink: it needs both directions, and is computed when they are done.
 */
#define TSD_TERMINUS 32

static void tsd_word(char *buf, const struct sequenceLibrary *lib, const struct coreAlignment *s, int64_t from, int k)
{
  for (int j = 0; j < k; j++)
  {
    const int64_t p = from + j;
    const int in = p >= 0 && (uint64_t)p < lib->length && p >= (int64_t)s->lowerSeqBound && p <= (int64_t)s->upperSeqBound;
    buf[j] = in ? code_to_char(ramx_lib_code(lib, (uint64_t)p)) : 'N';
  }
  buf[k] = 0;
}

/* rec: the records of the family's cores */
static void tsd_write(FILE *fp, const struct family_outputs *fo, const ramx_tsd_params *tp, const ramx_tsd *rec)
{
  const int L = fo->o->L, l = 1, nl = fo->leftbp > 0 ? fo->leftbp : 0, nr = fo->rightbp > 0 ? fo->rightbp : 0, n = fo->n_cores;
  const char *master = fo->master;
  int8_t *cl = (int8_t *)malloc((size_t)(nl > 0 ? nl : 1));
  for (int r = 0; r < nl; r++) cl[r] = (int8_t)master[(size_t)L - r - 1];        /* the left rows run outward from the core */
  char five[TSD_TERMINUS + 1], three[TSD_TERMINUS + 1];
  int32_t tir = 0;
  ramx_tsd_hist h;
  if (ramx_termini(cl, nl, (const int8_t *)master + L + l, nr, TSD_TERMINUS, five, three, &tir) != RAMX_OK || ramx_tsd_summary(rec, n, tp, &h) != RAMX_OK)
  { fprintf(stderr, "RAMExtend(ramx): target-site duplications: %s\n", ramx_last_error()); exit(1); }
  free(cl);
  fprintf(fp, "#tsd\tslack=%d\tkmin=%d\tkmax=%d\tmm_div=%d\n", tp->slack, tp->kmin, tp->kmax, tp->mm_div);
  fprintf(fp, "#rows\tleft_rows=%d\tright_rows=%d\n", nl, nr);
  fprintf(fp, "#termini\tfive=%s\tthree=%s\ttir=%d\n", five[0] ? five : "-", three[0] ? three : "-", (int)tir);
  fprintf(fp, "#hist");
  for (int k = 0; k <= 32; k++) if (h.hist[k] > 0) fprintf(fp, "\t%d:%d", k, h.hist[k]);
  fprintf(fp, "\n#mode\tmode=%d\tmode_count=%d\tnull=%.4f\n", h.mode, h.mode_count, h.null[h.mode]);
  fputs("core\tseqid\tstart\tend\tstrand\text_left\text_right\ttsd_len\tmismatches\tshift_left\tshift_right\tleft_word\tright_word\n", fp);
  for (int x = 0; x < n; x++)
  {
    const struct core_view *v = &fo->cores[x];
    const int64_t shift = (int64_t)v->off - (int64_t)v->lo + 1;          /* library position -> what -outtsv prints */
    char lw[33] = "-", rw[33] = "-";
    const ramx_tsd *t = &rec[x];
    if (t->k > 0)
    {
      tsd_word(lw, fo->lib, v->s, v->e_lo + t->dl - t->k, t->k);
      tsd_word(rw, fo->lib, v->s, v->e_hi + 1 + t->dr, t->k);
    }
    fprintf(fp, "%d\t%s\t%ld\t%ld\t%c\t%s\t%s\t%d\t%d\t%d\t%d\t%s\t%s\n", x, v->ident, (long)(v->e_lo + shift), (long)(v->e_hi + shift), v->orient,
            v->left, v->right, t->k, t->mm, t->dl, t->dr, lw, rw);
  }
}

/*
 * -outperiod <file>: the tandem periodicity of the extended copies (include/ramx.h, ramx_period) as a TSV.  "#period" carries the
 * parameters; per part -- left, right, and whole with -periodwhole -- "#part" carries what the family's records say together
 * and "#consensus" the record of that direction's kept consensus in reading order (whole: the left one followed by the right
 * one).  Then one line per core and part, the cores in list order: named and placed as -outtsv places the copy, the part and its
 * length, the record, the periodic region in the coordinates of start and end, and the first bases of the region as the library
 * has them on its forward strand ("-" without a tract).  Like -outtsd this is no sink: it is computed when both directions are done.
 */
/* rec[w] / segs[w]: the records and segments of the family's cores in part w (w = 2 only with -periodwhole) */
static void period_write(FILE *fp, const struct family_outputs *fo, const ramx_period_params *pp, ramx_period *const rec[3], ramx_period_seg *const segs[3])
{
  const int L = fo->o->L, l = 1, nl = fo->leftbp > 0 ? fo->leftbp : 0, nr = fo->rightbp > 0 ? fo->rightbp : 0, parts = fo->o->periodwhole ? 3 : 2;
  const int n = fo->n_cores;
  const struct sequenceLibrary *lib = fo->lib;
  const char *master = fo->master;
  int8_t *cons = (int8_t *)malloc((size_t)(nl + nr > 0 ? nl + nr : 1));
  for (int r = 0; r < nl; r++) cons[r] = (int8_t)master[(size_t)L - nl + r];          /* the left rows run outward from the core */
  for (int r = 0; r < nr; r++) cons[nl + r] = (int8_t)master[(size_t)L + l + r];
  fprintf(fp, "#period\tpmax=%d\tmm=%d\tmin_score=%d\n", pp->pmax, pp->mm, pp->min_score);
  for (int w = 0; w < parts; w++)
  {
    ramx_period_hist h;
    ramx_period cr;
    const int8_t *cw = w == 1 ? cons + nl : cons;
    const int cn = w == 0 ? nl : w == 1 ? nr : nl + nr;
    if (ramx_period_summary(rec[w], segs[w], n, pp, &h) != RAMX_OK || ramx_period_sequence(cw, cn, pp, &cr) != RAMX_OK)
    { fprintf(stderr, "RAMExtend(ramx): periodicity: %s\n", ramx_last_error()); exit(1); }
    fprintf(fp, "#part\tpart=%s\tn=%d\tn_tract=%d\tn_mono=%d\tn_simple=%d\tn_tandem=%d\tat_lo=%d\tat_hi=%d\tmode=%d\tmode_count=%d\n", k_dir[w],
            h.n, h.n_tract, h.n_mono, h.n_simple, h.n_tandem, h.at_lo, h.at_hi, h.mode, h.mode_count);
    fprintf(fp, "#consensus\tpart=%s\tlength=%d\tperiod=%d\tscore=%d\tstart=%d\tend=%d\tagree=%d\tdisagree=%d\n", k_dir[w], cn, cr.period,
            cr.score, cr.start, cr.end, cr.agree, cr.disagree);
  }
  free(cons);
  fputs("core\tseqid\tstart\tend\tstrand\tpart\tlength\tperiod\tunits\tscore\tregion_start\tregion_end\tagree\tdisagree\tunit\n", fp);
  for (int x = 0; x < n; x++)
  {
    const struct core_view *v = &fo->cores[x];
    const int64_t shift = (int64_t)v->off - (int64_t)v->lo + 1;          /* library position -> what -outtsv prints */
    for (int w = 0; w < parts; w++)
    {
      const ramx_period *t = &rec[w][x];
      const ramx_period_seg *g = &segs[w][x];
      char unit[33] = "-";
      int64_t r_lo = 0, r_hi = 0;
      if (t->period > 0)
      {
        r_lo = g->lo + t->start; r_hi = g->lo + t->end + t->period;
        const int k = t->period < 32 ? t->period : 32;
        for (int j = 0; j < k; j++)
        {
          const int64_t p = r_lo + j;
          unit[j] = p >= 0 && (uint64_t)p < lib->length ? (char)toupper((unsigned char)code_to_char(ramx_lib_code(lib, (uint64_t)p))) : 'N';
        }
        unit[k] = 0;
      }
      fprintf(fp, "%d\t%s\t%ld\t%ld\t%c\t%s\t%ld\t%d\t%.2f\t%d\t%ld\t%ld\t%d\t%d\t%s\n", x, v->ident, (long)(v->e_lo + shift), (long)(v->e_hi + shift),
              v->orient, k_dir[w], (long)(g->hi + 1 - g->lo), t->period,
              t->period > 0 ? (double)(t->end - t->start + 1 + t->period) / (double)t->period : 0.0, t->score,
              t->period > 0 ? (long)(r_lo + shift) : 0L, t->period > 0 ? (long)(r_hi + shift) : 0L, t->agree, t->disagree, unit);
    }
  }
}

/*
 * -outterm <file>: the terminal repeats of the extended copies (include/ramx.h, ramx_term) as a TSV.  "#term" carries the
 * parameters, "#family" what the family's records say together (the verdict spelled none, LTR or TIR), and one "#consensus"
 * line per orientation the record of the extended consensus: its outermost min(tmax, left rows, right rows) kept columns at
 * either end (ramx_term_pair).  Then two lines per core in list order, direct and inverted: named and placed as -outtsv places
 * the copy, T, the record, both aligned stretches in the coordinates of start and end (0 without a repeat), matches / columns to
 * three decimals, and whether the record is anchored.  Like -outtsd this is no sink: it is computed when both directions are done.
 */
static const char *const k_term_orient[2] = { "direct", "inverted" };
static const char *const k_term_verdict[3] = { "none", "LTR", "TIR" };

static int term_anchored(const ramx_term *t, int w, int slack)
{
  if (t->score <= 0 || t->a_start > slack) return 0;
  return w == 0 ? t->b_end >= t->T - 1 - slack : t->b_start <= slack;
}

/* rec: two records per core of the family */
static void term_write(FILE *fp, const struct family_outputs *fo, const ramx_term_params *tp, const ramx_term *rec)
{
  const int L = fo->o->L, l = 1, nl = fo->leftbp > 0 ? fo->leftbp : 0, nr = fo->rightbp > 0 ? fo->rightbp : 0, n = fo->n_cores;
  const char *master = fo->master;
  int w = tp->tmax < nl ? tp->tmax : nl;
  if (nr < w) w = nr;
  int8_t *win = (int8_t *)malloc(3 * (size_t)(w > 0 ? w : 1)), *a = win, *b = win + w, *c = win + 2 * w;
  for (int j = 0; j < w; j++)
  {
    a[j] = (int8_t)master[(size_t)L - nl + j];                            /* the left rows run outward from the core */
    b[j] = (int8_t)master[(size_t)L + l + nr - w + j];
    const int8_t x = (int8_t)master[(size_t)L + l + nr - 1 - j];
    c[j] = (int8_t)(x >= 0 && x <= 3 ? 3 - x : x);
  }
  ramx_term_family fam;
  ramx_term cr[2];
  if (ramx_term_summary(rec, n, tp, &fam) != RAMX_OK || ramx_term_pair(a, w, b, w, tp, &cr[0]) != RAMX_OK ||
      ramx_term_pair(a, w, c, w, tp, &cr[1]) != RAMX_OK)
  { fprintf(stderr, "RAMExtend(ramx): terminal repeats: %s\n", ramx_last_error()); exit(1); }
  free(win);
  fprintf(fp, "#term\ttmax=%d\tmatch=%d\tmismatch=%d\tgap=%d\tmin_score=%d\tslack=%d\n", tp->tmax, tp->match, tp->mismatch, tp->gap,
          tp->min_score, tp->slack);
  fprintf(fp, "#family\tn=%d\tn_direct=%d\tn_inverted=%d\tdirect_anchored=%d\tinverted_anchored=%d\tdirect_median=%d\tinverted_median=%d\t"
          "direct_matches=%lld\tdirect_columns=%lld\tinverted_matches=%lld\tinverted_columns=%lld\tverdict=%s\n", fam.n, fam.n_direct,
          fam.n_inverted, fam.direct_anchored, fam.inverted_anchored, fam.direct_median, fam.inverted_median, (long long)fam.direct_matches,
          (long long)fam.direct_columns, (long long)fam.inverted_matches, (long long)fam.inverted_columns, k_term_verdict[fam.verdict]);
  for (int o = 0; o < 2; o++)
    fprintf(fp, "#consensus\torientation=%s\tT=%d\tscore=%d\ta_start=%d\ta_end=%d\tb_start=%d\tb_end=%d\tmatches=%d\tcolumns=%d\n",
            k_term_orient[o], cr[o].T, cr[o].score, cr[o].a_start, cr[o].a_end, cr[o].b_start, cr[o].b_end, cr[o].matches, cr[o].columns);
  fputs("core\tseqid\tstart\tend\tstrand\torientation\tT\tscore\ta_start\ta_end\tb_start\tb_end\tfive_start\tfive_end\tthree_start\tthree_end\t"
        "matches\tcolumns\tidentity\tanchored\n", fp);
  for (int x = 0; x < n; x++)
  {
    const struct core_view *v = &fo->cores[x];
    const int64_t shift = (int64_t)v->off - (int64_t)v->lo + 1;          /* library position -> what -outtsv prints */
    for (int o = 0; o < 2; o++)
    {
      const ramx_term *t = &rec[2 * (size_t)x + o];
      int64_t f_lo = 0, f_hi = 0, t_lo = 0, t_hi = 0;
      if (t->score > 0)
      {
        f_lo = v->e_lo + t->a_start + shift; f_hi = v->e_lo + t->a_end + shift;
        /* the direct partner is read forward from hi + 1 - T, the inverted one backward from hi */
        if (o == 0) { t_lo = v->e_hi + 1 - t->T + t->b_start + shift; t_hi = v->e_hi + 1 - t->T + t->b_end + shift; }
        else { t_lo = v->e_hi - t->b_end + shift; t_hi = v->e_hi - t->b_start + shift; }
      }
      fprintf(fp, "%d\t%s\t%ld\t%ld\t%c\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%ld\t%ld\t%ld\t%ld\t%d\t%d\t%.3f\t%d\n", x, v->ident,
              (long)(v->e_lo + shift), (long)(v->e_hi + shift), v->orient, k_term_orient[o], t->T, t->score, t->a_start, t->a_end,
              t->b_start, t->b_end, (long)f_lo, (long)f_hi, (long)t_lo, (long)t_hi, t->matches, t->columns,
              t->columns > 0 ? (double)t->matches / (double)t->columns : 0.0, term_anchored(t, o, tp->slack));
    }
  }
}

/* the post-passes: after both directions of every family, one compute call for all of them (fns), then the files */
static void tsd_post(const struct cli_opts *o, struct family_outputs *fams, int F, size_t total, const struct outputs_post_fns *fns, void *ctx)
{
  ramx_tsd *rec = (ramx_tsd *)calloc(total ? total : 1, sizeof(ramx_tsd));
  if (fns->tsd(ctx, &o->tsd, rec) < 0) { fprintf(stderr, "RAMExtend(ramx): target-site duplications failed: %s\n", ramx_last_error()); exit(1); }
  size_t at = 0;
  FILE *fp;
  for (int i = 0; i < F; at += (size_t)fams[i].n_cores, i++)
    if ((fp = row_open(&fams[i], OUT_TSD, "w")) != NULL) { tsd_write(fp, &fams[i], &o->tsd, rec + at); fclose(fp); }
  free(rec);
}

static void period_post(const struct cli_opts *o, struct family_outputs *fams, int F, size_t total, const struct outputs_post_fns *fns, void *ctx)
{
  /* one call per part */
  const int parts = o->periodwhole ? 3 : 2;
  ramx_period *rec[3] = { NULL, NULL, NULL };
  ramx_period_seg *segs[3] = { NULL, NULL, NULL };
  for (int w = 0; w < parts; w++)
  {
    rec[w] = (ramx_period *)calloc(total ? total : 1, sizeof(ramx_period));
    segs[w] = (ramx_period_seg *)calloc(total ? total : 1, sizeof(ramx_period_seg));
    if (fns->period(ctx, w, &o->period, rec[w], segs[w]) < 0) { fprintf(stderr, "RAMExtend(ramx): periodicity failed: %s\n", ramx_last_error()); exit(1); }
  }
  size_t at = 0;
  FILE *fp;
  for (int i = 0; i < F; at += (size_t)fams[i].n_cores, i++)
    if ((fp = row_open(&fams[i], OUT_PERIOD, "w")) != NULL)
    {
      ramx_period *const r3[3] = { rec[0] + at, rec[1] + at, rec[2] ? rec[2] + at : NULL };
      ramx_period_seg *const s3[3] = { segs[0] + at, segs[1] + at, segs[2] ? segs[2] + at : NULL };
      period_write(fp, &fams[i], &o->period, r3, s3);
      fclose(fp);
    }
  for (int w = 0; w < 3; w++) { free(rec[w]); free(segs[w]); }
}

static void term_post(const struct cli_opts *o, struct family_outputs *fams, int F, size_t total, const struct outputs_post_fns *fns, void *ctx)
{
  ramx_term *rec = (ramx_term *)calloc(total ? 2 * total : 1, sizeof(ramx_term));
  if (fns->term(ctx, &o->term, rec) < 0) { fprintf(stderr, "RAMExtend(ramx): terminal repeats failed: %s\n", ramx_last_error()); exit(1); }
  size_t at = 0;
  FILE *fp;
  for (int i = 0; i < F; at += (size_t)fams[i].n_cores, i++)
    if ((fp = row_open(&fams[i], OUT_TERM, "w")) != NULL) { term_write(fp, &fams[i], &o->term, rec + 2 * at); fclose(fp); }
  free(rec);
}

/* ------------------------------------------------------------------ the table: one row per output file */
#define REFUSE(what) "RAMExtend(ramx): with -batch every family's " what "\n"
#define REFUSE_PILEUP REFUSE("pileup file is the eighth field of its line in the list and its refined consensus the ninth")
#define REFUSE_CPG REFUSE("CpG-aware consensus file is the fourteenth field of its line in the list; -outdinuc writes one family")
const struct output_row k_outputs[N_OUTPUTS] = {
  /*                 flag         field  word                      refusal                                                                 start / write / post */
  [OUT_PROFILE] = { "-outprofile",  6, "profile",                 REFUSE("profile file is the sixth field of its line in the list"),     .start = profile_start },
  [OUT_ALN]     = { "-outaln",      7, "alignment",               REFUSE("alignment file is the seventh field of its line in the list"), .write = aln_write },
  [OUT_PILEUP]  = { "-outpileup",   8, "pileup",                  REFUSE_PILEUP,                                                         .start = pileup_start },
  [OUT_REFINED] = { "-outrefined",  9, "refined consensus",       REFUSE_PILEUP,                                                         .write = refined_write },
  [OUT_COPIES]  = { "-outcopies",  10, "copies",                  REFUSE("copies file is the tenth field of its line in the list"),      .write = copies_write },
  [OUT_CPG]     = { "-outcpg",     14, "CpG-aware consensus",     REFUSE_CPG,                                                            .write = cpg_write },
  [OUT_DINUC]   = { "-outdinuc",    0, "dinucleotide",            REFUSE_CPG,                                                            .start = dinuc_start },
  [OUT_LINKAGE] = { "-outlinkage", 11, "linkage",                 REFUSE("linkage file is the eleventh field of its line in the list"),  .write = linkage_write },
  [OUT_SUBFAM]  = { "-outsubfam",  12, "subfamily",               REFUSE("subfamily file is the twelfth field of its line in the list"), .write = subfam_write },
  [OUT_TSD]     = { "-outtsd",     13, "target-site duplication", REFUSE("target-site duplication file is the thirteenth field of its line in the list"), .post = tsd_post },
  [OUT_PERIOD]  = { "-outperiod",  15, "periodicity",             REFUSE("periodicity file is the fifteenth field of its line in the list"), .post = period_post },
  [OUT_TERM]    = { "-outterm",    16, "terminal repeat",         REFUSE("terminal repeat file is the sixteenth field of its line in the list"), .post = term_post },
  [OUT_DIST]    = { "-outdist",    17, "pairwise distance",       REFUSE("pairwise distance file is the seventeenth field of its line in the list"), .write = dist_write },
};

void outputs_refuse_flags(const struct cli_opts *o)
{
  for (int r = 0; r < N_OUTPUTS; r++)
    if (o->out[r] != NULL) { fputs(k_outputs[r].refusal, stderr); exit(1); }
}

void outputs_parse_fields(struct family_outputs *fo, char *const f[BATCH_FIELDS])
{
  for (int r = 0; r < N_OUTPUTS; r++)
  {
    const char *s = k_outputs[r].batch_field ? f[k_outputs[r].batch_field - 1] : NULL;
    fo->paths[r] = (s == NULL || s[0] == 0 || strcmp(s, "-") == 0) ? NULL : strdup(s);
  }
}

void outputs_free_fields(struct family_outputs *fo)
{
  for (int r = 0; r < N_OUTPUTS; r++) { free((char *)fo->paths[r]); fo->paths[r] = NULL; }
}

void outputs_begin(const struct cli_opts *o, struct family_outputs *fams, int F)
{
  for (int i = 0; i < F; i++) fams[i].o = o;
  for (int r = 0; r < N_OUTPUTS; r++)
  {
    const struct output_row *row = &k_outputs[r];
    FILE *fp;
    for (int i = 0; row->start != NULL && i < F; i++)
      if ((fp = row_open(&fams[i], r, "w")) != NULL) { row->start(fp); fclose(fp); }
  }
  install_sinks(o, fams, F);
}

void outputs_family_done(struct family_outputs *fo, const struct coreAlignment *cores, const char *master, int rightbp, int leftbp)
{
  outputs_family_cores(fo, cores);
  fo->master = master; fo->rightbp = rightbp; fo->leftbp = leftbp;
  FILE *fp;
  for (int r = 0; r < N_OUTPUTS; r++)
    if (k_outputs[r].write != NULL && (fp = row_open(fo, r, "w")) != NULL) { k_outputs[r].write(fp, fo); fclose(fp); }
}

void outputs_post(const struct cli_opts *o, struct family_outputs *fams, int F, const struct outputs_post_fns *fns, void *ctx)
{
  size_t total = 0;
  for (int i = 0; i < F; i++) total += (size_t)fams[i].n_cores;
  for (int r = 0; r < N_OUTPUTS; r++)
    if (k_outputs[r].post != NULL && any_wants(fams, F, r)) k_outputs[r].post(o, fams, F, total, fns, ctx);
}

void outputs_end(struct family_outputs *fams, int F)
{
  static const struct cli_opts k_defaults = { .refine = DEF_REFINE, .cpgscore = DEF_CPGSCORE, .linkcount = DEF_LINKCOUNT, .linkfrac = DEF_LINKFRAC,
                                              .linkscore = DEF_LINKSCORE, .subfamk = DEF_SUBFAMK, .subfammin = DEF_SUBFAMMIN, .subfamiter = DEF_SUBFAMITER,
                                              .distmin = 1, .distmax = DEF_DISTMAX };
  install_sinks(&k_defaults, NULL, 0);          /* the one reset */
  for (int i = 0; i < F; i++) { free(fams[i].cores); fams[i].cores = NULL; }
}

/* -outxfam <file>: the overlaps between the extended consensi (include/ramx_xfam.h), once per run, after the post-passes.  The
 * sequences are every family's left and right extension as -cons writes them, index 2 f and 2 f + 1; within = 1, so a family's
 * own two extensions are compared too (the LTR or TIR at consensus level, at any length).  One header line; one line per record
 * with a score, in pair order: family index, ranges file and left|right of A, the same of B, +|-, score, a_from, a_to, len_a,
 * b_from, b_to (in B's own reading coordinates, b_from <= b_to whatever the orientation), len_b, matches, columns, identity
 * with three decimals, link (the record counts and joins two different families); then one "#group" line per component: its
 * id, its size and its families.  A consensus above RAMX_XFAM_MAXLEN is left out and named by a "#skipped" line.  Standard
 * output gets one summary line. */
int outputs_xfam_check(const struct cli_opts *o)
{
  extern int ramx_pair_check_params(const ramx_pair_params *pp);
  if (!(o->xfamseed == 0 || (o->xfamseed >= 8 && o->xfamseed <= 16)))
  { ramx_set_error("-xfamseed %d: 0, or a word of 8..16 bases", o->xfamseed); return RAMX_ERR_ARG; }
  if (o->xfamlink.min_columns < 0 || o->xfamlink.min_permille < 0 || o->xfamlink.min_permille > 1000)
  { ramx_set_error("-xfamcols %d (>= 0), -xfamident %d (0..1000)", o->xfamlink.min_columns, o->xfamlink.min_permille); return RAMX_ERR_ARG; }
  return ramx_pair_check_params(&o->xfam);
}

void outputs_xfam(const struct cli_opts *o, const struct family_outputs *fams, int F, const char *const *names)
{
  const int L = o->L, l = 1, S = 2 * F;
  FILE *fp = open_or_die(o->outxfam, "w", "cross-family overlap");
  fprintf(fp, "#family_a\tranges_a\tside_a\tfamily_b\tranges_b\tside_b\torient\tscore\ta_from\ta_to\tlen_a\tb_from\tb_to\tlen_b\tmatches\tcolumns\tidentity\tlink\n");
  int64_t *off = (int64_t *)calloc((size_t)S + 1, sizeof(int64_t));
  int32_t *owner = (int32_t *)malloc(sizeof(int32_t) * (size_t)(S ? S : 1)), *group = (int32_t *)malloc(sizeof(int32_t) * (size_t)(F ? F : 1));
  for (int s = 0; s < S; s++)
  {
    const struct family_outputs *fo = &fams[s / 2];
    int n = s % 2 ? fo->rightbp : fo->leftbp;
    if (n < 0) n = 0;
    if (n > RAMX_XFAM_MAXLEN) { fprintf(fp, "#skipped\t%d\t%s\t%s\t%d\n", s / 2, names[s / 2], s % 2 ? "right" : "left", n); n = 0; }
    off[s + 1] = off[s] + n;
    owner[s] = s / 2;
  }
  int8_t *codes = (int8_t *)malloc((size_t)(off[S] ? off[S] : 1));
  int *len = (int *)malloc(sizeof(int) * (size_t)(S ? S : 1));
  for (int s = 0; s < S; s++)
  {
    const struct family_outputs *fo = &fams[s / 2];
    len[s] = (int)(off[s + 1] - off[s]);
    if (len[s]) memcpy(codes + off[s], fo->master + (s % 2 ? (long)L + l : (long)L - len[s]), (size_t)len[s]);
  }
  const int64_t n = ramx_xfam_candidates(codes, off, S, owner, o->xfamseed, 1, NULL, 0);
  if (n < 0 || n > INT32_MAX) { fprintf(stderr, "RAMExtend(ramx): cross-family candidates failed: %s\n", n < 0 ? ramx_last_error() : "too many pairs"); exit(1); }
  ramx_seq_pair *pairs = (ramx_seq_pair *)malloc(sizeof(ramx_seq_pair) * (size_t)(n ? n : 1));
  ramx_term *rec = (ramx_term *)malloc(sizeof(ramx_term) * (size_t)(n ? n : 1));
  int32_t *counts = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n ? n : 1));
  if (ramx_xfam_candidates(codes, off, S, owner, o->xfamseed, 1, pairs, n) != n ||
      ramx_dev_seq_pairs(NULL, codes, off, S, pairs, (int32_t)n, &o->xfam, rec, NULL) != RAMX_OK ||
      ramx_xfam_groups(pairs, rec, (int32_t)n, owner, F, &o->xfamlink, counts, group) != RAMX_OK)
  { fprintf(stderr, "RAMExtend(ramx): cross-family overlap failed: %s\n", ramx_last_error()); exit(1); }
  long n_rec = 0, n_link = 0, n_big = 0;
  for (int64_t p = 0; p < n; p++)
  {
    const ramx_term *r = &rec[p];
    if (r->score <= 0) continue;
    const int a = pairs[p].a, b = pairs[p].b, inv = pairs[p].inverted, link = counts[p] && owner[a] != owner[b];
    const int b_from = inv ? len[b] - 1 - r->b_end : r->b_start, b_to = inv ? len[b] - 1 - r->b_start : r->b_end;
    const long ident = (2000L * r->matches + r->columns) / (2L * r->columns);       /* per thousand, rounded half up */
    fprintf(fp, "%d\t%s\t%s\t%d\t%s\t%s\t%c\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%ld.%03ld\t%d\n", owner[a], names[owner[a]], a % 2 ? "right" : "left",
            owner[b], names[owner[b]], b % 2 ? "right" : "left", inv ? '-' : '+', r->score, r->a_start, r->a_end, len[a], b_from, b_to, len[b],
            r->matches, r->columns, ident / 1000, ident % 1000, link);
    n_rec++; n_link += link;
  }
  for (int g = 0; g < F; g++)
  {
    int size = 0;
    for (int f = 0; f < F; f++) size += group[f] == g;
    if (!size) continue;
    n_big += size > 1;
    fprintf(fp, "#group\t%d\t%d\t", g, size);
    for (int f = 0, k = 0; f < F; f++) if (group[f] == g) fprintf(fp, "%s%d", k++ ? "," : "", f);
    fprintf(fp, "\n");
  }
  fclose(fp);
  printf("xfam: %lld candidates, %ld records, %ld links, %ld groups with more than one family\n", (long long)n, n_rec, n_link, n_big);
  free(off); free(owner); free(group); free(codes); free(len); free(pairs); free(rec); free(counts);
}
