/*
 * ramx_cli.c -- the RAMExtend command line (reference ram_extend.c:123-826 main/usage/
 * print_parameters, cmd_line_opts.c).  Same argv semantics (prefix matching, per-matrix
 * defaults), same stdout / -cons / -outtsv / -outfa bytes; the two extend_alignment calls go to
 * the device path (ramx_extend_alignment).
 */
#include <ctype.h>
#include <fcntl.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include "ramx_internal.h"

static const char *k_version = "0.0.7";          /* interface level of the reference this mirrors */
static const char *k_build = "ramx-gfx950";
static const char *k_build_date = "20261003";

/* ------------------------------------------------------------------ argv scanning
 * cmd_line_opts.c:9-107: the FIRST argv entry that begins with '-' and of which `text` is a
 * prefix wins; its value is the following argv entry. */
static int opt_find(int argc, char **argv, const char *text)
{
  const size_t n = strlen(text);
  for (int i = 0; i < argc; i++)
    if (argv[i][0] == '-' && strncmp(text, argv[i], n) == 0) return i;
  return -1;
}
static const char *opt_value(int argc, char **argv, int i) { return (i + 1 < argc) ? argv[i + 1] : ""; }
static int opt_int(int argc, char **argv, const char *text, int *res)
{
  int i = opt_find(argc, argv, text);
  if (i < 0) return 0;
  *res = atoi(opt_value(argc, argv, i));
  return 1;
}
static int opt_bool(int argc, char **argv, const char *text) { return opt_find(argc, argv, text) >= 0; }
static int opt_string(int argc, char **argv, const char *text, const char **res)
{
  int i = opt_find(argc, argv, text);
  if (i < 0) return 0;
  *res = (i + 1 < argc) ? argv[i + 1] : NULL;
  return 1;
}

static char code_to_char(int z)
{
  static const char t[8] = { 'A', 'C', 'G', 'T', 'a', 'c', 'g', 't' };
  return (z >= 0 && z < 8) ? t[z] : 'N';
}
static int code_compl(int c)
{
  if (c >= 0 && c <= 3) return 3 - c;
  if (c >= 4 && c <= 7) return 4 + (7 - c);
  return RAMX_SYM_N;
}

static void usage(void)
{
  printf("RAMExtend Version %s - build %s date %s\n", k_version, k_build, k_build_date);
  fputs(
    "\n"
    "  Perform a multiple sequence alignment (MSA) extension given\n"
    "  an existing core MSA and the flanking sequences.  The core\n"
    "  may be a set of word matches, a previously development MSA,\n"
    "  or the the result of any process that defines a core set of\n"
    "  sequence relationships.  The only requirement is that the sequences are\n"
    "  aligned to nearly the same point along one or both of the core\n"
    "  edges.  The extension process is a form of anchored alignment\n"
    "  where the details of the core alignment are considered fixed.\n"
    "\n"
    "Usage: \n"
    "  RAMExtend -twobit <seq.2bit> -ranges <ranges.tsv> [opts]\n"
    "\n"
    "--------------------------------------------------------------------------------------------\n"
    "     -cons <seq.fa>        # Save the left/right consensus sequences to a FASTA file.\n"
    "     -outtsv <final.tsv>   # Save the final sequence ranges to a TSV file.\n"
    "     -outfa <seq.fa>       # Save all the final sequences ( original range + extension )\n"
    "                           #   to a file.\n"
    "     -addflanking <num>    # Include an additional<num> bp of sequence to each sequence\n"
    "                           #   when using the -outfa option.\n"
    "     -L <num>              # Size of region to extend left or right (10000). \n"
    "     -minimprovement <num> # Amount that a the alignment score needs to improve each step\n"
    "                           #   to be considered progress (original: 3, nucleotide matrix: 27).\n"
    "     -maxoccurrences <num> # Cap on the number of sequences to align (10,000). \n"
    "     -cappenalty <num>     # Cap on penalty for exiting alignment of a sequence \n"
    "                           #   (original: -20, nucleotide matrix:-90).\n"
    "     -stopafter <num>      # Stop the alignment after this number of no-progress columns (100).\n"
    "     -minlength <num>      # Minimum required length for a sequence to be reported (50).\n"
    "     -outmat <file>        # Dump the dp matrix paths to a file for debugging.\n"
    "     -outcopies <file>     # Save every copy's divergence from the extension consensus\n"
    "                           #   ( matches, transitions, transversions, gaps, Kimura ) to a TSV file.\n"
    "     -outcpg <file>        # Save the extension consensus re-called with the CpG-aware rule ( a CG whose\n"
    "                           #   copies have mostly deaminated to TG / CA / TA is called CG ) to a FASTA file,\n"
    "     -outdinuc <file>      # ... and the dinucleotide counts of its adjacent columns to a TSV file.\n"
    "     -cpgscore <num>       # ... the score of a deaminated base under the CpG hypothesis (0).\n"
    "     -outlinkage <file>    # Save the pairs of variant columns of the extension consensus whose variants\n"
    "                           #   travel together in the copies ( a sign of subfamilies ) to a TSV file.\n"
    "     -linkcount <num>      # ... a variant needs this many copies (4),\n"
    "     -linkfrac <num>       # ... and this many per thousand of the copies that cover its column (100).\n"
    "     -linkscore <num>      # ... a pair is written from this -log10 p of its hypergeometric test (3).\n"
    "     -outsubfam <file>     # Save the split of the copies into subfamilies by the linked variants they carry\n"
    "                           #   (selection and threshold: -linkcount, -linkfrac, -linkscore), every group\n"
    "                           #   with its own refined consensus (-refine replays), as a TSV.\n"
    "     -subfamk <num>        # ... at most this many groups, 1..8 (4),\n"
    "     -subfammin <num>      # ... a group gets a consensus of its own from this many copies (4),\n"
    "     -subfamiter <num>     # ... at most this many assignments (8).\n"
    "     -outtsd <file>        # Save the target-site duplication of every extended copy ( the direct repeat\n"
    "                           #   just outside its two ends ) and the family's modal length to a TSV file.\n"
    "     -tsdslack <num>       # ... either end may lie this many bases off the reported one, 0..7 (3),\n"
    "     -tsdmin <num>         # ... shortest and\n"
    "     -tsdmax <num>         # ... longest duplication looked for, 1..32 (4, 20),\n"
    "     -tsdmm <num>          # ... one mismatch allowed per this many bases, 0 = none (10).\n"
    "     -outperiod <file>     # Save the tandem periodicity of every copy's left and right extension ( did the\n"
    "                           #   extension run into a simple repeat or a satellite? ) to a TSV file.\n"
    "     -periodmax <num>      # ... the longest period looked for, 1..8192 (1024),\n"
    "     -periodmm <num>       # ... what a disagreeing pair costs, 1..15 (3),\n"
    "     -periodmin <num>      # ... the lowest score reported (16),\n"
    "     -periodwhole          # ... also for the whole extended copy.\n"
    "     -version              # Print out one-line version information\n"
    "     -v[v[v[v]]]           # How verbose do you want it to be?  -vvvv is super-verbose.\n"
    "\n"
    "   New Scoring System Options:\n"
    "     -matrix 14p43g |      # There are several internally-coded matrices available.\n"
    "             18p43g |      #   The DNA substitution matrices are borrowed from RepeatMasker\n"
    "             20p43g |      #   and are tuned for a 43% GC background.  The four encoded\n"
    "             25p43g        #   matrices are are divergence tuned, ranging from 14% to 25%.\n"
    "                           #   For example the '14p43g' matrix is tuned for 14% divergence\n"
    "                           #   43% GC background.  Each matrix has it's own default gap_open,\n"
    "                           #   gap_extension parameters.  These may be overrided by using the\n"
    "                           #   -gapopen and -gapextn options.\n"
    "     -gapopen <num>        # Affine gap open penalty to override per-matrix default\n"
    "     -gapextn <num>        # Affine gap extension penalty to override per-matrix default\n"
    "\n"
    "     -bandwidth <num>      # The maximum number of unbalanced gaps allowed (14)\n"
    "                           #   Half the bandwidth of the banded Smith-Waterman\n"
    "                           #   algorithm.  The default allows for at most 14bp\n"
    "                           #   of unbalanced insertions/deletions in any aligned\n"
    "                           #   sequence.  The full bandwidth is 2*bandwidth+1.\n"
    " or\n"
    "   Original RepeatScout Scoring System:\n"
    "     -matrix repeatscout   # The original RepeatScout scoring system is enabled if this\n"
    "                           #   option is set.  This uses a simple match/mismatch penalty\n"
    "                           #   and a linear gap model.  The original RepeatScout values\n"
    "                           #   for these parameters may be overriden with the following\n"
    "                           #   additional options:\n"
    "     -match <num>          # If '-matrix repeatscout' used, apply this reward for match\n"
    "                           #   (default +1)  \n"
    "     -mismatch <num>       # If '-matrix repeatscout' used, apply this penalty for a mismatch\n"
    "                           #   (default: -1) \n"
    "     -gap <num>            # If '-matrix repeatscout' used, apply this penalty for a gap\n"
    "                           #   (default: -5)\n"
    "\n"
    "Ranges:\n\n"
    "   Ranges are supplied in the form of a modified BED-6 format:\n\n"
    "      field-1:chrom     : sequence identifier\n"
    "      field-2:chromStart: lower aligned position ( 0 based )\n"
    "      field-3:chromEnd  : upper aligned position ( 0 based, half open )\n"
    "      field-4:left-ext  : left extendable flag ( 0 = no, 1 = yes ) [BED-6 'name' field]\n"
    "      field-5:right-ext : right extendable flag ( 0 = no, 1 = yes ) [BED-6 'score' field]\n"
    "      field-6:strand    : strand ( '+' = forward, '-' = reverse )\n"
    "\n"
    "   The fields are tab separated. Coordinates are zero-based half\n"
    "   open.\n"
    "\n"
    "   Left/Right extension flags are used to turn off extension for sequences that\n"
    "   do not reach the edge of the core alignment (e.g. fragments aligning in the\n"
    "   center of the core MSA, or one or the other edge only).  These sequences are\n"
    "   less likely to include related flanking sequence and weigh down the extension\n"
    "   score uneccesarily.  For these sequences it is desirable to flag one edge or\n"
    "   the other as 'unextendable'.  The 'left'/'right' designations refer to the\n"
    "   edges of the core MSA alignment. The 'left' flag may refer to the start or\n"
    "   the end coordinate depending on the state of the orientation flag\n"
    "   ('+' left=start, '-' left=end etc.).\n", stdout);
  exit(1);
}

/* one FASTA record body, 80-column wrap whose phase is keyed on masterstart for BOTH records
 * (reference ram_extend.c:518-540 / :561-584) */
static void write_wrapped(FILE *fp, const char *master, uint64_t from, uint64_t to, uint64_t masterstart)
{
  uint64_t x;
  for (x = from; x < to; x++)
  {
    fputc(code_to_char(master[x]), fp);
    if ((x - masterstart) % 80 == 79) fputc('\n', fp);
  }
  if ((x - masterstart) % 80 > 0) fputc('\n', fp);
}


/* RAMX_TIMING=1: phase timings on stderr (stdout stays byte-compatible) */
static double now_s(void)
{
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
static int g_timing = 0;
static double g_t_last = 0, g_t_main = 0;
static void phase_done(const char *what)
{
  if (!g_timing) return;
  fflush(stdout);
  const double t = now_s();
  fprintf(stderr, "RAMX_TIMING %-18s %10.3f ms   (at %8.3f ms after main)\n", what, (t - g_t_last) * 1e3, (t - g_t_main) * 1e3);
  g_t_last = t;
}
static void timing_at_exit(void) { if (g_timing) { const double t = now_s(); fprintf(stderr, "RAMX_TIMING %-18s %10.3f ms   (at %8.3f ms after main)\n", "first atexit handler", (t - g_t_last) * 1e3, (t - g_t_main) * 1e3); } }

/* The first HIP call of a process costs 0.1-0.3 s (runtime start-up, device context).  It does not depend on the
 * input, so it runs in a helper thread while the loader reads the .2bit; joined before the first extension. */
static pthread_t g_warm_thread;
static int g_warm_started = 0;
/* the helper thread starts the HIP runtime while the loader works and then, as soon as the main thread hands it the
 * library, uploads it while the main thread prints the core table (1 GB of flanks: ~60 ms that would otherwise sit in
 * front of the right extension) */
static pthread_mutex_t g_warm_mu = PTHREAD_MUTEX_INITIALIZER;
static pthread_cond_t g_warm_cv = PTHREAD_COND_INITIALIZER;
static const struct sequenceLibrary *g_warm_lib = NULL;
static int g_warm_quit = 0;
static void *warm_device(void *unused)
{
  (void)unused;
  (void)ramx_default_device();          /* failure is reported by the main thread's own call later */
  /* (Loading the code objects here as well -- ramx_dev_warm -- was measured and dropped: the runtime's start-up already takes as
   * long as the loader does, the main thread then WAITS for this thread (20-100 ms), and the first launches were no faster.) */
  pthread_mutex_lock(&g_warm_mu);
  while (g_warm_lib == NULL && !g_warm_quit) pthread_cond_wait(&g_warm_cv, &g_warm_mu);
  const struct sequenceLibrary *lib = g_warm_lib;
  pthread_mutex_unlock(&g_warm_mu);
  if (lib != NULL)                      /* a failure: seam 1 uploads (and reports) itself */
  {
    const ramx_packed_library *pl = ramx_packed_of(lib);
    if (pl) (void)ramx_preload_library_packed(lib, pl);
    else if (lib->sequence) (void)ramx_preload_library((const int8_t *)lib->sequence, lib->length);
  }
  return NULL;
}
static void warm_offer_library(const struct sequenceLibrary *lib)
{
  pthread_mutex_lock(&g_warm_mu);
  g_warm_lib = lib;
  pthread_cond_signal(&g_warm_cv);
  pthread_mutex_unlock(&g_warm_mu);
}
static void warm_join(void)
{
  if (g_warm_started)
  {
    g_warm_started = 0;
    pthread_mutex_lock(&g_warm_mu);
    g_warm_quit = 1;
    pthread_cond_signal(&g_warm_cv);
    pthread_mutex_unlock(&g_warm_mu);
    pthread_join(g_warm_thread, NULL);
  }
}
static void warm_start(void)
{
  if (getenv("RAMX_NO_WARM_THREAD") == NULL && pthread_create(&g_warm_thread, NULL, warm_device, NULL) == 0)
  {
    g_warm_started = 1;
    atexit(warm_join);                  /* every exit path (loader errors exit(255)) lets the runtime finish starting first */
  }
}

/* everything the command line decides */
struct cli_opts
{
  const char *ranges_file, *outtsv, *outfa, *outmat, *cons_file, *seq_file, *matrix_name, *batch_file, *outprofile, *outaln, *outpileup, *outrefined, *outcpg, *outdinuc, *outcopies, *outlinkage, *outsubfam, *outtsd, *outperiod;
  ramx_tsd_params tsd;
  ramx_period_params period;
  int periodwhole;
  int refine, cpgscore, linkcount, linkfrac, linkscore, subfamk, subfammin, subfamiter;
  int flanking, L, bandwidth, maxn, when_to_stop, num_threads, verbose;
  int gap_ext, gap_open, match, mismatch, cappenalty, minimprovement, is_rs;
  struct scoringSystem *sp;
};

/* banner + parameters, ram_extend.c:397-400, 793-826 */
static void print_header(const struct cli_opts *o, const char *ranges_file, int N, const struct sequenceLibrary *lib)
{
  printf("\nRAMExtend Version %s - build %s date %s\n", k_version, k_build, k_build_date);
  printf("--------------------------------------------------------------\n");
  printf("Parameters:\n");
  printf("  VERBOSE %d\n", o->verbose);
  printf("  SEQUENCE_FILE %s\n", o->seq_file);
  printf("  RANGES_FILE %s\n", ranges_file);
  if (o->num_threads)
    printf("  Multi-Threaded-Masking (EXPERIMENTAL): num_threads = %d\n", o->num_threads);
  printf("  L %d\n", o->L);
  printf("  BANDWIDTH (bandwidth) %d\n", o->bandwidth);
  printf("  MAXN %d\n", o->maxn);
  if (o->is_rs)
  {
    printf("  SCORING SYSTEM: Original RepeatScout method\n");
    printf("     - GAP = %d\n", o->sp->gapextn);
    printf("     - MATCH = %d\n", o->match);
    printf("     - MISMATCH = %d\n", o->mismatch);
  }
  else
  {
    printf("  SCORING SYSTEM: Internally coded matrix '%s'\n", o->matrix_name);
    printf("     - GAP_OPEN = %d\n", o->sp->gapopen);
    printf("     - GAP_EXT = %d\n", o->sp->gapextn);
  }
  printf("     - CAPPENALTY %d\n", o->cappenalty);
  printf("     - MINIMPROVEMENT %d\n", o->minimprovement);
  printf("  WHEN_TO_STOP %d\n", o->when_to_stop);
  printf("--------------------------------------------------------------\n");
  printf("Read in %d ranges, and %ld bp of sequence\n\n", N, (long)lib->length);
}

/* rows [lo_i, hi_i) of the report (stdout), of -outtsv and of -outfa: reference ram_extend.c:606-779 */
struct results_ctx
{
  struct coreAlignment **arr;
  struct sequenceLibrary *lib;
  int flanking;
};

static void results_rows(int lo_i, int hi_i, FILE **outs, void *user)
{
  const struct results_ctx *t = (const struct results_ctx *)user;
  struct sequenceLibrary *lib = t->lib;
  const int flanking = t->flanking;
  FILE *out = outs[0], *fp = outs[1], *fp_fa = outs[2];
  for (long x = lo_i; x < hi_i; x++)
  {
    struct coreAlignment *s = t->arr[x];

      const int si = s->seqIdx;
      const char *ident = lib->identifiers[si];
      const uint64_t lo = si > 0 ? lib->boundaries[si - 1] : 0;
      const uint64_t hi = lib->boundaries[si];
      const uint64_t off = (lib->offsets != NULL && lib->offsets[si] > 0) ? lib->offsets[si] : 0;
      uint64_t ext_start, ext_end, core_start, core_end;
      char orient = '+';
      if (s->orient)
      {
        orient = '-';
        ext_end = (s->leftSeqPos + (uint64_t)s->leftExtensionLen) - lo + 1;
        ext_start = (s->rightSeqPos - (uint64_t)s->rightExtensionLen) - lo + 1;
        core_start = s->rightSeqPos - lo + 1 + off;
        core_end = s->leftSeqPos - lo + 1 + off;
      }
      else
      {
        ext_start = s->leftSeqPos - (uint64_t)s->leftExtensionLen - lo + 1;
        ext_end = (s->rightSeqPos + (uint64_t)s->rightExtensionLen) - lo + 1;
        core_start = s->leftSeqPos - lo + 1 + off;
        core_end = s->rightSeqPos - lo + 1 + off;
      }
      const int ext_len = (int)(ext_end - ext_start + 1);
      char lbuf[32], rbuf[32];
      if (s->leftExtendable) snprintf(lbuf, sizeof(lbuf), "%d", s->leftExtensionLen); else strcpy(lbuf, "*");
      if (s->rightExtendable) snprintf(rbuf, sizeof(rbuf), "%d", s->rightExtensionLen); else strcpy(rbuf, "*");

      fprintf(out, "%s\t%ld\t%ld\t%c\tn=%ld,anchor_range=%ld-%ld,extended_left=%s,extended_right=%s,len=%d,score=%d",
             ident, (long)(off + ext_start), (long)(off + ext_end), orient, x, (long)core_start, (long)core_end,
             lbuf, rbuf, ext_len, s->score);
      /* limit annotations, ram_extend.c:669-693 */
      if (orient == '+')
      {
        if (s->leftExtendable && ((s->leftSeqPos - (uint64_t)s->leftExtensionLen) - s->lowerSeqBound) < 20)
        {
          if (s->lowerSeqBoundFlag == SEQ_BOUNDARY) fprintf(out, ",leftSeqLimit");
          else if (s->lowerSeqBoundFlag == L_BOUNDARY) fprintf(out, ",leftExtLimit");
          else if (s->lowerSeqBoundFlag == CORE_BOUNDARY) fprintf(out, ",leftCoreLimit");
        }
        if (s->rightExtendable && (s->upperSeqBound - (s->rightSeqPos + (uint64_t)s->rightExtensionLen)) < 20)
        {
          if (s->upperSeqBoundFlag == SEQ_BOUNDARY) fprintf(out, ",rightSeqLimit");
          else if (s->upperSeqBoundFlag == L_BOUNDARY) fprintf(out, ",rightExtLimit");
          else if (s->upperSeqBoundFlag == CORE_BOUNDARY) fprintf(out, ",rightCoreLimit");
        }
      }
      else
      {
        if (s->leftExtendable && (s->upperSeqBound - (s->leftSeqPos + (uint64_t)s->leftExtensionLen)) < 20) fprintf(out, ",leftCoreLimit");
        if (s->rightExtendable && ((s->rightSeqPos - (uint64_t)s->rightExtensionLen) - s->lowerSeqBound) < 20) fprintf(out, ",rightCoreLimit");
      }
      fprintf(out, "\n");

      if (fp != NULL)   /* NB: anchor_range here is window-relative, without the genomic offset (ram_extend.c:696-712) */
        fprintf(fp, "%s\t%ld\t%ld\t%c\tn=%ld,anchor_range=%ld-%ld,extended_left=%s,extended_right=%s,len=%d,score=%d\n",
                ident, (long)(off + ext_start), (long)(off + ext_end), orient, x, (long)(s->leftSeqPos - lo + 1),
                (long)(s->rightSeqPos - lo + 1), lbuf, rbuf, ext_len, s->score);

      if (fp_fa != NULL)
      {
        if (s->leftExtensionLen < 0 || s->rightExtensionLen < 0) { fprintf(stderr, "Error: Negative extension length detected\n"); exit(1); }
        uint64_t from = s->leftSeqPos - (uint64_t)s->leftExtensionLen, to = s->rightSeqPos + (uint64_t)s->rightExtensionLen;
        if (s->orient) { to = s->leftSeqPos + (uint64_t)s->leftExtensionLen; from = s->rightSeqPos - (uint64_t)s->rightExtensionLen; }
        if (flanking > 0)
        {
          if (lo == 0 && (uint64_t)flanking > from) from = 1;   /* sic: ram_extend.c:729-730 */
          else from -= (uint64_t)flanking;
          if (to + (uint64_t)flanking > hi) to = hi;
          else to += (uint64_t)flanking;
          fprintf(fp_fa, ">%s:%ld-%ld_%c  n=%ld,anchor_range=%ld-%ld,extended_left=%d,extended_right=%d,len=%d,flanking=%d,score=%d\n",
                  ident, (long)(off + from - lo + 1), (long)(off + to - lo + 1), orient, x, (long)(s->leftSeqPos - lo + 1),
                  (long)(s->rightSeqPos - lo + 1), s->leftExtensionLen, s->rightExtensionLen, ext_len, flanking, s->score);
        }
        else
          fprintf(fp_fa, ">%s:%ld-%ld_%c  n=%ld,anchor_range=%ld-%ld,extended_left=%d,extended_right=%d,len=%d,score=%d\n",
                  ident, (long)(off + from - lo + 1), (long)(off + to - lo + 1), orient, x, (long)(s->leftSeqPos - lo + 1),
                  (long)(s->rightSeqPos - lo + 1), s->leftExtensionLen, s->rightExtensionLen, ext_len, s->score);
        /* sequence line: one buffer + one fwrite instead of a fprintf per base */
        size_t cnt = 0;
        if (to >= from)
        {
          const size_t len = (size_t)(to - from + 1);
          char *buf = (char *)malloc(len + 1);
          const char *codes = lib->sequence ? lib->sequence + from : NULL;
          char *tmpc = NULL;
          if (!codes)                   /* packed library: decode just this stretch */
          {
            tmpc = (char *)malloc(len + 1);
            const ramx_packed_library *pl = ramx_packed_of(lib);
            if (!pl || ramx_packed_decode(pl, from, len, tmpc) != RAMX_OK) { fprintf(stderr, "RAMExtend(ramx): cannot read %zu bases at %ld of the packed library\n", len, (long)from); exit(1); }
            codes = tmpc;
          }
          if (orient == '-')
            for (size_t j = len; j-- > 0;) buf[cnt++] = code_to_char(code_compl(codes[j]));
          else
            for (size_t j = 0; j < len; j++) buf[cnt++] = code_to_char(codes[j]);
          fwrite(buf, 1, cnt, fp_fa);
          free(buf); free(tmpc);
        }
        else if (orient == '-')
        {
          /* the reference's do/while emits one base even for an inverted interval */
          fputc(code_to_char(code_compl(ramx_lib_code(lib, to))), fp_fa);
          cnt = 1;
        }
        fputc('\n', fp_fa);
        if (cnt == 0) { fprintf(stderr, "Error: No sequence emitted for %s:%ld-%ld_%c\n", ident, (long)from, (long)to, orient); exit(1); }
      }
      }
}

/* consensus records, report table, -cons / -outtsv / -outfa: reference ram_extend.c:515-781 */
static void write_results(const struct cli_opts *o, struct coreAlignment *cores, struct sequenceLibrary *lib, const char *master,
                          int rightbp, int leftbp, const char *cons_file, const char *outtsv, const char *outfa)
{
  const int L = o->L, l = 1, flanking = o->flanking;
  const long masterend = (long)L + l + rightbp;
  const long masterstart = (long)L - leftbp;
  if (rightbp > 0 || leftbp > 0)
  {
    FILE *fp = NULL, *fp_fa = NULL;
    if (leftbp > 0) { printf(">left-extension\n"); write_wrapped(stdout, master, (uint64_t)masterstart, (uint64_t)L, (uint64_t)masterstart); }
    if (rightbp > 0) { printf(">right-extension\n"); write_wrapped(stdout, master, (uint64_t)L + l, (uint64_t)masterend, (uint64_t)masterstart); }
    if (cons_file != NULL)
    {
      if ((fp = fopen(cons_file, "w")) == NULL) { fprintf(stderr, "Could not open input file %s\n", cons_file); exit(1); }
      if (leftbp > 0) { fprintf(fp, ">left-extension %d bp\n", leftbp); write_wrapped(fp, master, (uint64_t)masterstart, (uint64_t)L, (uint64_t)masterstart); }
      if (rightbp > 0) { fprintf(fp, ">right-extension %d bp\n", rightbp); write_wrapped(fp, master, (uint64_t)L + l, (uint64_t)masterend, (uint64_t)masterstart); }
      fclose(fp);   /* the reference only closes it inside the right-extension branch (ram_extend.c:583) */
      fp = NULL;
    }
    if (outtsv != NULL && (fp = fopen(outtsv, "w")) == NULL) { fprintf(stderr, "Could not create the TSV output file %s\n", outtsv); exit(1); }
    if (outfa != NULL && (fp_fa = fopen(outfa, "w")) == NULL) { fprintf(stderr, "Could not create the FASTA output file %s\n", outfa); exit(1); }

    printf("\n\nExtended Sequences Report:\n");
    printf("  *** Extended sequences are in 1-based, fully closed coordinates ***\n");
    printf("SEQID  SEQSTART SEQEND ORIENT  EXTENSION_DETAILS\n");
    {
      int cnt = 0;
      for (struct coreAlignment *s = cores; s != NULL; s = s->next) cnt++;
      struct coreAlignment **arr = (struct coreAlignment **)malloc(sizeof(*arr) * (size_t)(cnt ? cnt : 1));
      cnt = 0;
      for (struct coreAlignment *s = cores; s != NULL; s = s->next) arr[cnt++] = s;
      struct results_ctx ctx;
      ctx.arr = arr; ctx.lib = lib; ctx.flanking = flanking;
      FILE *outs[3] = { stdout, fp, fp_fa };
      ramx_parallel_chunks(cnt, 3, outs, results_rows, &ctx);   /* formatted chunk by chunk on the host's cores, written in order */
      free(arr);
    }
    if (fp != NULL) fclose(fp);
    if (fp_fa != NULL) fclose(fp_fa);
  }

}


/*
 * -batch <list>: many families in one process and ONE launch per direction (no counterpart in the reference, whose
 * wrapper util/extend-stk.pl:242-371 starts one RAMExtend per family).  Every non-empty, non-# line of <list> is
 *     ranges.tsv <TAB> log <TAB> cons.fa <TAB> out.tsv <TAB> out.fa [<TAB> profile.tsv [<TAB> aln.a2m]]   ("-" = not wanted)
 * All other options (-twobit, -L, -bandwidth, -matrix ...) are shared.  For every family the log file receives
 * exactly what a stand-alone run prints on stdout, and the three output files are what -cons/-outtsv/-outfa give.
 */
struct batch_item
{
  char *ranges, *log, *cons, *tsv, *fa, *profile, *aln, *pileup, *refined, *copies, *linkage, *subfam, *tsd, *cpg, *period;
  struct coreAlignment *cores;
  struct sequenceLibrary *lib;
  int N, rightbp, leftbp;
  char *master;
};

static void to_log(const char *path, int truncate)
{
  fflush(stdout);
  int fd = open(path, O_WRONLY | O_CREAT | (truncate ? O_TRUNC : O_APPEND), 0644);
  if (fd < 0) { fprintf(stderr, "Could not open log file %s\n", path); exit(1); }
  dup2(fd, 1);
  close(fd);
}

static char *field_or_null(char *s) { return (s == NULL || s[0] == 0 || strcmp(s, "-") == 0) ? NULL : s; }

/*
 * -outprofile <file>: the per-column support profile of both extensions (include/ramx.h, ramx_set_profile_sink) as a TSV, the
 * right direction's rows first.  score is the reference's curr_extension_score (ram_extend.c:1064-1086), new_max its
 * MINIMPROVEMENT rule (:1194-1201), kept says whether the column is part of the returned extension.
 */
struct profile_out
{
  const char *single;          /* one family: its file */
  char *const *per_family;     /* -batch: the sixth field of every line (NULL: not wanted) */
  int minimprovement;
};
static const char k_profile_header[] =
  "dir\trow\tbase\ttotal_A\ttotal_C\ttotal_G\ttotal_T\tscore\tmargin\tn_flanks\tn_uncapped\tn_new_high\tn_out_of_seq\tnew_max\tkept\n";
static void profile_start(const char *path)
{
  FILE *fp = fopen(path, "w");
  if (!fp) { fprintf(stderr, "Could not create the profile file %s\n", path); exit(1); }
  fputs(k_profile_header, fp);
  fclose(fp);
}
static void profile_sink(const ramx_profile *pr, void *user)
{
  const struct profile_out *po = (const struct profile_out *)user;
  const char *path = po->per_family ? po->per_family[pr->family] : po->single;
  if (!path) return;
  FILE *fp = fopen(path, "a");
  if (!fp) { fprintf(stderr, "Could not append to the profile file %s\n", path); exit(1); }
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
    const int new_max = score >= max_ext + (long long)abs(max_row - r) * po->minimprovement;
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
struct aln_rec { int core, end_row, start, end, score; char *body; };
struct aln_block { int have, ret, n; char *cons; struct aln_rec *rec; };
struct aln_family { const char *path; struct sequenceLibrary *lib; struct aln_block blk[2]; };
struct aln_out { struct aln_family *fam; };

static void reverse_chars(char *s, size_t n)
{
  for (size_t i = 0; i + 1 < n - i; i++) { const char t = s[i]; s[i] = s[n - 1 - i]; s[n - 1 - i] = t; }
}

static void aln_sink(const ramx_alignment *al, void *user)
{
  struct aln_family *af = &((const struct aln_out *)user)->fam[al->family];
  if (!af->path) return;
  struct aln_block *b = &af->blk[al->direction ? 1 : 0];
  const int rows = al->rows;
  b->have = 1; b->ret = rows; b->n = al->n_flanks;
  b->cons = (char *)malloc((size_t)rows + 1);
  for (int r = 0; r < rows; r++) b->cons[r] = code_to_char(al->cons[r]);
  b->cons[rows] = 0;
  if (!al->direction) reverse_chars(b->cons, (size_t)rows);
  b->rec = (struct aln_rec *)calloc((size_t)(al->n_flanks > 0 ? al->n_flanks : 1), sizeof(struct aln_rec));
  const uint64_t lib_len = af->lib->length;
  for (int i = 0; i < al->n_flanks; i++)
  {
    const ramx_aln_end *e = &al->ends[i];
    const ramx_flank *f = &al->flanks[i];
    struct aln_rec *rc = &b->rec[i];
    rc->core = al->core_index[i]; rc->end_row = e->end_row; rc->start = e->start_idx; rc->end = e->end_idx; rc->score = e->score;
    const long consumed = e->end_row >= 0 ? (long)e->end_idx - e->start_idx + 1 : 0;
    char *body = (char *)malloc((size_t)rows + (size_t)(consumed > 0 ? consumed : 0) + 1);
    size_t k = 0;
    long t = e->start_idx;
#define ALN_BASE(upper) do { \
      const int64_t at_ = f->start + (int64_t)f->step * t; \
      int code_ = (at_ >= 0 && (uint64_t)at_ < lib_len) ? ramx_lib_code(af->lib, (uint64_t)at_) : RAMX_SYM_N; \
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
    rc->body = body;
  }
}

/* the record id -outfa gives a core (results_rows, above): ident:from-to_orient over the extended range plus the flanking */
static void aln_record_id(char *buf, size_t n, const struct coreAlignment *s, const struct sequenceLibrary *lib, int flanking)
{
  const int si = s->seqIdx;
  const uint64_t lo = si > 0 ? lib->boundaries[si - 1] : 0;
  const uint64_t hi = lib->boundaries[si];
  const uint64_t off = (lib->offsets != NULL && lib->offsets[si] > 0) ? lib->offsets[si] : 0;
  uint64_t from = s->leftSeqPos - (uint64_t)s->leftExtensionLen, to = s->rightSeqPos + (uint64_t)s->rightExtensionLen;
  if (s->orient) { to = s->leftSeqPos + (uint64_t)s->leftExtensionLen; from = s->rightSeqPos - (uint64_t)s->rightExtensionLen; }
  if (flanking > 0)
  {
    if (lo == 0 && (uint64_t)flanking > from) from = 1;
    else from -= (uint64_t)flanking;
    if (to + (uint64_t)flanking > hi) to = hi;
    else to += (uint64_t)flanking;
  }
  snprintf(buf, n, "%s:%ld-%ld_%c", lib->identifiers[si], (long)(off + from - lo + 1), (long)(off + to - lo + 1), s->orient ? '-' : '+');
}

/* after both directions: the file, then the buffers are released */
static void aln_write(struct aln_family *af, struct coreAlignment *cores, int flanking)
{
  if (!af->path) return;
  FILE *fp = fopen(af->path, "w");
  if (!fp) { fprintf(stderr, "Could not create the alignment file %s\n", af->path); exit(1); }
  int cnt = 0;
  for (struct coreAlignment *s = cores; s != NULL; s = s->next) cnt++;
  struct coreAlignment **arr = (struct coreAlignment **)malloc(sizeof(*arr) * (size_t)(cnt ? cnt : 1));
  cnt = 0;
  for (struct coreAlignment *s = cores; s != NULL; s = s->next) arr[cnt++] = s;
  for (int dir = 1; dir >= 0; dir--)
  {
    struct aln_block *b = &af->blk[dir];
    if (!b->have) continue;
    fprintf(fp, ">%s-extension %d bp\n%s\n", dir ? "right" : "left", b->ret, b->cons);
    for (int i = 0; i < b->n; i++)
    {
      const struct aln_rec *rc = &b->rec[i];
      char id[1024];
      if (rc->core < 0 || rc->core >= cnt) { fprintf(stderr, "RAMExtend(ramx): alignment record of an unknown core %d\n", rc->core); exit(1); }
      aln_record_id(id, sizeof(id), arr[rc->core], af->lib, flanking);
      fprintf(fp, ">%s  dir=%s,end_row=%d,start=%d,end=%d,score=%d\n%s\n", id, dir ? "right" : "left", rc->end_row, rc->start, rc->end,
              rc->score, rc->body);
      free(rc->body);
    }
    free(b->rec); free(b->cons);
    memset(b, 0, sizeof(*b));
  }
  free(arr);
  fclose(fp);
}

/*
 * -outpileup <file>: the pileup of both extensions' kept consensus (include/ramx.h, ramx_col_pileup, ramx_set_refine_sink) as a
 * TSV, one line per kept column, the right direction first.  -outrefined <file>: the kept consensus refined over at most
 * -refine <n> replays (default 10) as FASTA, ">right-extension-refined <n> bp replays=<k> converged=<0|1>" and the left one,
 * which reads as -cons writes it; nothing is wrapped.  With both files the pileup of a refined consensus that differs from the
 * kept one follows the kept one's block as right-refined / left-refined lines.
 */
struct refine_family { const char *pileup, *refined; int have[2], rows[2], replays[2], converged[2]; char *seq[2]; };
struct refine_out { struct refine_family *fam; };
static const char k_pileup_header[] =
  "dir\trow\tbase\tcover\tA\tC\tG\tT\tN\tdel\tins_open\tins_long\tins_bases"
  "\ti0_A\ti0_C\ti0_G\ti0_T\ti0_N\ti1_A\ti1_C\ti1_G\ti1_T\ti1_N\ti2_A\ti2_C\ti2_G\ti2_T\ti2_N\ti3_A\ti3_C\ti3_G\ti3_T\ti3_N\n";
static void pileup_start(const char *path)
{
  FILE *fp = fopen(path, "w");
  if (!fp) { fprintf(stderr, "Could not create the pileup file %s\n", path); exit(1); }
  fputs(k_pileup_header, fp);
  fclose(fp);
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
  struct refine_family *f = &((const struct refine_out *)user)->fam[rf->family];
  const int d = rf->direction ? 1 : 0;
  if (f->pileup)
  {
    FILE *fp = fopen(f->pileup, "a");
    if (!fp) { fprintf(stderr, "Could not append to the pileup file %s\n", f->pileup); exit(1); }
    pileup_block(fp, d ? "right" : "left", rf->cols, rf->rows);
    if (f->refined && rf->replays > 1) pileup_block(fp, d ? "right-refined" : "left-refined", rf->refined_cols, rf->refined_rows);
    fclose(fp);
  }
  if (f->refined)
  {
    const int n = rf->refined_rows;
    f->have[d] = 1; f->rows[d] = n; f->replays[d] = rf->replays; f->converged[d] = rf->converged;
    f->seq[d] = (char *)malloc((size_t)n + 1);
    for (int r = 0; r < n; r++) f->seq[d][r] = code_to_char(rf->refined_cons[d ? r : n - 1 - r]);
    f->seq[d][n] = 0;
  }
}
static void refined_write(struct refine_family *f)
{
  if (!f->refined) return;
  FILE *fp = fopen(f->refined, "w");
  if (!fp) { fprintf(stderr, "Could not create the refined consensus file %s\n", f->refined); exit(1); }
  for (int d = 1; d >= 0; d--)
  {
    if (!f->have[d]) continue;
    fprintf(fp, ">%s-extension-refined %d bp replays=%d converged=%d\n%s\n", d ? "right" : "left", f->rows[d], f->replays[d], f->converged[d], f->seq[d]);
    free(f->seq[d]);
    f->seq[d] = NULL; f->have[d] = 0;
  }
  fclose(fp);
}

/*
 * -outcpg <file>: the kept consensus refined over at most -refine <n> replays with the CpG-aware re-call (include/ramx.h,
 * ramx_recall_cpg, ramx_set_cpg_sink; -cpgscore <n> is its cpg_ts, default 0) as FASTA, ">right-extension-cpg <n> bp replays=<k>
 * converged=<0|1> cpg=<pairs called CG>" and the left one, which reads as -cons writes it.  -outdinuc <file>: the dinucleotide
 * pileup of that result (ramx_col_dinuc) as a TSV, one line per column of the result, the right direction first; the rows are
 * the device's (a left extension's run outward from the core), xy counts class x in row and class y in row + 1.
 */
struct cpg_family { const char *fasta, *dinuc; int have[2], rows[2], replays[2], converged[2], n_cpg[2]; char *seq[2]; };
struct cpg_out { struct cpg_family *fam; };
static void dinuc_start(const char *path)
{
  FILE *fp = fopen(path, "w");
  if (!fp) { fprintf(stderr, "Could not create the dinucleotide file %s\n", path); exit(1); }
  fputs("dir\trow\tbase\tnext\tboth\tadjacent\tsplit\tgapped", fp);
  for (int x = 0; x < 5; x++)
    for (int y = 0; y < 5; y++) fprintf(fp, "\t%c%c", "ACGTN"[x], "ACGTN"[y]);
  fputc('\n', fp);
  fclose(fp);
}
static void cpg_sink(const ramx_cpg_refinement *cr, void *user)
{
  struct cpg_family *f = &((const struct cpg_out *)user)->fam[cr->family];
  const int d = cr->direction ? 1 : 0, n = cr->refined_rows;
  if (f->dinuc)
  {
    FILE *fp = fopen(f->dinuc, "a");
    if (!fp) { fprintf(stderr, "Could not append to the dinucleotide file %s\n", f->dinuc); exit(1); }
    for (int r = 0; r < n; r++)
    {
      const ramx_col_dinuc *c = &cr->refined_di[r];
      fprintf(fp, "%s\t%d\t%c\t%c\t%d\t%d\t%d\t%d", d ? "right" : "left", r, code_to_char(c->base), c->next < 0 ? '-' : code_to_char(c->next),
              c->both, c->adjacent, c->split, c->gapped);
      for (int x = 0; x < 5; x++)
        for (int y = 0; y < 5; y++) fprintf(fp, "\t%d", c->di[x][y]);
      fputc('\n', fp);
    }
    fclose(fp);
  }
  if (f->fasta)
  {
    f->have[d] = 1; f->rows[d] = n; f->replays[d] = cr->replays; f->converged[d] = cr->converged; f->n_cpg[d] = cr->n_cpg;
    f->seq[d] = (char *)malloc((size_t)n + 1);
    for (int r = 0; r < n; r++) f->seq[d][r] = code_to_char(cr->refined_cons[d ? r : n - 1 - r]);
    f->seq[d][n] = 0;
  }
}
static void cpg_write(struct cpg_family *f)
{
  if (!f->fasta) return;
  FILE *fp = fopen(f->fasta, "w");
  if (!fp) { fprintf(stderr, "Could not create the CpG-aware consensus file %s\n", f->fasta); exit(1); }
  for (int d = 1; d >= 0; d--)
  {
    if (!f->have[d]) continue;
    fprintf(fp, ">%s-extension-cpg %d bp replays=%d converged=%d cpg=%d\n%s\n", d ? "right" : "left", f->rows[d], f->replays[d], f->converged[d],
            f->n_cpg[d], f->seq[d]);
    free(f->seq[d]);
    f->seq[d] = NULL; f->have[d] = 0;
  }
  fclose(fp);
}

/*
 * -outcopies <file>: every extendable core's divergence from the kept consensus of both extensions (include/ramx.h,
 * ramx_copy_stats, ramx_set_copies_sink) as a TSV, the right block first: one line per extendable core in flank order, named as
 * -outaln names it, then one summary line "#<dir> copies= used= kimura=" with the family's mean Kimura divergence over the
 * copies that have one (min_sites = 1).  The names need both directions' lengths, so the sink keeps the records and the file
 * is written with the other results.
 */
struct copies_rec { int core, end_row, start, end; ramx_copy_stats st; };
struct copies_block { int have, n; struct copies_rec *rec; };
struct copies_family { const char *path; struct sequenceLibrary *lib; struct copies_block blk[2]; };
struct copies_out { struct copies_family *fam; };
static const char k_copies_header[] =
  "dir\tcopy\tend_row\tstart\tend\tscore\tcols\tmatch\tts\ttv\tn\tdel\tdel_open\tins\tins_open\tcpg_cols\tcpg_ts\tkimura\n";

static void copies_sink(const ramx_copies *cp, void *user)
{
  struct copies_family *cf = &((const struct copies_out *)user)->fam[cp->family];
  if (!cf->path) return;
  struct copies_block *b = &cf->blk[cp->direction ? 1 : 0];
  b->have = 1; b->n = cp->n_flanks;
  b->rec = (struct copies_rec *)calloc((size_t)(cp->n_flanks > 0 ? cp->n_flanks : 1), sizeof(struct copies_rec));
  for (int i = 0; i < cp->n_flanks; i++)
  {
    const ramx_aln_end *e = &cp->ends[i];
    struct copies_rec *rc = &b->rec[i];
    rc->core = cp->core_index[i]; rc->end_row = e->end_row; rc->start = e->start_idx; rc->end = e->end_idx; rc->st = cp->stats[i];
  }
}

/* after both directions: the file, then the buffers are released */
static void copies_write(struct copies_family *cf, struct coreAlignment *cores, int flanking)
{
  if (!cf->path) return;
  FILE *fp = fopen(cf->path, "w");
  if (!fp) { fprintf(stderr, "Could not create the copies file %s\n", cf->path); exit(1); }
  fputs(k_copies_header, fp);
  int cnt = 0;
  for (struct coreAlignment *s = cores; s != NULL; s = s->next) cnt++;
  struct coreAlignment **arr = (struct coreAlignment **)malloc(sizeof(*arr) * (size_t)(cnt ? cnt : 1));
  cnt = 0;
  for (struct coreAlignment *s = cores; s != NULL; s = s->next) arr[cnt++] = s;
  for (int dir = 1; dir >= 0; dir--)
  {
    struct copies_block *b = &cf->blk[dir];
    if (!b->have) continue;
    const char *tag = dir ? "right" : "left";
    ramx_copy_stats *all = (ramx_copy_stats *)malloc(sizeof(ramx_copy_stats) * (size_t)(b->n > 0 ? b->n : 1));
    for (int i = 0; i < b->n; i++)
    {
      const struct copies_rec *rc = &b->rec[i];
      const ramx_copy_stats *t = &rc->st;
      char id[1024];
      if (rc->core < 0 || rc->core >= cnt) { fprintf(stderr, "RAMExtend(ramx): copy record of an unknown core %d\n", rc->core); exit(1); }
      aln_record_id(id, sizeof(id), arr[rc->core], cf->lib, flanking);
      fprintf(fp, "%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t", tag, id, rc->end_row, rc->start, rc->end, t->score,
              t->cols, t->match, t->ts, t->tv, t->n_match, t->del, t->del_open, t->ins, t->ins_open, t->cpg_cols, t->cpg_ts);
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
  free(arr);
  fclose(fp);
}

/*
 * -outlinkage <file>: the co-segregation of the variants of both extensions (include/ramx.h, ramx_set_linkage_sink,
 * ramx_link_pairs) as a TSV, the right block first: one line per pair of variants on different columns whose -log10 p reaches
 * -linkscore, in (p, q) order, then one summary line "#<dir> variants= pairs= linked=": the variants selected, the pairs tested
 * and the pairs written.
 */
struct linkage_block { int have, P; ramx_plane *planes; int32_t *co; };
struct linkage_family { const char *path; struct linkage_block blk[2]; };
struct linkage_out { struct linkage_family *fam; };
static const char k_linkage_header[] = "dir\trow_a\tvar_a\tcount_a\trow_b\tvar_b\tcount_b\tn\tn_a\tn_b\tn_ab\texpected\tmlog10p\n";

static void linkage_sink(const ramx_linkage *lk, void *user)
{
  struct linkage_family *lf = &((const struct linkage_out *)user)->fam[lk->family];
  if (!lf->path) return;
  struct linkage_block *b = &lf->blk[lk->direction ? 1 : 0];
  const size_t P = (size_t)lk->n_planes;
  b->have = 1; b->P = lk->n_planes;
  b->planes = (ramx_plane *)malloc(sizeof(ramx_plane) * (P ? P : 1));
  b->co = (int32_t *)malloc(sizeof(int32_t) * (P ? P * P : 1));
  if (P) { memcpy(b->planes, lk->planes, sizeof(ramx_plane) * P); memcpy(b->co, lk->co, sizeof(int32_t) * P * P); }
}

/* after both directions: the file, then the buffers are released */
static void linkage_write(struct linkage_family *lf, int min_score)
{
  static const char *const var_name[8] = { "A", "C", "G", "T", "N", "del", "cover", "ins" };
  if (!lf->path) return;
  FILE *fp = fopen(lf->path, "w");
  if (!fp) { fprintf(stderr, "Could not create the linkage file %s\n", lf->path); exit(1); }
  fputs(k_linkage_header, fp);
  for (int dir = 1; dir >= 0; dir--)
  {
    struct linkage_block *b = &lf->blk[dir];
    if (!b->have) continue;
    const char *tag = dir ? "right" : "left";
    const int32_t P = b->P;
    /* the pairs tested: every pair scores at least 0 */
    const int32_t tested = ramx_link_pairs(b->planes, P, b->co, 0.0, NULL, 0);
    ramx_link *ln = (ramx_link *)malloc(sizeof(ramx_link) * (size_t)(tested > 0 ? tested : 1));
    const int32_t linked = ramx_link_pairs(b->planes, P, b->co, (double)min_score, ln, tested);
    int variants = 0;
    for (int32_t i = 0; i < P; i++) variants += b->planes[i].cls != RAMX_PLANE_COVER;
    for (int32_t i = 0; i < linked; i++)
    {
      const ramx_link *l = &ln[i];
      const ramx_plane *a = &b->planes[l->p], *c = &b->planes[l->q];
      fprintf(fp, "%s\t%d\t%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%.4f\t%.4f\n", tag, a->row, var_name[a->cls & 7],
              b->co[(size_t)l->p * P + l->p], c->row, var_name[c->cls & 7], b->co[(size_t)l->q * P + l->q], l->n, l->n_p, l->n_q, l->n_pq,
              l->expected, l->mlog10p);
    }
    fprintf(fp, "#%s\tvariants=%d\tpairs=%d\tlinked=%d\n", tag, variants, (int)tested, (int)linked);
    free(ln); free(b->planes); free(b->co);
    memset(b, 0, sizeof(*b));
  }
  fclose(fp);
}

/*
 * -outsubfam <file>: the copies of both extensions split into subfamilies (include/ramx.h, ramx_set_subfam_sink) as a TSV, the
 * right block first.  Per group a line "group": direction, group, size, the assignments made and whether they converged, the
 * group's pattern as a list of row:variant ("-": none), and -- for a group of at least -subfammin copies -- the length of its
 * refined consensus, the replays, whether those converged, and the consensus in reading order (else NA NA NA -).  After it one
 * line "copy" per copy of the group in flank order: the -outfa record name, its label and its distance to every pattern.  The
 * names need both directions' lengths, so the sink keeps the records and the file is written with the other results.
 */
struct subfam_block { int have, n, K, iterations, converged; int32_t *core, *labels, *dist, *size; char **pattern, **cons; int *rows, *replays, *conv; };
struct subfam_family { const char *path; struct sequenceLibrary *lib; struct subfam_block blk[2]; };
struct subfam_out { struct subfam_family *fam; };
static const char k_subfam_header[] =
  "#group\tdir\tgroup\tsize\titerations\tconverged\tpattern\trefined_bp\treplays\trefined_converged\tconsensus\n"
  "#copy\tdir\tcopy\tlabel\tdistances\n";

static void subfam_sink(const ramx_subfamilies *sf, void *user)
{
  static const char *const var_name[8] = { "A", "C", "G", "T", "N", "del", "cover", "ins" };
  struct subfam_family *f = &((const struct subfam_out *)user)->fam[sf->family];
  if (!f->path) return;
  struct subfam_block *b = &f->blk[sf->direction ? 1 : 0];
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
      if (sf->patterns[(size_t)v * K + (size_t)k]) w += sprintf(w, "%s%d:%s", w == txt ? "" : ",", sf->planes[i].row, var_name[sf->planes[i].cls & 7]);
      v++;
    }
    if (w == txt) *w++ = '-';
    *w = 0;
    b->pattern[k] = txt;
  }
  for (int g = 0; g < sf->n_groups; g++)
  {
    const ramx_subfam_group *gr = &sf->groups[g];
    const int rn = gr->refined_rows, d = sf->direction ? 1 : 0;
    char *seq = (char *)malloc((size_t)rn + 2);
    for (int r = 0; r < rn; r++) seq[r] = code_to_char(gr->refined_cons[d ? r : rn - 1 - r]);
    if (rn == 0) { seq[0] = '-'; seq[1] = 0; } else seq[rn] = 0;
    b->cons[gr->group] = seq; b->rows[gr->group] = rn; b->replays[gr->group] = gr->replays; b->conv[gr->group] = gr->converged;
  }
}

/* after both directions: the file, then the buffers are released */
static void subfam_write(struct subfam_family *f, struct coreAlignment *cores, int flanking)
{
  if (!f->path) return;
  FILE *fp = fopen(f->path, "w");
  if (!fp) { fprintf(stderr, "Could not create the subfamily file %s\n", f->path); exit(1); }
  fputs(k_subfam_header, fp);
  int cnt = 0;
  for (struct coreAlignment *s = cores; s != NULL; s = s->next) cnt++;
  struct coreAlignment **arr = (struct coreAlignment **)malloc(sizeof(*arr) * (size_t)(cnt ? cnt : 1));
  cnt = 0;
  for (struct coreAlignment *s = cores; s != NULL; s = s->next) arr[cnt++] = s;
  for (int dir = 1; dir >= 0; dir--)
  {
    struct subfam_block *b = &f->blk[dir];
    if (!b->have) continue;
    const char *tag = dir ? "right" : "left";
    for (int k = 0; k < b->K; k++)
    {
      fprintf(fp, "group\t%s\t%d\t%d\t%d\t%d\t%s\t", tag, k, b->size[k], b->iterations, b->converged, b->pattern[k]);
      if (b->cons[k]) fprintf(fp, "%d\t%d\t%d\t%s\n", b->rows[k], b->replays[k], b->conv[k], b->cons[k]);
      else fputs("NA\tNA\tNA\t-\n", fp);
      for (int i = 0; i < b->n; i++)
      {
        if (b->labels[i] != k) continue;
        char id[1024];
        if (b->core[i] < 0 || b->core[i] >= cnt) { fprintf(stderr, "RAMExtend(ramx): subfamily record of an unknown core %d\n", b->core[i]); exit(1); }
        aln_record_id(id, sizeof(id), arr[b->core[i]], f->lib, flanking);
        fprintf(fp, "copy\t%s\t%s\t%d", tag, id, b->labels[i]);
        for (int j = 0; j < b->K; j++) fprintf(fp, "\t%d", b->dist[(size_t)i * b->K + j]);
        fputc('\n', fp);
      }
      free(b->pattern[k]); free(b->cons[k]);
    }
    free(b->core); free(b->labels); free(b->dist); free(b->size); free(b->pattern); free(b->cons); free(b->rows);
    memset(b, 0, sizeof(*b));
  }
  free(arr);
  fclose(fp);
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
static const char k_tsd_header[] = "core\tseqid\tstart\tend\tstrand\text_left\text_right\ttsd_len\tmismatches\tshift_left\tshift_right\tleft_word\tright_word\n";

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

static void tsd_write(const char *path, const ramx_tsd_params *tp, struct coreAlignment *cores, struct sequenceLibrary *lib, const char *master,
                      int L, int rightbp, int leftbp, const ramx_tsd *rec, int n)
{
  FILE *fp = fopen(path, "w");
  if (!fp) { fprintf(stderr, "Could not create the target-site duplication file %s\n", path); exit(1); }
  const int l = 1, nl = leftbp > 0 ? leftbp : 0, nr = rightbp > 0 ? rightbp : 0;
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
  fputs(k_tsd_header, fp);
  int x = 0;
  for (struct coreAlignment *s = cores; s != NULL && x < n; s = s->next, x++)
  {
    const int si = s->seqIdx;
    const uint64_t lo = si > 0 ? lib->boundaries[si - 1] : 0;
    const uint64_t off = (lib->offsets != NULL && lib->offsets[si] > 0) ? lib->offsets[si] : 0;
    /* the copy's ends in the library, and as -outtsv prints them */
    const int64_t e_lo = s->orient ? (int64_t)s->rightSeqPos - s->rightExtensionLen : (int64_t)s->leftSeqPos - s->leftExtensionLen;
    const int64_t e_hi = s->orient ? (int64_t)s->leftSeqPos + s->leftExtensionLen : (int64_t)s->rightSeqPos + s->rightExtensionLen;
    char lbuf[32], rbuf[32], lw[33] = "-", rw[33] = "-";
    if (s->leftExtendable) snprintf(lbuf, sizeof(lbuf), "%d", s->leftExtensionLen); else strcpy(lbuf, "*");
    if (s->rightExtendable) snprintf(rbuf, sizeof(rbuf), "%d", s->rightExtensionLen); else strcpy(rbuf, "*");
    const ramx_tsd *t = &rec[x];
    if (t->k > 0)
    {
      tsd_word(lw, lib, s, e_lo + t->dl - t->k, t->k);
      tsd_word(rw, lib, s, e_hi + 1 + t->dr, t->k);
    }
    fprintf(fp, "%d\t%s\t%ld\t%ld\t%c\t%s\t%s\t%d\t%d\t%d\t%d\t%s\t%s\n", x, lib->identifiers[si], (long)((int64_t)off + e_lo - (int64_t)lo + 1),
            (long)((int64_t)off + e_hi - (int64_t)lo + 1), s->orient ? '-' : '+', lbuf, rbuf, t->k, t->mm, t->dl, t->dr, lw, rw);
  }
  fclose(fp);
}

/*
 * -outperiod <file>: the tandem periodicity of the extended copies (include/ramx.h, ramx_period) as a TSV.  "#period" carries the
 * parameters; per part -- left, right, and whole with -periodwhole -- "#part" carries what the family's records say together
 * and "#consensus" the record of that direction's kept consensus in reading order (whole: the left one followed by the right
 * one).  Then one line per core and part, the cores in list order: named and placed as -outtsv places the copy, the part and its
 * length, the record, the periodic region in the coordinates of start and end, and the first bases of the region as the library
 * has them on its forward strand ("-" without a tract).  Like -outtsd this is no sink: it is computed when both directions are done.
 */
static const char *const k_period_part[3] = { "left", "right", "whole" };
static const char k_period_header[] = "core\tseqid\tstart\tend\tstrand\tpart\tlength\tperiod\tunits\tscore\tregion_start\tregion_end\tagree\tdisagree\tunit\n";

/* rec[w] / segs[w]: the n records and segments of part w (w = 2 only with whole) */
static void period_write(const char *path, const ramx_period_params *pp, int whole, struct coreAlignment *cores, struct sequenceLibrary *lib,
                         const char *master, int L, int rightbp, int leftbp, ramx_period *const rec[3], ramx_period_seg *const segs[3], int n)
{
  FILE *fp = fopen(path, "w");
  if (!fp) { fprintf(stderr, "Could not create the periodicity file %s\n", path); exit(1); }
  const int l = 1, nl = leftbp > 0 ? leftbp : 0, nr = rightbp > 0 ? rightbp : 0, parts = whole ? 3 : 2;
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
    fprintf(fp, "#part\tpart=%s\tn=%d\tn_tract=%d\tn_mono=%d\tn_simple=%d\tn_tandem=%d\tat_lo=%d\tat_hi=%d\tmode=%d\tmode_count=%d\n", k_period_part[w],
            h.n, h.n_tract, h.n_mono, h.n_simple, h.n_tandem, h.at_lo, h.at_hi, h.mode, h.mode_count);
    fprintf(fp, "#consensus\tpart=%s\tlength=%d\tperiod=%d\tscore=%d\tstart=%d\tend=%d\tagree=%d\tdisagree=%d\n", k_period_part[w], cn, cr.period,
            cr.score, cr.start, cr.end, cr.agree, cr.disagree);
  }
  free(cons);
  fputs(k_period_header, fp);
  int x = 0;
  for (struct coreAlignment *s = cores; s != NULL && x < n; s = s->next, x++)
  {
    const int si = s->seqIdx;
    const uint64_t lo = si > 0 ? lib->boundaries[si - 1] : 0;
    const uint64_t off = (lib->offsets != NULL && lib->offsets[si] > 0) ? lib->offsets[si] : 0;
    /* the copy's ends in the library, and as -outtsv prints them */
    const int64_t e_lo = s->orient ? (int64_t)s->rightSeqPos - s->rightExtensionLen : (int64_t)s->leftSeqPos - s->leftExtensionLen;
    const int64_t e_hi = s->orient ? (int64_t)s->leftSeqPos + s->leftExtensionLen : (int64_t)s->rightSeqPos + s->rightExtensionLen;
    const int64_t shift = (int64_t)off - (int64_t)lo + 1;
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
      fprintf(fp, "%d\t%s\t%ld\t%ld\t%c\t%s\t%ld\t%d\t%.2f\t%d\t%ld\t%ld\t%d\t%d\t%s\n", x, lib->identifiers[si], (long)(e_lo + shift), (long)(e_hi + shift),
              s->orient ? '-' : '+', k_period_part[w], (long)(g->hi + 1 - g->lo), t->period,
              t->period > 0 ? (double)(t->end - t->start + 1 + t->period) / (double)t->period : 0.0, t->score,
              t->period > 0 ? (long)(r_lo + shift) : 0L, t->period > 0 ? (long)(r_hi + shift) : 0L, t->agree, t->disagree, unit);
    }
  }
  fclose(fp);
}

/* flat view of a core list for ramx_extend_batch (arrays owned by the caller's arena) */
static void flatten_cores(struct coreAlignment *cores, int N, ramx_flat_cores *fc)
{
  int64_t *i64 = (int64_t *)malloc(sizeof(int64_t) * 4 * (size_t)(N + 1));
  int8_t *i8 = (int8_t *)malloc(3 * (size_t)(N + 1));
  int32_t *i32 = (int32_t *)calloc(3 * (size_t)(N + 1), sizeof(int32_t));
  fc->n = N;
  fc->left_pos = i64; fc->right_pos = i64 + N; fc->lower = i64 + 2 * N; fc->upper = i64 + 3 * N;
  fc->orient = i8; fc->left_ext = i8 + N; fc->right_ext = i8 + 2 * N;
  fc->left_len = i32; fc->right_len = i32 + N; fc->score = i32 + 2 * N;
  int k = 0;
  for (struct coreAlignment *c = cores; c != NULL && k < N; c = c->next, k++)
  {
    i64[k] = (int64_t)c->leftSeqPos; i64[N + k] = (int64_t)c->rightSeqPos;
    i64[2 * N + k] = (int64_t)c->lowerSeqBound; i64[3 * N + k] = (int64_t)c->upperSeqBound;
    i8[k] = c->orient ? 1 : 0; i8[N + k] = c->leftExtendable ? 1 : 0; i8[2 * N + k] = c->rightExtendable ? 1 : 0;
    i32[k] = c->leftExtensionLen; i32[N + k] = c->rightExtensionLen; i32[2 * N + k] = c->score;
  }
}
static void unflatten_results(struct coreAlignment *cores, const ramx_flat_cores *fc)
{
  int k = 0;
  for (struct coreAlignment *c = cores; c != NULL && k < fc->n; c = c->next, k++)
  {
    c->leftExtensionLen = fc->left_len[k]; c->rightExtensionLen = fc->right_len[k]; c->score = fc->score[k];
  }
}
static void free_flat(ramx_flat_cores *fc) { free((void *)fc->left_pos); free((void *)fc->orient); free(fc->left_len); }

/* the lines extend_alignment prints around the loop (ram_extend.c:886-892, 1216-1231) */
static void print_loop_lines(int direction, int N, int verbose, int when_to_stop, int L, const ramx_run_info *info, int before)
{
  if (before)
  {
    if (verbose >= 3) printf(direction ? "extend_alignment(right): Called with %d edges\n" : "extend_alignment(left): Called with %d edges\n", N);
    return;
  }
  if (info->rows_executed > 0 && verbose >= 3)
  {
    const int last = info->rows_executed - 1;
    if (abs(last - (info->ret - 1)) >= when_to_stop)
      printf("Ending...due to row_idx=%d - max_extension_score_row_idx=%d <= -WHEN_TO_STOP=%d\n", last, info->ret - 1, when_to_stop);
  }
  if (info->limit_warning)
    printf(direction ? "WARNING: Extended sequence right to the limit ( L=%d ).\n" : "WARNING: Extended sequence left to the limit ( L=%d ).\n", L);
}

static int run_batch(struct cli_opts *o, time_t t_start)
{
  const int L = o->L, l = 1;
  if (o->outmat != NULL) { fprintf(stderr, "RAMExtend(ramx): -outmat traces one family; it cannot be combined with -batch\n"); exit(1); }
  if (o->outprofile != NULL) { fprintf(stderr, "RAMExtend(ramx): with -batch every family's profile file is the sixth field of its line in the list\n"); exit(1); }
  if (o->outaln != NULL) { fprintf(stderr, "RAMExtend(ramx): with -batch every family's alignment file is the seventh field of its line in the list\n"); exit(1); }
  if (o->outpileup != NULL || o->outrefined != NULL)
  { fprintf(stderr, "RAMExtend(ramx): with -batch every family's pileup file is the eighth field of its line in the list and its refined consensus the ninth\n"); exit(1); }
  if (o->outcopies != NULL) { fprintf(stderr, "RAMExtend(ramx): with -batch every family's copies file is the tenth field of its line in the list\n"); exit(1); }
  if (o->outlinkage != NULL) { fprintf(stderr, "RAMExtend(ramx): with -batch every family's linkage file is the eleventh field of its line in the list\n"); exit(1); }
  if (o->outsubfam != NULL) { fprintf(stderr, "RAMExtend(ramx): with -batch every family's subfamily file is the twelfth field of its line in the list\n"); exit(1); }
  if (o->outtsd != NULL) { fprintf(stderr, "RAMExtend(ramx): with -batch every family's target-site duplication file is the thirteenth field of its line in the list\n"); exit(1); }
  if (o->outperiod != NULL) { fprintf(stderr, "RAMExtend(ramx): with -batch every family's periodicity file is the fifteenth field of its line in the list\n"); exit(1); }
  if (o->outcpg != NULL || o->outdinuc != NULL)
  { fprintf(stderr, "RAMExtend(ramx): with -batch every family's CpG-aware consensus file is the fourteenth field of its line in the list; -outdinuc writes one family\n"); exit(1); }
  FILE *lf = fopen(o->batch_file, "r");
  if (!lf) { fprintf(stderr, "Could not open batch list %s\n", o->batch_file); exit(1); }
  size_t cap = 64, F = 0;
  struct batch_item *it = (struct batch_item *)calloc(cap, sizeof(*it));
  char *line = NULL;
  size_t lcap = 0;
  ssize_t len;
  while ((len = getline(&line, &lcap, lf)) >= 0)
  {
    while (len > 0 && (line[len - 1] == '\n' || line[len - 1] == '\r')) line[--len] = 0;
    if (line[0] == '#' || line[0] == 0) continue;
    char *f[15] = { NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL };
    char *p = line;
    for (int k = 0; k < 15 && p; k++) { f[k] = p; char *t = strchr(p, '\t'); if (t) { *t = 0; p = t + 1; } else p = NULL; }
    if (!f[0] || !f[1]) { fprintf(stderr, "batch list: every line needs at least <ranges><TAB><log>\n"); exit(1); }
    if (F == cap) { cap *= 2; it = (struct batch_item *)realloc(it, cap * sizeof(*it)); memset(it + F, 0, (cap - F) * sizeof(*it)); }
    it[F].ranges = strdup(f[0]); it[F].log = strdup(f[1]);
    it[F].cons = field_or_null(f[2]) ? strdup(f[2]) : NULL;
    it[F].tsv = field_or_null(f[3]) ? strdup(f[3]) : NULL;
    it[F].fa = field_or_null(f[4]) ? strdup(f[4]) : NULL;
    it[F].profile = field_or_null(f[5]) ? strdup(f[5]) : NULL;       /* optional sixth field: the family's -outprofile file */
    it[F].aln = field_or_null(f[6]) ? strdup(f[6]) : NULL;           /* optional seventh field: the family's -outaln file */
    it[F].pileup = field_or_null(f[7]) ? strdup(f[7]) : NULL;        /* optional eighth field: the family's -outpileup file */
    it[F].refined = field_or_null(f[8]) ? strdup(f[8]) : NULL;       /* optional ninth field: the family's -outrefined file */
    it[F].copies = field_or_null(f[9]) ? strdup(f[9]) : NULL;        /* optional tenth field: the family's -outcopies file */
    it[F].linkage = field_or_null(f[10]) ? strdup(f[10]) : NULL;     /* optional eleventh field: the family's -outlinkage file */
    it[F].subfam = field_or_null(f[11]) ? strdup(f[11]) : NULL;      /* optional twelfth field: the family's -outsubfam file */
    it[F].tsd = field_or_null(f[12]) ? strdup(f[12]) : NULL;         /* optional thirteenth field: the family's -outtsd file */
    it[F].cpg = field_or_null(f[13]) ? strdup(f[13]) : NULL;         /* optional fourteenth field: the family's -outcpg file */
    it[F].period = field_or_null(f[14]) ? strdup(f[14]) : NULL;      /* optional fifteenth field: the family's -outperiod file */
    F++;
  }
  free(line);
  fclose(lf);
  fflush(stdout);
  const int saved = dup(1);

  /* phase 1: load every family; its log gets the banner, the parameters and the core table */
  ramx_family *fam = (ramx_family *)calloc(F ? F : 1, sizeof(*fam));
  for (size_t i = 0; i < F; i++)
  {
    to_log(it[i].log, 1);
    it[i].lib = ramx_load_sequence_subset_minimal(o->seq_file, it[i].ranges, &it[i].cores, &it[i].N, L + o->bandwidth);
    print_header(o, it[i].ranges, it[i].N, it[i].lib);
    ramx_print_core_edges(it[i].cores, it[i].lib, 0, o->verbose ? 1 : 0);
    it[i].master = (char *)calloc((size_t)(2 * (long)L + l + 1), 1);
    it[i].master[L] = RAMX_SYM_N;
    fam[i].sequence = (const int8_t *)it[i].lib->sequence;
    fam[i].seq_len = it[i].lib->length;
    fam[i].master = (int8_t *)it[i].master;
  }
  fflush(stdout);
  dup2(saved, 1);

  int32_t *mflat = (int32_t *)calloc(100 * 100, sizeof(int32_t));
  for (int a = 0; a < 4; a++)
  {
    for (int b = 0; b < 8; b++) mflat[a * 100 + b] = o->sp->matrix[a][b];
    mflat[a * 100 + RAMX_SYM_N] = o->sp->matrix[a][RAMX_SYM_N];
  }
  ramx_params p;
  p.bandwidth = o->bandwidth; p.cappenalty = o->cappenalty; p.minimprovement = o->minimprovement; p.L = L;
  p.when_to_stop = o->when_to_stop; p.l = l; p.gapopen = o->sp->gapopen; p.gapextn = o->sp->gapextn; p.matrix = mflat;
  ramx_run_info *ir = (ramx_run_info *)calloc(F ? F : 1, sizeof(*ir)), *il = (ramx_run_info *)calloc(F ? F : 1, sizeof(*il));

  warm_join();
  char **profile_paths = (char **)calloc(F ? F : 1, sizeof(char *));
  struct profile_out pout = { NULL, profile_paths, o->minimprovement };
  int any_profile = 0;
  for (size_t i = 0; i < F; i++)
    if ((profile_paths[i] = it[i].profile) != NULL) { profile_start(it[i].profile); any_profile = 1; }
  if (any_profile) ramx_set_profile_sink(profile_sink, &pout);
  struct aln_out aout = { (struct aln_family *)calloc(F ? F : 1, sizeof(struct aln_family)) };
  int any_aln = 0;
  for (size_t i = 0; i < F; i++)
    if ((aout.fam[i].path = it[i].aln) != NULL) { aout.fam[i].lib = it[i].lib; any_aln = 1; }
  if (any_aln) ramx_set_align_sink(aln_sink, &aout);
  struct refine_out rout = { (struct refine_family *)calloc(F ? F : 1, sizeof(struct refine_family)) };
  int any_pileup = 0, any_refined = 0;
  for (size_t i = 0; i < F; i++)
  {
    if ((rout.fam[i].pileup = it[i].pileup) != NULL) { pileup_start(it[i].pileup); any_pileup = 1; }
    if ((rout.fam[i].refined = it[i].refined) != NULL) any_refined = 1;
  }
  if (any_pileup || any_refined) ramx_set_refine_sink(refine_sink, &rout, any_refined ? o->refine : 1);
  struct copies_out cout = { (struct copies_family *)calloc(F ? F : 1, sizeof(struct copies_family)) };
  int any_copies = 0;
  for (size_t i = 0; i < F; i++)
    if ((cout.fam[i].path = it[i].copies) != NULL) { cout.fam[i].lib = it[i].lib; any_copies = 1; }
  if (any_copies) ramx_set_copies_sink(copies_sink, &cout);
  struct cpg_out gout = { (struct cpg_family *)calloc(F ? F : 1, sizeof(struct cpg_family)) };
  int any_cpg = 0;
  for (size_t i = 0; i < F; i++)
    if ((gout.fam[i].fasta = it[i].cpg) != NULL) any_cpg = 1;
  if (any_cpg) ramx_set_cpg_sink(cpg_sink, &gout, o->refine, o->cpgscore);
  struct linkage_out lout = { (struct linkage_family *)calloc(F ? F : 1, sizeof(struct linkage_family)) };
  int any_linkage = 0;
  for (size_t i = 0; i < F; i++)
    if ((lout.fam[i].path = it[i].linkage) != NULL) any_linkage = 1;
  if (any_linkage) ramx_set_linkage_sink(linkage_sink, &lout, o->linkcount, o->linkfrac, 1024);
  struct subfam_out sout = { (struct subfam_family *)calloc(F ? F : 1, sizeof(struct subfam_family)) };
  int any_subfam = 0;
  for (size_t i = 0; i < F; i++)
    if ((sout.fam[i].path = it[i].subfam) != NULL) { sout.fam[i].lib = it[i].lib; any_subfam = 1; }
  if (any_subfam) ramx_set_subfam_sink(subfam_sink, &sout, o->linkcount, o->linkfrac, 1024, (double)o->linkscore, o->subfamk, o->subfamiter, o->subfammin, o->refine);
  /* phase 2: right extension of all families in one launch; phase 3: per family, overlap avoidance */
  for (size_t i = 0; i < F; i++) flatten_cores(it[i].cores, it[i].N, &fam[i].cores);
  if (ramx_extend_batch(1, fam, (int32_t)F, &p, ir) < 0) { fprintf(stderr, "RAMExtend(ramx): batch extension failed: %s\n", ramx_last_error()); exit(1); }
  for (size_t i = 0; i < F; i++)
  {
    unflatten_results(it[i].cores, &fam[i].cores);
    free_flat(&fam[i].cores);
    it[i].rightbp = ir[i].ret;
    to_log(it[i].log, 0);
    print_loop_lines(1, it[i].N, o->verbose, o->when_to_stop, L, &ir[i], 1);
    print_loop_lines(1, it[i].N, o->verbose, o->when_to_stop, L, &ir[i], 0);
    printf("Extended right: %d bp\n", it[i].rightbp);
    ramx_overlap_avoidance(it[i].cores, it[i].lib);
  }
  fflush(stdout);
  dup2(saved, 1);

  /* phase 4: left extension in one launch; phase 5: per family, results */
  for (size_t i = 0; i < F; i++) flatten_cores(it[i].cores, it[i].N, &fam[i].cores);
  if (ramx_extend_batch(0, fam, (int32_t)F, &p, il) < 0) { fprintf(stderr, "RAMExtend(ramx): batch extension failed: %s\n", ramx_last_error()); exit(1); }
  for (size_t i = 0; i < F; i++)
  {
    unflatten_results(it[i].cores, &fam[i].cores);
    free_flat(&fam[i].cores);
    it[i].leftbp = il[i].ret;
    to_log(it[i].log, 0);
    print_loop_lines(0, it[i].N, o->verbose, o->when_to_stop, L, &il[i], 1);
    print_loop_lines(0, it[i].N, o->verbose, o->when_to_stop, L, &il[i], 0);
    printf("Extended left : %d bp\n", it[i].leftbp);
    write_results(o, it[i].cores, it[i].lib, it[i].master, it[i].rightbp, it[i].leftbp, it[i].cons, it[i].tsv, it[i].fa);
    aln_write(&aout.fam[i], it[i].cores, o->flanking);
    refined_write(&rout.fam[i]);
    copies_write(&cout.fam[i], it[i].cores, o->flanking);
    cpg_write(&gout.fam[i]);
    linkage_write(&lout.fam[i], o->linkscore);
    subfam_write(&sout.fam[i], it[i].cores, o->flanking);
    const double duration = difftime(time(0), t_start);
    printf("Program duration is %.1f sec = %.1f min = %.1f hr\n", duration, duration / 60.0, duration / 3600.0);
  }
  fflush(stdout);
  dup2(saved, 1);
  close(saved);
  /* phase 6, only where a family asks for it: the target-site duplications of all families in one launch, on the library the two
   * launches left on the device */
  int any_tsd = 0;
  for (size_t i = 0; i < F; i++) any_tsd |= it[i].tsd != NULL;
  if (any_tsd)
  {
    size_t total = 0;
    for (size_t i = 0; i < F; i++) { flatten_cores(it[i].cores, it[i].N, &fam[i].cores); total += (size_t)it[i].N; }
    ramx_tsd *rec = (ramx_tsd *)calloc(total ? total : 1, sizeof(ramx_tsd));
    if (ramx_tsd_batch(fam, (int32_t)F, &o->tsd, rec) < 0) { fprintf(stderr, "RAMExtend(ramx): target-site duplications failed: %s\n", ramx_last_error()); exit(1); }
    size_t at = 0;
    for (size_t i = 0; i < F; i++)
    {
      if (it[i].tsd != NULL) tsd_write(it[i].tsd, &o->tsd, it[i].cores, it[i].lib, it[i].master, L, it[i].rightbp, it[i].leftbp, rec + at, it[i].N);
      at += (size_t)it[i].N;
      free_flat(&fam[i].cores);
    }
    free(rec);
  }
  /* phase 7, only where a family asks for it: the periodicity of all families, one call per part */
  int any_period = 0;
  for (size_t i = 0; i < F; i++) any_period |= it[i].period != NULL;
  if (any_period)
  {
    size_t total = 0;
    for (size_t i = 0; i < F; i++) { flatten_cores(it[i].cores, it[i].N, &fam[i].cores); total += (size_t)it[i].N; }
    const int parts = o->periodwhole ? 3 : 2;
    ramx_period *rec[3] = { NULL, NULL, NULL };
    ramx_period_seg *segs[3] = { NULL, NULL, NULL };
    for (int w = 0; w < parts; w++)
    {
      rec[w] = (ramx_period *)calloc(total ? total : 1, sizeof(ramx_period));
      segs[w] = (ramx_period_seg *)calloc(total ? total : 1, sizeof(ramx_period_seg));
      if (ramx_period_batch(fam, (int32_t)F, w, &o->period, rec[w]) < 0) { fprintf(stderr, "RAMExtend(ramx): periodicity failed: %s\n", ramx_last_error()); exit(1); }
      size_t at = 0;
      for (size_t i = 0; i < F; i++) { ramx_period_segments(&fam[i].cores, w, segs[w] + at); at += (size_t)it[i].N; }
    }
    size_t at = 0;
    for (size_t i = 0; i < F; i++)
    {
      ramx_period *const r3[3] = { rec[0] + at, rec[1] + at, rec[2] ? rec[2] + at : NULL };
      ramx_period_seg *const s3[3] = { segs[0] + at, segs[1] + at, segs[2] ? segs[2] + at : NULL };
      if (it[i].period != NULL)
        period_write(it[i].period, &o->period, o->periodwhole, it[i].cores, it[i].lib, it[i].master, L, it[i].rightbp, it[i].leftbp, r3, s3, it[i].N);
      at += (size_t)it[i].N;
      free_flat(&fam[i].cores);
    }
    for (int w = 0; w < 3; w++) { free(rec[w]); free(segs[w]); }
  }
  printf("RAMExtend(ramx) batch: %zu families done\n", F);
  for (size_t i = 0; i < F; i++)
  {
    ramx_free_library(it[i].lib, it[i].cores);
    free(it[i].master); free(it[i].ranges); free(it[i].log); free(it[i].cons); free(it[i].tsv); free(it[i].fa); free(it[i].profile); free(it[i].aln);
    free(it[i].pileup); free(it[i].refined); free(it[i].copies); free(it[i].linkage); free(it[i].subfam); free(it[i].tsd); free(it[i].cpg); free(it[i].period);
  }
  ramx_set_profile_sink(NULL, NULL);
  ramx_set_align_sink(NULL, NULL);
  ramx_set_refine_sink(NULL, NULL, 1);
  ramx_set_copies_sink(NULL, NULL);
  ramx_set_cpg_sink(NULL, NULL, 1, 0);
  ramx_set_linkage_sink(NULL, NULL, 4, 100, 1024);
  ramx_set_subfam_sink(NULL, NULL, 4, 100, 1024, 3.0, 4, 8, 4, 10);
  free(aout.fam); free(rout.fam); free(cout.fam); free(gout.fam); free(lout.fam); free(sout.fam);
  free(profile_paths);
  free(it); free(fam); free(ir); free(il); free(mflat);
  ramx_free_scoring_system(o->sp);
  return 0;
}

int ramx_cli_main(int argc, char **argv)
{
  const time_t t_start = time(0);
  struct cli_opts o;
  memset(&o, 0, sizeof(o));
  const int l = 1;
  g_t_main = now_s();

  if (opt_bool(argc, argv, "-version"))
  {
    printf("RAMExtend Version %s - build %s date %s\n", k_version, k_build, k_build_date);
    exit(0);
  }
  opt_string(argc, argv, "-batch", &o.batch_file);
  if (!opt_string(argc, argv, "-ranges", &o.ranges_file) && !o.batch_file) usage();

  opt_int(argc, argv, "-addflanking", &o.flanking);
  opt_string(argc, argv, "-outtsv", &o.outtsv);
  opt_string(argc, argv, "-outfa", &o.outfa);
  opt_string(argc, argv, "-outmat", &o.outmat);
  opt_string(argc, argv, "-cons", &o.cons_file);
  opt_string(argc, argv, "-outprofile", &o.outprofile);
  opt_string(argc, argv, "-outaln", &o.outaln);
  opt_string(argc, argv, "-outpileup", &o.outpileup);
  opt_string(argc, argv, "-outrefined", &o.outrefined);
  opt_string(argc, argv, "-outcopies", &o.outcopies);
  opt_string(argc, argv, "-outcpg", &o.outcpg);
  opt_string(argc, argv, "-outdinuc", &o.outdinuc);
  if (!opt_int(argc, argv, "-cpgscore", &o.cpgscore)) o.cpgscore = 0;
  opt_string(argc, argv, "-outlinkage", &o.outlinkage);
  if (!opt_int(argc, argv, "-linkcount", &o.linkcount)) o.linkcount = 4;
  if (!opt_int(argc, argv, "-linkfrac", &o.linkfrac)) o.linkfrac = 100;
  if (!opt_int(argc, argv, "-linkscore", &o.linkscore)) o.linkscore = 3;
  opt_string(argc, argv, "-outsubfam", &o.outsubfam);
  if (!opt_int(argc, argv, "-subfamk", &o.subfamk)) o.subfamk = 4;
  if (!opt_int(argc, argv, "-subfammin", &o.subfammin)) o.subfammin = 4;
  if (!opt_int(argc, argv, "-subfamiter", &o.subfamiter)) o.subfamiter = 8;
  if (o.subfamk < 1 || o.subfamk > RAMX_SUBFAM_MAX || o.subfamiter < 1)
  { fprintf(stderr, "RAMExtend(ramx): -subfamk takes 1..%d groups, -subfamiter at least 1 assignment\n", RAMX_SUBFAM_MAX); exit(1); }
  opt_string(argc, argv, "-outtsd", &o.outtsd);
  if (!opt_int(argc, argv, "-tsdslack", &o.tsd.slack)) o.tsd.slack = 3;
  if (!opt_int(argc, argv, "-tsdmin", &o.tsd.kmin)) o.tsd.kmin = 4;
  if (!opt_int(argc, argv, "-tsdmax", &o.tsd.kmax)) o.tsd.kmax = 20;
  if (!opt_int(argc, argv, "-tsdmm", &o.tsd.mm_div)) o.tsd.mm_div = 10;
  if (ramx_tsd_check_params(&o.tsd) != RAMX_OK) { fprintf(stderr, "RAMExtend(ramx): %s\n", ramx_last_error()); exit(1); }
  opt_string(argc, argv, "-outperiod", &o.outperiod);
  if (!opt_int(argc, argv, "-periodmax", &o.period.pmax)) o.period.pmax = 1024;
  if (!opt_int(argc, argv, "-periodmm", &o.period.mm)) o.period.mm = 3;
  if (!opt_int(argc, argv, "-periodmin", &o.period.min_score)) o.period.min_score = 16;
  o.period.reserved = 0;
  o.periodwhole = opt_bool(argc, argv, "-periodwhole");
  if (ramx_period_check_params(&o.period) != RAMX_OK) { fprintf(stderr, "RAMExtend(ramx): %s\n", ramx_last_error()); exit(1); }
  if (!opt_int(argc, argv, "-refine", &o.refine)) o.refine = 10;
  if (o.refine < 1) { fprintf(stderr, "RAMExtend(ramx): -refine takes the largest number of replays, at least 1\n"); exit(1); }
  if (!opt_int(argc, argv, "-L", &o.L)) o.L = 10000;
  if (!opt_int(argc, argv, "-bandwidth", &o.bandwidth)) o.bandwidth = 14;
  if (!opt_int(argc, argv, "-maxoccurrences", &o.maxn)) o.maxn = 10000;
  if (!opt_int(argc, argv, "-stopafter", &o.when_to_stop)) o.when_to_stop = 100;
  if (!opt_int(argc, argv, "-threads", &o.num_threads)) o.num_threads = 0;
  o.verbose = opt_bool(argc, argv, "-vvvvvv") ? 20 : opt_bool(argc, argv, "-vvvvv") ? 12 :
              opt_bool(argc, argv, "-vvvv") ? 10 : opt_bool(argc, argv, "-vvv") ? 3 :
              opt_bool(argc, argv, "-vv") ? 2 : opt_bool(argc, argv, "-v") ? 1 : 0;

  if (!opt_string(argc, argv, "-matrix", &o.matrix_name)) o.matrix_name = "20p43g";
  if (o.matrix_name == NULL) o.matrix_name = "";
  o.is_rs = strcmp(o.matrix_name, "repeatscout") == 0;
  if (o.is_rs)
  {
    if (opt_int(argc, argv, "-match", &o.match) && opt_int(argc, argv, "-mismatch", &o.mismatch) &&
        opt_int(argc, argv, "-gap", &o.gap_ext))
      o.sp = ramx_get_repeatscout_matrix(o.match, o.mismatch, o.gap_ext);
    else
      o.sp = ramx_get_repeatscout_matrix(1, -1, -5);
  }
  else
  {
    if (opt_int(argc, argv, "-gapopen", &o.gap_open) && opt_int(argc, argv, "-gapext", &o.gap_ext))
      o.sp = ramx_get_matrix_using_gap_penalties(o.matrix_name, o.gap_open, o.gap_ext);
    else
      o.sp = ramx_get_matrix(o.matrix_name);
  }
  /* per-matrix defaults, ram_extend.c:301-344 */
  {
    int def_min, def_cap;
    if (!strcmp(o.matrix_name, "14p43g") || !strcmp(o.matrix_name, "18p43g") || !strcmp(o.matrix_name, "20p43g")) { def_min = 27; def_cap = -90; }
    else if (!strcmp(o.matrix_name, "25p43g")) { def_min = 24; def_cap = -90; }
    else if (o.is_rs) { def_min = 3; def_cap = -20; }
    else { printf("Matrix name not found!\n"); exit(1); }
    if (!opt_int(argc, argv, "-minimprovement", &o.minimprovement)) o.minimprovement = def_min;
    if (!opt_int(argc, argv, "-cappenalty", &o.cappenalty)) o.cappenalty = def_cap;
  }
  if (!opt_string(argc, argv, "-twobit", &o.seq_file))
  {
    if (opt_string(argc, argv, "-sequence", &o.seq_file))
    {
      printf("-sequence is deprecated!....may return someday\n");
      exit(1);
    }
    usage();
  }
  warm_start();
  if (o.batch_file) return run_batch(&o, t_start);

  g_timing = getenv("RAMX_TIMING") != NULL;
  g_t_last = now_s();
  if (g_timing) atexit(timing_at_exit);
  phase_done("options");
  const int L = o.L;
  char *master = (char *)malloc((size_t)(2 * (long)L + l + 1));
  if (!master) { fprintf(stderr, "Could not allocate space for master array\n"); exit(1); }
  memset(master, 0, (size_t)(2 * (long)L + l + 1));

  struct coreAlignment *cores = NULL;
  int N = 0;
  /* the windows stay packed (4 bases per byte, as in the .2bit file) on the host and go to the device packed: the report and
   * -outfa decode the few bases they print.  RAMX_CLI_BYTES=1: the one-byte-per-base library of the reference (A/B) */
  struct sequenceLibrary *lib = getenv("RAMX_CLI_BYTES") != NULL
                                    ? ramx_load_sequence_subset_minimal(o.seq_file, o.ranges_file, &cores, &N, L + o.bandwidth)
                                    : ramx_load_sequence_subset_packed(o.seq_file, o.ranges_file, &cores, &N, L + o.bandwidth, NULL);
  FILE *fp_mat = NULL;
  if (o.outmat != NULL)       /* ram_extend.c:384-390 */
  {
    if ((fp_mat = fopen(o.outmat, "w")) == NULL)
    {
      fprintf(stderr, "Could not create the output matrix file %s\n", o.outmat);
      exit(1);
    }
  }
  phase_done("load");
  if (g_warm_started && lib != NULL && N > 0) warm_offer_library(lib);
  print_header(&o, o.ranges_file, N, lib);
  ramx_print_core_edges(cores, lib, 0, o.verbose ? 1 : 0);
  phase_done("core table");
  master[L] = RAMX_SYM_N;   /* the l = 1 spacer, never printed (ram_extend.c:415-416) */

  ramx_set_runtime(o.verbose, o.when_to_stop, l);
  struct profile_out pout = { o.outprofile, NULL, o.minimprovement };
  if (o.outprofile != NULL)
  {
    profile_start(o.outprofile);
    ramx_set_profile_sink(profile_sink, &pout);
  }
  struct aln_family afam;
  memset(&afam, 0, sizeof(afam));
  afam.path = o.outaln; afam.lib = lib;
  struct aln_out aout = { &afam };
  if (o.outaln != NULL) ramx_set_align_sink(aln_sink, &aout);
  struct refine_family rfam;
  memset(&rfam, 0, sizeof(rfam));
  rfam.pileup = o.outpileup; rfam.refined = o.outrefined;
  struct refine_out rout = { &rfam };
  if (o.outpileup != NULL) pileup_start(o.outpileup);
  if (o.outpileup != NULL || o.outrefined != NULL) ramx_set_refine_sink(refine_sink, &rout, o.outrefined != NULL ? o.refine : 1);
  struct copies_family cfam;
  memset(&cfam, 0, sizeof(cfam));
  cfam.path = o.outcopies; cfam.lib = lib;
  struct copies_out cout = { &cfam };
  if (o.outcopies != NULL) ramx_set_copies_sink(copies_sink, &cout);
  struct cpg_family gfam;
  memset(&gfam, 0, sizeof(gfam));
  gfam.fasta = o.outcpg; gfam.dinuc = o.outdinuc;
  struct cpg_out gout = { &gfam };
  if (o.outdinuc != NULL) dinuc_start(o.outdinuc);
  if (o.outcpg != NULL || o.outdinuc != NULL) ramx_set_cpg_sink(cpg_sink, &gout, o.refine, o.cpgscore);
  struct linkage_family lfam;
  memset(&lfam, 0, sizeof(lfam));
  lfam.path = o.outlinkage;
  struct linkage_out lout = { &lfam };
  if (o.outlinkage != NULL) ramx_set_linkage_sink(linkage_sink, &lout, o.linkcount, o.linkfrac, 1024);
  struct subfam_family sfam;
  memset(&sfam, 0, sizeof(sfam));
  sfam.path = o.outsubfam; sfam.lib = lib;
  struct subfam_out sout = { &sfam };
  if (o.outsubfam != NULL) ramx_set_subfam_sink(subfam_sink, &sout, o.linkcount, o.linkfrac, 1024, (double)o.linkscore, o.subfamk, o.subfamiter, o.subfammin, o.refine);
  fflush(stdout);
  warm_join();
  phase_done("device ready");
  int rightbp = ramx_extend_alignment(1, cores, NULL, lib, master, o.bandwidth, o.cappenalty, o.minimprovement, L, N, o.sp, fp_mat);
  printf("Extended right: %d bp\n", rightbp);
  phase_done("extend right");
  ramx_overlap_avoidance(cores, lib);
  phase_done("overlap avoidance");
  int leftbp = ramx_extend_alignment(0, cores, NULL, lib, master, o.bandwidth, o.cappenalty, o.minimprovement, L, N, o.sp, fp_mat);
  printf("Extended left : %d bp\n", leftbp);
  phase_done("extend left");
  ramx_set_profile_sink(NULL, NULL);
  ramx_set_align_sink(NULL, NULL);
  ramx_set_refine_sink(NULL, NULL, 1);
  ramx_set_copies_sink(NULL, NULL);
  ramx_set_cpg_sink(NULL, NULL, 1, 0);
  ramx_set_linkage_sink(NULL, NULL, 4, 100, 1024);
  ramx_set_subfam_sink(NULL, NULL, 4, 100, 1024, 3.0, 4, 8, 4, 10);
  write_results(&o, cores, lib, master, rightbp, leftbp, o.cons_file, o.outtsv, o.outfa);
  aln_write(&afam, cores, o.flanking);
  refined_write(&rfam);
  copies_write(&cfam, cores, o.flanking);
  cpg_write(&gfam);
  linkage_write(&lfam, o.linkscore);
  subfam_write(&sfam, cores, o.flanking);
  if (o.outtsd != NULL)
  {
    /* after both directions, on the library they left on the device */
    int cnt = 0;
    for (struct coreAlignment *s = cores; s != NULL; s = s->next) cnt++;
    ramx_tsd *rec = (ramx_tsd *)calloc((size_t)(cnt ? cnt : 1), sizeof(ramx_tsd));
    if (ramx_tsd_alignment(cores, lib, &o.tsd, rec) != RAMX_OK) { fprintf(stderr, "RAMExtend(ramx): target-site duplications failed: %s\n", ramx_last_error()); exit(1); }
    tsd_write(o.outtsd, &o.tsd, cores, lib, master, L, rightbp, leftbp, rec, cnt);
    free(rec);
  }
  if (o.outperiod != NULL)
  {
    /* after both directions, on the library they left on the device: one call per part */
    int cnt = 0;
    for (struct coreAlignment *s = cores; s != NULL; s = s->next) cnt++;
    ramx_flat_cores fc;
    flatten_cores(cores, cnt, &fc);
    ramx_period *rec[3] = { NULL, NULL, NULL };
    ramx_period_seg *segs[3] = { NULL, NULL, NULL };
    for (int w = 0; w < (o.periodwhole ? 3 : 2); w++)
    {
      rec[w] = (ramx_period *)calloc((size_t)(cnt ? cnt : 1), sizeof(ramx_period));
      segs[w] = (ramx_period_seg *)calloc((size_t)(cnt ? cnt : 1), sizeof(ramx_period_seg));
      ramx_period_segments(&fc, w, segs[w]);
      if (ramx_period_alignment(cores, lib, w, &o.period, rec[w]) != RAMX_OK) { fprintf(stderr, "RAMExtend(ramx): periodicity failed: %s\n", ramx_last_error()); exit(1); }
    }
    period_write(o.outperiod, &o.period, o.periodwhole, cores, lib, master, L, rightbp, leftbp, rec, segs, cnt);
    for (int w = 0; w < 3; w++) { free(rec[w]); free(segs[w]); }
    free_flat(&fc);
  }
  if (fp_mat != NULL) fclose(fp_mat);     /* ram_extend.c:778-779 */
  phase_done("report + outputs");

  const double duration = difftime(time(0), t_start);
  printf("Program duration is %.1f sec = %.1f min = %.1f hr\n", duration, duration / 60.0, duration / 3600.0);
  ramx_free_scoring_system(o.sp);
  ramx_free_library(lib, cores);
  free(master);
  phase_done("free");
  return 0;
}
