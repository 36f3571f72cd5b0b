/* ramx_cli_outputs.h -- what ramx_cli.c and ramx_cli_outputs.c share (not installed): the options of the command line, a core
 * as every output prints it, the table of the analysis outputs and what a family keeps for them. */
#ifndef RAMX_CLI_OUTPUTS_H
#define RAMX_CLI_OUTPUTS_H

#include "ramx_internal.h"
#include "ramx_dist.h"
#include "ramx_xfam.h"

/* the rows of the table of analysis outputs (ramx_cli_outputs.c, k_outputs), in the order in which their files are started and
 * written */
enum
{
  OUT_PROFILE, OUT_ALN, OUT_PILEUP, OUT_REFINED, OUT_COPIES, OUT_CPG, OUT_DINUC, OUT_LINKAGE, OUT_SUBFAM, OUT_TSD, OUT_PERIOD,
  OUT_TERM, OUT_DIST,
  N_OUTPUTS
};
#define BATCH_FIELDS 17          /* of a -batch line: ranges, log, -cons, -outtsv, -outfa and the rows' batch_field */

/* the defaults of the options the sinks take: what the command line starts from and what a sink is reset to */
enum { DEF_REFINE = 10, DEF_CPGSCORE = 0, DEF_LINKCOUNT = 4, DEF_LINKFRAC = 100, DEF_LINKSCORE = 3, DEF_SUBFAMK = 4, DEF_SUBFAMMIN = 4, DEF_SUBFAMITER = 8,
       DEF_DISTMIN = 20, DEF_DISTMAX = 256 };

/* everything the command line decides */
struct cli_opts
{
  const char *ranges_file, *outtsv, *outfa, *outmat, *cons_file, *seq_file, *matrix_name, *batch_file;
  const char *out[N_OUTPUTS];          /* the analysis outputs' flags */
  ramx_tsd_params tsd;
  ramx_period_params period;
  int periodwhole;
  ramx_term_params term;
  int refine, cpgscore, linkcount, linkfrac, linkscore, subfamk, subfammin, subfamiter, distmin, distmax;
  const char *outxfam;                 /* one file a run, not a family's: no row of the table */
  ramx_pair_params xfam;
  ramx_xfam_link_params xfamlink;
  int xfamseed;
  int flanking, L, bandwidth, maxn, when_to_stop, num_threads, verbose;
  int gap_ext, gap_open, match, mismatch, cappenalty, minimprovement, is_rs;
  struct scoringSystem *sp;
};

/* A core as the report, -outtsv, -outfa and every analysis output place it.  lo / hi: its record's first base and end in the
 * library; off: the record's genomic offset; e_lo / e_hi: the extended copy's ends in the library (the strand decides which
 * extension lies at which end); left / right: the extension lengths as printed, "*" for an end that is not extendable. */
struct core_view
{
  const struct coreAlignment *s;
  const char *ident;
  uint64_t lo, hi, off;
  int64_t e_lo, e_hi;
  char orient;
  char left[16], right[16];
};
/* the stretch -outfa writes: the extended copy plus the -addflanking bases, clamped as the reference clamps them */
void core_fa_range(const struct core_view *v, int flanking, uint64_t *from, uint64_t *to);
/* the record id -outfa gives that stretch: ident:from-to_orient */
void core_fa_id(char *buf, size_t n, const struct core_view *v, int flanking);

/* -outtsd, -outperiod and -outterm are computed after both directions, on the library they left on the device.  All of it is
 * shared but the compute entries: tsd fills rec with the records of every core of every family, in order; period does so for
 * one part (0 left, 1 right, 2 whole) and gives the cores' segments of that part; term fills two records per core, direct and
 * inverted.  All return < 0 on failure. */
struct outputs_post_fns
{
  int (*tsd)(void *ctx, const ramx_tsd_params *tp, ramx_tsd *rec);
  int (*period)(void *ctx, int part, const ramx_period_params *pp, ramx_period *rec, ramx_period_seg *segs);
  int (*term)(void *ctx, const ramx_term_params *tp, ramx_term *rec);
};

/* one row per output file */
struct family_outputs;
struct output_row
{
  const char *flag;              /* on the command line of a single family */
  int batch_field;               /* 1-based field of a -batch line, 0: the flag writes one family only */
  const char *word;              /* "Could not create the <word> file" */
  const char *refusal;           /* what the bare flag is told with -batch */
  void (*start)(FILE *fp);       /* the header, written before the first direction (the sink appends) */
  void (*write)(FILE *fp, struct family_outputs *fo);      /* after both directions, from what the sink kept */
  /* or, without a sink: after both directions of every family (total cores), one compute call and the files of all of them */
  void (*post)(const struct cli_opts *o, struct family_outputs *fams, int F, size_t total, const struct outputs_post_fns *fns, void *ctx);
};
extern const struct output_row k_outputs[N_OUTPUTS];

/* what the sinks keep of a direction (0 left, 1 right) until the file is written */
struct flank_rec { int core, end_row, start, end, score; char *body; ramx_copy_stats st; };       /* body: -outaln, st: -outcopies */
struct flank_block { int have, ret, n; char *cons; struct flank_rec *rec; };
struct kept_fasta { int have[2], rows[2], replays[2], converged[2], n_cpg[2]; char *seq[2]; };
struct linkage_block { int have, P; ramx_plane *planes; int32_t *co; };
struct dist_block { int have, n, C; int32_t *core, *sel; ramx_copy_dist *m; };   /* core: [n] every flank's; sel: [C] flanks; m: [C][C] */
struct subfam_block { int have, n, K, iterations, converged; int32_t *core, *labels, *dist, *size; char **pattern, **cons; int *rows, *replays, *conv; };

/* one family's outputs; the sinks get the array of these as `user` and index it by the record's family */
struct family_outputs
{
  const char *paths[N_OUTPUTS];  /* by table row, NULL: not wanted */
  const struct cli_opts *o;
  struct sequenceLibrary *lib;
  struct core_view *cores;       /* between outputs_family_done and outputs_end */
  int n_cores, rightbp, leftbp;
  const char *master;
  struct flank_block aln[2], copies[2];
  struct kept_fasta refined, cpg;
  struct linkage_block linkage[2];
  struct subfam_block subfam[2];
  struct dist_block dist[2];
};

FILE *open_or_die(const char *path, const char *mode, const char *word);

/* -batch: a bare flag is refused */
void outputs_refuse_flags(const struct cli_opts *o);
/* -batch: the optional fields of a line (f[k] NULL past its end) -> fo->paths, owned; and their release */
void outputs_parse_fields(struct family_outputs *fo, char *const f[BATCH_FIELDS]);
void outputs_free_fields(struct family_outputs *fo);

/* before the first direction (fams[i].paths and .lib set): the files that begin with a header are started, the sinks installed */
void outputs_begin(const struct cli_opts *o, struct family_outputs *fams, int F);
/* after both directions of a family, behind the report: the files of what the sinks kept */
void outputs_family_done(struct family_outputs *fo, const struct coreAlignment *cores, const char *master, int rightbp, int leftbp);
/* the core array of a family, built once after both directions: fo->cores, fo->n_cores (the report uses it too) */
void outputs_family_cores(struct family_outputs *fo, const struct coreAlignment *cores);
/* after outputs_family_done of every family: the rows with a post-pass that some family wants */
void outputs_post(const struct cli_opts *o, struct family_outputs *fams, int F, const struct outputs_post_fns *fns, void *ctx);
/* -outxfam: the options' ranges (RAMX_OK, or RAMX_ERR_ARG with the error text set), and the file itself: once a run, after
 * outputs_post and before outputs_end, from the families' masters; names[f] is family f's ranges file */
int outputs_xfam_check(const struct cli_opts *o);
void outputs_xfam(const struct cli_opts *o, const struct family_outputs *fams, int F, const char *const *names);
/* every sink reset, everything the families kept released */
void outputs_end(struct family_outputs *fams, int F);

#endif
