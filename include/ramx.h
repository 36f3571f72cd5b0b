/*
 * ramx.h -- C-ABI of libramx.so: the MI355X-native RAMExtend extension loop.
 *
 * Plain C, plain pointers and sizes; no torch / HIP types cross this boundary.
 * Two concentric seams:
 *
 *   seam 1  extend_alignment()-compatible entry      (replaces reference ram_extend.c:859-1258,
 *           ramx_extend_alignment / ramx_extend_flat   declared ram_extend.h:9-13)
 *   seam 2  thin device API  ramx_dev_*               (init / upload / run_direction / download /
 *                                                       destroy; what seam 1 is built from)
 *
 * plus the surfaces either side of the path that the RAMExtend CLI needs:
 *   ramx_get_matrix* / ramx_free_scoring_system       (replaces score_system.c:23-30,91-180,182-400)
 *   ramx_load_sequence_subset_minimal                 (replaces sequence.c:505-923 + 942-976)
 *   ramx_print_core_edges                             (replaces report.c:161-502)
 *   ramx_allocate_score / ramx_free_score             (replaces bnw_extend.c:87-155; the device path
 *                                                       keeps its own state, these are kept only so a
 *                                                       caller written against the reference still links)
 *
 * There is NO CPU fallback behind any of these: every entry that computes runs the HIP kernels and
 * fails loudly (message on stderr + non-zero status / exit(1) where the reference would exit) if
 * no gfx950 device is usable.
 */
#ifndef RAMX_H
#define RAMX_H

#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Data model -- layout-identical to the reference structs so a reference caller can pass its
 * own objects (common.h:80-98, sequence.h:36-46, score_system.h:7-17).  When compiling inside
 * the reference tree define RAMX_USE_REFERENCE_STRUCTS and include its headers first.
 * ------------------------------------------------------------------------------------------ */
#ifndef RAMX_USE_REFERENCE_STRUCTS
enum CoreBoundFlag { L_BOUNDARY = 0, SEQ_BOUNDARY = 1, CORE_BOUNDARY = 2, EXT_BOUNDARY = 3 };

struct coreAlignment
{
  struct coreAlignment *next;
  int seqIdx;
  uint64_t leftSeqPos;
  uint64_t rightSeqPos;
  char leftExtendable;
  char rightExtendable;
  uint64_t lowerSeqBound;
  uint64_t upperSeqBound;
  enum CoreBoundFlag lowerSeqBoundFlag;
  enum CoreBoundFlag upperSeqBoundFlag;
  int leftExtensionLen;
  int rightExtensionLen;
  int score;
  char orient;
};

struct sequenceLibrary
{
  char *sequence;
  char **identifiers;
  uint64_t *boundaries;
  uint64_t *offsets;
  uint64_t length;
  int count;
  int markov_chain_order;
  uint32_t **markov_chain_prob_tables;
};

struct scoringSystem
{
  char *name;
  int **matrix;
  int msize;
  char *alphabet;
  double m_lambda;
  double m_bg_freqs[4];
  int gapopen;
  int gapextn;
};
#endif

/* base codes, reference sequence.h:7-15 */
#define RAMX_SYM_N 99

/* ------------------------------------------------------------------------------------------
 * Seam 1: the extension loop
 * ------------------------------------------------------------------------------------------ */

/* The three globals the reference reads inside the hot path (ram_extend.c:40 `l`, :52 `VERBOSE`,
 * :61 `WHEN_TO_STOP`).  Call before ramx_extend_alignment; defaults are 0 / 100 / 1. */
void ramx_set_runtime(int verbose, int when_to_stop, int l);

/* Drop-in for reference extend_alignment (ram_extend.h:9-13, ram_extend.c:859-1258): same
 * arguments, same return value (max_extension_score_row_idx + 1), same side effects on
 * master[], coreAlign[*].{left,right}ExtensionLen and .score, same stdout lines at VERBOSE<10.
 * `score` (the reference's int**** DP state) is ignored: state lives in HBM.  With pathStringFile
 * (-outmat) the direction runs one column launch at a time and the reference's trace lines
 * (ram_extend.c:1122-1132) are written from the device's per-cell path codes. */
int ramx_extend_alignment(int direction, struct coreAlignment *coreAlign, int ****score,
                          struct sequenceLibrary *seqLib, char *master, int BANDWIDTH,
                          int CAPPENALTY, int MINIMPROVEMENT, int L, int N,
                          struct scoringSystem *scoreParams, FILE *pathStringFile);

/* Same loop on flat arrays (what ramx_extend_alignment flattens to, and what the Python mirror
 * binds).  matrix is int32[100*100], row-major [consensus][sequence base].  Returns the
 * reference's return value, or a negative ramx error code. */
typedef struct ramx_flat_cores
{
  int32_t n;
  const int64_t *left_pos, *right_pos, *lower, *upper;
  const int8_t *orient, *left_ext, *right_ext;
  int32_t *left_len, *right_len, *score;       /* in/out */
} ramx_flat_cores;

typedef struct ramx_params
{
  int32_t bandwidth, cappenalty, minimprovement, L, when_to_stop, l, gapopen, gapextn;
  const int32_t *matrix;
} ramx_params;

typedef struct ramx_run_info
{
  int32_t ret;              /* max_extension_score_row_idx + 1 */
  int32_t rows_executed;    /* row_idx iterations executed (the metric's "columns") */
  int32_t limit_warning;    /* 1 iff the reference would print "WARNING: Extended ... to the limit" */
  int32_t overflow32;       /* 1 iff a column sum left the int32 range (reference would have wrapped) */
  int32_t n_extendable;     /* flanks on the device in this direction */
  int32_t launches;         /* column-kernel launches issued (>= rows_executed: the host runs ahead) */
  double  loop_ms;          /* HIP-event time of the column loop on the library's stream */
  double  kernel_ms_avg;    /* mean duration of sampled single column-kernel launches (HIP events) */
  int32_t kernel_samples;
  double  prep_ms;          /* host flatten + H2D + pack kernel (wall clock) */
  int32_t persistent;       /* 1: the whole loop ran as ONE persistent launch (rows resident on chip) */
  int32_t lanes_per_flank;  /* 1: one lane per flank; 2..16: the cell-parallel kernels split a band row over that many lanes */
  int32_t respeculated_rows; /* device-wide cell-parallel kernel and packed-row kernel: rows that workgroup 0 computed a second time
                               because its own guess of the vote was wrong (it runs ahead of the device-wide vote); 0 on every other route */
  int32_t packed_rows;      /* columns that ran in the packed-row persistent kernel (two cells per register, int16 relative to a
                               per-flank base: csrc/ramx_kernels_packed.h); 0 on every other route */
  int32_t lean_rows;        /* ... of which the first wave ran as LEAN rows (no candidate rows, no best-cell index) */
} ramx_run_info;

int ramx_extend_flat(int direction, ramx_flat_cores *cores, const int8_t *sequence, uint64_t seq_len,
                     int8_t *master, const ramx_params *p, ramx_run_info *info);

/* Profile sink of seam 1.  With a sink set, ramx_extend_flat, ramx_extend_alignment and ramx_extend_batch replay every
 * direction they have run (ramx_dev_profile, below, on the session's device) along the consensus the loop chose, on whatever
 * route the loop took, and hand the result to the sink once per direction and family before they return: n_cols =
 * rows_executed columns (ret = the call's return value: columns [0, ret) are the kept ones), n_flanks per-flank entries with
 * core_index[i] the position of flank i in the core list.  A direction without an extendable core is answered on the host:
 * rows_executed columns of zeros with base A.  The pointers are valid during the call only.  cb == NULL (the default): off --
 * nothing is launched or allocated for it. */
struct ramx_col_profile;
typedef struct ramx_profile
{
  int32_t direction, family /* index in a batch, else 0 */, n_cols, ret, n_flanks;
  const struct ramx_col_profile *cols;
  const int32_t *core_index, *last_uncapped_row;
} ramx_profile;
typedef void (*ramx_profile_cb)(const ramx_profile *pr, void *user);
void ramx_set_profile_sink(ramx_profile_cb cb, void *user);

/* Alignment sink of seam 1, as the profile sink: with a sink set every direction that has run is replayed (ramx_dev_align,
 * below) along the kept consensus -- rows = ret columns -- and handed over once per direction and family.  ends is
 * [n_flanks]; col_idx / col_ins are [rows][stride] row-major (column r of flank i at [r * stride + i]).  A direction without an
 * extendable core or with ret = 0 is answered on the host (no flank has an alignment).  cb == NULL (the default): off --
 * nothing is launched or allocated for it. */
struct ramx_aln_end;
typedef struct ramx_alignment
{
  int32_t direction, family /* index in a batch, else 0 */, rows /* = ret */, n_flanks, stride;
  const int8_t *cons;                 /* [rows] */
  const struct ramx_flank *flanks;    /* [n_flanks], positions in the family's own library */
  const int32_t *core_index;          /* [n_flanks] */
  const struct ramx_aln_end *ends;    /* [n_flanks] */
  const int32_t *col_idx, *col_ins;   /* [rows][stride]; NULL when rows == 0 or n_flanks == 0 */
} ramx_alignment;
typedef void (*ramx_align_cb)(const ramx_alignment *al, void *user);
void ramx_set_align_sink(ramx_align_cb cb, void *user);

/* Refinement sink of seam 1, as the other sinks: with a sink set the kept consensus of every direction that has run -- rows =
 * ret columns -- is piled up (ramx_dev_pileup, below) and refined over at most max_replays replays (ramx_dev_refine), and both
 * are handed over once per direction and family: the kept consensus with its pileup, the refined one with its pileup (the
 * same when replays == 1), replays and converged.  A direction without an extendable core or with ret = 0 is answered on the
 * host.  cb == NULL (the default): off -- nothing is launched or allocated for it. */
struct ramx_col_pileup;
typedef struct ramx_refinement
{
  int32_t direction, family /* index in a batch, else 0 */, rows /* = ret */, refined_rows, replays, converged, n_flanks, pad_;
  const int8_t *cons;                       /* [rows] */
  const struct ramx_col_pileup *cols;       /* [rows] */
  const int8_t *refined_cons;               /* [refined_rows] */
  const struct ramx_col_pileup *refined_cols;
} ramx_refinement;
typedef void (*ramx_refine_cb)(const ramx_refinement *rf, void *user);
void ramx_set_refine_sink(ramx_refine_cb cb, void *user, int32_t max_replays);

/* CpG sink of seam 1, as the other sinks: with a sink set the kept consensus of every direction that has run -- rows = ret
 * columns -- is refined over at most max_replays replays with the CpG-aware re-call (ramx_dev_refine_cpg, below; rows_reversed =
 * !direction as the copies sink, cpg_ts as ramx_recall_cpg) and handed over once per direction and family: the kept consensus,
 * the refined one with its pileup and its dinucleotide pileup, replays, converged and n_cpg.  A direction without an extendable
 * core or with ret = 0 is answered on the host.  It comes after the copies sink.  cb == NULL (the default): off -- nothing is
 * launched or allocated for it. */
struct ramx_col_dinuc;
typedef struct ramx_cpg_refinement
{
  int32_t direction, family /* index in a batch, else 0 */, rows /* = ret */, refined_rows, replays, converged, n_flanks, n_cpg;
  const int8_t *cons;                       /* [rows] */
  const int8_t *refined_cons;               /* [refined_rows] */
  const struct ramx_col_pileup *refined_cols;
  const struct ramx_col_dinuc *refined_di;
} ramx_cpg_refinement;
typedef void (*ramx_cpg_cb)(const ramx_cpg_refinement *cr, void *user);
void ramx_set_cpg_sink(ramx_cpg_cb cb, void *user, int32_t max_replays, int32_t cpg_ts);

/* Copies sink of seam 1, as the other sinks: with a sink set the per-copy statistics of every direction that has run
 * (ramx_dev_copy_stats, below) are taken along the kept consensus -- rows = ret columns, rows_reversed = !direction -- and
 * handed over once per direction and family.  ends and stats are [n_flanks].  A direction without an extendable core or with
 * ret = 0 is answered on the host (zero records).  cb == NULL (the default): off -- nothing is launched or allocated for it. */
struct ramx_copy_stats;
typedef struct ramx_copies
{
  int32_t direction, family /* index in a batch, else 0 */, rows /* = ret */, n_flanks;
  const int8_t *cons;                 /* [rows] */
  const struct ramx_flank *flanks;    /* [n_flanks], positions in the family's own library */
  const int32_t *core_index;          /* [n_flanks] */
  const struct ramx_aln_end *ends;    /* [n_flanks] */
  const struct ramx_copy_stats *stats;/* [n_flanks] */
} ramx_copies;
typedef void (*ramx_copies_cb)(const ramx_copies *cp, void *user);
void ramx_set_copies_sink(ramx_copies_cb cb, void *user);

/* Seam 1 keeps the library on the device between calls, keyed on (pointer, length, 64-bit content fingerprint), so
 * the second direction does not upload it again (libraries above 64 MiB are fingerprinted in chunks by worker threads; when
 * pointer and length match the device copy the content check runs beside the direction and is joined before the write-back).
 * The reference has no such state (ram_extend.c reads seqLib->sequence on every call): a caller who
 * wants to be explicit can drop the device copy with this call. */
void ramx_invalidate_library(void);
/* Upload a library ahead of the first extension call (e.g. from a helper thread while the caller still prints its
 * report tables): the next ramx_extend_flat / ramx_extend_alignment calls on the same (pointer, length) use the device
 * copy without looking at the buffer again -- the caller vouches that it does not change until
 * ramx_invalidate_library() or a call with another buffer. */
int ramx_preload_library(const int8_t *sequence, uint64_t seq_len);
/* The packed twin of a library loaded with ramx_load_sequence_subset_packed goes to the device; ramx_extend_alignment calls
 * on that seqLib (whose ->sequence is NULL) then run on it, until ramx_invalidate_library() or another preload. */
struct ramx_packed_library;
int ramx_preload_library_packed(const struct sequenceLibrary *seqLib, const struct ramx_packed_library *pl);

/* ------------------------------------------------------------------------------------------
 * Seam 2: thin device API (one ramx_dev per GPU / per process rank)
 * ------------------------------------------------------------------------------------------ */
typedef struct ramx_dev ramx_dev;

#define RAMX_OK            0
#define RAMX_ERR_NO_DEVICE (-101)
#define RAMX_ERR_HIP       (-102)
#define RAMX_ERR_ARG       (-103)
#define RAMX_ERR_STATE     (-104)
#define RAMX_ERR_COMM      (-105)
#define RAMX_ERR_UNSUPPORTED (-106)

const char *ramx_last_error(void);
int ramx_device_count(void);                                   /* gfx950 devices visible; <0 on error */
int ramx_dev_create(int device_ordinal, ramx_dev **out);       /* init */
void ramx_dev_destroy(ramx_dev *d);                            /* destroy */

/* upload: the 1-byte-per-base library (seqLib->sequence) goes to HBM once and is shared by both
 * directions. */
int ramx_dev_load_library(ramx_dev *d, const int8_t *sequence, uint64_t length);
/* upload of a packed library (ramx_packed_library, below): the pack kernel of every direction then builds the flank windows
 * straight from the 2-bit payload; the one-byte-per-base form never exists on the host or the device */
struct ramx_packed_library;
int ramx_dev_load_library_packed(ramx_dev *d, const struct ramx_packed_library *pl);

/* One flank (an extendable core seen from one direction), already resolved by the host:
 * the base aligned to band cell (row r, offset o) is library[start + step*(o + r)], complemented
 * if compl != 0, and is inside the flank iff t_lo <= o + r <= t_hi  (SURVEY.md App. D rule 1). */
typedef struct ramx_flank
{
  int64_t start;
  int32_t t_lo, t_hi;
  int8_t  step;       /* +1 / -1 */
  int8_t  compl_;     /* reverse-strand core: complement the base */
  int8_t  pad_[6];
} ramx_flank;

/* Host-side resolution of the cores that are extendable in `direction` into flank descriptors
 * (reference bnw_extend.c:778-788,824-868).  flanks / core_index must hold cores->n entries;
 * core_index[i] is the position in the core list of flank i.  Returns the number of flanks. */
int ramx_resolve_flanks(int direction, const ramx_flat_cores *cores, int bandwidth, int L,
                        ramx_flank *flanks, int32_t *core_index);

/* upload (per direction): flank descriptors -> HBM, pack kernel builds the transposed 4-bit
 * windows, DP state / vote / control buffers are (re)initialised. */
int ramx_dev_begin_direction(ramx_dev *d, const ramx_flank *flanks, int32_t n_flanks, const ramx_params *p);

/* run_direction: the whole column loop, asynchronous on the device's stream with the stop rule
 * evaluated on the device; returns when the loop has stopped. */
int ramx_dev_run_direction(ramx_dev *d, ramx_run_info *info);

/* download: consensus bases of the executed columns (cons[0..rows_executed)), and the
 * trimmed per-flank high score / position (trimmed_sequence_high_score[_pos], ram_extend.c:902-903). */
int ramx_dev_download(ramx_dev *d, int8_t *cons, int32_t cons_cap, int32_t *trim_high, int32_t *trim_pos);

/* debug / test hook: current DP row state of one flank as [2W+1][2] int32 + high,pos.  The device stores each
 * cell transformed: (m, e) = (max(sub,gap), max(sub+gapopen,gap)+gapextn) -- see csrc/ramx_kernels_common.h. */
int ramx_dev_peek_state(ramx_dev *d, int32_t flank, int32_t *cells, int32_t *high, int32_t *pos);

/* debug / test hook: the transposed 4-bit flank windows and the bounds as the last pack call on this device left them -- a
 * direction's (begin_direction and the pieces packed while it ran), a replay's or ramx_dev_tsd's.  Nothing is packed here: how
 * many words a run chose to pack is part of what is read.  A piece still being packed on the second stream is waited for.
 * *packed_words = K and *lanes = Np are written first; words receives [K][Np] uint32 (nibble i of word k of lane n is flank
 * position t = 8k + i - W - 8, class 8 where there is no base), bounds [Np][2] int32 (t_lo + W, t_hi + W; (1, 0) for a lane
 * without a flank).  words_cap / lanes_cap are the buffers' capacities in words / lanes: RAMX_ERR_ARG, with the two counts
 * written, when they are too small or a buffer is NULL (a first call with capacity 0 sizes the buffers); RAMX_ERR_ARG also for
 * a device on which nothing has been packed yet. */
int ramx_dev_peek_windows(ramx_dev *d, uint32_t *words, int64_t words_cap, int32_t *bounds, int64_t lanes_cap,
                          int32_t *packed_words, int32_t *lanes);

/* debug / test hook: with RAMX_CP_PEEK=1 in the environment the cell-parallel family kernel keeps the final DP row of
 * every flank of the last ramx_dev_run_families call; cells receives [2W+1][2] int32 in the (m, e) encoding of
 * ramx_dev_peek_state.  `flank` indexes the (padded) flank array of that call; d == NULL means the process-wide
 * session that seam 1 (ramx_extend_flat / ramx_extend_batch) runs on. */
int ramx_dev_peek_family_state(ramx_dev *d, int32_t flank, int32_t *cells);

/* -outmat support (reference ram_extend.c:1122-1132, bnw_extend.c:1027-1044): with a trace callback set, a direction runs
 * one column launch at a time and hands every executed row to the callback: the winning base, and per flank (in flank
 * order) the path code of each band cell (0: the substitution holds the cell's score, 1: the deletion, 2: the insertion),
 * the row's best score and its sequence index (row + offset).  d == NULL: the process-wide session of seam 1.  A
 * debugging aid: slow by construction.  cb == NULL switches it off. */
typedef void (*ramx_row_trace_cb)(int32_t row, int32_t besta, const int8_t *codes /* [n_flanks][2W+1] */,
                                  const int32_t *best_score, const int32_t *best_idx, void *user);
int ramx_dev_set_row_trace(ramx_dev *d, ramx_row_trace_cb cb, void *user);

/* Batch mode (no counterpart in the reference, whose wrapper util/extend-stk.pl:242-371 starts one
 * RAMExtend process per family): many families in ONE launch, one workgroup per family, every family with its own
 * consensus / vote / stop rule.  Flanks are family-major; every family starts at a multiple of 64 in the flank
 * array (pad with empty flanks: t_lo = 1, t_hi = 0) and has at most 512 flanks (else RAMX_ERR_UNSUPPORTED: run such
 * a family through seam 1).  Band widths 14, 20 and 40 with non-positive gap penalties keep the rows in registers
 * (infos[].persistent == 1); every other band width / gap sign streams them through L2 (persistent == 2).
 * cons is [n_families][L]; trim_* are per (padded) flank; infos per family.  The library must be loaded first. */
int ramx_dev_run_families(ramx_dev *d, const ramx_flank *flanks, int32_t n_padded, const int32_t *fam_first,
                          const int32_t *fam_count, int32_t n_families, const ramx_params *p,
                          ramx_run_info *infos, int8_t *cons, int32_t *trim_high, int32_t *trim_pos);

/* The same on the reference-like flat data model: family f = cores[f] on its own library sequence[f]; master[f] and
 * the cores' extension lengths / scores are updated exactly as ramx_extend_flat does for one family.  Families with
 * more than 512 extendable cores are run one by one.  Returns 0 or a negative error code; infos[f].ret is the per-family
 * return value of extend_alignment. */
typedef struct ramx_family
{
  ramx_flat_cores cores;
  const int8_t *sequence;
  uint64_t seq_len;
  int8_t *master;
} ramx_family;
int ramx_extend_batch(int direction, ramx_family *families, int32_t n_families, const ramx_params *p, ramx_run_info *infos);

/* Support profile of an extension: every flank's band replayed along a GIVEN consensus (no vote, no stop rule), per column
 * the quantities the loop decides from.  For row r = 0 .. rows-1, exactly as the loop computes them (ram_extend.c:1042-1062,
 * 1134-1151): total[a] is the true (int64) sum over the flanks of candidate a's contribution -- max(best_a, 0), or
 * high + CAPPENALTY where that is larger (the flank is then "capped" under a) --; base is the given cons[r]; n_capped counts
 * the flanks capped under base, n_new_high those whose kept row set a new per-flank high score, n_out_of_seq those whose kept
 * row has run out of sequence (gap state of the far edge cell < -279000; the far edge is band cell 2W for a flank as
 * ramx_resolve_flanks makes it for direction 1 -- step +1 uncomplemented or step -1 complemented -- and cell 0 otherwise).
 * The struct is 48 bytes without padding. */
typedef struct ramx_col_profile
{
  int64_t total[4];
  int32_t base, n_capped, n_new_high, n_out_of_seq;
} ramx_col_profile;

/* The replay on the device.  Flank layout as in ramx_dev_run_families: tiles of 64 flanks, every family starting at a
 * multiple of 64, padding flanks (beyond a family's count) contribute to nothing and are counted nowhere -- but a family
 * may have ANY number of flanks, and every band width >= 1 and gap sign is served by the same entry (rows on chip for W = 14,
 * 20, 40, 80 without a positive gap penalty, otherwise in a global buffer private to each wave).  cons is [n_families][L] (p->L), rows[f] <= L the columns to replay of family f; it need not be the
 * consensus the vote would choose.  cols is [n_families][L]: only the first rows[f] entries of a family are written.
 * last_uncapped_row is [n_padded] (may be NULL): the last row at which the flank was not capped under the column's base, -1
 * if none (and for padding flanks).  row_best / row_best_idx: both NULL, or both [max_f rows[f]][n_padded] row-major (row r
 * of flank i at [r * n_padded + i]): the kept row's unclamped best score and its sequence index row + offset; entries of rows
 * beyond a family's rows[f] and of padding tiles are 0.  kernel_ms (may be NULL): HIP-event time of the replay and its
 * reduction.  The call is self-contained: it uploads the flanks and packs their windows itself from the library on the device
 * (ramx_dev_load_library*), so it can follow any direction, or none; a following ramx_dev_run_direction needs a new
 * ramx_dev_begin_direction.  With a communicator or mailbox route active the call is rank-local: the sums are those over
 * this rank's flanks and add up across ranks.  RAMX_ERR_ARG: a family not at a multiple of 64 or outside n_padded,
 * overlapping families, rows[f] outside [0, L], a consensus base outside 0..3, one row buffer without the other. */
int ramx_dev_profile(ramx_dev *d, const ramx_flank *flanks, int32_t n_padded, const int32_t *fam_first,
                     const int32_t *fam_count, int32_t n_families, const ramx_params *p,
                     const int8_t *cons, const int32_t *rows, ramx_col_profile *cols, int32_t *last_uncapped_row,
                     int32_t *row_best, int32_t *row_best_idx, double *kernel_ms);

/* Per-copy alignments of an extension: every flank's band replayed along a GIVEN consensus, then walked back from the
 * flank's end cell.  Positions are flank positions t = offset + row (ramx_flank): t may be negative, the reference's band may
 * step back into the core.
 *   End cell: end_row is the first row r < rows whose best cell score is strictly above every earlier row's and above 0 (the
 *   record setters of ram_extend.c:1140-1150); score is that maximum, end_idx = row + offset of that row's best cell (lowest
 *   offset on ties, bnw_extend.c:1020-1024).  Along the loop's own consensus with rows = ret these are the loop's trimmed
 *   high score and position.  No such row: end_row = -1, end_idx = -1, score = 0 -- the flank has no alignment.
 *   Walk back: the start state is gap iff gap > sub in the end cell (:1015).  Substitution state at (r, j): column r is
 *   matched to base t = j - W + r; go to (r-1, j); gap next iff S1 > S0 there (:950-956).  Gap state: del =
 *   max(S0(r-1,j+1)+go+ge, S1(r-1,j+1)+ge) for j < 2W, ins = max(S0(r,j-1)+go+ge, S1(r,j-1)+ge) for j > 0; an insertion iff
 *   ins > del (:1007): base t is inserted, go to (r, j-1); else column r is deleted, go to (r-1, j+1); gap next iff the
 *   extension term is strictly larger than the opening term (:896-904, :976-984).  On the boundary row at offset o >= 0 the
 *   first o bases are a leading insertion; in a cell outside the flank (it holds the matrix-edge fill, :990-994) columns 0..r
 *   are deletions.  The path's score -- matrix[cons[r]][base] over matched columns plus go + len * ge per run of gap moves,
 *   without go for a run that begins at the origin cell -- equals `score`.
 * start_idx is the first consumed position (end_idx + 1 if the path consumes none); consumed positions are contiguous up to
 * end_idx.  tail_ins: insertions after the last column move. */
typedef struct ramx_aln_end
{
  int32_t end_row, end_idx, score, start_idx, tail_ins;
} ramx_aln_end;
#define RAMX_ALN_DELETED INT32_MIN          /* col_idx: the column is deleted in this flank */
#define RAMX_ALN_NONE    (INT32_MIN + 1)    /* col_idx: a column above end_row, or a flank without an alignment */

/* The replay on the device.  Flank layout, argument checks and self-containedness as ramx_dev_profile (any number of flanks
 * per family, every band width >= 1 and gap sign; rank-local under a communicator).  ends is [n_padded]; col_idx / col_ins
 * are both NULL or both [max_f rows[f]][n_padded] row-major: col_idx the matched position of column r, RAMX_ALN_DELETED or
 * RAMX_ALN_NONE; col_ins the number of bases inserted, in path order, between the moves of column r - 1 and of column r (for
 * r = 0 the leading run).  Entries of the tiles of a family are all written (padding flanks and rows beyond rows[f]: no
 * alignment, RAMX_ALN_NONE, 0); entries of tiles outside every family are left as they are.  The decision codes (4 bits a
 * cell) live in a device buffer of at most RAMX_ALIGN_BYTES bytes (environment; default 1 GiB): tiles are processed in groups
 * that fit; RAMX_ERR_UNSUPPORTED if one tile alone does not.  kernel_ms (may be NULL): two values, the HIP-event times of the
 * forward kernels and of the walk kernels. */
int ramx_dev_align(ramx_dev *d, const ramx_flank *flanks, int32_t n_padded, const int32_t *fam_first,
                   const int32_t *fam_count, int32_t n_families, const ramx_params *p,
                   const int8_t *cons, const int32_t *rows, ramx_aln_end *ends, int32_t *col_idx, int32_t *col_ins,
                   double *kernel_ms);

/* Pileup of an extension: what the alignments of ramx_dev_align put into every column of a GIVEN consensus cons[0..rows).
 * Everything is defined on each flank's ramx_aln_end, col_idx[r], col_ins[r] and the path order of its inserted bases.
 *   Base class of flank position t: the code the alignment sees (complemented when compl is set); codes 0..3 are classes
 *   0..3 (A C G T), lower-case codes 4..7 are code - 4, everything else is class 4 (N, a position outside the flank's bounds
 *   t_lo..t_hi, a position outside the library).
 *   The run "before column r" is col_ins[r] (for r = 0 the leading run); tail_ins belongs to no column and is counted
 *   nowhere.  Padding flanks and flanks without an alignment contribute nothing.
 * The struct is 128 bytes without padding. */
#define RAMX_PILEUP_INS 4
typedef struct ramx_col_pileup
{
  int32_t base;                         /* cons[r] */
  int32_t cover;                        /* flanks with end_row >= r */
  int32_t match[5];                     /* column r matched to a base of class A C G T N */
  int32_t del;                          /* col_idx[r] == RAMX_ALN_DELETED */
  int32_t ins_open;                     /* flanks of the cover with col_ins[r] > 0 */
  int32_t ins_long;                     /* ... with col_ins[r] > RAMX_PILEUP_INS */
  int64_t ins_bases;                    /* sum of col_ins[r] over the cover */
  int32_t ins[RAMX_PILEUP_INS][5];      /* slot k: class of the k-th base, in path order (increasing t), of the run before column r */
} ramx_col_pileup;

/* The pileup on the device: ramx_dev_align's forward pass and walk, then one wave per tile counts its 64 flanks' columns and a
 * second kernel adds the tiles of every family.  Flank layout, argument checks and self-containedness as ramx_dev_align.  cols
 * is [n_families][L]: only the first rows[f] entries of a family are written.  ends is [n_padded] or NULL: what ramx_dev_align
 * writes there.  The walked columns never exist for the whole flank set: they are held for one group of tiles at a time and
 * count, with the group's decision codes, against RAMX_ALIGN_BYTES (rows * 64 * (4 * (W / 4 + 1) + 8) bytes per tile;
 * RAMX_ERR_UNSUPPORTED if one tile alone does not fit); the grouping does not show in the result.  kernel_ms (may be NULL):
 * three values, the HIP-event times of the forward kernels, of the walk kernels, and of the pileup kernels and the sum.  With a
 * communicator or mailbox route active the call is rank-local and the counts add up across ranks. */
int ramx_dev_pileup(ramx_dev *d, const ramx_flank *flanks, int32_t n_padded, const int32_t *fam_first,
                    const int32_t *fam_count, int32_t n_families, const ramx_params *p,
                    const int8_t *cons, const int32_t *rows, ramx_col_pileup *cols, ramx_aln_end *ends, double *kernel_ms);

/* Re-call of a consensus from its pileup: one pass over the columns in order (plain host C).  Let c = cols[r].cover.
 *   1. c == 0: the column is kept as it is, and nothing is inserted before it.
 *   2. Inserted columns: for k = 0, 1, ... RAMX_PILEUP_INS - 1 let n_k = sum_b ins[k][b]; while 2 * n_k > c and some
 *      ins[k][0..3] > 0, emit the plurality base of ins[k][0..3] (the lowest code wins ties, N is never a candidate); stop at
 *      the first k that fails.
 *   3. The column itself is dropped iff 2 * del > c.  Otherwise its base is the plurality of match[0..3]: the current base
 *      if it is among the maxima or if all four counts are 0, else the lowest code among the maxima.
 *   4. The output is cut to its first L columns.
 * Exactly half is not a majority anywhere.  out holds L entries; returns the new length. */
int32_t ramx_recall_consensus(const int8_t *cons, int32_t rows, const ramx_col_pileup *cols, int32_t L, int8_t *out);

/* Refinement: cons_0 = cons_in; for i = 0, 1, ...: P_i = pileup(cons_i), cons_{i+1} = recall(cons_i, P_i).  If cons_{i+1} ==
 * cons_i: converged = 1, the result is cons_i with P_i, replays = i + 1.  Else if i + 1 == max_replays: converged = 0, the
 * result is cons_i with P_i (the last consensus that has a pileup), replays = i + 1.  Families proceed independently, and a
 * converged family is not replayed again.  max_replays >= 1; 1 is "pileup only".  cons_in / cons_out are [n_families][L],
 * rows_in / rows_out / replays / converged [n_families], cols [n_families][L] (the result's pileup), ends [n_padded] or NULL
 * (the alignments along the result).  The library's windows are packed once per call.  kernel_ms as ramx_dev_pileup, summed
 * over the replays.  RAMX_ERR_UNSUPPORTED with a communicator or mailbox route active: the re-call needs global counts. */
int ramx_dev_refine(ramx_dev *d, const ramx_flank *flanks, int32_t n_padded, const int32_t *fam_first,
                    const int32_t *fam_count, int32_t n_families, const ramx_params *p,
                    const int8_t *cons_in, const int32_t *rows_in, int32_t max_replays,
                    int8_t *cons_out, int32_t *rows_out, int32_t *replays, int32_t *converged,
                    ramx_col_pileup *cols, ramx_aln_end *ends, double *kernel_ms);

/* Dinucleotide pileup of an extension: the joint count of what a copy puts into two ADJACENT columns of a GIVEN consensus
 * cons[0..rows) -- what the marginals of ramx_col_pileup cannot give.  Everything is defined on each flank's ramx_aln_end,
 * col_idx[r] and col_ins[r]; base classes are the pileup's.  Record r describes the pair of ROWS (r, r + 1); which of the two is
 * 5' is the caller's business (rows_reversed, as in ramx_dev_copy_stats).  both == adjacent + split + gapped and adjacent ==
 * sum of di for every record; the record of row rows - 1 has next = -1 and zeros.  Padding flanks and flanks without an
 * alignment contribute nothing.  The struct is 128 bytes without padding. */
typedef struct ramx_col_dinuc
{
  int32_t base;                         /* cons[r] */
  int32_t next;                         /* cons[r + 1]; -1 for r == rows - 1 */
  int32_t both;                         /* flanks with end_row >= r + 1 */
  int32_t adjacent;                     /* ... both columns matched (neither RAMX_ALN_DELETED) and col_ins[r + 1] == 0 */
  int32_t split;                        /* ... both columns matched and col_ins[r + 1] > 0 */
  int32_t gapped;                       /* ... at least one of the two deleted */
  int32_t di[5][5];                     /* over the adjacent flanks: class x in row r and class y in row r + 1 */
  int32_t reserved;                     /* written as 0 */
} ramx_col_dinuc;

/* The dinucleotide pileup on the device: ONE forward pass and ONE walk per group of tiles, as ramx_dev_pileup, then the pileup
 * kernel (only if cols is given) and the dinucleotide kernel on the same walked columns: one wave per tile counts the row pairs
 * of its 64 flanks, and a second kernel adds the tiles of every family.  Flank layout, argument checks, self-containedness, the
 * budget of RAMX_ALIGN_BYTES and rank-local behaviour exactly as ramx_dev_pileup; the grouping does not show in the result.
 * cols (may be NULL) and di are [n_families][L]: only the first rows[f] entries of a family are written.  ends is [n_padded] or
 * NULL.  kernel_ms (may be NULL): FOUR values, the HIP-event times of the forward kernels, of the walk kernels, of the pileup
 * kernels and their sum (0 without cols), and of the dinucleotide kernels and their sum. */
int ramx_dev_dinuc(ramx_dev *d, const ramx_flank *flanks, int32_t n_padded, const int32_t *fam_first,
                   const int32_t *fam_count, int32_t n_families, const ramx_params *p,
                   const int8_t *cons, const int32_t *rows, ramx_col_pileup *cols, ramx_col_dinuc *di, ramx_aln_end *ends,
                   double *kernel_ms);

/* CpG-aware re-call of a consensus from its pileup and its dinucleotide pileup (plain host C, exact integers).
 *   Pass 1 is ramx_recall_consensus, rule for rule: for every current row it decides whether the row is kept, with which base
 *   (its plain call), and which inserted columns are emitted before it (a row the cut to L columns does not reach is not kept).
 *   Pass 2 runs over every row pair (r, r + 1) of which both rows are kept and no inserted column is emitted before row r + 1.
 *   In reading order the 5' column is r and the 3' column r + 1, D[x][y] = di[r].di[x][y] (rows_reversed == 0), or the 5'
 *   column is r + 1, the 3' column r and D[x][y] = di[r].di[y][x] (rows_reversed == 1).  With (a, b) the plain calls of the 5'
 *   and 3' columns the pair is tested iff a is C or T and b is G or A.  Over x, y < 4 (class 4 is ignored), in int64, with
 *   M[c][s] = matrix[c * 100 + s]:
 *     S_plain = sum D[x][y] * (M[a][x] + M[b][y])
 *     S_CG    = sum D[x][y] * (mC(x) + mG(y)),  mC(x) = cpg_ts if x is T else M[C][x],  mG(y) = cpg_ts if y is A else M[G][y]
 *   The pair is called CG iff (a, b) is (C, G) already or S_CG > S_plain, strictly.
 * A column cannot be the 3' column of one tested pair and the 5' column of another: the 3' column's plain call is a purine, the
 * 5' column's a pyrimidine.  Tested pairs are therefore disjoint and the order of pass 2 does not matter.  cpg_ts is the score a
 * deaminated base (T for the C, A for the G) gets under the CpG hypothesis, in place of matrix[C][T] / matrix[G][A]; 0 says that
 * a deaminated CpG neither supports nor contradicts the call.  n_cpg (may be NULL): the pairs that came out as CG.  out holds L
 * entries; returns the new length, which is ramx_recall_consensus's. */
int32_t ramx_recall_cpg(const int8_t *cons, int32_t rows, const ramx_col_pileup *cols, const ramx_col_dinuc *di,
                        int32_t rows_reversed, const int32_t *matrix, int32_t cpg_ts, int32_t L, int8_t *out, int32_t *n_cpg);

/* CpG-aware refinement: ramx_dev_refine, word for word, with ramx_recall_cpg(rows_reversed, p->matrix, cpg_ts) as the re-call
 * and ramx_dev_dinuc as the replay.  cols and di are [n_families][L] (the result's pileup and dinucleotide pileup), n_cpg
 * [n_families]: the CG pairs of the re-call of the result (those the result holds when it has converged).  kernel_ms as
 * ramx_dev_dinuc, summed over the replays. */
int ramx_dev_refine_cpg(ramx_dev *d, const ramx_flank *flanks, int32_t n_padded, const int32_t *fam_first,
                        const int32_t *fam_count, int32_t n_families, const ramx_params *p,
                        const int8_t *cons_in, const int32_t *rows_in, int32_t max_replays, int32_t rows_reversed, int32_t cpg_ts,
                        int8_t *cons_out, int32_t *rows_out, int32_t *replays, int32_t *converged,
                        ramx_col_pileup *cols, ramx_col_dinuc *di, int32_t *n_cpg, ramx_aln_end *ends, double *kernel_ms);

/* Per-copy statistics of an extension: how the alignment of every flank to a GIVEN consensus cons[0..rows) divides up -- the
 * pileup's transpose, summed over the rows of a flank where the pileup sums over the flanks of a column.  Everything is defined
 * on the flank's ramx_aln_end, col_idx[r] and col_ins[r]; base classes are the pileup's.
 *   CpG: with rows_reversed == 0 the rows run 5'->3' (the right extension), with 1 against the reading order (the left
 *   extension, whose rows run outward from the core): the next column of r in reading order is r + 1, or r - 1 when reversed.
 *   Column r lies in a CpG if cons[r] is C and its next column exists and is G, or if cons[r] is G and its previous column
 *   exists and is C; only columns < rows exist.
 * match + ts + tv + n_match + del == cols for every flank.  Padding flanks and flanks without an alignment: all zero.  The
 * struct is 48 bytes without padding. */
typedef struct ramx_copy_stats
{
  int32_t cols;       /* columns the copy's path covers: end_row + 1; 0 without an alignment */
  int32_t match;      /* column matched to a base of class A C G T equal to cons[r] */
  int32_t ts;         /* ... to the other purine / the other pyrimidine (A<->G, C<->T) */
  int32_t tv;         /* ... to a base of the other kind */
  int32_t n_match;    /* column matched to class 4 (N, outside the flank's bounds, outside the library) */
  int32_t del;        /* col_idx[r] == RAMX_ALN_DELETED, r <= end_row */
  int32_t del_open;   /* ... of which r == 0, or col_idx[r-1] != RAMX_ALN_DELETED, or col_ins[r] > 0 */
  int32_t ins;        /* sum of col_ins[r] over r <= end_row (tail_ins is counted nowhere, as in the pileup) */
  int32_t ins_open;   /* rows r <= end_row with col_ins[r] > 0 */
  int32_t cpg_cols;   /* columns counted in match + ts + tv that lie in a CpG of the consensus */
  int32_t cpg_ts;     /* ... of which counted in ts */
  int32_t score;      /* ramx_aln_end.score */
} ramx_copy_stats;

/* The statistics on the device: ramx_dev_align's forward pass and walk, then one wave per tile with one lane per flank goes down
 * the tile's columns and every lane writes its flank's record.  Flank layout, argument checks, self-containedness and the
 * budget of RAMX_ALIGN_BYTES as ramx_dev_pileup.  stats is [n_padded]: the records of the tiles of every family are all
 * written, those of tiles outside every family are left as they are; ends is [n_padded] or NULL.  A family with rows[f] == 0 is
 * answered on the host (zero records, no alignment).  kernel_ms (may be NULL): three values, the HIP-event times of the forward
 * kernels, of the walk kernels and of the statistics kernel.  With a communicator or mailbox route active the call is
 * rank-local, which is all there is to it: the records are per flank. */
int ramx_dev_copy_stats(ramx_dev *d, const ramx_flank *flanks, int32_t n_padded, const int32_t *fam_first,
                        const int32_t *fam_count, int32_t n_families, const ramx_params *p,
                        const int8_t *cons, const int32_t *rows, int32_t rows_reversed,
                        ramx_copy_stats *stats, ramx_aln_end *ends, double *kernel_ms);

/* Kimura two-parameter divergence of a copy from its consensus, in percent (plain host C).  sites = match + ts + tv,
 * p = ts / sites, q = tv / sites, a = 1 - 2p - q, b = 1 - 2q: -1/2 ln(a sqrt(b)) * 100; -1 (undefined) if sites == 0, a <= 0
 * or b <= 0. */
double ramx_copy_kimura(const ramx_copy_stats *s);
/* The mean of ramx_copy_kimura over the copies with sites >= max(min_sites, 1) and a defined value; n_used (may be NULL)
 * receives their number.  0.0 when there are none. */
double ramx_family_divergence(const ramx_copy_stats *stats, int32_t n, int32_t min_sites, int32_t *n_used);

/* Co-segregation of an extension's variants: do the copies that differ from the consensus at column i also differ at column j?
 * The pileup and the per-copy statistics look at every position on its own; this is their second-order sibling.  A PLANE is
 * one bit per flank of a family: bit i is set iff flank i is a non-padding flank with an alignment, row <= its end_row, and
 *   cls 0..3: column row is matched to a base of class A C G T (the pileup's classes)
 *       4: matched to class N
 *       5: deleted (col_idx[row] == RAMX_ALN_DELETED)
 *       6: covered (end_row >= row)
 *       7: bases inserted before it (col_ins[row] > 0)
 * so every plane is a subset of the cover plane of its row, and tail_ins sets nothing. */
typedef struct ramx_plane { int32_t row, cls; } ramx_plane;
#define RAMX_PLANE_COVER 6
#define RAMX_LINKAGE_MAX_PLANES 2048        /* planes of one family in one Gram matrix: a 16 MB result */

/* The planes on the device: ramx_dev_pileup with a fourth stage.  Arguments, checks, self-containedness, the budget of
 * RAMX_ALIGN_BYTES and what is returned in cols / ends exactly as ramx_dev_pileup (rank-local under a communicator).  The fourth
 * stage takes, per tile and row, the eight ballots of one wave and keeps the planes of ALL rows and classes of every family
 * RESIDENT on the device, rows[f] * 8 * tiles_f 64-bit words a family, so that variants can be chosen afterwards without a
 * second replay.  That buffer does not count against RAMX_ALIGN_BYTES; it has a cap of its own, RAMX_LINKAGE_BYTES
 * (environment; default 2 GiB): RAMX_ERR_UNSUPPORTED beyond it.  The planes stay resident until the next replay that runs on
 * this device (ramx_dev_profile / _align / _pileup / _copy_stats / _refine / _planes), ramx_dev_begin_direction or
 * ramx_dev_run_families.  kernel_ms (may be NULL): FOUR values, forward, walk, pileup + sum, planes. */
int ramx_dev_planes(ramx_dev *d, const ramx_flank *flanks, int32_t n_padded, const int32_t *fam_first,
                    const int32_t *fam_count, int32_t n_families, const ramx_params *p,
                    const int8_t *cons, const int32_t *rows, ramx_col_pileup *cols, ramx_aln_end *ends, double *kernel_ms);

/* The Gram matrix of chosen planes of the resident replay (n_families as in that ramx_dev_planes call).  Family f's planes are
 * planes[plane_first[f] .. + plane_count[f]): strictly increasing in (row, cls), row < rows[f], cls in 0..7, at most
 * RAMX_LINKAGE_MAX_PLANES of them -- anything else is RAMX_ERR_ARG; RAMX_ERR_STATE without resident planes.  All lists are
 * checked before anything is launched or written.  co + co_first[f] receives [P_f][P_f] row-major: entry [p][q] is the number
 * of flanks of the family that have both bits set -- symmetric, the diagonal a plane's own count; exact integers (popcounts
 * summed over the tiles in registers, no atomics), so the result does not depend on any order.  bits (may be NULL) receives
 * the chosen planes' words themselves, family f at bits_first[f] as [P_f][T_f], T_f = (fam_count[f] + 63) / 64, bit i % 64 of
 * word i / 64 flank i.  A family with P_f == 0 or without tiles writes nothing.  The call may be repeated with other lists.
 * Rank-local under a communicator: for equal plane lists the counts add up across ranks. */
int ramx_dev_plane_gram(ramx_dev *d, int32_t n_families, const ramx_plane *planes, const int32_t *plane_first,
                        const int32_t *plane_count, int32_t *co, const int64_t *co_first, uint64_t *bits, const int64_t *bits_first);
/* HIP-event time (ms) of the Gram kernel of the last ramx_dev_plane_gram on this device; 0 if none was launched. */
double ramx_dev_plane_gram_ms(ramx_dev *d);

/* Which planes to ask for (plain host C): the variants of a pileup.  The candidates of row r are cls a in 0..3 with
 * a != cons[r] (count match[a]), cls 5 (count del) and cls 7 (count ins_open); class N and the consensus base are never
 * candidates.  A candidate is a VARIANT iff count >= min_count and 1000 * count >= min_permille * cover.  If more than
 * max_variants qualify, those with the largest count are kept, ties to the lower (row, cls).  out (room for 2 * max_variants)
 * receives, sorted by (row, cls), the variants and the cover plane (r, 6) of every row that has one; returns their number. */
int32_t ramx_select_planes(const int8_t *cons, int32_t rows, const ramx_col_pileup *cols, int32_t min_count, int32_t min_permille,
                           int32_t max_variants, ramx_plane *out);

/* The pair statistic (plain host C) over every pair of variant planes p < q (indices into planes[0..P), cls != 6) on DIFFERENT
 * rows whose rows' cover planes cp, cq are in the list: among the n = co[cp][cq] copies that cover both columns, n_p =
 * co[p][cq] carry the first variant, n_q = co[q][cp] the second and n_pq = co[p][q] both.  expected = n_p * n_q / n;
 * mlog10p = -log10 of the hypergeometric upper tail P(X >= n_pq), summed in log space with lgamma; 0 when n == 0 or n_pq == 0.
 * Pairs with mlog10p >= min_mlog10p are written to out[0..cap) in (p, q) order -- not sorted by score; the return value is
 * their number, even beyond cap.  There is NO multiple-testing correction: P (P - 1) / 2 pairs are tested, and the threshold is
 * the caller's to set with that in mind. */
typedef struct ramx_link { int32_t p, q, n, n_p, n_q, n_pq; double expected, mlog10p; } ramx_link;
int32_t ramx_link_pairs(const ramx_plane *planes, int32_t P, const int32_t *co, double min_mlog10p, ramx_link *out, int32_t cap);

/* Linkage sink of seam 1, as the other sinks: with a sink set, per direction and family that has run, along the kept consensus
 * (rows = ret): ramx_dev_planes, ramx_select_planes(min_count, min_permille, max_variants) on the pileup it returned, and
 * ramx_dev_plane_gram of the selection.  co is [n_planes][n_planes].  A direction without an extendable core or with ret = 0
 * is answered on the host with n_planes = 0.  With a communicator or mailbox route active the direction fails with
 * RAMX_ERR_UNSUPPORTED: the selection needs the counts of every rank.  max_variants is held to RAMX_LINKAGE_MAX_PLANES / 2 (the
 * cover planes double the list).  cb == NULL (the default): off. */
typedef struct ramx_linkage
{
  int32_t direction, family /* index in a batch, else 0 */, rows /* = ret */, n_planes;
  const int8_t *cons;                 /* [rows] */
  const ramx_col_pileup *cols;        /* [rows] */
  const ramx_plane *planes;           /* [n_planes] */
  const int32_t *co;                  /* [n_planes][n_planes] */
} ramx_linkage;
typedef void (*ramx_linkage_cb)(const ramx_linkage *lk, void *user);
void ramx_set_linkage_sink(ramx_linkage_cb cb, void *user, int32_t min_count, int32_t min_permille, int32_t max_variants);

/* Subfamilies of an extension: the copies of a family split by the variants they carry, the step after the linkage.  For one
 * family and one consensus, planes[0..P) is a list as ramx_select_planes returns it: variants (cls != 6) and the cover plane
 * (row, 6) of every row that has a variant.  The variants in list order are v = 0..V-1, cov(v) is the cover plane of v's row;
 * for copy i, x_i[v] is its bit in plane v and c_i[v] its bit in cov(v).
 *   Pattern: a bit per variant, pat_k[v]; K patterns, 1 <= K <= RAMX_SUBFAM_MAX.  Pattern 0 starts empty: the consensus itself.
 *   Distance: d(i, k) = the number of variants v with c_i[v] = 1 and x_i[v] != pat_k[v]; rows the copy does not cover count
 *   nothing.
 *   Assignment: label_i = argmin_k d(i, k), ties to the lowest k.  A non-padding copy without an alignment has d = 0 everywhere
 *   and label 0; padding flanks get label -1 and belong to no group.
 *   Counts: for every plane p of the list (variants AND covers) and every k, cnt[k][p] is the number of copies with label k
 *   whose bit in p is set; size[k] the number of copies with label k.
 *   Update: pat_k[v] = 1 iff 2 * cnt[k][v] > cnt[k][cov(v)] -- exactly half is not a majority, as in ramx_recall_consensus; a
 *   group with size[k] = 0 keeps its pattern.
 *   Iteration: assign, count; then update, assign, count again ... until an assignment after the first changes no label
 *   (converged = 1) or max_iter assignments have been made (converged = 0).  With K = 1 no assignment can change a label: the
 *   first one ends the family, converged = 1.  iterations is the number of assignments made; labels, counts and sizes are those
 *   of the last assignment and patterns_out the patterns it used (for a converged family also their own update).  Families
 *   proceed independently. */
#define RAMX_SUBFAM_MAX 8

/* The initial patterns (plain host C) from the output of ramx_link_pairs at the caller's threshold: links[0..n_links) with p, q
 * indices into planes[0..P).  The connected components of the graph whose edges are those pairs, the components with at least
 * two variants kept, ordered by decreasing size with ties to the lowest member, the first K - 1 of them kept: pattern j + 1
 * carries exactly the variants of component j, pattern 0 none.  Returns the number of patterns K' = 1 + kept components (<= K)
 * and writes init as [V][K'] bytes (0 / 1; room for V * K), V the variants of the list in list order; component (may be NULL)
 * receives, per variant, the pattern that carries it or 0.  0 for K outside 1..RAMX_SUBFAM_MAX or a link outside the list. */
int32_t ramx_link_components(const ramx_plane *planes, int32_t P, const ramx_link *links, int32_t n_links, int32_t K,
                             uint8_t *init, int32_t *component);

/* The iteration on the resident planes of the last ramx_dev_planes (n_families as in that call); plane lists as
 * ramx_dev_plane_gram, with the same checks -- RAMX_ERR_STATE without resident planes, RAMX_ERR_ARG for a bad list -- and
 * RAMX_ERR_ARG for a variant whose row's cover plane is not in the list, for K outside 1..RAMX_SUBFAM_MAX and for max_iter < 1.
 * Everything is checked before anything is launched or written.  With V_f variants and P_f planes in family f's list, and
 * v0(f) = sum of V_g, p0(f) = sum of P_g over g < f: init and patterns_out hold family f at K * v0(f) as [V_f][K] bytes
 * (0 / 1), cnt_out at K * p0(f) as [K][P_f], size_out is [n_families][K], iterations / converged [n_families], labels
 * [n_padded] of that ramx_dev_planes call (-1 for padding flanks and outside every family).  One wave per tile assigns (one lane
 * per flank, the distances in registers, the group masks as ballots); one wave per listed plane counts popcount(plane & mask)
 * over the family's tiles; between two assignments only the per-tile change counts and the counts come to the host, where the
 * update rule runs.  Exact integers, no atomics.  The planes stay resident and untouched.  Rank-local under a communicator. */
int ramx_dev_subfamilies(ramx_dev *d, int32_t n_families, const ramx_plane *planes, const int32_t *plane_first,
                         const int32_t *plane_count, const uint8_t *init, int32_t K, int32_t max_iter, int32_t *labels,
                         uint8_t *patterns_out, int32_t *cnt_out, int32_t *size_out, int32_t *iterations, int32_t *converged);
/* The group masks of the last ramx_dev_subfamilies (a diagnostic): mask receives [K][T_f] words, bit i % 64 of word i / 64 of
 * plane k set iff flank i of the family has label k.  RAMX_ERR_STATE without such a result. */
int ramx_dev_subfam_masks(ramx_dev *d, int32_t family, uint64_t *mask);
/* HIP-event times (ms) of the assign and of the count kernels of the last ramx_dev_subfamilies, each summed over its
 * iterations; 0 if none was launched. */
void ramx_dev_subfam_ms(ramx_dev *d, double ms[2]);

/* Subfamily sink of seam 1, as the other sinks (the sixth, after the linkage sink): with a sink set, per direction and family
 * that has run, along the kept consensus (rows = ret): ramx_dev_planes, ramx_select_planes(min_count, min_permille,
 * max_variants), ramx_dev_plane_gram, ramx_link_pairs at min_mlog10p, ramx_link_components with K and ramx_dev_subfamilies with
 * the K' it returned and max_iter.  The flanks of every group with size[k] >= min_members are then gathered into a family of
 * its own and ONE ramx_dev_refine call over all of them, starting from the kept consensus with max_replays, gives every kept
 * group its own consensus and pileup.  dist is [n_flanks][K]: d(i, k) to the patterns handed over.  A direction without an
 * extendable core or with ret = 0 is answered on the host: K = 1, every copy in group 0, no variant, no kept group.  With a
 * communicator or mailbox route active the direction fails with RAMX_ERR_UNSUPPORTED, as the linkage sink.  If the linkage
 * sink is set too, the planes and the Gram matrix are computed once for each.  cb == NULL (the default): off. */
typedef struct ramx_subfam_group
{
  int32_t group, size, refined_rows, replays, converged;
  const int8_t *refined_cons;             /* [refined_rows] */
  const ramx_col_pileup *refined_cols;    /* [refined_rows] */
} ramx_subfam_group;
typedef struct ramx_subfamilies
{
  int32_t direction, family /* index in a batch, else 0 */, rows /* = ret */, n_flanks, n_planes, n_variants, K, iterations, converged,
          n_groups /* kept: size >= min_members */;
  const int8_t *cons;                 /* [rows] */
  const ramx_flank *flanks;           /* [n_flanks], in the coordinates of the family's own library */
  const int32_t *core_index;          /* [n_flanks] */
  const ramx_plane *planes;           /* [n_planes] */
  const int32_t *labels;              /* [n_flanks] */
  const uint8_t *patterns;            /* [n_variants][K] */
  const int32_t *cnt;                 /* [K][n_planes] */
  const int32_t *size;                /* [K] */
  const int32_t *dist;                /* [n_flanks][K] */
  const ramx_subfam_group *groups;    /* [n_groups], ascending in group */
} ramx_subfamilies;
typedef void (*ramx_subfam_cb)(const ramx_subfamilies *sf, void *user);
void ramx_set_subfam_sink(ramx_subfam_cb cb, void *user, int32_t min_count, int32_t min_permille, int32_t max_variants,
                          double min_mlog10p, int32_t K, int32_t max_iter, int32_t min_members, int32_t max_replays);

/* Target-site duplications of the extended copies: the short direct repeat an insertion leaves immediately outside both termini
 * of the element.  Everything above looks at one direction of an extension; this looks at an extended copy as a whole element
 * with two ends, after both directions.  Exact integer arithmetic, every copy on its own.
 *   Site: the element occupies library positions lo..hi inclusive on the forward strand of the library; an empty element has
 *   lo == hi + 1.  seq_lo <= lo, lo <= hi + 1, hi <= seq_hi, else RAMX_ERR_ARG.
 *   Class of position p: library codes 0..3 are classes 0..3, codes 4..7 are code - 4, everything else is class 4: any other
 *   code, a position outside [seq_lo, seq_hi], a position outside the library.  Two positions AGREE iff both classes are below 4
 *   and equal.
 *   Candidate (dl, dr, k), |dl|, |dr| <= slack, kmin <= k <= kmax: the left word is positions lo + dl - k + j, the right word
 *   positions hi + 1 + dr + j, j = 0..k-1; mm is the number of j that do not agree.  With m(k) = mm_div ? k / mm_div : 0 the
 *   candidate is admissible iff (i) lo + dl <= hi + 1 + dr, (ii) j = 0 and j = k - 1 agree, (iii) mm <= m(k).  Its quality is
 *   q = 2 (k - 2 mm) - |dl| - |dr|.
 *   Best candidate: the largest q; ties to the smallest |dl| + |dr|, then the largest k, then the smallest dl, then the smallest
 *   dr -- a total order, so the record is unique.  All zeros when no candidate is admissible.
 * Parameters: slack 0..7, kmin 1..32, kmax kmin..32, mm_div 0 or >= 4; anything else is RAMX_ERR_ARG, raised before anything is
 * launched or written.  Defaults: 3, 4, 20, 10. */
typedef struct ramx_tsd_params { int32_t slack, kmin, kmax, mm_div; } ramx_tsd_params;
typedef struct ramx_tsd_site { int64_t lo, hi, seq_lo, seq_hi; } ramx_tsd_site;       /* 32 bytes */
typedef struct ramx_tsd { int32_t k, mm, dl, dr; } ramx_tsd;                          /* 16 bytes */

/* The records on the device, from the library it holds (ramx_dev_load_library*, either form): the two outside windows of every
 * site are packed as flanks by the pack kernels of the extension loop, then one lane per site scores every candidate in
 * registers and writes its record.  Self-contained like the replays (a following ramx_dev_run_direction needs a new
 * ramx_dev_begin_direction; resident bit planes are dropped); rank-local under a communicator, which is all there is to it: the
 * records are per site.  n_sites == 0 returns RAMX_OK and launches nothing.  kernel_ms (may be NULL): two values, the HIP-event
 * times of the pack of the 2 * n_sites windows and of the TSD kernel. */
int ramx_dev_tsd(ramx_dev *d, const ramx_tsd_site *sites, int32_t n_sites, const ramx_tsd_params *params, ramx_tsd *out,
                 double *kernel_ms);

/* One site per core, in list order, from cores that both directions have extended (plain host C): orient == 0: lo = left_pos -
 * left_len, hi = right_pos + right_len; otherwise lo = right_pos - right_len, hi = left_pos + left_len -- the extents the
 * reference prints (ram_extend.c:721-727); seq_lo / seq_hi are the core's lower / upper, the bounds the loop never reads past.
 * out holds cores->n sites; returns their number. */
int32_t ramx_tsd_sites(const ramx_flat_cores *cores, ramx_tsd_site *out);

/* What a family's records say together (plain host C): hist[k] counts the records by k, 0..32; mode is the k >= 1 with the
 * largest count, ties to the larger k, 0 if there is none, and mode_count that count; null[k] = n * min(1, (2 slack + 1)^2 *
 * sum_{j <= m(k)} C(k, j) 3^j / 4^k), the number of copies expected to show a word of that length by chance (null[0] = 0).
 * RAMX_ERR_ARG for bad parameters, n < 0 or a record with k outside 0..32. */
typedef struct ramx_tsd_hist { int32_t hist[33]; int32_t mode, mode_count, pad_; double null[33]; } ramx_tsd_hist;
int ramx_tsd_summary(const ramx_tsd *records, int32_t n, const ramx_tsd_params *params, ramx_tsd_hist *out);

/* The termini of the extended consensus (plain host C).  cons_left / cons_right are the kept columns of the two directions as
 * the loop hands them over (codes 0..3), ret_left / ret_right their numbers; the left rows run outward from the core.  five
 * receives the first min(T, ret_left) bases of the extended consensus in reading order, three the last min(T, ret_right), both
 * as upper-case characters with a terminating 0 (room for T + 1 each).  tir_len: the number of leading j < min(ret_left,
 * ret_right, 32) with cons_left[ret_left - 1 - j] == 3 - cons_right[ret_right - 1 - j], stopping at the first failure -- the
 * length of a terminal inverted repeat.  RAMX_ERR_ARG for T < 0, a negative length or a missing pointer. */
int ramx_termini(const int8_t *cons_left, int32_t ret_left, const int8_t *cons_right, int32_t ret_right, int32_t T,
                 char *five, char *three, int32_t *tir_len);

/* Seam 1, called after both extension calls: ramx_tsd_sites of the cores and ramx_dev_tsd on the session's device.  out holds
 * one record per core in list order.  The library the device holds is used when the cache key of seam 1 matches (the same
 * buffer the two directions ran on; the packed twin of seqLib; for the batch the concatenated library ramx_extend_batch leaves
 * there, with the families' offsets), otherwise it is uploaded -- and is then the resident one for the calls that follow.
 * ramx_tsd_alignment walks the whole core list; ramx_tsd_batch writes family f's records behind those of the families before it
 * (sum of their cores.n).  Return RAMX_OK or a negative error code. */
int ramx_tsd_flat(const ramx_flat_cores *cores, const int8_t *sequence, uint64_t seq_len, const ramx_tsd_params *params, ramx_tsd *out);
int ramx_tsd_alignment(struct coreAlignment *coreAlign, struct sequenceLibrary *seqLib, const ramx_tsd_params *params, ramx_tsd *out);
int ramx_tsd_batch(const ramx_family *families, int32_t n_families, const ramx_tsd_params *params, ramx_tsd *out);

/* Tandem periodicity of the extended copies: did the extension run into a tandem repeat -- a (CA)n, a poly-A tail, the next
 * units of a satellite?  For every shift p, how well does a copy's extension agree with itself moved by p, and where: an
 * ungapped local self-alignment on every diagonal of the dot plot.  Exact integer arithmetic, every segment on its own.
 *   Segment: library positions lo..hi inclusive on the forward strand; lo == hi + 1 is an empty segment, lo > hi + 1 is
 *   RAMX_ERR_ARG.  Its length is n = hi + 1 - lo; a length above RAMX_PERIOD_LEN_MAX is RAMX_ERR_UNSUPPORTED.
 *   Class x_j of position lo + j: library codes 0..3 are classes 0..3, codes 4..7 are code - 4, everything else is class 4,
 *   including any position outside the library.
 *   Pair: for a period p with 1 <= p <= min(pmax, n - 1), a pair is (j, j + p) with 0 <= j and j + p < n.  It AGREES iff both
 *   classes are below 4 and equal, DISAGREES iff both are below 4 and unequal; otherwise it counts for nothing.
 *   Block b holds the pairs with 8b <= j <= 8b + 7 that exist (the last block may be short): a_b is its number of agreeing
 *   pairs, d_b of disagreeing pairs, and its score is s_b = a_b - mm * d_b.
 *   Tract of p: a run of consecutive blocks b0..b1 with S = the sum of their s_b.  The best tract has the largest S; ties go to
 *   the smallest b1, then the largest b0.  That is the one-pass scan over b = 0, 1, ... which keeps a running sum and a start
 *   block, begins anew at b (running sum s_b, start b) whenever the running sum before b is <= 0 and adds s_b otherwise, and
 *   records (running sum, start, b) whenever the running sum is strictly above everything recorded before, beginning from 0.
 *   Record of the segment: the best tract over all p with the largest S, ties to the smallest p.  If S < min_score, or n < 2,
 *   the record is all zeros.  Otherwise period = p, score = S, start = 8 * b0, end = min(8 * b1 + 7, n - p - 1) -- the first
 *   members of the tract's first and last pair --, agree and disagree the sums of a_b and d_b over the tract; the periodic
 *   region is offsets start .. end + p of the segment.  reserved is written as 0.
 * Parameters: pmax 1..8192, mm 1..15, min_score >= 1; anything else is RAMX_ERR_ARG, raised before anything is launched or
 * written.  Defaults: 1024, 3, 16. */
#define RAMX_PERIOD_LEN_MAX 65536
#define RAMX_PERIOD_PMAX 8192
typedef struct ramx_period_params { int32_t pmax, mm, min_score, reserved; } ramx_period_params;
typedef struct ramx_period_seg { int64_t lo, hi; } ramx_period_seg;                      /* 16 bytes */
typedef struct ramx_period { int32_t period, score, start, end, agree, disagree, reserved[2]; } ramx_period;  /* 32 bytes */

/* The records on the device, from the library it holds (ramx_dev_load_library*, either form): every segment is packed as a
 * flank (start = lo, step = +1, t = 0 .. n - 1, W = 0) by the pack kernels of the extension loop; one wave per tile of 64
 * segments squeezes the transposed windows into every segment's own stream (two bits a base and a validity bit), and one
 * workgroup per segment scans it from LDS, a lane per period.  The windows and streams live in a device buffer of at most
 * RAMX_PERIOD_BYTES bytes (environment, read per call; default 1 GiB): a tile takes 64 * (4 * (ceil(nmax / 8) + 1) + 12 *
 * max(ceil(nmax / 32), 1)) bytes, nmax the longest segment of the call; the tiles are processed in groups that fit,
 * RAMX_ERR_UNSUPPORTED if one tile alone does not; the grouping does not show in the result.  Self-contained like the replays
 * and ramx_dev_tsd (a following ramx_dev_run_direction needs a new ramx_dev_begin_direction; resident bit planes are dropped);
 * rank-local under a communicator: the records are per segment.  n_segs == 0 returns RAMX_OK and launches nothing.  kernel_ms
 * (may be NULL): three values, the HIP-event times of the pack, the squeeze and the scan, summed over the groups. */
int ramx_dev_period(ramx_dev *d, const ramx_period_seg *segs, int32_t n_segs, const ramx_period_params *params, ramx_period *out,
                    double *kernel_ms);

/* The contract on an array of n library codes (plain host C; the class of codes[j] is x_j): what the device computes for a
 * segment, used for the kept consensus of a direction.  RAMX_ERR_ARG for bad parameters, n < 0 or a missing pointer,
 * RAMX_ERR_UNSUPPORTED for n > RAMX_PERIOD_LEN_MAX. */
int ramx_period_sequence(const int8_t *codes, int32_t n, const ramx_period_params *params, ramx_period *out);

/* One segment per core, in list order, from cores that both directions have extended (plain host C), with the extents of
 * ramx_tsd_sites (ram_extend.c:721-727).  which = 0, the left extension: orient == 0: [left_pos - left_len, left_pos - 1],
 * otherwise [left_pos + 1, left_pos + left_len]; which = 1, the right extension: orient == 0: [right_pos + 1, right_pos +
 * right_len], otherwise [right_pos - right_len, right_pos - 1]; which = 2, the whole element: lo..hi of the core's TSD site.
 * out holds cores->n segments; returns their number, RAMX_ERR_ARG for which outside 0..2. */
int32_t ramx_period_segments(const ramx_flat_cores *cores, int32_t which, ramx_period_seg *out);

/* What a family's records say together (plain host C): n; n_tract counts the records with period > 0, n_mono those with
 * period 1, n_simple 2..6, n_tandem >= 7; at_lo the records with period > 0 and start == 0, at_hi those with end == len -
 * period - 1 (the tract reaches the segment's first / last base; len = hi + 1 - lo of segs[i]); mode is the most frequent
 * period > 0, ties to the smaller one, 0 if there is none, and mode_count its count.  RAMX_ERR_ARG for bad parameters, n < 0,
 * a missing pointer or a record with a period outside 0..RAMX_PERIOD_PMAX. */
typedef struct ramx_period_hist { int32_t n, n_tract, n_mono, n_simple, n_tandem, at_lo, at_hi, mode, mode_count, reserved[3]; } ramx_period_hist;
int ramx_period_summary(const ramx_period *records, const ramx_period_seg *segs, int32_t n, const ramx_period_params *params,
                        ramx_period_hist *out);

/* Seam 1, called after both extension calls: ramx_period_segments(cores, which) and ramx_dev_period on the session's device.
 * out holds one record per core in list order.  The library rule is that of ramx_tsd_flat / _alignment / _batch; in a batch a
 * position outside a family's own library is outside the library (class 4), whatever lies beside it in the concatenation. */
int ramx_period_flat(const ramx_flat_cores *cores, const int8_t *sequence, uint64_t seq_len, int32_t which,
                     const ramx_period_params *params, ramx_period *out);
int ramx_period_alignment(struct coreAlignment *coreAlign, struct sequenceLibrary *seqLib, int32_t which,
                          const ramx_period_params *params, ramx_period *out);
int ramx_period_batch(const ramx_family *families, int32_t n_families, int32_t which, const ramx_period_params *params,
                      ramx_period *out);

/* Terminal repeats of the extended copies: is the beginning of a copy repeated at its end -- directly (the long terminal
 * repeats of an LTR retrotransposon) or as its reverse complement (the terminal inverted repeats of a DNA transposon)?  The TSDs
 * look just outside the termini of an element, this looks just inside them: a gapped local alignment of the element's first T
 * bases with its last T, once per orientation.  Exact integer arithmetic, every site on its own.
 *   Site: a ramx_tsd_site as defined for the TSDs: the element is library positions lo..hi, with the bounds seq_lo..seq_hi and
 *   the same argument checks.  n = hi + 1 - lo.
 *   Window length: T = min(tmax, n / 2) with integer division, so the two windows never overlap.  For T == 0 both records are
 *   all zeros.
 *   Class of a position: the rule of the TSDs: codes 0..3 and 4..7 are classes 0..3, everything else is class 4, including
 *   positions outside seq_lo..seq_hi and outside the library.
 *   Windows: a_i = class(lo + i), i = 0..T-1: the 5' end read inward.  Direct partner: b_j = class(hi + 1 - T + j): the 3' end in
 *   the same reading order; a 3' LTR ends at j = T - 1.  Inverted partner: c_j = class(hi - j), complemented (3 - x) when the
 *   class is below 4: the 3' end read inward on the other strand; a TIR begins at i = 0, j = 0.
 *   Agreement: a pair agrees iff both classes are below 4 and equal.  Every other pair is a mismatch.
 *   Cells: i, j = 1..T with H[0][*] = H[*][0] = 0 and
 *     D = H[i-1][j-1] + (agree(a_{i-1}, b_{j-1}) ? match : -mismatch),  U = H[i-1][j] - gap,  L = H[i][j-1] - gap,
 *     H[i][j] = max(0, D, U, L).  The gap cost is linear.
 *   Payload: every cell carries (i0, j0, matches, columns).  If H[i][j] == 0 the payload is (i, j, 0, 0).  Otherwise it is the
 *   payload of the first of D, U, L, in that order, whose value equals H[i][j]; columns goes up by 1, and through D matches goes
 *   up by 1 if the pair agrees.  Boundary cells carry (i, j, 0, 0).
 *   Record of one orientation: the cell with the largest H, ties to the smallest i, then the smallest j.  If that H < min_score
 *   the record is all zeros except T.  Otherwise score = H, a_start = i0, a_end = i - 1, b_start = j0, b_end = j - 1, matches
 *   and columns from the payload, T as above: the starts and ends are 0-based window offsets of the first and last aligned base.
 *   Output order: out[2 s] is site s direct, out[2 s + 1] is site s inverted.
 * Parameters: tmax 1..RAMX_TERM_TMAX, match 1..15, mismatch 1..15, gap 1..31, min_score >= 1, slack 0..15, reserved 0; anything
 * else is RAMX_ERR_ARG, raised before anything is launched or written.  Defaults: 512, 2, 3, 5, 40, 3 (the largest best score of
 * 200 pairs of independent random windows at T = 512 under these scores was 30 in the restatement tests/term_ref.py). */
#define RAMX_TERM_TMAX 1024
typedef struct ramx_term_params { int32_t tmax, match, mismatch, gap, min_score, slack, reserved[2]; } ramx_term_params;
typedef struct ramx_term { int32_t score, a_start, a_end, b_start, b_end, matches, columns, T; } ramx_term;   /* 32 bytes */

/* The records on the device, from the library it holds (ramx_dev_load_library*, either form): every site packs three windows
 * with the pack kernels of the extension loop at W = 0 (A: start = lo, step = +1; B: start = hi + 1 - T, step = +1; C: start =
 * hi, step = -1, complemented; t = 0 .. T - 1 cut by the site's bounds), the squeeze kernel of ramx_dev_period turns them into
 * one stream per window (two bits a base and a validity bit), and one wave per (site, orientation) sweeps the T x T cells in
 * registers (csrc/ramx_kernels_term.h).  The windows and streams live in a device buffer of at most RAMX_TERM_BYTES bytes
 * (environment, read per call; default 1 GiB): a tile of 64 sites takes 3 * 64 * (4 * (ceil(Tmax / 8) + 1) + 12 * max(ceil(Tmax /
 * 32), 1)) bytes, Tmax the longest window of the call; the tiles are processed in groups that fit, RAMX_ERR_UNSUPPORTED if one
 * tile alone does not; the grouping does not show in the result.  Self-contained like ramx_dev_tsd and ramx_dev_period (a
 * following ramx_dev_run_direction needs a new ramx_dev_begin_direction; resident bit planes are dropped); rank-local under a
 * communicator.  out holds 2 * n_sites records.  n_sites == 0 returns RAMX_OK and launches nothing; more than 2^29 sites are
 * RAMX_ERR_UNSUPPORTED.  kernel_ms (may be NULL): three values, the HIP-event times of the pack, the squeeze and the alignment,
 * summed over the groups. */
int ramx_dev_term(ramx_dev *d, const ramx_tsd_site *sites, int32_t n_sites, const ramx_term_params *params, ramx_term *out,
                  double *kernel_ms);

/* The contract on two arrays of library codes (plain host C): the cells are i = 1..na, j = 1..nb, a_i the class of a[i], b_j the
 * class of b[j] as given (the caller reverses and complements for the inverted orientation); the record's T is min(na, nb).
 * The device case is na == nb == T.  RAMX_ERR_ARG for bad parameters, a negative length or a missing pointer,
 * RAMX_ERR_UNSUPPORTED for a length above 65536. */
int ramx_term_pair(const int8_t *a, int32_t na, const int8_t *b, int32_t nb, const ramx_term_params *params, ramx_term *out);

/* What a family's records say together (plain host C, integers only); records holds 2 * n records in the output order above.
 * n_direct, n_inverted: records with score > 0.  direct_anchored: score > 0, a_start <= slack and b_end >= T - 1 - slack;
 * inverted_anchored: score > 0, a_start <= slack and b_start <= slack.  direct_median, inverted_median: the lower median of
 * a_end - a_start + 1 over the anchored records, 0 if there are none; the sums of matches and columns run over the anchored
 * records of each orientation.  verdict: 1 (LTR) if 2 * direct_anchored > n and direct_anchored >= inverted_anchored; 2 (TIR) if
 * 2 * inverted_anchored > n and inverted_anchored > direct_anchored; 0 otherwise.  RAMX_ERR_ARG for bad parameters, n < 0 or a
 * missing pointer. */
typedef struct ramx_term_family
{
  int32_t n, n_direct, n_inverted, direct_anchored, inverted_anchored, direct_median, inverted_median, verdict;
  int64_t direct_matches, direct_columns, inverted_matches, inverted_columns;
} ramx_term_family;                                                                      /* 64 bytes */
int ramx_term_summary(const ramx_term *records, int32_t n, const ramx_term_params *params, ramx_term_family *out);

/* Seam 1, called after both extension calls: ramx_tsd_sites of the cores and ramx_dev_term on the session's device.  out holds
 * two records per core in list order.  The library rule is that of ramx_tsd_flat / _alignment / _batch; in a batch a family's
 * records come after those of the families before it, and a position outside a family's own library is class 4. */
int ramx_term_flat(const ramx_flat_cores *cores, const int8_t *sequence, uint64_t seq_len, const ramx_term_params *params, ramx_term *out);
int ramx_term_alignment(struct coreAlignment *coreAlign, struct sequenceLibrary *seqLib, const ramx_term_params *params, ramx_term *out);
int ramx_term_batch(const ramx_family *families, int32_t n_families, const ramx_term_params *params, ramx_term *out);

/* multi-GPU: flanks are sharded over ranks; each column's 4 candidate sums are all-reduced
 * (4 x int64, RCCL over xGMI).  unique_id is the 128-byte ncclUniqueId made by rank 0
 * (ramx_comm_unique_id) and handed to the other ranks by the launcher (e.g. torch.distributed). */
int ramx_comm_unique_id(uint8_t id[128]);
int ramx_dev_comm_init(ramx_dev *d, const uint8_t id[128], int rank, int nranks);
/* ranks of the RCCL communicator as RCCL itself counts them (ncclCommCount); 1 without a communicator */
int ramx_dev_comm_size(ramx_dev *d);
/* Cross-device persistent path (optional, faster than one RCCL call per column): every rank exports the IPC handle
 * of its mailbox (64 bytes), the launcher all-gathers the handles, every rank imports them; a two-phase self-test
 * (phase 0: write tokens into all boxes -- synchronise the ranks -- phase 1: returns 1 if every rank's token arrived)
 * lets the launcher enable the path only if it works on ALL ranks.  With the path enabled the whole direction runs
 * as one persistent launch per rank and the per-column vote travels over xGMI from inside the kernels; if any rank
 * gives up (bounded spins) all ranks repeat the direction with per-column launches + RCCL. */
int ramx_dev_peer_export(ramx_dev *d, uint8_t handle[64]);
int ramx_dev_peer_import(ramx_dev *d, const uint8_t *handles /* [nranks][64] */, int rank, int nranks);
int ramx_dev_peer_selftest(ramx_dev *d, int phase, unsigned long long token);
int ramx_dev_peer_enable(ramx_dev *d, int on);

/* Host-memory variant of the same mailboxes (second choice when the device-memory boxes cannot be mapped into the
 * other processes or fail their self-test): every rank's box lives in one POSIX shared-memory segment that each
 * process registers with HIP; the kernels' system-scope stores and polls then cross PCIe.  All ranks of the node
 * call attach with the same name, run the self-test of ramx_dev_peer_selftest and ramx_dev_peer_enable as above;
 * afterwards rank 0 may unlink the name. */
int ramx_dev_hostbox_attach(ramx_dev *d, const char *shm_name, int rank, int nranks);
int ramx_hostbox_unlink(const char *shm_name);

/* test hook: replaces RCCL by a caller-supplied all-reduce so the sharded control flow (fold kernel, reduced
 * vote consumed by the next column, replicated stop rule) can be exercised where RCCL cannot run, e.g. two
 * ranks sharing the single GPU of a test box.  cb must sum 4 int64 in place across ranks and block until
 * done.  Slow by construction (one stream synchronisation per column); never used by bench.py. */
typedef void (*ramx_allreduce_cb)(long long *vals4, void *user);
int ramx_dev_set_allreduce_cb(ramx_dev *d, ramx_allreduce_cb cb, void *user);

/* ------------------------------------------------------------------------------------------
 * Scoring systems (reference score_system.h:23-37)
 * ------------------------------------------------------------------------------------------ */
struct scoringSystem *ramx_get_matrix(const char *matrixName);                       /* getMatrix */
struct scoringSystem *ramx_get_matrix_using_gap_penalties(const char *matrixName,
                                                          int gapopen, int gapextn); /* getMatrixUsingGapPenalties */
struct scoringSystem *ramx_get_repeatscout_matrix(int match, int mismatch, int gap); /* getRepeatScoutMatrix */
void ramx_free_scoring_system(struct scoringSystem *s);                              /* freeScoringSystem */
double ramx_calculate_lambda(struct scoringSystem *s);                               /* calculateLambda */

/* ------------------------------------------------------------------------------------------
 * Input surface (reference sequence.h:58-61): BED-6 ranges + 2bit -> library + cores
 * ------------------------------------------------------------------------------------------ */
struct sequenceLibrary *ramx_load_sequence_subset_minimal(const char *twoBitName, const char *rangeBEDName,
                                                          struct coreAlignment **core_align,
                                                          int *num_cores, int max_flanking_bp);
void ramx_free_library(struct sequenceLibrary *lib, struct coreAlignment *cores);

/* The same windows kept as the .2bit file stores them (replaces the expansion to one byte per base of
 * kentsrc/twoBitNew.c:531-613 + sequence.c:759,812-822): four bases per byte, first base in the most significant bits,
 * T C A G = 0 1 2 3; runs of N as (start, length) in library coordinates -- the coordinates of seqLib->sequence, i.e. what
 * coreAlignment.leftSeqPos / lowerSeqBound ... count in.  A quarter of the bytes to read, keep, upload and free. */
typedef struct ramx_packed_library
{
  uint64_t length;             /* bases */
  int32_t n_windows;
  const uint64_t *win_start;   /* [n_windows + 1] first base of window i; win_start[n_windows] = length */
  const uint64_t *win_byte;    /* [n_windows + 1] offset of window i's first packed byte in bytes[] */
  const uint8_t *win_phase;    /* [n_windows] position (0..3) of the window's first base inside that byte */
  const uint8_t *bytes;        /* the windows' bytes of the records' packed DNA, window after window */
  uint64_t n_bytes;
  const uint64_t *n_start;     /* runs of N, clipped to the windows, sorted */
  const uint32_t *n_len;
  int32_t n_blocks;
} ramx_packed_library;

/* loadSequenceSubsetMinimal without the expansion: lib->sequence is NULL, *packed (owned by the library, released by
 * ramx_free_library) holds the bases.  Everything else -- identifiers, boundaries, offsets, cores -- as above. */
struct sequenceLibrary *ramx_load_sequence_subset_packed(const char *twoBitName, const char *rangeBEDName,
                                                         struct coreAlignment **core_align, int *num_cores,
                                                         int max_flanking_bp, const ramx_packed_library **packed);
/* bases [from, from + count) as the reference's codes (A C G T = 0..3, N = 99): what seqLib->sequence would hold there */
int ramx_packed_decode(const ramx_packed_library *pl, uint64_t from, uint64_t count, char *out);

/* overlap avoidance between the two directions (reference ram_extend.c:445-499), prints the same lines */
void ramx_overlap_avoidance(struct coreAlignment *coreAlign, struct sequenceLibrary *seqLib);

/* report.c:161-502 */
void ramx_print_core_edges(struct coreAlignment *coreAlign, struct sequenceLibrary *seqLib,
                           char omitBlanks, char debug);

/* bnw_extend.c:87-155 -- link compatibility only (see top of file) */
int ****ramx_allocate_score(int num_align, int bandwidth);
void ramx_free_score(int num_align, int bandwidth, int ****score);

/* the CLI, callable as a function (RAMExtend's main(); reference ram_extend.c:217-790) */
int ramx_cli_main(int argc, char **argv);

#ifdef __cplusplus
}
#endif
#endif
