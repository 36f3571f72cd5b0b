/*
 * ramx_extend.c -- seam 1 of include/ramx.h: the extend_alignment()-compatible entry.
 *
 * Host side of the extension loop (reference ram_extend.c:859-1258): walks the caller's core
 * list, resolves every extendable core into a flank descriptor (start, step, complement, in-bounds
 * interval), hands the flanks to the device layer (ramx_device.hip), and writes the results back
 * into master[] and the cores exactly where the reference does.  No DP arithmetic happens here.
 */
#include <ctype.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <pthread.h>

#include "ramx_internal.h"
#include "ramx_dist.h"

/* the reference's hot-path globals (ram_extend.c:40,52,61) */
static int g_verbose = 0;
static int g_when_to_stop = 100;
static int g_l = 1;

void ramx_set_runtime(int verbose, int when_to_stop, int l)
{
  g_verbose = verbose;
  g_when_to_stop = when_to_stop;
  g_l = l;
}
int ramx_runtime_verbose(void) { return g_verbose; }
int ramx_runtime_when_to_stop(void) { return g_when_to_stop; }
int ramx_runtime_l(void) { return g_l; }

/* profile sink (include/ramx.h): off unless set */
static ramx_profile_cb g_profile_cb = NULL;
static void *g_profile_user = NULL;
void ramx_set_profile_sink(ramx_profile_cb cb, void *user)
{
  g_profile_cb = cb;
  g_profile_user = user;
}

/* alignment sink (include/ramx.h): off unless set */
static ramx_align_cb g_align_cb = NULL;
static void *g_align_user = NULL;
void ramx_set_align_sink(ramx_align_cb cb, void *user)
{
  g_align_cb = cb;
  g_align_user = user;
}

static ramx_dev *g_dev = NULL;
/* The device keeps the library between calls (the reference's main() runs both directions on one seqLib).  The
 * cache key is (pointer, length, content fingerprint): a caller that rewrites the buffer in place, or whose new
 * library lands at a recycled address with the same length, must never be served the stale device copy.  Libraries
 * above 64 MiB are fingerprinted in 16 MiB chunks on the host's cores (round 4: ~6 ms for 1 GB on 16 threads against 18 ms
 * for sending it again, which is what every call did before); batch mode keeps RAMX_FP_MAX for its concatenated libraries.
 * ramx_invalidate_library() drops the cache explicitly. */
#define RAMX_FP_MAX (64ull << 20)
#define RAMX_FP_CHUNK (16ull << 20)
static const int8_t *g_lib_ptr = NULL;
static uint64_t g_lib_len = 0, g_lib_fp = 0;
static int g_lib_trusted = 0;      /* ramx_preload_library: the caller vouches for the buffer until ramx_invalidate_library() */
/* batch mode: the (pointer, length, fingerprint) of every family whose concatenation the device currently holds */
static const int8_t **g_bl_ptr = NULL;
static uint64_t *g_bl_len = NULL, *g_bl_fp = NULL;
static int g_bl_n = 0;

static uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }

/* 64-bit content fingerprint, four independent multiply-rotate lanes over 32-byte stripes (memory-bound, ~10 GB/s) */
static uint64_t fingerprint(const int8_t *p, uint64_t n)
{
  const uint64_t P1 = 0x9E3779B185EBCA87ull, P2 = 0xC2B2AE3D27D4EB4Full;
  uint64_t a = P1 ^ n, b = P2, c = ~P1, d = ~P2, w[4];
  uint64_t i = 0;
  for (; i + 32 <= n; i += 32)
  {
    memcpy(w, p + i, 32);
    a = rotl64(a + w[0] * P2, 31) * P1; b = rotl64(b + w[1] * P2, 31) * P1;
    c = rotl64(c + w[2] * P2, 31) * P1; d = rotl64(d + w[3] * P2, 31) * P1;
  }
  uint64_t h = rotl64(a, 1) + rotl64(b, 7) + rotl64(c, 12) + rotl64(d, 18);
  for (; i < n; i++) h = rotl64(h ^ ((uint64_t)(uint8_t)p[i] * P1), 11) * P2;
  h ^= h >> 33; h *= P2; h ^= h >> 29; h *= P1; h ^= h >> 32;
  return h ? h : 1;
}

/* the same over a large buffer: chunk fingerprints by worker threads, folded in chunk order (ramx_par.c) */
struct fp_ctx { const int8_t *p; uint64_t n; uint64_t *out; };
static void fp_range(int lo, int hi, void *user)
{
  struct fp_ctx *c = (struct fp_ctx *)user;
  for (int i = lo; i < hi; i++)
  {
    const uint64_t at = (uint64_t)i * RAMX_FP_CHUNK, len = c->n - at < RAMX_FP_CHUNK ? c->n - at : RAMX_FP_CHUNK;
    c->out[i] = fingerprint(c->p + at, len);
  }
}
static uint64_t fingerprint_large(const int8_t *p, uint64_t n)
{
  if (n <= RAMX_FP_MAX) return fingerprint(p, n);
  const uint64_t nchunk = (n + RAMX_FP_CHUNK - 1) / RAMX_FP_CHUNK;
  if (nchunk > 0x7fffffffull) return 0;
  uint64_t *h = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)nchunk);
  if (h == NULL) return 0;                     /* 0 = not fingerprinted: the caller uploads */
  struct fp_ctx c = { p, n, h };
  ramx_parallel_for((int)nchunk, 1, fp_range, &c);
  const uint64_t r = fingerprint((const int8_t *)h, sizeof(uint64_t) * nchunk) ^ rotl64(n, 17);
  free(h);
  return r ? r : 1;
}

/* the fingerprint of a buffer the device copy is believed to match, taken BESIDE the direction it is needed for (seam 1 joins
 * it before anything is written back; a mismatch repeats the direction on the new content) */
struct fp_bg { const int8_t *p; uint64_t n; uint64_t fp; };
static void *fp_bg_worker(void *arg)
{
  struct fp_bg *j = (struct fp_bg *)arg;
  j->fp = fingerprint_large(j->p, j->n);
  return NULL;
}
#define RAMX_FP_ASYNC_MIN (4ull << 20)      /* below this the fingerprint costs less than a thread */

/* the library the device holds came from a packed twin (ramx_preload_library_packed): the seqLib it belongs to */
static const struct sequenceLibrary *g_packed_owner = NULL;

void ramx_invalidate_library(void)
{
  g_lib_ptr = NULL; g_lib_len = 0; g_lib_fp = 0; g_lib_trusted = 0; g_bl_n = 0; g_packed_owner = NULL;
}

/* the loader calls this when it frees a library: a later library that malloc places at the same address must not be taken for the
 * one the device holds (the packed path is keyed on the owner's pointer alone; the one-byte path also checks length and content) */
void ramx_forget_library_owner(const struct sequenceLibrary *lib)
{
  if (lib != NULL && g_packed_owner == lib) ramx_invalidate_library();
}

int ramx_preload_library_packed(const struct sequenceLibrary *seqLib, const struct ramx_packed_library *pl)
{
  if (!seqLib || !pl) { ramx_set_error("ramx_preload_library_packed: bad argument"); return RAMX_ERR_ARG; }
  ramx_dev *d = ramx_default_device();
  if (!d) return RAMX_ERR_NO_DEVICE;
  ramx_invalidate_library();
  const int rc = ramx_dev_load_library_packed(d, pl);
  if (rc != RAMX_OK) return rc;
  g_packed_owner = seqLib;
  return RAMX_OK;
}

int ramx_preload_library(const int8_t *sequence, uint64_t seq_len)
{
  if (!sequence && seq_len) { ramx_set_error("ramx_preload_library: bad argument"); return RAMX_ERR_ARG; }
  ramx_dev *d = ramx_default_device();
  if (!d) return RAMX_ERR_NO_DEVICE;
  ramx_invalidate_library();
  const int rc = ramx_dev_load_library(d, sequence, seq_len);
  if (rc != RAMX_OK) return rc;
  g_lib_ptr = sequence; g_lib_len = seq_len; g_lib_fp = 0; g_lib_trusted = 1;
  return RAMX_OK;
}

ramx_dev *ramx_default_device(void)
{
  if (!g_dev)
  {
    int ord = 0;
    const char *e = getenv("RAMX_DEVICE");
    if (e) ord = atoi(e);
    if (ramx_dev_create(ord, &g_dev) != RAMX_OK) g_dev = NULL;
  }
  return g_dev;
}

/* ---- -outmat: the reference's per-row trace (ram_extend.c:1122-1132, bnw_extend.c:1027-1044) -------------------------
 * written from what the device reports for every executed row: per band cell which state holds the cell's score, per
 * flank the row's best score and index.  The characters themselves come from the caller's library. */
struct trace_ctx
{
  FILE *out;
  int direction, W, nx;
  const int32_t *core_index;      /* flank -> position of its core in the list (the reference's n) */
  const ramx_flank *flanks;
  const ramx_flat_cores *cores;
  const int8_t *sequence;               /* one byte per base, or NULL: */
  const ramx_packed_library *packed;    /* the packed twin */
};
static FILE *g_trace_file = NULL;

/* ---- -vvvv: the reference's per-row lines (ram_extend.c:992-1090 candidate passes, 1134-1214 after the winner's pass), written
 * from what the device reports for every launch: the four candidate rows of the NEXT row (best cell, its band cell, gap state of
 * the first / last cell) and the winner row's best cell and end-cell gap states.  All sums in `int`, as the reference's. */
struct verbose_ctx
{
  int direction, W, cap, minimp, nx;
  const int32_t *core_index;       /* flank -> position of its core in the list (the reference's n) */
  int *high;                       /* overall_sequence_high_score per flank */
  int32_t *cand_prev;              /* [nx][16]: the candidate rows of the row about to be reported */
  int max_ext, max_row;
  /* -vvvvv (VERBOSE >= 12): every cell of those candidate rows (ram_extend.c:1013-1024) and the sequence around the edge of
   * every core (:1066, report.c printExtensionRegion) */
  int level;
  int32_t *band_prev;              /* [nx][4][2W+1][2] */
  const ramx_flat_cores *cores;
  const int8_t *sequence;          /* one byte per base, or NULL: */
  const ramx_packed_library *packed;
  uint64_t seq_len;
  const int32_t *seq_idx;          /* per core: its record of the library (NULL: the caller came through ramx_extend_flat) */
  const uint64_t *boundaries;
};
/* set by ramx_extend_alignment for the duration of a call: which record a core belongs to, and the records' ends */
static const int32_t *g_edge_seq_idx = NULL;
static const uint64_t *g_edge_boundaries = NULL;

static char trace_num_to_char(int8_t z);
static int edge_code(const struct verbose_ctx *t, int64_t p, int complement)
{
  int c = RAMX_SYM_N;
  if (p >= 0 && (uint64_t)p < t->seq_len)
  {
    if (t->sequence) c = t->sequence[p];
    else if (t->packed) { char b = RAMX_SYM_N; (void)ramx_packed_decode(t->packed, (uint64_t)p, 1, &b); c = (int8_t)b; }
  }
  if (complement && c >= 0 && c < 8) c = (c & 4) | (3 - (c & 3));       /* A<->T, C<->G, case kept (sequence.c:1141-1160) */
  return c;
}

/* The line report.c:20-150 prints for a core at VERBOSE >= 12: ten bases on the core side of the last aligned position, that
 * base, and the bases the extension is about to walk into -- '*' on a record's end, blanks beyond it; minus-strand cores read
 * the other way round and complemented; right extensions put the core first, left extensions last.  (One quirk is part of the
 * format: a left extension of a minus-strand core shows nine bases ahead, not ten.) */
static void print_edge_region(const struct verbose_ctx *t, int n, int row)
{
  const int sidx = t->seq_idx ? t->seq_idx[n] : 0;
  const int64_t lo = (t->boundaries && sidx > 0) ? (int64_t)t->boundaries[sidx - 1] : 0;
  const int64_t up = t->boundaries ? (int64_t)t->boundaries[sidx] : (int64_t)t->seq_len;
  const int minus = t->cores->orient[n] ? 1 : 0;
  /* the walk goes up the library for (right, +) and (left, -), down for the other two */
  const int up_walk = (t->direction != 0) != (minus != 0);
  const int64_t edge = t->direction ? t->cores->right_pos[n] : t->cores->left_pos[n];
  const int64_t last = up_walk ? edge + row + 1 : edge - row - 1;
  char core[16], ext[16];
  int nc = 0, ne = 0;
  /* core side: behind the walk; written in reading order of the printed strand */
  for (int k = 10; k >= 1; k--)
  {
    /* position k steps behind `last` */
    const int64_t p = up_walk ? last - k : last + k;
    char ch;
    if (up_walk) ch = (p == lo) ? '*' : (p < lo) ? ' ' : trace_num_to_char((int8_t)edge_code(t, p, minus));
    else ch = (p == up) ? '*' : (p > up) ? ' ' : trace_num_to_char((int8_t)edge_code(t, p, minus));
    core[nc++] = ch;
  }
  const int ahead = (!t->direction && minus) ? 9 : 10;
  for (int k = 1; k <= ahead; k++)
  {
    const int64_t p = up_walk ? last + k : last - k;
    char ch;
    if (up_walk) ch = (p == up) ? '*' : (p > up) ? ' ' : trace_num_to_char((int8_t)edge_code(t, p, minus));
    else ch = (p == lo) ? '*' : (p < lo) ? ' ' : trace_num_to_char((int8_t)edge_code(t, p, minus));
    ext[ne++] = ch;
  }
  core[nc] = '\0'; ext[ne] = '\0';
  const char mid = trace_num_to_char((int8_t)edge_code(t, last, minus));
  printf("C_EDGE: sIdx=%d, orient=%d, pos=%ld: ", sidx, minus, (long)(last - lo + 1));
  if (t->direction) printf("%s] {%c} %s\n", core, mid, ext);
  else
  {
    /* left extensions: what lies ahead first (furthest base first), the core side behind the bracket (nearest base first) */
    char r1[16], r2[16];
    for (int k = 0; k < ne; k++) r1[k] = ext[ne - 1 - k];
    for (int k = 0; k < nc; k++) r2[k] = core[nc - 1 - k];
    r1[ne] = '\0'; r2[nc] = '\0';
    printf("%s {%c} [%s\n", r1, mid, r2);
  }
}

static void verbose_row(int32_t row, int32_t besta, int32_t n_flanks, const int32_t *best_score, const int32_t *best_idx,
                        const int32_t *gfl, const int32_t *cand, const int32_t *band, void *user)
{
  struct verbose_ctx *t = (struct verbose_ctx *)user;
  static const char base[4] = { 'A', 'C', 'G', 'T' };
  (void)besta; (void)best_idx;
  const int nx = n_flanks < t->nx ? n_flanks : t->nx;
  if (row >= 0)
  {
    int curr = 0, chosen = 0;
    for (int a = 0; a < 4; a++)
    {
      int sum = 0;
      for (int i = 0; i < nx; i++)
      {
        const int32_t *c = t->cand_prev + (size_t)i * 16;
        printf(t->direction ? "RIGHT ROW %d with '%c': n = %d\n" : "LEFT ROW %d with '%c': n = %d\n", row, base[a], t->core_index[i]);
        if (t->level >= 12 && t->band_prev)
        {
          const int Bw = 2 * t->W + 1;
          const int32_t *bp = t->band_prev + ((size_t)i * 4 + a) * Bw * 2;
          printf("    Gap: ");
          for (int j = 0; j < Bw; j++) printf(" %d", bp[2 * j + 1]);
          printf("\n    Sub: ");
          for (int j = 0; j < Bw; j++) printf(" %d", bp[2 * j]);
          printf("\n");
        }
        int b = c[a];
        const int col = row + c[4 + a] - t->W, hi = t->high[i];
        if (b < 0) printf("  best score = %d @ column %d -- max(0,best_score) = 0!, prev best score = %d\n", b, col, hi);
        else printf("  best score = %d @ column %d, prev best score = %d\n", b, col, hi);
        if ((t->direction && c[8 + a] < -279000) || (!t->direction && c[12 + a] < -279000)) printf(" **OUT_OF_SEQ**");
        if (b < 0) b = 0;
        if (b >= hi + t->cap) sum += b;
        else { printf(" **CAPPED** contributing = %d", hi + t->cap); sum += hi + t->cap; }
        printf("\n");
        if (t->level >= 12 && t->cores) print_edge_region(t, t->core_index[i], row);
      }
      printf("  Total Score for '%c' = %d\n", base[a], sum);
      if (sum > curr) { curr = sum; chosen = a; }
    }
    printf("ROW %d complete, '%c' chosen as the consensus. curr_ext_score = %d\n", row, base[chosen], curr);
    int num_out = 0, num_high = 0;
    for (int i = 0; i < nx; i++)
    {
      if ((!t->direction && gfl[2 * i] < -279000) || (t->direction && gfl[2 * i + 1] < -279000)) num_out++;
      if (best_score[i] > t->high[i]) { t->high[i] = best_score[i]; num_high++; }
    }
    float since = 0.0f;
    if (abs(row - t->max_row) > 0) since = ((float)(curr - t->max_ext) / abs(row - t->max_row));
    printf("Alignment Extension: curr_extension_score = %d, max_extension_score = %d @ row %d\n                     "
           "score_per_position_overall = %0.1f, score_per_position_since_max = %0.1f\n"
           "                     total_edges = %d, num_extending = %d, num_out_of_seq = %d\n",
           curr, t->max_ext, t->max_row, ((float)curr / (row + 1)), since, nx, num_high, num_out);
    if (curr >= t->max_ext + (abs(t->max_row - row) * t->minimp))
    {
      printf("                     **This row is now the new max**\n");
      t->max_row = row;
      t->max_ext = curr;
    }
    else
      printf("                     extensions since last max score %d\n", abs(row - t->max_row));
  }
  memcpy(t->cand_prev, cand, sizeof(int32_t) * 16 * (size_t)nx);
  if (t->band_prev && band) memcpy(t->band_prev, band, sizeof(int32_t) * 8 * (size_t)(2 * t->W + 1) * (size_t)nx);
}

static char trace_num_to_char(int8_t z)      /* sequence.c:1091-1111 */
{
  static const char t[8] = { 'A', 'C', 'G', 'T', 'a', 'c', 'g', 't' };
  return (z >= 0 && z < 8) ? t[z] : 'N';
}

static int8_t trace_code(const struct trace_ctx *t, uint64_t p)
{
  if (t->sequence) return t->sequence[p];
  char c = RAMX_SYM_N;
  if (t->packed) (void)ramx_packed_decode(t->packed, p, 1, &c);
  return (int8_t)c;
}

static void trace_row(int32_t row, int32_t besta, const int8_t *codes, const int32_t *best_score, const int32_t *best_idx, void *user)
{
  const struct trace_ctx *t = (const struct trace_ctx *)user;
  const int W = t->W, B = 2 * W + 1;
  char *path = (char *)malloc((size_t)B + 1);
  for (int i = 0; i < t->nx; i++)
  {
    const ramx_flank *f = &t->flanks[i];
    const int n = t->core_index[i];
    for (int j = 0; j < B; j++)
    {
      /* bnw_extend.c:1029-1031: the base as stored (not complemented), 'X' outside the flank */
      const int64_t tt = (int64_t)(j - W) + row;
      const int64_t p = f->start + (int64_t)f->step * tt;
      char base = 'X';
      if (p >= 0 && p >= t->cores->lower[n] && p <= t->cores->upper[n]) base = trace_num_to_char(trace_code(t, (uint64_t)p));
      const int c = codes[(size_t)i * B + j];
      path[j] = c == 0 ? base : (c == 1 ? '-' : (char)tolower((unsigned char)base));
    }
    path[2 * W] = '\0';                              /* ram_extend.c:1123: the last cell is cut off */
    fprintf(t->out, "dir=%s:n=%d:row=%d: %s best:score=%d:offset=%d:cons=%c\n", t->direction ? "right" : "left", n, row, path,
            best_score[i], best_idx[i] - row + W, trace_num_to_char((int8_t)besta));
  }
  free(path);
}

static double wall_ms(void)
{
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

static int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

/*
 * Resolve one core into a flank for `direction` (reference bnw_extend.c:778-788, 824-868).
 * With p(t) = start + step * t, t = offset + row, the reference's unsigned index logic is
 * equivalent to "out of bounds iff p < lowerSeqBound || p > upperSeqBound || p < 0"
 * (SURVEY.md App. D rule 1; tests/test_scoring_and_flanks.py re-checks it against the oracle).
 */
static void resolve_flank(int direction, int64_t left_pos, int64_t right_pos, int64_t lower, int64_t upper,
                          int orient, int W, int L, ramx_flank *f)
{
  int64_t start, lo = lower < 0 ? 0 : lower, tlo, thi;
  if (direction)
    start = orient ? right_pos - 1 : right_pos + 1;
  else
    start = orient ? left_pos + 1 : left_pos - 1;
  f->start = start;
  f->step = ((direction != 0) == (orient != 0)) ? -1 : 1;
  f->compl_ = orient ? 1 : 0;
  memset(f->pad_, 0, sizeof(f->pad_));
  if (f->step > 0) { tlo = lo - start; thi = upper - start; }
  else { tlo = start - upper; thi = start - lo; }
  /* only t in [-W, L+W] is ever looked at; clamp so the device can use int32 */
  f->t_lo = (int32_t)clamp64(tlo, -(int64_t)W - 2, (int64_t)L + W + 2);
  f->t_hi = (int32_t)clamp64(thi, -(int64_t)W - 2, (int64_t)L + W + 2);
}

int ramx_resolve_flanks(int direction, const ramx_flat_cores *c, int bandwidth, int L, ramx_flank *flanks,
                        int32_t *core_index)
{
  int nx = 0;
  for (int n = 0; n < c->n; n++)
  {
    /* ram_extend.c:984-985: only cores extendable in this direction take part (but keep index n) */
    if ((direction && c->right_ext[n]) || (!direction && c->left_ext[n]))
    {
      resolve_flank(direction, c->left_pos[n], c->right_pos[n], c->lower[n], c->upper[n], c->orient[n], bandwidth, L,
                    &flanks[nx]);
      core_index[nx++] = n;
    }
  }
  return nx;
}

/* What every sink is fed from: nb families laid out in tiles, with what the loop returned for each.  ramx_extend_batch fills it
 * from the arrays of its launch, extend_flat_impl builds one of a single family (one_family_view); neither does unless a sink
 * is set. */
struct sink_view
{
  ramx_dev *d;
  int direction;
  const ramx_params *p;
  int nb;
  const int32_t *fidx;               /* [nb]: the family index a sink is told */
  const ramx_flank *fl;              /* [npad]: every family's flanks padded to whole tiles of 64 */
  const int32_t *map;                /* [npad]: the flanks' positions in their core lists */
  int32_t npad;
  const int32_t *first, *count;      /* [nb]: where a family's flanks begin in fl, and how many they are */
  const int8_t *cons;                /* [nb][L]: the bases the loop chose */
  const int32_t *rows_executed;      /* [nb] */
  const int32_t *ret;                /* [nb]: the kept columns, clamped at 0 */
  const uint64_t *lib_at;            /* by family index: where a family's own library begins in the one fl addresses (NULL: all 0) */
};

/* nx flanks padded to whole tiles of 64 with empty flanks (no base: t_lo > t_hi): a malloc'ed copy, for nx = 0 too; *npad its length */
static ramx_flank empty_flank(void) { ramx_flank x; memset(&x, 0, sizeof(x)); x.t_lo = 1; x.t_hi = 0; x.step = 1; return x; }
static ramx_flank *pad_to_tiles(const ramx_flank *fl, int nx, int *npad)
{
  const int n = *npad = (nx + 63) & ~63;
  ramx_flank *pf = (ramx_flank *)malloc(sizeof(ramx_flank) * (size_t)(n > 0 ? n : 1));
  if (nx > 0) memcpy(pf, fl, sizeof(ramx_flank) * (size_t)nx);
  for (int i = nx; i < n; i++) pf[i] = empty_flank();
  return pf;
}

/* The view of one direction of one family: its flanks padded once, and the rows_executed bases of the direction's own buffer
 * copied once into an [1][L] block with zeros behind them.  free_one_family_view releases what this allocated. */
static void one_family_view(struct sink_view *v, ramx_dev *d, int direction, const ramx_params *p, int family, const ramx_flank *fl,
                            const int32_t *map, int nx, const int8_t *cons, int rows_executed, int ret)
{
  int npad;
  int8_t *c1 = (int8_t *)calloc((size_t)(p->L > 0 ? p->L : 1), 1);
  int32_t *one = (int32_t *)malloc(sizeof(int32_t) * 5);
  if (rows_executed > 0) memcpy(c1, cons, (size_t)(rows_executed < p->L ? rows_executed : p->L));
  one[0] = family; one[1] = 0; one[2] = nx; one[3] = rows_executed; one[4] = ret > 0 ? ret : 0;
  memset(v, 0, sizeof(*v));
  v->d = d; v->direction = direction; v->p = p; v->nb = 1;
  v->fl = pad_to_tiles(fl, nx, &npad); v->map = map; v->npad = npad;
  v->fidx = one; v->first = one + 1; v->count = one + 2; v->rows_executed = one + 3; v->ret = one + 4;
  v->cons = c1;
}
static void free_one_family_view(struct sink_view *v)
{
  free((void *)v->fl); free((void *)v->cons); free((void *)v->fidx);
}

/* family b's flanks in the coordinates of its own library: a malloc'ed copy */
static ramx_flank *own_flanks(const struct sink_view *v, int b)
{
  const int n = v->count[b];
  ramx_flank *own = (ramx_flank *)malloc(sizeof(ramx_flank) * (size_t)(n > 0 ? n : 1));
  for (int i = 0; i < n; i++) { own[i] = v->fl[v->first[b] + i]; if (v->lib_at) own[i].start -= (int64_t)v->lib_at[v->fidx[b]]; }
  return own;
}

/* With a profile sink set: every family replayed in one call along the consensus the loop chose, over its rows_executed columns,
 * handed over family by family.  A view without any flank is answered here (the device may hold no library then): every
 * candidate total of every column is 0 and the vote gives the loop's base, A. */
static int profile_families(const struct sink_view *v)
{
  const ramx_params *p = v->p;
  ramx_col_profile *cols = (ramx_col_profile *)calloc((size_t)v->nb * (size_t)(p->L > 0 ? p->L : 1), sizeof(ramx_col_profile));
  int32_t *last = (int32_t *)malloc(sizeof(int32_t) * (size_t)(v->npad > 0 ? v->npad : 1));
  int rc = RAMX_OK;
  if (v->npad == 0)
  {
    for (int b = 0; b < v->nb; b++)
      for (int r = 0; r < v->rows_executed[b]; r++) cols[(size_t)b * p->L + r].base = v->cons[(size_t)b * p->L + r];
  }
  else
    rc = ramx_dev_profile(v->d, v->fl, v->npad, v->first, v->count, v->nb, p, v->cons, v->rows_executed, cols, last, NULL, NULL, NULL);
  for (int b = 0; b < v->nb && rc == RAMX_OK; b++)
  {
    ramx_profile pr;
    pr.direction = v->direction; pr.family = v->fidx[b]; pr.n_cols = v->rows_executed[b]; pr.ret = v->ret[b]; pr.n_flanks = v->count[b];
    pr.cols = cols + (size_t)b * p->L; pr.core_index = v->map + v->first[b]; pr.last_uncapped_row = last + v->first[b];
    g_profile_cb(&pr, g_profile_user);
  }
  free(cols); free(last);
  return rc;
}

/* "no alignment" in every end: what a replay leaves of a flank it does not walk */
static void blank_ends(ramx_aln_end *ends, int32_t n)
{ for (int32_t i = 0; i < n; i++) { ends[i].end_row = -1; ends[i].end_idx = -1; ends[i].score = 0; ends[i].start_idx = 0; ends[i].tail_ins = 0; } }

/* With an alignment sink set: every family replayed in one call along its kept consensus (rows = ret), every flank walked back,
 * handed over family by family.  ramx_dev_align answers the families without a flank or a kept column over the prefilled ends. */
static int align_families(const struct sink_view *v)
{
  const size_t n = (size_t)(v->npad > 0 ? v->npad : 1);
  int maxret = 0;
  for (int b = 0; b < v->nb; b++) if (v->ret[b] > maxret) maxret = v->ret[b];
  ramx_aln_end *ends = (ramx_aln_end *)malloc(sizeof(ramx_aln_end) * n);
  int32_t *idx = (int32_t *)malloc(sizeof(int32_t) * n * (size_t)(maxret > 0 ? maxret : 1));
  int32_t *ins = (int32_t *)malloc(sizeof(int32_t) * n * (size_t)(maxret > 0 ? maxret : 1));
  blank_ends(ends, v->npad);
  const int rc = ramx_dev_align(v->d, v->fl, v->npad, v->first, v->count, v->nb, v->p, v->cons, v->ret, ends, idx, ins, NULL);
  for (int b = 0; b < v->nb && rc == RAMX_OK; b++)
  {
    ramx_flank *own_fl = own_flanks(v, b);
    ramx_alignment al;
    memset(&al, 0, sizeof(al));
    al.direction = v->direction; al.family = v->fidx[b]; al.rows = v->ret[b]; al.n_flanks = v->count[b]; al.stride = v->npad;
    al.cons = v->cons + (size_t)b * v->p->L; al.flanks = own_fl; al.core_index = v->map + v->first[b]; al.ends = ends + v->first[b];
    if (v->ret[b] > 0 && v->count[b] > 0) { al.col_idx = idx + v->first[b]; al.col_ins = ins + v->first[b]; }
    g_align_cb(&al, g_align_user);
    free(own_fl);
  }
  free(ends); free(idx); free(ins);
  return rc;
}

static ramx_refine_cb g_refine_cb = NULL;
static void *g_refine_user = NULL;
static int g_refine_replays = 10;
void ramx_set_refine_sink(ramx_refine_cb cb, void *user, int32_t max_replays)
{
  g_refine_cb = cb;
  g_refine_user = user;
  g_refine_replays = max_replays >= 1 ? max_replays : 1;
}

/* With a refinement sink set: the pileup of the families' kept consensus (rows = ret) and their refinement, handed over family
 * by family.  The refinement's first replay IS the kept consensus' pileup: only when some family's consensus moved is the kept
 * one piled up in a call of its own. */
static int refine_families(const struct sink_view *v)
{
  const ramx_params *p = v->p;
  const int nb = v->nb;
  const size_t L = (size_t)(p->L > 0 ? p->L : 1);
  int32_t *rrows = (int32_t *)calloc((size_t)(nb > 0 ? nb : 1) * 3, sizeof(int32_t)), *replays = rrows + nb, *conv = replays + nb;
  ramx_col_pileup *kept = (ramx_col_pileup *)calloc((size_t)nb * L, sizeof(ramx_col_pileup));
  ramx_col_pileup *refd = (ramx_col_pileup *)calloc((size_t)nb * L, sizeof(ramx_col_pileup));
  int8_t *rcons = (int8_t *)calloc((size_t)nb * L, 1);
  int moved = 0;
  int rc = ramx_dev_refine(v->d, v->fl, v->npad, v->first, v->count, nb, p, v->cons, v->ret, g_refine_replays, rcons, rrows, replays, conv, refd, NULL, NULL);
  for (int b = 0; b < nb && rc == RAMX_OK; b++) moved |= replays[b] > 1;
  if (rc == RAMX_OK && moved) rc = ramx_dev_pileup(v->d, v->fl, v->npad, v->first, v->count, nb, p, v->cons, v->ret, kept, NULL, NULL);
  for (int b = 0; b < nb && rc == RAMX_OK; b++)
  {
    ramx_refinement rf;
    memset(&rf, 0, sizeof(rf));
    rf.direction = v->direction; rf.family = v->fidx[b]; rf.rows = v->ret[b]; rf.refined_rows = rrows[b];
    rf.replays = replays[b]; rf.converged = conv[b]; rf.n_flanks = v->count[b];
    rf.cons = v->cons + (size_t)b * p->L; rf.cols = (moved ? kept : refd) + (size_t)b * p->L;
    rf.refined_cons = rcons + (size_t)b * p->L; rf.refined_cols = refd + (size_t)b * p->L;
    g_refine_cb(&rf, g_refine_user);
  }
  free(rrows); free(kept); free(refd); free(rcons);
  return rc;
}

static ramx_cpg_cb g_cpg_cb = NULL;
static void *g_cpg_user = NULL;
static int g_cpg_replays = 10, g_cpg_ts = 0;
void ramx_set_cpg_sink(ramx_cpg_cb cb, void *user, int32_t max_replays, int32_t cpg_ts)
{
  g_cpg_cb = cb;
  g_cpg_user = user;
  g_cpg_replays = max_replays >= 1 ? max_replays : 1;
  g_cpg_ts = cpg_ts;
}

/* With a CpG sink set: the CpG-aware refinement of the families' kept consensus (rows = ret, rows_reversed = !direction as the
 * copies sink), handed over family by family. */
static int cpg_families(const struct sink_view *v)
{
  const ramx_params *p = v->p;
  const int nb = v->nb;
  const size_t L = (size_t)(p->L > 0 ? p->L : 1);
  int32_t *rrows = (int32_t *)calloc((size_t)(nb > 0 ? nb : 1) * 4, sizeof(int32_t)), *replays = rrows + nb, *conv = replays + nb, *ncpg = conv + nb;
  ramx_col_pileup *cols = (ramx_col_pileup *)calloc((size_t)nb * L, sizeof(ramx_col_pileup));
  ramx_col_dinuc *di = (ramx_col_dinuc *)calloc((size_t)nb * L, sizeof(ramx_col_dinuc));
  int8_t *rcons = (int8_t *)calloc((size_t)nb * L, 1);
  const int rc = ramx_dev_refine_cpg(v->d, v->fl, v->npad, v->first, v->count, nb, p, v->cons, v->ret, g_cpg_replays, !v->direction, g_cpg_ts,
                                     rcons, rrows, replays, conv, cols, di, ncpg, NULL, NULL);
  for (int b = 0; b < nb && rc == RAMX_OK; b++)
  {
    ramx_cpg_refinement cr;
    memset(&cr, 0, sizeof(cr));
    cr.direction = v->direction; cr.family = v->fidx[b]; cr.rows = v->ret[b]; cr.refined_rows = rrows[b];
    cr.replays = replays[b]; cr.converged = conv[b]; cr.n_flanks = v->count[b]; cr.n_cpg = ncpg[b];
    cr.cons = v->cons + (size_t)b * p->L; cr.refined_cons = rcons + (size_t)b * p->L;
    cr.refined_cols = cols + (size_t)b * p->L; cr.refined_di = di + (size_t)b * p->L;
    g_cpg_cb(&cr, g_cpg_user);
  }
  free(rrows); free(cols); free(di); free(rcons);
  return rc;
}

static ramx_copies_cb g_copies_cb = NULL;
static void *g_copies_user = NULL;
void ramx_set_copies_sink(ramx_copies_cb cb, void *user)
{
  g_copies_cb = cb;
  g_copies_user = user;
}

/* With a copies sink set: the per-copy statistics of the families along their kept consensus (rows = ret), handed over family by
 * family. */
static int copies_families(const struct sink_view *v)
{
  const size_t n = (size_t)(v->npad > 0 ? v->npad : 1);
  ramx_copy_stats *stats = (ramx_copy_stats *)calloc(n, sizeof(ramx_copy_stats));
  ramx_aln_end *ends = (ramx_aln_end *)malloc(sizeof(ramx_aln_end) * n);
  const int rc = ramx_dev_copy_stats(v->d, v->fl, v->npad, v->first, v->count, v->nb, v->p, v->cons, v->ret, !v->direction, stats, ends, NULL);
  for (int b = 0; b < v->nb && rc == RAMX_OK; b++)
  {
    ramx_flank *own_fl = own_flanks(v, b);
    ramx_copies cp;
    memset(&cp, 0, sizeof(cp));
    cp.direction = v->direction; cp.family = v->fidx[b]; cp.rows = v->ret[b]; cp.n_flanks = v->count[b];
    cp.cons = v->cons + (size_t)b * v->p->L; cp.flanks = own_fl; cp.core_index = v->map + v->first[b];
    cp.ends = ends + v->first[b]; cp.stats = stats + v->first[b];
    g_copies_cb(&cp, g_copies_user);
    free(own_fl);
  }
  free(stats); free(ends);
  return rc;
}

static ramx_linkage_cb g_linkage_cb = NULL;
static void *g_linkage_user = NULL;
static int32_t g_linkage_count = 4, g_linkage_permille = 100, g_linkage_max = 1024;
void ramx_set_linkage_sink(ramx_linkage_cb cb, void *user, int32_t min_count, int32_t min_permille, int32_t max_variants)
{
  g_linkage_cb = cb;
  g_linkage_user = user;
  g_linkage_count = min_count; g_linkage_permille = min_permille;
  g_linkage_max = max_variants < 0 ? 0 : max_variants > RAMX_LINKAGE_MAX_PLANES / 2 ? RAMX_LINKAGE_MAX_PLANES / 2 : max_variants;
}

/* The sinks that select over all copies of a family refuse a session that sees only its rank's. */
static int refuse_multi(const struct sink_view *v, const char *who, const char *why)
{
  if (!ramx_dev_is_multi(v->d)) return RAMX_OK;
  ramx_set_error("%s sink: not with a communicator or mailbox route active (%s)", who, why);
  return RAMX_ERR_UNSUPPORTED;
}

/* The head of the linkage and the subfamily sink: the bit planes of the families along their kept consensus (rows = ret), the
 * variants selected from the pileup of that replay and their Gram matrix; with_bits: the selected planes' words too. */
struct plane_head
{
  ramx_col_pileup *cols;             /* [nb][L] */
  ramx_plane *planes;                /* family b's list: pcount[b] planes from pfirst[b] on, planes_total in all */
  int32_t *pfirst, *pcount, planes_total;
  int64_t *cfirst, *bfirst;          /* [nb]: where family b's [P][P] begins in co and its [P][T] in bits */
  int32_t *co;
  uint64_t *bits;                    /* NULL without the words */
};
static void free_plane_head(struct plane_head *h) { free(h->cols); free(h->planes); free(h->pfirst); free(h->cfirst); free(h->co); free(h->bits); }
static int plane_head(const struct sink_view *v, int32_t min_count, int32_t min_permille, int32_t max_variants, int with_bits, struct plane_head *h)
{
  const ramx_params *p = v->p;
  const int nb = v->nb;
  const size_t L = (size_t)(p->L > 0 ? p->L : 1), n = (size_t)(nb > 0 ? nb : 1);
  int64_t cells = 0, words = 0;
  memset(h, 0, sizeof(*h));
  h->pfirst = (int32_t *)calloc(n * 2, sizeof(int32_t)); h->pcount = h->pfirst + n;
  h->cfirst = (int64_t *)calloc(n * 2, sizeof(int64_t)); h->bfirst = h->cfirst + n;
  h->cols = (ramx_col_pileup *)calloc(n * L, sizeof(ramx_col_pileup));
  h->planes = (ramx_plane *)calloc(n * 2 * (size_t)(max_variants > 0 ? max_variants : 1), sizeof(ramx_plane));
  const int rc = ramx_dev_planes(v->d, v->fl, v->npad, v->first, v->count, nb, p, v->cons, v->ret, h->cols, NULL, NULL);
  if (rc != RAMX_OK) return rc;
  for (int b = 0; b < nb; b++)
  {
    h->pfirst[b] = h->planes_total;
    /* a family without a flank has no tile to take a plane from */
    h->pcount[b] = v->count[b] > 0 ? ramx_select_planes(v->cons + (size_t)b * p->L, v->ret[b], h->cols + (size_t)b * L, min_count, min_permille, max_variants, h->planes + h->planes_total) : 0;
    h->cfirst[b] = cells; h->bfirst[b] = words;
    h->planes_total += h->pcount[b];
    cells += (int64_t)h->pcount[b] * h->pcount[b]; words += (int64_t)h->pcount[b] * ((v->count[b] + 63) / 64);
  }
  h->co = (int32_t *)calloc((size_t)(cells > 0 ? cells : 1), sizeof(int32_t));
  if (with_bits) h->bits = (uint64_t *)calloc((size_t)(words > 0 ? words : 1), sizeof(uint64_t));
  return ramx_dev_plane_gram(v->d, nb, h->planes, h->pfirst, h->pcount, h->co, h->cfirst, h->bits, with_bits ? h->bfirst : NULL);
}

/* With a linkage sink set: the head at the sink's selection, handed over family by family. */
static int linkage_families(const struct sink_view *v)
{
  struct plane_head h;
  int rc = refuse_multi(v, "linkage", "the selection needs the counts of every rank");
  if (rc != RAMX_OK) return rc;
  rc = plane_head(v, g_linkage_count, g_linkage_permille, g_linkage_max, 0, &h);
  for (int b = 0; b < v->nb && rc == RAMX_OK; b++)
  {
    ramx_linkage lk;
    memset(&lk, 0, sizeof(lk));
    lk.direction = v->direction; lk.family = v->fidx[b]; lk.rows = v->ret[b]; lk.n_planes = h.pcount[b];
    lk.cons = v->cons + (size_t)b * v->p->L; lk.cols = h.cols + (size_t)b * (size_t)(v->p->L > 0 ? v->p->L : 1);
    lk.planes = h.planes + h.pfirst[b]; lk.co = h.co + h.cfirst[b];
    g_linkage_cb(&lk, g_linkage_user);
  }
  free_plane_head(&h);
  return rc;
}

static ramx_subfam_cb g_subfam_cb = NULL;
static void *g_subfam_user = NULL;
static int32_t g_subfam_count = 4, g_subfam_permille = 100, g_subfam_max = 1024, g_subfam_K = 4, g_subfam_iter = 8, g_subfam_members = 4,
               g_subfam_replays = 10;
static double g_subfam_score = 3.0;
void ramx_set_subfam_sink(ramx_subfam_cb cb, void *user, int32_t min_count, int32_t min_permille, int32_t max_variants,
                          double min_mlog10p, int32_t K, int32_t max_iter, int32_t min_members, int32_t max_replays)
{
  g_subfam_cb = cb;
  g_subfam_user = user;
  g_subfam_count = min_count; g_subfam_permille = min_permille;
  g_subfam_max = max_variants < 0 ? 0 : max_variants > RAMX_LINKAGE_MAX_PLANES / 2 ? RAMX_LINKAGE_MAX_PLANES / 2 : max_variants;
  g_subfam_score = min_mlog10p;
  g_subfam_K = K < 1 ? 1 : K > RAMX_SUBFAM_MAX ? RAMX_SUBFAM_MAX : K;
  g_subfam_iter = max_iter >= 1 ? max_iter : 1;
  g_subfam_members = min_members;
  g_subfam_replays = max_replays >= 1 ? max_replays : 1;
}

/* What the subfamily sink's steps work on.  The result tables are laid out as the callback gets them, family b's block of each
 * at RAMX_SUBFAM_MAX times its place: patterns [V][K] at vfirst[b], cnt [K][P] at pfirst[b], size [K] at b, dist [count][K] at
 * first[b]; the labels at first[b]. */
struct subfam_work
{
  struct plane_head h;
  int32_t *on;                                   /* [nb]: the family takes part: it has a flank and a kept column */
  int32_t *Kb, *vfirst, *vcount, *iters, *conv;  /* [nb]: its patterns, where its variants begin and how many, what its split took */
  int32_t *labels, *cnt, *size, *dist;
  uint8_t *init, *pats;
  /* one ramx_dev_subfamilies call, from subfam_gather to subfam_scatter: its lists and what it returns */
  int32_t *qfirst, *qcount, *lab1, *cnt1, *size1, *it1, *cv1;
  ramx_plane *qplanes;
  uint8_t *init1, *pats1;
  /* the kept groups as families of their own: group ggroup[g] of family gof[g] */
  int32_t ng, gpad, *gfirst, *gcount, *grows, *gout, *greplays, *gconv, *gof, *ggroup;
  ramx_flank *gfl;
  int8_t *gcons, *gref;
  ramx_col_pileup *gcols;
  ramx_subfam_group *groups;
};
static void free_subfam_work(struct subfam_work *w)
{
  free_plane_head(&w->h);
  free(w->on); free(w->labels); free(w->cnt); free(w->size); free(w->dist); free(w->init); free(w->qplanes);
  free(w->gfirst); free(w->gfl); free(w->gcons); free(w->gref); free(w->gcols); free(w->groups);
}

/* the linked pairs of a list, malloc'ed: room for 4096, and a list with more is asked again with room for all it has */
static ramx_link *linked_pairs(const ramx_plane *planes, int32_t P, const int32_t *co, int32_t *nl)
{
  ramx_link *links = (ramx_link *)malloc(sizeof(ramx_link) * 4096);
  *nl = P > 0 ? ramx_link_pairs(planes, P, co, g_subfam_score, links, 4096) : 0;
  if (*nl <= 4096) return links;
  free(links);
  links = (ramx_link *)malloc(sizeof(ramx_link) * (size_t)*nl);
  *nl = ramx_link_pairs(planes, P, co, g_subfam_score, links, *nl);
  return links;
}

/* Behind the head: who takes part, the tables, and every family's initial patterns, the components of its linked pairs.  A
 * family that no call splits keeps what it gets here: one group of all its flanks after one assignment. */
static void subfam_initial(const struct sink_view *v, struct subfam_work *w)
{
  const size_t n = (size_t)(v->nb > 0 ? v->nb : 1), np1 = (size_t)(v->npad > 0 ? v->npad : 1), KM = RAMX_SUBFAM_MAX;
  const size_t pt = (size_t)(w->h.planes_total > 0 ? w->h.planes_total : 1);
  int32_t var_total = 0, nl;
  w->on = (int32_t *)calloc(n * 10, sizeof(int32_t)); w->Kb = w->on + n; w->vfirst = w->Kb + n; w->vcount = w->vfirst + n;
  w->iters = w->vcount + n; w->conv = w->iters + n; w->qfirst = w->conv + n; w->qcount = w->qfirst + n; w->it1 = w->qcount + n; w->cv1 = w->it1 + n;
  for (int b = 0; b < v->nb; b++)
  {
    w->on[b] = v->count[b] > 0 && v->ret[b] > 0;
    w->vfirst[b] = var_total;
    for (int32_t i = 0; i < w->h.pcount[b]; i++) w->vcount[b] += w->h.planes[w->h.pfirst[b] + i].cls != RAMX_PLANE_COVER;
    var_total += w->vcount[b];
  }
  const size_t vt = (size_t)(var_total > 0 ? var_total : 1);
  w->labels = (int32_t *)malloc(sizeof(int32_t) * 2 * np1); w->lab1 = w->labels + np1;
  w->size = (int32_t *)calloc(2 * n * KM, sizeof(int32_t)); w->size1 = w->size + n * KM;
  w->cnt = (int32_t *)calloc(2 * pt * KM, sizeof(int32_t)); w->cnt1 = w->cnt + pt * KM;
  w->dist = (int32_t *)calloc(np1 * KM, sizeof(int32_t));
  w->init = (uint8_t *)calloc(4 * vt * KM, 1); w->pats = w->init + vt * KM; w->init1 = w->pats + vt * KM; w->pats1 = w->init1 + vt * KM;
  w->qplanes = (ramx_plane *)calloc(pt, sizeof(ramx_plane));
  for (int32_t i = 0; i < v->npad; i++) w->labels[i] = -1;
  for (int b = 0; b < v->nb; b++)
  {
    const ramx_plane *pp = w->h.planes + w->h.pfirst[b];
    ramx_link *links = linked_pairs(pp, w->h.pcount[b], w->h.co + w->h.cfirst[b], &nl);
    w->Kb[b] = ramx_link_components(pp, w->h.pcount[b], links, nl, g_subfam_K, w->init + KM * w->vfirst[b], NULL);
    free(links);
    w->iters[b] = 1; w->conv[b] = 1;
    for (int32_t i = 0; i < v->count[b]; i++) w->labels[v->first[b] + i] = 0;
    w->size[KM * b] = v->count[b];
  }
}

/* The lists of the call for K patterns: those of the families that have K one after the other, their places the running sums,
 * the others with none.  Returns how many families the call splits. */
static int subfam_gather(struct subfam_work *w, int nb, int K)
{
  int any = 0;
  int32_t at = 0, vat = 0;
  for (int b = 0; b < nb; b++)
  {
    const int in = w->on[b] && w->Kb[b] == K;
    w->qfirst[b] = at; w->qcount[b] = in ? w->h.pcount[b] : 0;
    if (!in) continue;
    memcpy(w->qplanes + at, w->h.planes + w->h.pfirst[b], sizeof(ramx_plane) * (size_t)w->h.pcount[b]);
    memcpy(w->init1 + (size_t)K * vat, w->init + (size_t)RAMX_SUBFAM_MAX * w->vfirst[b], (size_t)K * w->vcount[b]);
    at += w->h.pcount[b]; vat += w->vcount[b]; any++;
  }
  return any;
}
/* what that call returned, into the blocks of the families it split (the labels it gave the others are not used) */
static void subfam_scatter(struct subfam_work *w, const int32_t *first, const int32_t *count, int nb, int K)
{
  const size_t KM = RAMX_SUBFAM_MAX;
  int32_t vat = 0;
  for (int b = 0; b < nb; b++)
  {
    if (!(w->on[b] && w->Kb[b] == K)) continue;
    memcpy(w->labels + first[b], w->lab1 + first[b], sizeof(int32_t) * (size_t)count[b]);
    memcpy(w->pats + KM * w->vfirst[b], w->pats1 + (size_t)K * vat, (size_t)K * w->vcount[b]);
    memcpy(w->cnt + KM * w->h.pfirst[b], w->cnt1 + (size_t)K * w->qfirst[b], sizeof(int32_t) * (size_t)K * w->h.pcount[b]);
    memcpy(w->size + KM * b, w->size1 + (size_t)K * b, sizeof(int32_t) * (size_t)K);
    w->iters[b] = w->it1[b]; w->conv[b] = w->cv1[b];
    vat += w->vcount[b];
  }
}

/* the distances of every flank to the patterns handed over (include/ramx.h: cover AND (bit XOR pattern), summed over the
 * variants), from the words of the selected planes, into the family's [count][K] block */
static void subfam_distances(struct subfam_work *w, const int32_t *first, const int32_t *count, int nb)
{
  for (int b = 0; b < nb; b++)
  {
    const int32_t P = w->h.pcount[b], T = (count[b] + 63) / 64, K = w->Kb[b];
    const ramx_plane *pp = w->h.planes + w->h.pfirst[b];
    const uint64_t *wd = w->h.bits + w->h.bfirst[b];
    const uint8_t *pat = w->pats + (size_t)RAMX_SUBFAM_MAX * w->vfirst[b];
    int32_t *d = w->dist + (size_t)RAMX_SUBFAM_MAX * first[b], vn = 0;
    if (!w->on[b]) continue;
    /* the cover plane of every plane's row, looked up once as ramx_link_pairs does: ramx_select_planes emits the cover of every
     * row it lists, so every entry is set */
    int32_t *cover = (int32_t *)malloc(sizeof(int32_t) * (size_t)(P > 0 ? P : 1));
    for (int32_t i = 0; i < P; i++)
    {
      if (pp[i].cls != RAMX_PLANE_COVER) continue;
      for (int32_t j = i; j >= 0 && pp[j].row == pp[i].row; j--) cover[j] = i;
      for (int32_t j = i + 1; j < P && pp[j].row == pp[i].row; j++) cover[j] = i;
    }
    for (int32_t i = 0; i < P; i++)
    {
      if (pp[i].cls == RAMX_PLANE_COVER) continue;
      const uint64_t *xw = wd + (size_t)i * T, *cw = wd + (size_t)cover[i] * T;
      for (int32_t f = 0; f < count[b]; f++)
      {
        const int x = (int)((xw[f / 64] >> (f % 64)) & 1), cv = (int)((cw[f / 64] >> (f % 64)) & 1);
        for (int k = 0; k < K; k++) d[(size_t)f * K + k] += cv & (x ^ pat[(size_t)vn * K + k]);
      }
      vn++;
    }
    free(cover);
  }
}

/* the groups of at least min_members flanks as families of their own: each one's flanks in whole tiles, padded with empty ones,
 * under the kept consensus of the family it comes from */
static void subfam_kept_groups(const struct sink_view *v, struct subfam_work *w)
{
  const size_t L = (size_t)(v->p->L > 0 ? v->p->L : 1), gmax = (size_t)(v->nb > 0 ? v->nb : 1) * RAMX_SUBFAM_MAX;
  w->gfirst = (int32_t *)calloc(gmax * 8, sizeof(int32_t)); w->gcount = w->gfirst + gmax; w->grows = w->gcount + gmax; w->gout = w->grows + gmax;
  w->greplays = w->gout + gmax; w->gconv = w->greplays + gmax; w->gof = w->gconv + gmax; w->ggroup = w->gof + gmax;
  for (int b = 0; b < v->nb; b++)
    for (int k = 0; k < w->Kb[b]; k++)
    {
      const int32_t sz = w->size[(size_t)b * RAMX_SUBFAM_MAX + k], g = w->ng;
      if (!(w->on[b] && sz >= g_subfam_members && sz > 0)) continue;
      w->gfirst[g] = w->gpad; w->gcount[g] = sz; w->grows[g] = v->ret[b]; w->gof[g] = b; w->ggroup[g] = k;
      w->gpad += (sz + 63) & ~63;
      w->ng++;
    }
  const size_t g1 = (size_t)(w->ng > 0 ? w->ng : 1);
  w->gcons = (int8_t *)calloc(g1 * L, 1); w->gref = (int8_t *)calloc(g1 * L, 1);
  w->gcols = (ramx_col_pileup *)calloc(g1 * L, sizeof(ramx_col_pileup));
  w->groups = (ramx_subfam_group *)calloc(g1, sizeof(ramx_subfam_group));
  w->gfl = (ramx_flank *)malloc(sizeof(ramx_flank) * (size_t)(w->gpad > 0 ? w->gpad : 1));
  for (int32_t i = 0; i < w->gpad; i++) w->gfl[i] = empty_flank();
  for (int g = 0; g < w->ng; g++)
  {
    const int b = w->gof[g];
    int32_t at = w->gfirst[g];
    memcpy(w->gcons + (size_t)g * L, v->cons + (size_t)b * v->p->L, (size_t)v->ret[b]);
    for (int32_t f = 0; f < v->count[b]; f++) if (w->labels[v->first[b] + f] == w->ggroup[g]) w->gfl[at++] = v->fl[v->first[b] + f];
  }
}
/* one refinement over all of them, and their records */
static int subfam_refine_groups(const struct sink_view *v, struct subfam_work *w)
{
  const size_t L = (size_t)(v->p->L > 0 ? v->p->L : 1);
  const int rc = w->ng == 0 ? RAMX_OK : ramx_dev_refine(v->d, w->gfl, w->gpad, w->gfirst, w->gcount, w->ng, v->p, w->gcons, w->grows, g_subfam_replays,
                                                       w->gref, w->gout, w->greplays, w->gconv, w->gcols, NULL, NULL);
  for (int g = 0; g < w->ng; g++)
  {
    ramx_subfam_group *gr = &w->groups[g];
    gr->group = w->ggroup[g]; gr->size = w->gcount[g]; gr->refined_rows = w->gout[g]; gr->replays = w->greplays[g];
    gr->converged = w->gconv[g]; gr->refined_cons = w->gref + (size_t)g * L; gr->refined_cols = w->gcols + (size_t)g * L;
  }
  return rc;
}

/* family by family; a family that does not take part is handed over without planes, as one group */
static void subfam_hand_over(const struct sink_view *v, const struct subfam_work *w)
{
  const size_t KM = RAMX_SUBFAM_MAX;
  int g0 = 0;
  for (int b = 0; b < v->nb; b++)
  {
    ramx_flank *own_fl = own_flanks(v, b);
    ramx_subfamilies sf;
    memset(&sf, 0, sizeof(sf));
    sf.direction = v->direction; sf.family = v->fidx[b]; sf.rows = v->ret[b]; sf.n_flanks = v->count[b];
    sf.n_planes = w->on[b] ? w->h.pcount[b] : 0; sf.n_variants = w->on[b] ? w->vcount[b] : 0; sf.K = w->on[b] ? w->Kb[b] : 1;
    sf.iterations = w->iters[b]; sf.converged = w->conv[b];
    while (g0 + sf.n_groups < w->ng && w->gof[g0 + sf.n_groups] == b) sf.n_groups++;
    sf.cons = v->cons + (size_t)b * v->p->L; sf.flanks = own_fl; sf.core_index = v->map + v->first[b];
    sf.planes = w->h.planes + w->h.pfirst[b]; sf.labels = w->labels + v->first[b];
    sf.patterns = w->pats + KM * w->vfirst[b]; sf.cnt = w->cnt + KM * w->h.pfirst[b]; sf.size = w->size + KM * b; sf.dist = w->dist + KM * v->first[b];
    sf.groups = w->groups + g0;
    g_subfam_cb(&sf, g_subfam_user);
    g0 += sf.n_groups;
    free(own_fl);
  }
}

/* With a subfamily sink set: the linkage sink's head with the planes' words; the linked pairs' components as initial patterns;
 * the split on the device, one call per number of patterns that some family has, ascending; the distances to the final patterns;
 * and one refinement over the flanks of every kept group as a family of its own. */
static int subfam_families(const struct sink_view *v)
{
  struct subfam_work w;
  int rc = refuse_multi(v, "subfamily", "the selection needs the counts of every rank");
  if (rc != RAMX_OK) return rc;
  memset(&w, 0, sizeof(w));
  rc = plane_head(v, g_subfam_count, g_subfam_permille, g_subfam_max, 1, &w.h);
  if (rc == RAMX_OK) subfam_initial(v, &w);
  for (int K = 1; K <= g_subfam_K && rc == RAMX_OK; K++)
  {
    if (!subfam_gather(&w, v->nb, K)) continue;
    rc = ramx_dev_subfamilies(v->d, v->nb, w.qplanes, w.qfirst, w.qcount, w.init1, K, g_subfam_iter, w.lab1, w.pats1, w.cnt1, w.size1, w.it1, w.cv1);
    if (rc == RAMX_OK) subfam_scatter(&w, v->first, v->count, v->nb, K);
  }
  if (rc == RAMX_OK)
  {
    subfam_distances(&w, v->first, v->count, v->nb);
    subfam_kept_groups(v, &w);
    rc = subfam_refine_groups(v, &w);
  }
  if (rc == RAMX_OK) subfam_hand_over(v, &w);
  free_subfam_work(&w);
  return rc;
}

static ramx_dist_cb g_dist_cb = NULL;
static void *g_dist_user = NULL;
static int32_t g_dist_cols = 1, g_dist_max = 256;
void ramx_set_dist_sink(ramx_dist_cb cb, void *user, int32_t min_cols, int32_t max_copies)
{
  g_dist_cb = cb;
  g_dist_user = user;
  g_dist_cols = min_cols;
  g_dist_max = max_copies < 0 ? 0 : max_copies > RAMX_DIST_MAX_COPIES ? RAMX_DIST_MAX_COPIES : max_copies;
}

/* With a distance sink set: the bit planes of the families along their kept consensus (rows = ret), the copies selected from the
 * ends of that replay and their pair matrix, handed over family by family. */
static int dist_families(const struct sink_view *v)
{
  int rc = refuse_multi(v, "dist", "a rank sees only its own copies");
  if (rc != RAMX_OK) return rc;
  const ramx_params *p = v->p;
  const int nb = v->nb;
  const size_t L = (size_t)(p->L > 0 ? p->L : 1), n = (size_t)(nb > 0 ? nb : 1), np = (size_t)(v->npad > 0 ? v->npad : 1);
  int32_t *cfirst = (int32_t *)calloc(n * 2, sizeof(int32_t)), *ccount = cfirst + n;
  int64_t *ofirst = (int64_t *)calloc(n, sizeof(int64_t));
  ramx_col_pileup *cols = (ramx_col_pileup *)calloc(n * L, sizeof(ramx_col_pileup));
  ramx_aln_end *ends = (ramx_aln_end *)malloc(sizeof(ramx_aln_end) * np);
  int32_t *copies = (int32_t *)calloc(n * (size_t)(g_dist_max > 0 ? g_dist_max : 1), sizeof(int32_t));
  ramx_copy_dist *dist = NULL;
  blank_ends(ends, v->npad);
  rc = ramx_dev_planes(v->d, v->fl, v->npad, v->first, v->count, nb, p, v->cons, v->ret, cols, ends, NULL);
  if (rc == RAMX_OK)
  {
    int32_t at = 0;
    int64_t cells = 0;
    for (int b = 0; b < nb; b++)
    {
      cfirst[b] = at;
      ccount[b] = v->count[b] > 0 && v->ret[b] > 0 ? ramx_select_copies(ends + v->first[b], v->count[b], v->ret[b], g_dist_cols, g_dist_max, copies + at) : 0;
      ofirst[b] = cells;
      at += ccount[b]; cells += (int64_t)ccount[b] * ccount[b];
    }
    dist = (ramx_copy_dist *)calloc((size_t)(cells > 0 ? cells : 1), sizeof(ramx_copy_dist));
    rc = ramx_dev_copy_dist(v->d, nb, copies, cfirst, ccount, dist, ofirst);
  }
  for (int b = 0; b < nb && rc == RAMX_OK; b++)
  {
    ramx_dist ds;
    memset(&ds, 0, sizeof(ds));
    ds.direction = v->direction; ds.family = v->fidx[b]; ds.rows = v->ret[b]; ds.n_flanks = v->count[b]; ds.n_copies = ccount[b];
    ds.cons = v->cons + (size_t)b * p->L; ds.core_index = v->map + v->first[b]; ds.ends = ends + v->first[b];
    ds.copies = copies + cfirst[b]; ds.dist = dist + ofirst[b];
    g_dist_cb(&ds, g_dist_user);
  }
  free(cfirst); free(ofirst); free(cols); free(ends); free(copies); free(dist);
  return rc;
}

static int any_sink(void) { return g_profile_cb || g_align_cb || g_refine_cb || g_cpg_cb || g_copies_cb || g_linkage_cb || g_subfam_cb || g_dist_cb; }

/* one RAMX_TIMING line: the time since the phase before, under the caller's name */
static void phase_line(const char *who, int width, const char *name, double *since)
{
  const double t = wall_ms();
  fprintf(stderr, "RAMX_TIMING     %s %-*s %8.3f ms\n", who, width, name, t - *since);
  *since = t;
}

/* every sink that is set, in this order, families ascending within a sink; stops at the first error */
static int run_sinks(const struct sink_view *v, const char *who, int width, int timing, double *since)
{
  const struct { int on; int (*feed)(const struct sink_view *); const char *phase; } sinks[] = {
    { g_profile_cb != NULL, profile_families, "profile replay" },
    { g_align_cb != NULL, align_families, "alignment replay" },
    { g_refine_cb != NULL, refine_families, "pileup + refinement" },
    { g_copies_cb != NULL, copies_families, "per-copy statistics" },
    { g_cpg_cb != NULL, cpg_families, "CpG-aware refinement" },
    { g_linkage_cb != NULL, linkage_families, "linkage" },
    { g_subfam_cb != NULL, subfam_families, "subfamilies" },
    { g_dist_cb != NULL, dist_families, "pairwise distances" },
  };
  int rc = RAMX_OK;
  for (size_t i = 0; i < sizeof(sinks) / sizeof(sinks[0]) && rc == RAMX_OK; i++)
  {
    if (!sinks[i].on) continue;
    rc = sinks[i].feed(v);
    if (timing) phase_line(who, width, sinks[i].phase, since);
  }
  return rc;
}

/* what a finished direction leaves with the caller: the executed columns in master (ram_extend.c:1092-1095), and per flank with
 * a positive trimmed score the extension length and score of its core (ram_extend.c:1234-1247) */
static void write_back(int direction, const ramx_params *p, int8_t *master, ramx_flat_cores *c, const int8_t *cons, int rows_executed,
                       const int32_t *map, const int32_t *th, const int32_t *tp, int nx)
{
  for (int r = 0; r < rows_executed; r++)
  {
    if (direction) master[(size_t)p->L + p->l + r] = cons[r];
    else master[(size_t)p->L - r - 1] = cons[r];
  }
  for (int i = 0; i < nx; i++)
  {
    if (th[i] > 0 && tp[i] >= 0)
    {
      const int n = map[i];
      if (direction) c->right_len[n] = tp[i] + 1;
      else c->left_len[n] = tp[i] + 1;
      c->score[n] += th[i];
    }
  }
}

/* packed != NULL: the device already holds the library (ramx_preload_library_packed); `sequence` is not looked at;
   family: the index the sinks are told (ramx_extend_batch running a family on its own, else 0) */
static int extend_flat_impl(int direction, ramx_flat_cores *c, const int8_t *sequence, uint64_t seq_len,
                            int8_t *master, const ramx_params *p, ramx_run_info *info, const ramx_packed_library *packed, int family)
{
  ramx_run_info local;
  if (!info) info = &local;
  memset(info, 0, sizeof(*info));
  if (!c || !p || !master || (c->n > 0 && !sequence && !packed)) { ramx_set_error("ramx_extend_flat: bad argument"); return RAMX_ERR_ARG; }
  ramx_dev *d = ramx_default_device();
  if (!d) return RAMX_ERR_NO_DEVICE;
  const double t0 = wall_ms();
  const int timing = getenv("RAMX_TIMING") != NULL;
  double tph = t0;
#define SEAM1_PHASE(name) do { if (timing) phase_line("seam1", 22, name, &tph); } while (0)
  const int N = c->n, W = p->bandwidth, L = p->L;
  int rc;
  int *map = (int *)malloc(sizeof(int) * (N > 0 ? N : 1));
  ramx_flank *fl = (ramx_flank *)malloc(sizeof(ramx_flank) * (N > 0 ? N : 1));
  const int nx = ramx_resolve_flanks(direction, c, W, L, fl, map);
  SEAM1_PHASE("resolve flanks");
  /* the library is shared by both directions: upload once per (pointer, length, content); nothing to upload when no
   * core is extendable in this direction */
  /* Round 4: when pointer and length are those of the device copy, the content check (6-8 ms for 1 GB even on 16 threads) runs in
   * a helper thread BESIDE the direction, which starts on the device copy at once; the thread is joined before anything is
   * written back, and a mismatch (the caller rewrote the buffer in place) uploads the buffer and repeats the direction.  Not
   * with the row traces (-outmat, -vvvv: they print while the direction runs).  RAMX_SYNC_FINGERPRINT=1: check first, as before. */
  int fp_async = 0;
  pthread_t fp_tid;
  struct fp_bg bg;
  memset(&bg, 0, sizeof(bg));
  if (!packed && nx > 0 && !(g_lib_trusted && sequence == g_lib_ptr && seq_len == g_lib_len) && sequence == g_lib_ptr &&
      seq_len == g_lib_len && g_lib_fp != 0 && seq_len >= RAMX_FP_ASYNC_MIN && g_trace_file == NULL && g_verbose < 10 &&
      getenv("RAMX_SYNC_FINGERPRINT") == NULL)
  {
    bg.p = sequence; bg.n = seq_len;
    if (pthread_create(&fp_tid, NULL, fp_bg_worker, &bg) == 0) fp_async = 1;
  }
#define FP_JOIN() do { if (fp_async) { pthread_join(fp_tid, NULL); fp_async = 0; } } while (0)
  if (!fp_async && !packed && nx > 0 && !(g_lib_trusted && sequence == g_lib_ptr && seq_len == g_lib_len))
  {
    const uint64_t fp = fingerprint_large(sequence, seq_len);
    if (sequence != g_lib_ptr || seq_len != g_lib_len || fp == 0 || fp != g_lib_fp)
    {
      ramx_invalidate_library();
      if ((rc = ramx_dev_load_library(d, sequence, seq_len)) != RAMX_OK) { free(map); free(fl); return rc; }
      g_lib_ptr = sequence;
      g_lib_len = seq_len;
      g_lib_fp = fp;
    }
  }
  SEAM1_PHASE("library (hash/upload)");
  int8_t *cons;
  int32_t *th, *tp;
run_again:
  cons = (int8_t *)malloc((size_t)L + 16);
  th = NULL; tp = NULL;
  struct trace_ctx tctx;
  if (g_trace_file != NULL)
  {
    tctx.out = g_trace_file; tctx.direction = direction; tctx.W = W; tctx.nx = nx; tctx.core_index = map; tctx.flanks = fl;
    tctx.cores = c; tctx.sequence = sequence; tctx.packed = packed;
    ramx_dev_set_row_trace(d, trace_row, &tctx);
  }
  /* -vvvv and above: the per-row lines of the reference, one column launch at a time */
  struct verbose_ctx vctx;
  memset(&vctx, 0, sizeof(vctx));
  const int verbose_rows = g_verbose >= 10;
  if (verbose_rows)
  {
    vctx.direction = direction; vctx.W = W; vctx.cap = p->cappenalty; vctx.minimp = p->minimprovement; vctx.nx = nx; vctx.core_index = map;
    vctx.high = (int *)calloc((size_t)(nx > 0 ? nx : 1), sizeof(int));
    vctx.cand_prev = (int32_t *)calloc((size_t)(nx > 0 ? nx : 1) * 16, sizeof(int32_t));
    vctx.max_ext = 0; vctx.max_row = -1;
    vctx.level = g_verbose;
    if (g_verbose >= 12)
    {
      vctx.band_prev = (int32_t *)calloc((size_t)(nx > 0 ? nx : 1) * 8 * (size_t)(2 * W + 1), sizeof(int32_t));
      vctx.cores = c; vctx.sequence = sequence; vctx.packed = packed; vctx.seq_len = packed ? packed->length : seq_len;
      vctx.seq_idx = g_edge_seq_idx; vctx.boundaries = g_edge_boundaries;
      ramx_dev_set_verbose_band(d, 1);
    }
    ramx_dev_set_row_verbose(d, verbose_row, &vctx);
  }
  if (g_trace_file == NULL && !verbose_rows && nx == 0 && getenv("RAMX_NO_HOST_EMPTY") == NULL)
  {
    /* No core is extendable in this direction: every candidate sum of every row is 0, so the vote (ram_extend.c:1064-1086:
     * strict > from 0) gives 'A' with a score of 0 in every row and the fit-preferred rule (:1194-1223) runs on scalars.
     * Nothing to launch (the reference walks its L rows over an empty list the same way). */
    long long max_ext = 0;
    int max_row = -1, rows_done = 0, stopped = 0;
    for (int r = 0; r < L; r++)
    {
      long long dist = (long long)max_row - r;
      if (dist < 0) dist = -dist;
      if (0 >= max_ext + dist * (long long)p->minimprovement) { max_row = r; max_ext = 0; }
      int d2 = r - max_row;
      if (d2 < 0) d2 = -d2;
      stopped = d2 >= p->when_to_stop;
      cons[r] = 0;
      rows_done = r + 1;
      if (stopped) break;
    }
    info->ret = max_row + 1;
    info->rows_executed = rows_done;
    info->limit_warning = (stopped && rows_done - 1 == L - 1) ? 1 : 0;
    info->persistent = 1; info->launches = 0; info->lanes_per_flank = 1; info->n_extendable = 0;     /* (no column launches) */
    info->prep_ms = wall_ms() - t0;
    th = (int32_t *)malloc(sizeof(int32_t));
    tp = (int32_t *)malloc(sizeof(int32_t));
    rc = RAMX_OK;
  }
  else if (g_trace_file == NULL && !verbose_rows && nx > 0 && nx <= ramx_dev_family_route_max(d, p) && L > 0 && W >= 1 && getenv("RAMX_NO_FAMILY_ROUTE") == NULL)
  {
    /* a family that fits one workgroup needs no device-wide barrier: run it as a batch of one (block-local vote) */
    int npad; ramx_flank *pf = pad_to_tiles(fl, nx, &npad);
    th = (int32_t *)malloc(sizeof(int32_t) * (size_t)npad);
    tp = (int32_t *)malloc(sizeof(int32_t) * (size_t)npad);
    const int32_t first = 0, count = nx;
    info->prep_ms = wall_ms() - t0;
    rc = ramx_dev_run_families(d, pf, npad, &first, &count, 1, p, info, cons, th, tp);
    free(pf);
    if (rc != RAMX_OK) { FP_JOIN(); free(cons); free(th); free(tp); free(map); free(fl); return rc; }
  }
  else
  {
    rc = ramx_dev_begin_direction(d, fl, nx, p);
    info->prep_ms = wall_ms() - t0;
    SEAM1_PHASE("begin (alloc, pack)");
    if (rc == RAMX_OK) rc = ramx_dev_run_direction(d, info);
    SEAM1_PHASE("run direction");
    if (g_trace_file != NULL) ramx_dev_set_row_trace(d, NULL, NULL);
    if (verbose_rows) { ramx_dev_set_row_verbose(d, NULL, NULL); ramx_dev_set_verbose_band(d, 0); free(vctx.high); free(vctx.cand_prev); free(vctx.band_prev); vctx.high = NULL; vctx.cand_prev = NULL; vctx.band_prev = NULL; }
    if (rc != RAMX_OK) { FP_JOIN(); free(cons); free(map); free(fl); return rc; }
    th = (int32_t *)malloc(sizeof(int32_t) * (nx > 0 ? nx : 1));
    tp = (int32_t *)malloc(sizeof(int32_t) * (nx > 0 ? nx : 1));
    rc = ramx_dev_download(d, cons, L + 16, th, tp);
  }
  if (fp_async)
  {
    FP_JOIN();
    if (bg.fp == 0 || bg.fp != g_lib_fp)
    {
      /* the buffer no longer holds what the device copy was made from: nothing has been written back yet -- upload it and run
       * the direction again */
      free(cons); free(th); free(tp);
      ramx_invalidate_library();
      if ((rc = ramx_dev_load_library(d, sequence, seq_len)) != RAMX_OK) { free(map); free(fl); return rc; }
      g_lib_ptr = sequence; g_lib_len = seq_len; g_lib_fp = bg.fp;
      memset(info, 0, sizeof(*info));
      goto run_again;
    }
    SEAM1_PHASE("fingerprint joined");
  }
  if (rc == RAMX_OK) write_back(direction, p, master, c, cons, info->rows_executed, map, th, tp, nx);
  SEAM1_PHASE("download + write-back");
  if (rc == RAMX_OK && any_sink())
  {
    struct sink_view v;
    one_family_view(&v, d, direction, p, family, fl, map, nx, cons, info->rows_executed, info->ret);
    rc = run_sinks(&v, "seam1", 22, timing, &tph);
    free_one_family_view(&v);
  }
#undef SEAM1_PHASE
#undef FP_JOIN
  free(cons); free(th); free(tp); free(map); free(fl);
  return rc == RAMX_OK ? info->ret : rc;
}

int ramx_extend_flat(int direction, ramx_flat_cores *c, const int8_t *sequence, uint64_t seq_len,
                     int8_t *master, const ramx_params *p, ramx_run_info *info)
{
  return extend_flat_impl(direction, c, sequence, seq_len, master, p, info, NULL, 0);
}

int ramx_extend_alignment(int direction, struct coreAlignment *coreAlign, int ****score,
                          struct sequenceLibrary *seqLib, char *master, int BANDWIDTH,
                          int CAPPENALTY, int MINIMPROVEMENT, int L, int N,
                          struct scoringSystem *scoreParams, FILE *pathStringFile)
{
  (void)score;
  g_trace_file = pathStringFile;          /* -outmat: ramx_extend_flat runs the direction row by row and writes the trace */
  if (g_verbose >= 3)   /* ram_extend.c:886-892 */
  {
    if (direction) printf("extend_alignment(right): Called with %d edges\n", N);
    else printf("extend_alignment(left): Called with %d edges\n", N);
  }
  if (g_verbose > 12)
    fprintf(stderr, "RAMExtend(ramx): the per-cell lines compute_nw_row prints above -vvvvv (bnw_extend.c, VERBOSE > 12) are not "
                    "produced by the device path; the band dumps of -vvvvv and the per-row lines of -vvvv are\n");
  if (g_verbose >= 12)
  {
    /* ram_extend.c:949-959: the boundary row of every core, as initialised at :909-946 */
    for (int k = 0; k < N; k++)
    {
      printf("SW Matrix Boundary Conditions ( n = %d ):\n", k);
      for (int st = 0; st < 2; st++)
      {
        printf(st == 0 ? "  GAP: " : "\n  SUB: ");
        for (int o = -BANDWIDTH; o <= BANDWIDTH; o++)
          printf(" %d", o == 0 ? 0 : (o < 0 ? -o : o) * scoreParams->gapextn + scoreParams->gapopen);
      }
      printf("\n");
    }
  }

  const int n = N > 0 ? N : 0;
  int64_t *i64 = (int64_t *)malloc(sizeof(int64_t) * 4 * (n + 1));
  int8_t *i8 = (int8_t *)malloc(3 * (n + 1));
  int32_t *i32 = (int32_t *)calloc(3 * (n + 1), sizeof(int32_t));
  int32_t *sidx = (int32_t *)calloc((size_t)n + 1, sizeof(int32_t));      /* -vvvvv: the record of every core (print_edge_region) */
  ramx_flat_cores fc;
  fc.left_pos = i64; fc.right_pos = i64 + n; fc.lower = i64 + 2 * n; fc.upper = i64 + 3 * n;
  fc.orient = i8; fc.left_ext = i8 + n; fc.right_ext = i8 + 2 * n;
  fc.left_len = i32; fc.right_len = i32 + n; fc.score = i32 + 2 * n;
  int k = 0;
  struct coreAlignment *cc;
  /* the reference walks the whole list for the DP but only the first N nodes for the write-back
   * (ram_extend.c:980 vs :1235); score[] is sized for N, so N nodes is all that is meaningful */
  for (cc = coreAlign; cc != NULL && k < n; cc = cc->next, k++)
  {
    ((int64_t *)fc.left_pos)[k] = (int64_t)cc->leftSeqPos;
    ((int64_t *)fc.right_pos)[k] = (int64_t)cc->rightSeqPos;
    ((int64_t *)fc.lower)[k] = (int64_t)cc->lowerSeqBound;
    ((int64_t *)fc.upper)[k] = (int64_t)cc->upperSeqBound;
    ((int8_t *)fc.orient)[k] = cc->orient ? 1 : 0;
    ((int8_t *)fc.left_ext)[k] = cc->leftExtendable ? 1 : 0;
    ((int8_t *)fc.right_ext)[k] = cc->rightExtendable ? 1 : 0;
    fc.left_len[k] = cc->leftExtensionLen;
    fc.right_len[k] = cc->rightExtensionLen;
    fc.score[k] = cc->score;
    sidx[k] = cc->seqIdx;
  }
  fc.n = k;
  g_edge_seq_idx = sidx; g_edge_boundaries = seqLib->boundaries;

  int32_t *mflat = (int32_t *)malloc(sizeof(int32_t) * 100 * 100);
  /* only [0..3][0..7,99] is defined in the reference's matrix (score_system.c:187-395) */
  memset(mflat, 0, sizeof(int32_t) * 100 * 100);
  for (int a = 0; a < 4; a++)
  {
    for (int b = 0; b < 8; b++) mflat[a * 100 + b] = scoreParams->matrix[a][b];
    mflat[a * 100 + RAMX_SYM_N] = scoreParams->matrix[a][RAMX_SYM_N];
  }
  ramx_params p;
  p.bandwidth = BANDWIDTH; p.cappenalty = CAPPENALTY; p.minimprovement = MINIMPROVEMENT; p.L = L;
  p.when_to_stop = g_when_to_stop; p.l = g_l; p.gapopen = scoreParams->gapopen; p.gapextn = scoreParams->gapextn;
  p.matrix = mflat;
  ramx_run_info info;
  /* a library that was loaded packed (ramx_load_sequence_subset_packed: ->sequence is NULL) runs from its packed twin, which
   * goes to the device now unless ramx_preload_library_packed has put it there already */
  const ramx_packed_library *packed = NULL;
  if (seqLib->sequence == NULL && fc.n > 0)
  {
    packed = ramx_packed_of(seqLib);
    if (!packed) { fprintf(stderr, "RAMExtend(ramx): the sequence library holds no bases (sequence == NULL and no packed twin)\n"); exit(1); }
    if (g_packed_owner != seqLib && ramx_preload_library_packed(seqLib, packed) != RAMX_OK)
    {
      fprintf(stderr, "RAMExtend(ramx): device extension failed: %s\n", ramx_last_error());
      exit(1);
    }
  }
  int ret = extend_flat_impl(direction, &fc, (const int8_t *)seqLib->sequence, seqLib->length, (int8_t *)master, &p, &info, packed, 0);
  if (ret < 0)
  {
    /* the reference has no error return on this path: print + exit(1) like its other failures */
    fprintf(stderr, "RAMExtend(ramx): device extension failed: %s\n", ramx_last_error());
    exit(1);
  }
  if (info.overflow32)
    fprintf(stderr, "RAMExtend(ramx): note: a column sum exceeded the int32 range; the reference's int accumulator "
                    "(ram_extend.c:874-878) would have wrapped here, the device keeps int64\n");
  if (info.ret >= 0 && info.rows_executed > 0 && g_verbose >= 3 && info.rows_executed <= L)
  {
    /* ram_extend.c:1216-1223: printed only when the loop broke */
    const int last = info.rows_executed - 1;
    if (abs(last - (info.ret - 1)) >= g_when_to_stop)
      printf("Ending...due to row_idx=%d - max_extension_score_row_idx=%d <= -WHEN_TO_STOP=%d\n", last,
             info.ret - 1, g_when_to_stop);
  }
  if (info.limit_warning)   /* ram_extend.c:1225-1231 */
  {
    if (direction) printf("WARNING: Extended sequence right to the limit ( L=%d ).\n", L);
    else printf("WARNING: Extended sequence left to the limit ( L=%d ).\n", L);
  }
  k = 0;
  for (cc = coreAlign; cc != NULL && k < fc.n; cc = cc->next, k++)
  {
    cc->leftExtensionLen = fc.left_len[k];
    cc->rightExtensionLen = fc.right_len[k];
    cc->score = fc.score[k];
  }
  g_edge_seq_idx = NULL; g_edge_boundaries = NULL;
  free(i64); free(i8); free(i32); free(sidx); free(mflat);
  g_trace_file = NULL;
  return ret;
}


/* batch mode's host passes over every family's library (fingerprints; the copy into the concatenated library): by family, threaded */
struct batch_lib_ctx { const ramx_family *fam; uint64_t *fps; const uint64_t *at_of; int8_t *lib; int do_fp; };
static void batch_lib_range(int lo, int hi, void *user)
{
  const struct batch_lib_ctx *c = (const struct batch_lib_ctx *)user;
  for (int f = lo; f < hi; f++)
  {
    if (c->fps) c->fps[f] = c->do_fp ? fingerprint(c->fam[f].sequence, c->fam[f].seq_len) : 0;
    if (c->lib && c->fam[f].seq_len) memcpy(c->lib + c->at_of[f], c->fam[f].sequence, c->fam[f].seq_len);
  }
}

/* Does the device hold the concatenation of these families' libraries (family f at at_of[f], total_len bases in all)?  fps
 * receives every family's fingerprint (0 beyond RAMX_FP_MAX in all: such a batch is always sent again). */
static int batch_lib_cached(const ramx_family *fam, int F, const uint64_t *at_of, uint64_t total_len, uint64_t *fps)
{
  int cached = (g_lib_ptr == (const int8_t *)&g_bl_n) && g_bl_n == F && g_lib_len == total_len && total_len <= RAMX_FP_MAX;
  struct batch_lib_ctx bc = { fam, fps, at_of, NULL, total_len <= RAMX_FP_MAX };
  ramx_parallel_for(F, 8, batch_lib_range, &bc);       /* ~10 GB/s per thread: 100 MB of families cost 10 ms on one */
  for (int f = 0; f < F && cached; f++)
    if (g_bl_ptr[f] != fam[f].sequence || g_bl_len[f] != fam[f].seq_len || g_bl_fp[f] != fps[f]) cached = 0;
  return cached;
}

/* the concatenated library goes to the device and becomes the one the cache key describes */
static int batch_lib_upload(ramx_dev *d, const ramx_family *fam, int F, const int8_t *lib, uint64_t total_len, const uint64_t *fps)
{
  g_lib_ptr = NULL; g_lib_len = 0; g_lib_fp = 0; g_lib_trusted = 0; g_packed_owner = NULL; /* whatever library the device held is replaced */
  const int rc = ramx_dev_load_library(d, lib, total_len);
  if (rc != RAMX_OK) return rc;
  g_bl_ptr = (const int8_t **)realloc((void *)g_bl_ptr, sizeof(*g_bl_ptr) * (size_t)(F ? F : 1));
  g_bl_len = (uint64_t *)realloc(g_bl_len, sizeof(*g_bl_len) * (size_t)(F ? F : 1));
  g_bl_fp = (uint64_t *)realloc(g_bl_fp, sizeof(*g_bl_fp) * (size_t)(F ? F : 1));
  for (int f = 0; f < F; f++) { g_bl_ptr[f] = fam[f].sequence; g_bl_len[f] = fam[f].seq_len; g_bl_fp[f] = fps[f]; }
  g_bl_n = F;
  g_lib_ptr = (const int8_t *)&g_bl_n;         /* sentinel: the device holds the batch library described by g_bl_* */
  g_lib_len = total_len;
  return RAMX_OK;
}

/*
 * Batch mode: many families, one launch (include/ramx.h).  Libraries are concatenated into one device buffer,
 * every family's flanks are padded to a multiple of 64 with empty flanks, results are written back per family
 * exactly as ramx_extend_flat does (ram_extend.c:1092-1095, 1234-1247).
 */
int ramx_extend_batch(int direction, ramx_family *fam, int32_t F, const ramx_params *p, ramx_run_info *infos)
{
  if (F < 0 || (F && !fam) || !p) { ramx_set_error("ramx_extend_batch: bad argument"); return RAMX_ERR_ARG; }
  ramx_run_info *own = NULL;
  if (!infos) infos = own = (ramx_run_info *)calloc((size_t)(F ? F : 1), sizeof(ramx_run_info));
  ramx_dev *d = ramx_default_device();
  if (!d) { free(own); return RAMX_ERR_NO_DEVICE; }
  const int W = p->bandwidth, L = p->L;
  int rc = RAMX_OK;
  const int timing = getenv("RAMX_TIMING") != NULL;
  double tph = timing ? wall_ms() : 0;
#define BATCH_PHASE(name) do { if (timing) phase_line("batch", 26, name, &tph); } while (0)
  /* which families can the batch kernel take? */
  /* every band width and gap sign has a family kernel (register-resident for W = 14/20/40 with non-positive
   * penalties, streaming otherwise); only families above one workgroup (512 flanks) go one by one */
  int batchable = W >= 1 && L >= 0;
  uint64_t total_len = 0;
  size_t total_pad = 0;
  int *take = (int *)calloc((size_t)(F ? F : 1), sizeof(int));
  for (int f = 0; f < F; f++)
  {
    int nx = 0;
    for (int n = 0; n < fam[f].cores.n; n++)
      if ((direction && fam[f].cores.right_ext[n]) || (!direction && fam[f].cores.left_ext[n])) nx++;
    take[f] = batchable && nx <= 512;
    if (take[f]) { total_len += fam[f].seq_len; total_pad += (size_t)((nx + 63) / 64) * 64; }
  }
  /* The concatenated library holds EVERY family at a fixed offset (prefix sums of seq_len), so it is the same for both
   * directions: like seam 1, it is built and uploaded again only when a family's (pointer, length) changes. */
  uint64_t *at_of = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)(F ? F : 1));
  total_len = 0;
  for (int f = 0; f < F; f++) { at_of[f] = total_len; total_len += fam[f].seq_len; }
  uint64_t *fps = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)(F ? F : 1));
  const int lib_cached = batch_lib_cached(fam, F, at_of, total_len, fps);
  BATCH_PHASE("library fingerprints");
  int8_t *lib = lib_cached ? NULL : (int8_t *)malloc(total_len ? total_len : 1);
  ramx_flank *fl = (ramx_flank *)malloc(sizeof(ramx_flank) * (total_pad ? total_pad : 1));
  int32_t *map = (int32_t *)malloc(sizeof(int32_t) * (total_pad ? total_pad : 1));
  int32_t *first = (int32_t *)malloc(sizeof(int32_t) * (size_t)(F ? F : 1));
  int32_t *count = (int32_t *)malloc(sizeof(int32_t) * (size_t)(F ? F : 1));
  int32_t *fidx = (int32_t *)malloc(sizeof(int32_t) * (size_t)(F ? F : 1));
  size_t fpos = 0;
  int nb = 0;
  if (lib)
  {
    struct batch_lib_ctx bc = { fam, NULL, at_of, lib, 0 };
    ramx_parallel_for(F, 8, batch_lib_range, &bc);
  }
  BATCH_PHASE("library copy");
  for (int f = 0; f < F; f++)
  {
    if (!take[f]) continue;
    const uint64_t at = at_of[f];
    ramx_flank *tmp = (ramx_flank *)malloc(sizeof(ramx_flank) * (size_t)(fam[f].cores.n > 0 ? fam[f].cores.n : 1));
    int32_t *tmap = (int32_t *)malloc(sizeof(int32_t) * (size_t)(fam[f].cores.n > 0 ? fam[f].cores.n : 1));
    const int nx = ramx_resolve_flanks(direction, &fam[f].cores, W, L, tmp, tmap);
    first[nb] = (int32_t)fpos; count[nb] = nx; fidx[nb] = f;
    for (int i = 0; i < nx; i++) { fl[fpos] = tmp[i]; fl[fpos].start += (int64_t)at; map[fpos] = tmap[i]; fpos++; }
    while (fpos & 63) { fl[fpos] = empty_flank(); map[fpos] = -1; fpos++; }
    free(tmp); free(tmap);
    nb++;
  }
  BATCH_PHASE("resolve flanks");
  if (nb > 0)
  {
    ramx_run_info *binfo = (ramx_run_info *)calloc((size_t)nb, sizeof(ramx_run_info));
    int8_t *cons = (int8_t *)malloc((size_t)nb * (size_t)(L > 0 ? L : 1));
    int32_t *th = (int32_t *)malloc(sizeof(int32_t) * (fpos ? fpos : 1));
    int32_t *tp = (int32_t *)malloc(sizeof(int32_t) * (fpos ? fpos : 1));
    if (!lib_cached) rc = batch_lib_upload(d, fam, F, lib, total_len, fps);
    BATCH_PHASE("library upload");
    if (rc == RAMX_OK) rc = ramx_dev_run_families(d, fl, (int32_t)fpos, first, count, nb, p, binfo, cons, th, tp);
    BATCH_PHASE("run families (device)");
    for (int b = 0; b < nb && rc == RAMX_OK; b++)
    {
      const int f = fidx[b];
      infos[f] = binfo[b];
      write_back(direction, p, fam[f].master, &fam[f].cores, cons + (size_t)b * L, binfo[b].rows_executed, map + first[b], th + first[b],
                 tp + first[b], count[b]);
    }
    if (rc == RAMX_OK && any_sink())
    {
      /* every family of the launch in one view: each sink replays them in one call, along their own consensus and over their
       * own number of columns, and sees a family's flanks in the coordinates of the family's own library */
      int32_t *rows = (int32_t *)malloc(sizeof(int32_t) * 2 * (size_t)nb), *ret = rows + nb;
      for (int b = 0; b < nb; b++) { rows[b] = binfo[b].rows_executed; ret[b] = binfo[b].ret > 0 ? binfo[b].ret : 0; }
      const struct sink_view v = { d, direction, p, nb, fidx, fl, map, (int32_t)fpos, first, count, cons, rows, ret, at_of };
      rc = run_sinks(&v, "batch", 26, timing, &tph);
      free(rows);
    }
    free(binfo); free(cons); free(th); free(tp);
    BATCH_PHASE("write-back");
  }
  /* families the batch kernel cannot take (other band widths, positive penalties, > 512 flanks): one by one */
  for (int f = 0; f < F && rc == RAMX_OK; f++)
  {
    if (take[f]) continue;
    int r1 = extend_flat_impl(direction, &fam[f].cores, fam[f].sequence, fam[f].seq_len, fam[f].master, p, &infos[f], NULL, f);
    if (r1 < 0) rc = r1;
  }
  free(lib); free(at_of); free(fl); free(map); free(first); free(count); free(fidx); free(take); free(own); free(fps);
  return rc;
}

/* ---- the site-window analyses (include/ramx.h: target-site duplications, tandem periodicity, terminal repeats): called after
 * the extension calls, on whatever library they left resident.  The three calls of an analysis -- flat, alignment, batch -- differ
 * from the other analyses' in their sites or segments and in the device call; what they share is written once, here ---- */

static int no_memory(const char *who) { ramx_set_error("%s: out of memory", who); return RAMX_ERR_ARG; }

/* the one-byte library on the device, by seam 1's cache key: the check extend_flat_impl makes, without its helper thread */
static int library_resident(ramx_dev *d, const int8_t *sequence, uint64_t seq_len)
{
  if (g_lib_trusted && sequence == g_lib_ptr && seq_len == g_lib_len) return RAMX_OK;
  const uint64_t fp = fingerprint_large(sequence, seq_len);
  if (sequence == g_lib_ptr && seq_len == g_lib_len && fp != 0 && fp == g_lib_fp) return RAMX_OK;
  ramx_invalidate_library();
  const int rc = ramx_dev_load_library(d, sequence, seq_len);
  if (rc != RAMX_OK) return rc;
  g_lib_ptr = sequence; g_lib_len = seq_len; g_lib_fp = fp;
  return RAMX_OK;
}

/* The checks of an *_alignment call after its parameters', the list's length and the session's device with the library of this
 * sequenceLibrary on it: the packed twin where it was loaded packed, its bytes otherwise.  *n == 0: nothing to do. */
static int alignment_resident(const char *who, struct coreAlignment *coreAlign, struct sequenceLibrary *seqLib, const void *out,
                              ramx_dev **d, int *n)
{
  *d = NULL; *n = 0;
  if (!seqLib) { ramx_set_error("%s: bad argument", who); return RAMX_ERR_ARG; }
  for (struct coreAlignment *cc = coreAlign; cc != NULL; cc = cc->next) (*n)++;
  if (*n == 0) return RAMX_OK;
  if (!out) { ramx_set_error("%s: bad argument", who); return RAMX_ERR_ARG; }
  if (!(*d = ramx_default_device())) return RAMX_ERR_NO_DEVICE;
  if (seqLib->sequence != NULL) return library_resident(*d, (const int8_t *)seqLib->sequence, seqLib->length);
  /* loaded packed: the twin goes to the device unless it is the library there already */
  const ramx_packed_library *packed = ramx_packed_of(seqLib);
  if (!packed) { ramx_set_error("%s: the sequence library holds no bases (sequence == NULL and no packed twin)", who); return RAMX_ERR_ARG; }
  return g_packed_owner != seqLib ? ramx_preload_library_packed(seqLib, packed) : RAMX_OK;
}

/* the n cores of a list as sites: ramx_tsd_sites on the list's own fields (NULL: no memory) */
static ramx_tsd_site *list_sites(struct coreAlignment *coreAlign, int n)
{
  ramx_tsd_site *sites = (ramx_tsd_site *)malloc(sizeof(ramx_tsd_site) * (size_t)n);
  int k = 0;
  for (struct coreAlignment *cc = coreAlign; cc != NULL && sites; cc = cc->next, k++)
  {
    const int64_t lp = (int64_t)cc->leftSeqPos, rp = (int64_t)cc->rightSeqPos;
    sites[k].lo = cc->orient ? rp - cc->rightExtensionLen : lp - cc->leftExtensionLen;
    sites[k].hi = cc->orient ? lp + cc->leftExtensionLen : rp + cc->rightExtensionLen;
    sites[k].seq_lo = (int64_t)cc->lowerSeqBound;
    sites[k].seq_hi = (int64_t)cc->upperSeqBound;
  }
  return sites;
}

/* The checks of a *_batch call after its parameters', the number of cores in all and the session's device with the concatenated
 * library of the batch on it: every family at the offset ramx_extend_batch gives it, at_of[f] (the caller's to free).
 * *total == 0: nothing to do, and no at_of. */
static int batch_resident(const char *who, const ramx_family *fam, int32_t F, const void *out, ramx_dev **d, uint64_t **at_of, int64_t *total)
{
  *d = NULL; *at_of = NULL; *total = 0;
  if (F < 0 || (F && !fam)) { ramx_set_error("%s: bad argument", who); return RAMX_ERR_ARG; }
  int64_t n = 0;
  for (int f = 0; f < F; f++)
  {
    if (fam[f].cores.n < 0 || (fam[f].cores.n > 0 && !fam[f].sequence)) { ramx_set_error("%s: bad family %d", who, f); return RAMX_ERR_ARG; }
    n += fam[f].cores.n;
  }
  if (n == 0) return RAMX_OK;
  if (!out || n > 0x7fffffff) { ramx_set_error("%s: bad argument", who); return RAMX_ERR_ARG; }
  if (!(*d = ramx_default_device())) return RAMX_ERR_NO_DEVICE;
  uint64_t *at = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)F), *fps = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)F);
  int rc = at && fps ? RAMX_OK : no_memory(who);
  uint64_t total_len = 0;
  for (int f = 0; f < F && rc == RAMX_OK; f++) { at[f] = total_len; total_len += fam[f].seq_len; }
  if (rc == RAMX_OK && !batch_lib_cached(fam, F, at, total_len, fps))
  {
    int8_t *lib = (int8_t *)malloc(total_len ? total_len : 1);
    struct batch_lib_ctx bc = { fam, NULL, at, lib, 0 };
    if (lib) ramx_parallel_for(F, 8, batch_lib_range, &bc);
    rc = lib ? batch_lib_upload(*d, fam, F, lib, total_len, fps) : no_memory(who);
    free(lib);
  }
  free(fps);
  if (rc != RAMX_OK) { free(at); return rc; }
  *at_of = at; *total = n;
  return RAMX_OK;
}

/* the sites of a batch's `total` cores in the concatenated library, family after family (NULL: no memory) */
static ramx_tsd_site *batch_sites(const ramx_family *fam, int32_t F, const uint64_t *at_of, int64_t total)
{
  ramx_tsd_site *sites = (ramx_tsd_site *)malloc(sizeof(ramx_tsd_site) * (size_t)total);
  int64_t at = 0;
  for (int f = 0; f < F && sites; f++)
  {
    ramx_tsd_sites(&fam[f].cores, sites + at);
    for (int i = 0; i < fam[f].cores.n; i++)
    {
      ramx_tsd_site *s = &sites[at + i];
      /* outside the family's own library is outside the library: its neighbours in the concatenation are never read */
      if (s->seq_lo < 0) s->seq_lo = 0;
      if (s->seq_hi > (int64_t)fam[f].seq_len - 1) s->seq_hi = (int64_t)fam[f].seq_len - 1;
      s->lo += (int64_t)at_of[f]; s->hi += (int64_t)at_of[f]; s->seq_lo += (int64_t)at_of[f]; s->seq_hi += (int64_t)at_of[f];
    }
    at += fam[f].cores.n;
  }
  return sites;
}

/* ---- target-site duplications ---- */

int ramx_tsd_flat(const ramx_flat_cores *cores, const int8_t *sequence, uint64_t seq_len, const ramx_tsd_params *params, ramx_tsd *out)
{
  int rc;
  if ((rc = ramx_tsd_check_params(params)) != RAMX_OK) return rc;
  if (!cores || cores->n < 0 || (cores->n > 0 && (!sequence || !out))) { ramx_set_error("ramx_tsd_flat: bad argument"); return RAMX_ERR_ARG; }
  if (cores->n == 0) return RAMX_OK;
  ramx_dev *d = ramx_default_device();
  if (!d) return RAMX_ERR_NO_DEVICE;
  ramx_tsd_site *sites = (ramx_tsd_site *)malloc(sizeof(ramx_tsd_site) * (size_t)cores->n);
  if (!sites) return no_memory("ramx_tsd_flat");
  ramx_tsd_sites(cores, sites);
  if ((rc = library_resident(d, sequence, seq_len)) == RAMX_OK) rc = ramx_dev_tsd(d, sites, cores->n, params, out, NULL);
  free(sites);
  return rc;
}

int ramx_tsd_alignment(struct coreAlignment *coreAlign, struct sequenceLibrary *seqLib, const ramx_tsd_params *params, ramx_tsd *out)
{
  int rc, n;
  ramx_dev *d;
  if ((rc = ramx_tsd_check_params(params)) != RAMX_OK) return rc;
  if ((rc = alignment_resident("ramx_tsd_alignment", coreAlign, seqLib, out, &d, &n)) != RAMX_OK || n == 0) return rc;
  ramx_tsd_site *sites = list_sites(coreAlign, n);
  rc = sites ? ramx_dev_tsd(d, sites, n, params, out, NULL) : no_memory("ramx_tsd_alignment");
  free(sites);
  return rc;
}

int ramx_tsd_batch(const ramx_family *fam, int32_t F, const ramx_tsd_params *params, ramx_tsd *out)
{
  int rc;
  ramx_dev *d;
  uint64_t *at_of;
  int64_t total;
  if ((rc = ramx_tsd_check_params(params)) != RAMX_OK) return rc;
  if ((rc = batch_resident("ramx_tsd_batch", fam, F, out, &d, &at_of, &total)) != RAMX_OK || total == 0) return rc;
  ramx_tsd_site *sites = batch_sites(fam, F, at_of, total);
  rc = sites ? ramx_dev_tsd(d, sites, (int32_t)total, params, out, NULL) : no_memory("ramx_tsd_batch");
  free(sites); free(at_of);
  return rc;
}

/* ---- tandem periodicity ---- */

int ramx_period_flat(const ramx_flat_cores *cores, const int8_t *sequence, uint64_t seq_len, int32_t which,
                     const ramx_period_params *params, ramx_period *out)
{
  int rc;
  if ((rc = ramx_period_check_params(params)) != RAMX_OK) return rc;
  if (!cores || cores->n < 0 || (cores->n > 0 && (!sequence || !out)) || which < 0 || which > 2)
  { ramx_set_error("ramx_period_flat: bad argument"); return RAMX_ERR_ARG; }
  if (cores->n == 0) return RAMX_OK;
  ramx_dev *d = ramx_default_device();
  if (!d) return RAMX_ERR_NO_DEVICE;
  ramx_period_seg *segs = (ramx_period_seg *)malloc(sizeof(ramx_period_seg) * (size_t)cores->n);
  if (!segs) return no_memory("ramx_period_flat");
  ramx_period_segments(cores, which, segs);
  if ((rc = library_resident(d, sequence, seq_len)) == RAMX_OK) rc = ramx_dev_period(d, segs, cores->n, params, out, NULL);
  free(segs);
  return rc;
}

int ramx_period_alignment(struct coreAlignment *coreAlign, struct sequenceLibrary *seqLib, int32_t which,
                          const ramx_period_params *params, ramx_period *out)
{
  int rc, n;
  ramx_dev *d;
  if ((rc = ramx_period_check_params(params)) != RAMX_OK) return rc;
  if (which < 0 || which > 2) { ramx_set_error("ramx_period_alignment: bad argument"); return RAMX_ERR_ARG; }
  if ((rc = alignment_resident("ramx_period_alignment", coreAlign, seqLib, out, &d, &n)) != RAMX_OK || n == 0) return rc;
  ramx_period_seg *segs = (ramx_period_seg *)malloc(sizeof(ramx_period_seg) * (size_t)n);
  if (!segs) return no_memory("ramx_period_alignment");
  int k = 0;
  for (struct coreAlignment *cc = coreAlign; cc != NULL; cc = cc->next, k++)
  {
    /* ramx_period_segments on the list's own fields */
    const int64_t lp = (int64_t)cc->leftSeqPos, rp = (int64_t)cc->rightSeqPos, ll = cc->leftExtensionLen, rl = cc->rightExtensionLen;
    if (which == 0) { segs[k].lo = cc->orient ? lp + 1 : lp - ll; segs[k].hi = cc->orient ? lp + ll : lp - 1; }
    else if (which == 1) { segs[k].lo = cc->orient ? rp - rl : rp + 1; segs[k].hi = cc->orient ? rp - 1 : rp + rl; }
    else { segs[k].lo = cc->orient ? rp - rl : lp - ll; segs[k].hi = cc->orient ? lp + ll : rp + rl; }
  }
  rc = ramx_dev_period(d, segs, n, params, out, NULL);
  free(segs);
  return rc;
}

int ramx_period_batch(const ramx_family *fam, int32_t F, int32_t which, const ramx_period_params *params, ramx_period *out)
{
  int rc;
  ramx_dev *d;
  uint64_t *at_of;
  int64_t total;
  if ((rc = ramx_period_check_params(params)) != RAMX_OK) return rc;
  if (which < 0 || which > 2) { ramx_set_error("ramx_period_batch: bad argument"); return RAMX_ERR_ARG; }
  if ((rc = batch_resident("ramx_period_batch", fam, F, out, &d, &at_of, &total)) != RAMX_OK || total == 0) return rc;
  ramx_period_seg *segs = (ramx_period_seg *)malloc(sizeof(ramx_period_seg) * 2 * (size_t)total), *bounds = segs + total;
  int64_t at = 0;
  for (int f = 0; f < F && segs; f++)
  {
    ramx_period_segments(&fam[f].cores, which, segs + at);
    for (int i = 0; i < fam[f].cores.n; i++)
    {
      /* outside the family's own library is outside the library: its neighbours in the concatenation are never read */
      segs[at + i].lo += (int64_t)at_of[f]; segs[at + i].hi += (int64_t)at_of[f];
      bounds[at + i].lo = (int64_t)at_of[f]; bounds[at + i].hi = (int64_t)at_of[f] + (int64_t)fam[f].seq_len - 1;
    }
    at += fam[f].cores.n;
  }
  rc = segs ? ramx_dev_period_bounded(d, segs, bounds, (int32_t)total, params, out, NULL) : no_memory("ramx_period_batch");
  free(segs); free(at_of);
  return rc;
}

/* ---- terminal repeats: the sites of the TSDs ---- */

int ramx_term_flat(const ramx_flat_cores *cores, const int8_t *sequence, uint64_t seq_len, const ramx_term_params *params, ramx_term *out)
{
  int rc;
  if ((rc = ramx_term_check_params(params)) != RAMX_OK) return rc;
  if (!cores || cores->n < 0 || (cores->n > 0 && (!sequence || !out))) { ramx_set_error("ramx_term_flat: bad argument"); return RAMX_ERR_ARG; }
  if (cores->n == 0) return RAMX_OK;
  ramx_dev *d = ramx_default_device();
  if (!d) return RAMX_ERR_NO_DEVICE;
  ramx_tsd_site *sites = (ramx_tsd_site *)malloc(sizeof(ramx_tsd_site) * (size_t)cores->n);
  if (!sites) return no_memory("ramx_term_flat");
  ramx_tsd_sites(cores, sites);
  if ((rc = library_resident(d, sequence, seq_len)) == RAMX_OK) rc = ramx_dev_term(d, sites, cores->n, params, out, NULL);
  free(sites);
  return rc;
}

int ramx_term_alignment(struct coreAlignment *coreAlign, struct sequenceLibrary *seqLib, const ramx_term_params *params, ramx_term *out)
{
  int rc, n;
  ramx_dev *d;
  if ((rc = ramx_term_check_params(params)) != RAMX_OK) return rc;
  if ((rc = alignment_resident("ramx_term_alignment", coreAlign, seqLib, out, &d, &n)) != RAMX_OK || n == 0) return rc;
  ramx_tsd_site *sites = list_sites(coreAlign, n);
  rc = sites ? ramx_dev_term(d, sites, n, params, out, NULL) : no_memory("ramx_term_alignment");
  free(sites);
  return rc;
}

int ramx_term_batch(const ramx_family *fam, int32_t F, const ramx_term_params *params, ramx_term *out)
{
  int rc;
  ramx_dev *d;
  uint64_t *at_of;
  int64_t total;
  if ((rc = ramx_term_check_params(params)) != RAMX_OK) return rc;
  if ((rc = batch_resident("ramx_term_batch", fam, F, out, &d, &at_of, &total)) != RAMX_OK || total == 0) return rc;
  ramx_tsd_site *sites = batch_sites(fam, F, at_of, total);
  rc = sites ? ramx_dev_term(d, sites, (int32_t)total, params, out, NULL) : no_memory("ramx_term_batch");
  free(sites); free(at_of);
  return rc;
}

/* bnw_extend.c:87-155 -- kept for link compatibility: the device path never reads it.  The block has the reference's
 * index shape score[2][num_align][2*bandwidth+1][2], so code written against the reference that dereferences it (the
 * VERBOSE >= 12 dump of ram_extend.c:949-959, unit tests) reads zeros instead of faulting -- but every [n] shares ONE
 * row of cells (2 * num_align * (2W+1) separate mallocs are exactly what this library exists to avoid). */
int ****ramx_allocate_score(int num_align, int bandwidth)
{
  if (num_align < 1 || bandwidth < 0) return NULL;
  const int B = 2 * bandwidth + 1;
  int ****score = (int ****)calloc(2, sizeof(int ***));
  int **row = (int **)calloc((size_t)B, sizeof(int *));
  int *cells = (int *)calloc((size_t)B * 2, sizeof(int));
  if (!score || !row || !cells) { free(score); free(row); free(cells); return NULL; }
  for (int j = 0; j < B; j++) row[j] = cells + 2 * j;
  for (int ff = 0; ff < 2; ff++)
  {
    score[ff] = (int ***)calloc((size_t)num_align, sizeof(int **));
    if (!score[ff]) { free(score[0]); free(score); free(row); free(cells); return NULL; }
    for (int n = 0; n < num_align; n++) score[ff][n] = row;
  }
  return score;
}

void ramx_free_score(int num_align, int bandwidth, int ****score)
{
  (void)bandwidth;
  if (!score) return;
  if (num_align >= 1 && score[0] && score[0][0])
  {
    free(score[0][0][0]);     /* the shared cells */
    free(score[0][0]);        /* the shared row */
  }
  free(score[0]); free(score[1]);
  free(score);
}
