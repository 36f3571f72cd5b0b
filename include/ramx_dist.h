/* ramx_dist.h -- pairwise divergence between the copies of an extension (libramx).  An addition to ramx.h, kept in a header
 * of its own: ramx.h is unchanged by it.
 *
 * The per-copy statistics compare every copy with the consensus, the plane Gram compares columns with columns over the copies;
 * this is the transpose of the second: copy against copy over the columns.  Everything is defined on the planes of ramx_plane
 * (ramx.h).  For copy i (flank index within its family) and row r:
 *   called    bit i of one of the planes (r, 0..3) is set; base(i, r) is that class
 *   deleted   plane (r, 5)
 *   covered   plane (r, 6)
 * Class N is covered but not called.  Inserted bases (class 7) and tail_ins count nowhere. */
#ifndef RAMX_DIST_H
#define RAMX_DIST_H

#include "ramx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One pair of copies (a, b), summed over the rows r < rows[f].  The struct is 24 bytes without padding. */
typedef struct ramx_copy_dist
{
  int32_t cover;      /* both covered */
  int32_t sites;      /* both called; matches are sites - ts - tv */
  int32_t ts;         /* both called, the bases A<->G or C<->T */
  int32_t tv;         /* both called, the bases of different kind (purine against pyrimidine) */
  int32_t del_one;    /* both covered, exactly one deleted */
  int32_t del_both;   /* both deleted */
} ramx_copy_dist;
#define RAMX_DIST_MAX_COPIES 2048           /* copies of one family in one matrix: a 96 MB result */

/* The pair matrix of chosen copies of the resident replay: it works on the planes the last ramx_dev_planes left on the device,
 * with the lifetime rule of ramx_dev_plane_gram (RAMX_ERR_STATE without resident planes; RAMX_ERR_ARG if n_families differs
 * from that call).  Family f's list is copies[copy_first[f] .. + copy_count[f]): flank indices within the family, strictly
 * increasing, each < fam_count[f] of that ramx_dev_planes call (the session keeps fam_count), at most RAMX_DIST_MAX_COPIES of
 * them -- anything else is RAMX_ERR_ARG.  Every list is checked before anything is launched or written.
 * out + out_first[f] receives [C_f][C_f] row-major records, C_f = copy_count[f]: entry [a][b] is the pair of the a-th and the
 * b-th copy of the list.  The matrix is symmetric.  The diagonal is a copy with itself: cover = its ramx_copy_stats.cols,
 * sites = its match + ts + tv, del_both = its del, ts = tv = del_one = 0.
 * A family with C_f == 0 writes nothing (a family without flanks can only have C_f == 0); a family with rows[f] == 0 receives
 * all-zero records, written on the host.
 * On the device a wave per tile and 64 rows transposes the planes into five bit streams over the rows per chosen copy, and a
 * blocked kernel counts every pair with ANDs, XORs and popcounts in registers: exact integers, no atomics, so the result does
 * not depend on any order.  The call may be repeated with other lists.  Rank-local under a communicator: a rank sees only its
 * own copies. */
int ramx_dev_copy_dist(ramx_dev *d, int32_t n_families, const int32_t *copies, const int32_t *copy_first,
                       const int32_t *copy_count, ramx_copy_dist *out, const int64_t *out_first);
/* HIP-event times (ms) of the transposition kernel (ms[0]) and the pair kernel (ms[1]) of the last ramx_dev_copy_dist on this
 * device; 0 where none was launched. */
void ramx_dev_copy_dist_ms(ramx_dev *d, double ms[2]);

/* Which copies to ask for (plain host C).  Copy i of ends[0..n) has cols(i) = min(end_row, rows - 1) + 1 columns and qualifies
 * iff end_row >= 0 and cols(i) >= max(min_cols, 1).  max_copies is held to [0, RAMX_DIST_MAX_COPIES].  If more than max_copies
 * qualify, those with the most columns are kept, ties to the lower index.  out (room for min(n, max_copies)) receives the
 * selection in ascending order; returns its length. */
int32_t ramx_select_copies(const ramx_aln_end *ends, int32_t n, int32_t rows, int32_t min_cols, int32_t max_copies, int32_t *out);

/* Kimura two-parameter distance of a pair, in percent: the formula of ramx_copy_kimura on sites, ts and tv.  -1 when
 * undefined (sites == 0, a <= 0 or b <= 0). */
double ramx_dist_kimura(const ramx_copy_dist *p);

/* Summary of one [n][n] matrix m (plain host C).  pairs = n (n - 1) / 2; used is the number of pairs a < b with
 * sites >= max(min_sites, 1) and a defined Kimura value, mean their mean (0.0 when there are none).  m(a) is the mean over the
 * used pairs that contain a; medoid is the a with the smallest defined m(a), ties to the lower a, -1 when there is none, and
 * medoid_mean that m(a) (0.0 without a medoid).  RAMX_ERR_ARG for n < 0 or a missing pointer. */
typedef struct ramx_dist_family { int32_t n, pairs, used, medoid; double mean, medoid_mean; } ramx_dist_family;
int ramx_dist_summary(const ramx_copy_dist *m, int32_t n, int32_t min_sites, ramx_dist_family *out);

/* Distance sink of seam 1, as the other sinks (the last of them): with a sink set, per direction and family that has run,
 * along the kept consensus (rows = ret): ramx_dev_planes with ends requested, ramx_select_copies(min_cols, max_copies) on those
 * ends, and ramx_dev_copy_dist of the selection.  copies is [n_copies], indices into the direction's flanks (ends, core_index:
 * [n_flanks]); dist is [n_copies][n_copies].  A direction without an extendable core or with ret = 0 is answered on the host
 * with n_copies = 0.  With a communicator or mailbox route active the direction fails with RAMX_ERR_UNSUPPORTED, as the
 * linkage sink.  cb == NULL (the default): off. */
typedef struct ramx_dist
{
  int32_t direction, family /* index in a batch, else 0 */, rows /* = ret */, n_flanks, n_copies;
  const int8_t *cons;                 /* [rows] */
  const int32_t *core_index;          /* [n_flanks] */
  const ramx_aln_end *ends;           /* [n_flanks] */
  const int32_t *copies;              /* [n_copies] */
  const ramx_copy_dist *dist;         /* [n_copies][n_copies] */
} ramx_dist;
typedef void (*ramx_dist_cb)(const ramx_dist *dist, void *user);
void ramx_set_dist_sink(ramx_dist_cb cb, void *user, int32_t min_cols, int32_t max_copies);

#ifdef __cplusplus
}
#endif

#endif
