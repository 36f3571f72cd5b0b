/* ramx_xfam.h -- cross-family overlap of the extended consensi (libramx).  An addition to ramx.h, kept in a header of its
 * own: ramx.h and ramx_dist.h are unchanged by it.
 *
 * Every other analysis looks inside one family.  Seed alignments from de-novo discovery are fragments of longer elements, and
 * two fragment families of one element extend into each other: this compares the extensions of a batch with each other -- a
 * gapped local alignment of every candidate pair of sequences, per orientation -- and groups the families that overlap.
 * Nothing about the alignment is defined anew: cells, payload, "first of D, U, L", the best cell by the smallest i, then the
 * smallest j, and min_score are those of ramx_term (ramx.h); the sequences are of any two lengths up to RAMX_XFAM_MAXLEN. */
#ifndef RAMX_XFAM_H
#define RAMX_XFAM_H

#include "ramx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The longest sequence of a pair: offsets and the count of matches fit 15 bits, the count of columns (at most the two lengths
 * together) 16, which is what the device kernel packs into the two payload words of a cell. */
#define RAMX_XFAM_MAXLEN 32767

/* match 1..15, mismatch 1..15, gap 1..31, min_score >= 1 (the ranges of ramx_term_params); anything else is RAMX_ERR_ARG.
 * Defaults: 2, 3, 5, 80.  80 is the score of 80 columns at 80 % identity (64 * 2 - 16 * 3), and it is more than twice what
 * chance gives under these scores: the largest best score of independent random sequences in the restatement
 * tests/term_ref.py was 30 over 200 pairs of 2,000 x 2,000 and 36 over 20 pairs of 10,000 x 10,000. */
typedef struct ramx_pair_params { int32_t match, mismatch, gap, min_score; } ramx_pair_params;

/* Two sequences of a set by index, and the orientation of the second; reserved is 0. */
typedef struct ramx_seq_pair { int32_t a, b, inverted, reserved; } ramx_seq_pair;

/* Sequences: one array of library codes and seq_off[n_seqs + 1], non-decreasing; sequence s is codes[seq_off[s] ..
 * seq_off[s + 1]).  Class of a code as for the terminal repeats: codes 0..7 are class code & 3, everything else is class 4.
 *
 * Record of a pair (a ramx_term, 32 bytes): what ramx_term_pair(A, na, B', nb, ...) gives for the same match, mismatch, gap and
 * min_score.  B' = B when inverted == 0; when inverted == 1, B reversed with the classes below 4 complemented (3 - x).
 * b_start and b_end are offsets in B'; T = min(na, nb); a zero-length side gives an all-zero record. */

/* The record of one pair on the host (plain host C; the cells are those of ramx_term_pair).  RAMX_ERR_ARG for bad parameters, a
 * negative length, inverted outside 0 / 1 or a missing pointer; RAMX_ERR_UNSUPPORTED above RAMX_XFAM_MAXLEN. */
int ramx_seq_pair_host(const int8_t *codes_a, int32_t na, const int8_t *codes_b, int32_t nb, int32_t inverted,
                       const ramx_pair_params *pp, ramx_term *out);

/* One record per pair, in pair order, on the device: one wave per pair sweeps the na x nb cells in strips of 64 C columns (C =
 * 4, 8 or 16 columns a lane, chosen by nb), the last column of a strip passing through a buffer of the wave's own
 * (csrc/ramx_kernels_xfam.h).  Self-contained in the manner of ramx_dev_term: it needs no library; a following
 * ramx_dev_run_direction needs a new ramx_dev_begin_direction; resident bit planes are dropped; rank-local under a communicator.
 * d == NULL: the process-wide session of seam 1.  n_pairs == 0 returns RAMX_OK and launches nothing.
 * RAMX_ERR_ARG, raised before anything is launched or written: bad parameters, a missing pointer, an index outside
 * 0..n_seqs-1, a == b, inverted outside 0 / 1, reserved != 0, a decreasing seq_off.  RAMX_ERR_UNSUPPORTED: a sequence of a
 * pair longer than RAMX_XFAM_MAXLEN.
 * Device memory is bounded by RAMX_XFAM_BYTES (environment, read per call; default 1 GiB): a pair takes 16 * na bytes for its
 * strip border plus 80 for its descriptor and record, and every sequence a group of pairs uses is uploaded once per group
 * (its length rounded up to 16); consecutive pairs are processed in groups that fit, RAMX_ERR_UNSUPPORTED if one pair alone does
 * not; the grouping does not show in the result.  kernel_ms (may be NULL): the HIP-event time of the alignment kernels, summed
 * over the groups. */
int ramx_dev_seq_pairs(ramx_dev *d, const int8_t *codes, const int64_t *seq_off, int32_t n_seqs, const ramx_seq_pair *pairs,
                       int32_t n_pairs, const ramx_pair_params *pp, ramx_term *out, double *kernel_ms);

/* Which pairs to align (plain host C): returns the number of candidates and writes the first cap of them (pairs may be NULL
 * when cap == 0).  Enumerated are a < b, then inverted = 0, 1, in ascending (a, b, inverted) order.  Skipped: a pair with
 * owner[a] == owner[b] unless within != 0, and a pair with an empty side.  With K == 0 every remaining pair is a candidate.
 * With K in 8..16 a pair is a candidate iff the two sequences share a K-mer in that orientation: there are offsets o_a, o_b with
 * K classes below 4 on both sides and a[o_a + t] == b[o_b + t] for all t < K (direct), a[o_a + t] == 3 - b[o_b + K - 1 - t]
 * (inverted).  Any other K, a negative count or cap, a missing pointer or a decreasing seq_off is RAMX_ERR_ARG (negative).
 * The default K is 16: two unrelated sequences share a K-mer by chance with probability about na * nb / 4^K, which is 0.023
 * at 10,000 x 10,000 and 0.37 with K = 14.
 * What the filter loses: an overlap near the reporting threshold -- 80 columns at 80 % identity have 16 mismatches, so a run of
 * 16 agreeing bases is the exception there -- has no common 16-mer in most cases and is never aligned.  An overlap of a few
 * hundred bases at 10 % substitutions and 2 % indels shared one in 50 of 50 trials.  K == 0 is the exact mode. */
int64_t ramx_xfam_candidates(const int8_t *codes, const int64_t *seq_off, int32_t n_seqs, const int32_t *owner, int32_t K,
                             int32_t within, ramx_seq_pair *pairs, int64_t cap);

/* Which families belong together (plain host C, integers only).  owner[s] is the family of sequence s, 0..n_families-1.
 * A record counts (counts[p] = 1, else 0) iff score > 0, columns >= min_columns and 1000 * matches >= min_permille * columns.
 * Two different families are linked iff a counting record joins one sequence of each; records between two sequences of one
 * family never link.  group[f] is the smallest family index of f's connected component.  Defaults: 80 and 800.
 * RAMX_ERR_ARG for min_columns < 0, min_permille outside 0..1000, a negative count, a missing pointer, or an owner outside
 * 0..n_families-1 among the pairs' sequences. */
typedef struct ramx_xfam_link_params { int32_t min_columns, min_permille; } ramx_xfam_link_params;
int ramx_xfam_groups(const ramx_seq_pair *pairs, const ramx_term *records, int32_t n_pairs, const int32_t *owner,
                     int32_t n_families, const ramx_xfam_link_params *lp, int32_t *counts, int32_t *group);

#ifdef __cplusplus
}
#endif

#endif
