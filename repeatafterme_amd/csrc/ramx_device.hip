// ramx_device.hip -- seam 2 of include/ramx.h: the thin device API and the gfx950 kernels.
//
// Replaces, on the device, the reference's per-column work:
//   compute_nw_row            bnw_extend.c:750-1048   (banded affine row, 2 states per cell)
//   candidate vote + cap      ram_extend.c:973-1086
//   recompute-with-winner     ram_extend.c:1097-1168  (folded away: see "column step" below)
//   fit-preferred stop rule   ram_extend.c:1169-1223
//   boundary row              ram_extend.c:909-960
//
// Layout in HBM (Np = flanks padded to a multiple of 64, W = half band, B = 2W+1, Q = W+1):
//   bases  uint32 [KW][Np]        4-bit base classes, 8 per word, pre-oriented per flank so that
//                                 nibble (t' & 7) of word (t' >> 3) is the base aligned to band
//                                 cell (row r, offset o) with t' = o + r + W.  Transposed: the 64
//                                 lanes of a wave read 256 contiguous bytes.
//   state  int4   [Np/64][Q][64]  one DP row per flank: slot q holds cells 2q and 2q+1 as
//                                 (sub,gap,sub,gap); the last slot holds cell B-1 and (high,pos)
//                                 (overall_sequence_high_score[_pos], ram_extend.c:900-901).
//                                 Exactly 16*B+16 bytes per flank, read once and written once per
//                                 column: the algorithmic traffic of SURVEY.md section 8(d).
//   trim   int2   [Np]            trimmed_sequence_high_score[_pos] (ram_extend.c:902-903)
//   sums   int64  [3][32][4]      sharded per-candidate column sums (vote), rotated by column
//   ctl    RamxCtl[2]             stop-rule state, flip-flopped by column
//
// Column step K(r), one launch per consensus column, ONE LANE PER FLANK:
//   every wave:  fold the 32x4 vote shards of row r -> besta(r), new-max / stop decision
//   every lane:  stream its previous row S(r-1) (coalesced 16 B loads, 8 deep in flight),
//                compute row r against besta(r) -> S(r) (stored), track best cell -> high/pos,
//                and, skewed by one cell, the four candidate rows r+1 from S(r) (never stored) ->
//                capped contributions -> wave shuffle reduce -> LDS block reduce -> 4 int64 atomics
//                into one of 32 shards.
// The serial dependency through the insertion term (cells -W..+W in order) stays a plain serial
// loop inside the lane, so the values are the reference's bit for bit; parallelism comes from the
// flanks (N >= 64 k fills the chip).  No MFMA: integer max-plus recurrences, HBM-bound.

#include <rccl/rccl.h>
#include <errno.h>
#include <fcntl.h>
#include <limits.h>
#include <sys/mman.h>
#include <unistd.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <algorithm>
#include <memory>
#include <vector>

#include "ramx_kernels_common.h"
#include "ramx_kernels_stream.h"
#include "ramx_kernels_resident.h"
#include "ramx_cp_api.h"
#include "ramx_pk_api.h"
#include "ramx_profile_api.h"
#include "ramx_align_api.h"
#include "ramx_pileup_api.h"
#include "ramx_dinuc_api.h"
#include "ramx_copystats_api.h"
#include "ramx_linkage_api.h"
#include "ramx_dist_api.h"
#include "ramx_subfam_api.h"
#include "ramx_tsd_api.h"
#include "ramx_period_api.h"
#include "ramx_term_api.h"
#include "ramx_xfam_api.h"

// ------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------
static thread_local char g_err[512];

extern "C" void ramx_set_error(const char *fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char *ramx_last_error(void) { return g_err; }

#define HIPCHK(call)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (call);                                                                       \
    if (e_ != hipSuccess) {                                                                       \
      ramx_set_error("HIP error %s at %s:%d (%s)", hipGetErrorString(e_), __FILE__, __LINE__, #call); \
      return RAMX_ERR_HIP;                                                                        \
    }                                                                                             \
  } while (0)

static double now_ms(void);
// RAMX_TIMING: host-side marks inside a direction (ms since the mark before)
static void rt_mark(const char *what)
{
  static double last = 0;
  static int on = -1;
  if (on < 0) on = getenv("RAMX_TIMING") != NULL;
  if (!on) return;
  const double t = now_ms();
  if (what) fprintf(stderr, "RAMX_TIMING       run: %-44s %8.3f ms\n", what, t - last);
  last = t;
}
static double now_ms(void)
{
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

// ------------------------------------------------------------------------------------------
// host side of seam 2
// ------------------------------------------------------------------------------------------
#define RAMX_NGROUP (RAMX_CP_NCLASS + 4)   // batch mode: cell-parallel classes, then the four lane-per-flank workgroup shapes

// a family of the replay whose bit planes are resident: its rows, its tiles, where its flanks lie, and the first word of its
// rows * 8 planes of `tiles` words each
struct ResidentFam { int rows, tiles, first, count; long long base; };
// a family of the last split: the first word of its K mask planes of `tiles` words each
struct SubfamLay { long long mask0; int tiles; };

struct ramx_dev
{
  int ordinal, cus;   // cus: compute units (what every co-resident launch is planned against)
  hipStream_t stream;
  signed char *d_lib; unsigned long long lib_len; unsigned long long lib_cap;
  // packed library (ramx_dev_load_library_packed): the .2bit payload of the windows + window / N-run tables; lib_packed = 1
  int lib_packed;
  unsigned char *d_pk_bytes, *d_pk_phase; unsigned long long *d_pk_wstart, *d_pk_wbyte, *d_pk_nstart; unsigned *d_pk_nlen;
  size_t cap_pk_bytes, cap_pk_phase, cap_pk_wstart, cap_pk_wbyte, cap_pk_nstart, cap_pk_nlen, cap_flank_win;
  int pk_windows, pk_nblocks; int *d_flank_win;
  // per direction
  ramx_flank *d_flanks; unsigned *d_bases; int2 *d_bounds; int4 *d_state[2]; int2 *d_trim;
  long long *d_sums; RamxCtl *d_ctl; signed char *d_cons;
  PShard *d_vote; unsigned *d_err;   // persistent kernel: fused vote / barrier words
  int last_persistent;
  size_t cap_flanks, cap_bases, cap_state, cap_cons, cap_bounds, cap_trim, cap_fam, cap_famctl;
  void *d_fam; RamxCtl *d_famctl;    // batch mode: family descriptors / per-family control blocks (kept between calls)
  RamxCtl *h_ctl;   // pinned, [2 checkpoints][2 slots]
  void *h_stage; size_t cap_stage;   // pinned staging buffer of ramx_dev_download (a pageable 800 KB copy took 8 ms)
  hipEvent_t ev_chk[2], ev_begin, ev_end, ev_s0[MAX_SAMPLES], ev_s1[MAX_SAMPLES];
  int Nx, Np, KW;
  ramx_params p; int tab[RAMX_NCLASS][4];
  int ready;
  RamxCtl final_ctl;
  // multi-GPU
  ncclComm_t comm; int rank, nranks;
  ramx_allreduce_cb cb; void *cb_user;
  // cross-device persistent path: this rank's box (fine-grained), every rank's box as mapped here, device copy of that table
  PeerBox *xbox; PeerBox *peer[RAMX_MAX_RANKS]; PeerBox **d_peer; int peer_ready;
  void *peer_ipc[RAMX_MAX_RANKS];   // what hipIpcOpenMemHandle returned for the other ranks' boxes (closed on re-import / destroy)
  // host-memory variant of the boxes (POSIX shared memory registered with HIP): xbox/peer point into it
  void *hostbox_map; size_t hostbox_bytes; PeerBox *hostbox_host; int hostbox_registered;
  PeerBox *hostbox_mirror;   // device-memory copy of my host box, kept current by block 0 (the other blocks poll it)
  PeerBox *devbox;     // this rank's fine-grained device-memory box (exported over hipIpc)
  hipStream_t cls_stream[RAMX_NGROUP]; hipEvent_t cls_ready, cls_done[RAMX_NGROUP]; int cls_init;   // batch mode: one stream per workgroup shape
  int force_chain;   // RAMX_FORCE_CHAIN=1: always run the full candidate recurrence (test hook)
  ramx_row_trace_cb trace_cb; void *trace_user;   // -outmat: per-row trace (forces the per-column launches)
  ramx_row_verbose_cb verbose_cb; void *verbose_user;   // -vvvv: per-row candidate trace (per-column launches, full candidate recurrence)
  signed char *d_dbg_codes; int2 *d_dbg_best; size_t cap_dbg_codes, cap_dbg_best;
  int *d_dbg_cand; int2 *d_dbg_gap; size_t cap_dbg_cand, cap_dbg_gap;
  int *d_dbg_band; size_t cap_dbg_band; int verbose_band;      // -vvvvv: every cell of the candidate rows
  CpDevDesc *d_devdesc; size_t cap_devdesc;       // device-wide cell-parallel launches: one descriptor per workgroup
  PShard *d_vote_sets; size_t cap_vote_sets; unsigned *d_err_sets; size_t cap_err_sets;   // batch mode: per-set vote / error words
  int packed_kw;       // words of every window packed so far (begin_direction packs the first piece, see pack_rest)
  int pk_last_lanes, pk_last_words;   // what launch_pack was last called with: lanes of d_bases, words packed (ramx_dev_peek_windows)
  hipStream_t pack_stream; hipEvent_t pack_done; int pack_busy;      // the following pieces are packed beside the running one
  int pk_r0;           // begin_direction: first row from which no flank has a low out-of-bounds cell (the packed-row kernel starts there); -1: none
  int last_packed_r0;  // last direction: first row of the packed-row kernel, -1 if it did not run
  int cp_flanks_ok;    // begin_direction: every flank is empty or has t_lo <= 0 (what the cell-parallel kernels take)
  int2 *d_cpstate; size_t cap_cpstate; int cpstate_W, cpstate_n;   // RAMX_CP_PEEK=1: final rows of the cell-parallel kernel (tests)
  // every replay along a given consensus (replay_setup, allocated on the first call): rows, consensus / rows / family / tile tables
  int4 *d_rp_state; signed char *d_rp_cons; int *d_rp_rows; int4 *d_rp_fam; int2 *d_rp_tile;
  size_t cap_rp_state, cap_rp_cons, cap_rp_rows, cap_rp_fam, cap_rp_tile;
  // ramx_dev_profile (allocated on its first call): per-wave records, summed columns, per-flank outputs
  ramx_col_profile *d_pf_slab, *d_pf_cols; int *d_pf_last, *d_pf_best, *d_pf_bidx;
  size_t cap_pf_slab, cap_pf_cols, cap_pf_last, cap_pf_best, cap_pf_bidx;
  // ramx_dev_align (allocated on its first call): decision codes, per-flank records (both also the pileup's), per-column outputs
  unsigned *d_al_codes; ramx_aln_end *d_al_ends; int *d_al_idx, *d_al_ins;
  size_t cap_al_codes, cap_al_ends, cap_al_idx, cap_al_ins;
  // ramx_dev_pileup / ramx_dev_refine (allocated on their first call): one group's walked columns, per-tile records, summed columns
  int *d_pl_idx, *d_pl_ins; ramx_col_pileup *d_pl_slab, *d_pl_cols;
  // ramx_dev_copy_stats (allocated on its first call): one record per flank
  ramx_copy_stats *d_cs_stats;
  size_t cap_pl_idx, cap_pl_ins, cap_pl_slab, cap_pl_cols, cap_cs_stats;
  // ramx_dev_dinuc / ramx_dev_refine_cpg (allocated on their first call): per-tile row-pair records, summed records
  ramx_col_dinuc *d_dn_slab, *d_dn_cols;
  size_t cap_dn_slab, cap_dn_cols;
  // ramx_dev_planes / ramx_dev_plane_gram (allocated on their first call): the bit planes of the whole flank set, which stay
  // resident between the two calls (planes_ready, dropped like `ready` by whatever reuses the replays' buffers); the host keeps
  // the resident replay's families (res_fam, malloc'd) and its n_padded for every call that answers from the planes
  unsigned long long *d_lk_planes; long long *d_lk_base, *d_lk_at, *d_lk_coat; int4 *d_lk_block, *d_lk_gfam; int *d_lk_co;
  size_t cap_lk_planes, cap_lk_base, cap_lk_at, cap_lk_coat, cap_lk_block, cap_lk_gfam, cap_lk_co;
  int planes_ready, res_families, res_npadded; ResidentFam *res_fam;
  double lk_gram_ms;        // HIP-event time of the last Gram kernel (ramx_dev_plane_gram_ms)
  // ramx_dev_copy_dist (allocated on its first call): the chosen copies' bit streams over the rows, the lists it uploads and
  // the pair records
  unsigned long long *d_lk_streams; DistFam *d_lk_dfam; int4 *d_lk_ditem, *d_lk_dblock; int *d_lk_dslot; ramx_copy_dist *d_lk_dist;
  size_t cap_lk_streams, cap_lk_dfam, cap_lk_ditem, cap_lk_dblock, cap_lk_dslot, cap_lk_dist;
  double lk_dist_ms[2];     // HIP-event times of the transposition and the pair kernel of the last ramx_dev_copy_dist
  // ramx_dev_subfamilies (allocated on its first call): the lists it uploads, the labels, the mask planes and the counts
  SubfamFam *d_sf_fam; long long *d_sf_at; longlong2 *d_sf_var; unsigned char *d_sf_pat; int2 *d_sf_tile, *d_sf_item;
  int *d_sf_count, *d_sf_labels, *d_sf_changed, *d_sf_cnt; unsigned long long *d_sf_mask;
  size_t cap_sf_fam, cap_sf_at, cap_sf_var, cap_sf_pat, cap_sf_tile, cap_sf_item, cap_sf_count, cap_sf_labels, cap_sf_changed,
         cap_sf_cnt, cap_sf_mask;
  SubfamLay *sf_lay; int sf_families, sf_K;       // the last result's mask planes, per family (malloc'd)
  double sf_ms[2];          // HIP-event times of the assign and the count kernels of the last ramx_dev_subfamilies, summed
  // ramx_dev_tsd (allocated on its first call): per site the room between the two words, and its record
  int *d_tsd_room; ramx_tsd *d_tsd_out; size_t cap_tsd_room, cap_tsd_out;
  // ramx_dev_period (allocated on its first call): the segments' streams (bases, validity), their lengths and records
  unsigned long long *d_per_bases; unsigned *d_per_valid; int *d_per_len; ramx_period *d_per_out;
  size_t cap_per_bases, cap_per_valid, cap_per_len, cap_per_out;
  // ramx_dev_term (allocated on its first call; its streams and window lengths live in the buffers of ramx_dev_period): the records
  ramx_term *d_term_out; size_t cap_term_out;
  // ramx_dev_seq_pairs (allocated on its first call): the sequences, pair descriptors, strip borders and records of a group
  signed char *d_xf_codes; XfamPair *d_xf_pairs; int4 *d_xf_border; ramx_term *d_xf_out;
  size_t cap_xf_codes, cap_xf_pairs, cap_xf_border, cap_xf_out;
};

extern "C" int ramx_device_count(void)
{
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { ramx_set_error("hipGetDeviceCount: %s", hipGetErrorString(e)); return RAMX_ERR_NO_DEVICE; }
  return n;
}

extern "C" int ramx_dev_create(int ordinal, ramx_dev **out)
{
  int n = ramx_device_count();
  if (n <= 0) { ramx_set_error("no HIP device visible (libramx has no CPU path)"); return RAMX_ERR_NO_DEVICE; }
  if (ordinal < 0 || ordinal >= n) { ramx_set_error("device ordinal %d out of range (%d devices)", ordinal, n); return RAMX_ERR_ARG; }
  HIPCHK(hipSetDevice(ordinal));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, ordinal));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
  {
    ramx_set_error("device %d is %s; libramx carries gfx950 code objects only", ordinal, prop.gcnArchName);
    return RAMX_ERR_NO_DEVICE;
  }
  ramx_dev *d = (ramx_dev *)calloc(1, sizeof(ramx_dev));
  d->ordinal = ordinal; d->cus = prop.multiProcessorCount;
  // any failure below releases what has been created so far (ramx_dev_destroy copes with a partly built session)
#define CRCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    ramx_set_error("HIP error %s at %s:%d (%s)", hipGetErrorString(e_), __FILE__, __LINE__, #call); ramx_dev_destroy(d); return RAMX_ERR_HIP; } } while (0)
  CRCHK(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
  CRCHK(hipStreamCreateWithFlags(&d->pack_stream, hipStreamNonBlocking));
  CRCHK(hipEventCreateWithFlags(&d->pack_done, hipEventDisableTiming));
  CRCHK(hipHostMalloc((void **)&d->h_ctl, 4 * sizeof(RamxCtl), hipHostMallocDefault));
  // staging buffer of ramx_dev_download: allocated here (pinning takes milliseconds; the executable creates the session in its
  // helper thread), 2 MB = 262,144 flanks, grown on demand
  CRCHK(hipHostMalloc(&d->h_stage, (size_t)2 << 20, hipHostMallocDefault));
  d->cap_stage = (size_t)2 << 20;
  CRCHK(hipMalloc((void **)&d->d_sums, (3 * NSHARD * 4 + 8) * sizeof(long long)));
  CRCHK(hipMalloc((void **)&d->d_ctl, 2 * sizeof(RamxCtl)));
  CRCHK(hipMalloc((void **)&d->d_vote, PRK_NSETS * NSHARD * sizeof(PShard)));   // four rotating vote sets (both persistent kernels)
  CRCHK(hipMalloc((void **)&d->d_err, 64));

  for (int i = 0; i < 2; i++) CRCHK(hipEventCreate(&d->ev_chk[i]));
  CRCHK(hipEventCreate(&d->ev_begin));
  CRCHK(hipEventCreate(&d->ev_end));
  for (int i = 0; i < MAX_SAMPLES; i++) { CRCHK(hipEventCreate(&d->ev_s0[i])); CRCHK(hipEventCreate(&d->ev_s1[i])); }
#undef CRCHK
  const char *eb = getenv("RAMX_FORCE_CHAIN");
  d->force_chain = (eb && atoi(eb) != 0) ? 1 : 0;
  *out = d;
  return RAMX_OK;
}

extern "C" void ramx_dev_destroy(ramx_dev *d)
{
  if (!d) return;
  (void)hipSetDevice(d->ordinal);
  if (d->stream) (void)hipStreamSynchronize(d->stream);
  if (d->pack_stream) { (void)hipStreamSynchronize(d->pack_stream); (void)hipStreamDestroy(d->pack_stream); }
  if (d->pack_done) (void)hipEventDestroy(d->pack_done);
  if (d->comm) (void)ncclCommDestroy(d->comm);
  // mappings of the other ranks' mailboxes (hipIpcOpenMemHandle): closed before anything of this device is released
  for (int q = 0; q < RAMX_MAX_RANKS; q++)
    if (d->peer_ipc[q]) { (void)hipIpcCloseMemHandle(d->peer_ipc[q]); d->peer_ipc[q] = NULL; }
  (void)hipFree(d->d_pk_bytes); (void)hipFree(d->d_pk_phase); (void)hipFree(d->d_pk_wstart); (void)hipFree(d->d_pk_wbyte);
  (void)hipFree(d->d_pk_nstart); (void)hipFree(d->d_pk_nlen); (void)hipFree(d->d_flank_win);
  (void)hipFree(d->d_lib); (void)hipFree(d->d_flanks); (void)hipFree(d->d_bases); (void)hipFree(d->d_bounds);
  (void)hipFree(d->d_state[0]); if (d->d_state[1] != d->d_state[0]) (void)hipFree(d->d_state[1]); (void)hipFree(d->d_trim); (void)hipFree(d->d_sums);
  (void)hipFree(d->d_ctl); (void)hipFree(d->d_cons); (void)hipFree(d->d_vote); (void)hipFree(d->d_err);
  if (d->h_ctl) (void)hipHostFree(d->h_ctl);
  if (d->h_stage) (void)hipHostFree(d->h_stage);
  if (d->hostbox_map)
  {
    if (d->hostbox_registered) (void)hipHostUnregister(d->hostbox_map);
    munmap(d->hostbox_map, d->hostbox_bytes);
  }
  if (d->cls_init)
  {
    for (int c = 0; c < RAMX_NGROUP; c++) { (void)hipStreamDestroy(d->cls_stream[c]); (void)hipEventDestroy(d->cls_done[c]); }
    (void)hipEventDestroy(d->cls_ready);
  }
  if (d->devbox) (void)hipFree(d->devbox);
  (void)hipFree(d->d_fam); (void)hipFree(d->d_famctl); (void)hipFree(d->d_cpstate); (void)hipFree(d->d_dbg_codes); (void)hipFree(d->d_dbg_best); (void)hipFree(d->d_dbg_cand); (void)hipFree(d->d_dbg_gap); (void)hipFree(d->d_dbg_band); (void)hipFree(d->d_devdesc); (void)hipFree(d->d_vote_sets); (void)hipFree(d->d_err_sets);
  (void)hipFree(d->d_rp_state); (void)hipFree(d->d_rp_cons); (void)hipFree(d->d_rp_rows); (void)hipFree(d->d_rp_fam); (void)hipFree(d->d_rp_tile);
  (void)hipFree(d->d_pf_slab); (void)hipFree(d->d_pf_cols); (void)hipFree(d->d_pf_last); (void)hipFree(d->d_pf_best); (void)hipFree(d->d_pf_bidx);
  (void)hipFree(d->d_al_codes); (void)hipFree(d->d_al_ends); (void)hipFree(d->d_al_idx); (void)hipFree(d->d_al_ins);
  (void)hipFree(d->d_pl_idx); (void)hipFree(d->d_pl_ins); (void)hipFree(d->d_pl_slab); (void)hipFree(d->d_pl_cols);
  (void)hipFree(d->d_cs_stats);
  (void)hipFree(d->d_dn_slab); (void)hipFree(d->d_dn_cols);
  (void)hipFree(d->d_lk_planes); (void)hipFree(d->d_lk_base); (void)hipFree(d->d_lk_at); (void)hipFree(d->d_lk_coat);
  (void)hipFree(d->d_lk_block); (void)hipFree(d->d_lk_gfam); (void)hipFree(d->d_lk_co);
  (void)hipFree(d->d_lk_streams); (void)hipFree(d->d_lk_dfam); (void)hipFree(d->d_lk_ditem); (void)hipFree(d->d_lk_dblock);
  (void)hipFree(d->d_lk_dslot); (void)hipFree(d->d_lk_dist);
  free(d->res_fam);
  (void)hipFree(d->d_sf_fam); (void)hipFree(d->d_sf_at); (void)hipFree(d->d_sf_var); (void)hipFree(d->d_sf_pat);
  (void)hipFree(d->d_sf_tile); (void)hipFree(d->d_sf_item); (void)hipFree(d->d_sf_count); (void)hipFree(d->d_sf_labels);
  (void)hipFree(d->d_sf_changed); (void)hipFree(d->d_sf_cnt); (void)hipFree(d->d_sf_mask);
  free(d->sf_lay);
  (void)hipFree(d->d_tsd_room); (void)hipFree(d->d_tsd_out);
  (void)hipFree(d->d_per_bases); (void)hipFree(d->d_per_valid); (void)hipFree(d->d_per_len); (void)hipFree(d->d_per_out);
  (void)hipFree(d->d_term_out);
  (void)hipFree(d->d_xf_codes); (void)hipFree(d->d_xf_pairs); (void)hipFree(d->d_xf_border); (void)hipFree(d->d_xf_out);
  if (d->hostbox_mirror) (void)hipFree(d->hostbox_mirror);
  if (d->d_peer) (void)hipFree(d->d_peer);
  for (int i = 0; i < 2; i++) if (d->ev_chk[i]) (void)hipEventDestroy(d->ev_chk[i]);
  if (d->ev_begin) (void)hipEventDestroy(d->ev_begin);
  if (d->ev_end) (void)hipEventDestroy(d->ev_end);
  for (int i = 0; i < MAX_SAMPLES; i++) { if (d->ev_s0[i]) (void)hipEventDestroy(d->ev_s0[i]); if (d->ev_s1[i]) (void)hipEventDestroy(d->ev_s1[i]); }
  if (d->stream) (void)hipStreamDestroy(d->stream);
  free(d);
}

extern "C" int ramx_dev_load_library(ramx_dev *d, const int8_t *sequence, uint64_t length)
{
  if (!d || (!sequence && length)) { ramx_set_error("ramx_dev_load_library: bad argument"); return RAMX_ERR_ARG; }
  HIPCHK(hipSetDevice(d->ordinal));
  if (length > d->lib_cap)
  {
    if (d->d_lib) HIPCHK(hipFree(d->d_lib));
    d->d_lib = NULL;
    HIPCHK(hipMalloc((void **)&d->d_lib, length ? length : 1));
    d->lib_cap = length;
  }
  if (length) HIPCHK(hipMemcpyAsync(d->d_lib, sequence, length, hipMemcpyHostToDevice, d->stream));
  HIPCHK(hipStreamSynchronize(d->stream));
  d->lib_len = length;
  d->lib_packed = 0;
  return RAMX_OK;
}

template <typename T>
static int ensure(T **p, size_t *cap, size_t need_bytes);

extern "C" int ramx_dev_load_library_packed(ramx_dev *d, const struct ramx_packed_library *pl)
{
  if (!d || !pl || pl->n_windows < 0 || (pl->n_windows && (!pl->win_start || !pl->win_byte || !pl->win_phase || !pl->bytes)) ||
      pl->n_blocks < 0 || (pl->n_blocks && (!pl->n_start || !pl->n_len)))
  { ramx_set_error("ramx_dev_load_library_packed: bad argument"); return RAMX_ERR_ARG; }
  HIPCHK(hipSetDevice(d->ordinal));
  const size_t nw = (size_t)pl->n_windows, nb = (size_t)pl->n_blocks;
  int rc;
  if ((rc = ensure(&d->d_pk_bytes, &d->cap_pk_bytes, (size_t)pl->n_bytes + 16))) return rc;
  if ((rc = ensure(&d->d_pk_wstart, &d->cap_pk_wstart, (nw + 1) * sizeof(unsigned long long)))) return rc;
  if ((rc = ensure(&d->d_pk_wbyte, &d->cap_pk_wbyte, (nw + 1) * sizeof(unsigned long long)))) return rc;
  if ((rc = ensure(&d->d_pk_phase, &d->cap_pk_phase, nw + 1))) return rc;
  if ((rc = ensure(&d->d_pk_nstart, &d->cap_pk_nstart, (nb + 1) * sizeof(unsigned long long)))) return rc;
  if ((rc = ensure(&d->d_pk_nlen, &d->cap_pk_nlen, (nb + 1) * sizeof(unsigned)))) return rc;
  if (pl->n_bytes) HIPCHK(hipMemcpyAsync(d->d_pk_bytes, pl->bytes, (size_t)pl->n_bytes, hipMemcpyHostToDevice, d->stream));
  if (nw)
  {
    HIPCHK(hipMemcpyAsync(d->d_pk_wstart, pl->win_start, (nw + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipMemcpyAsync(d->d_pk_wbyte, pl->win_byte, (nw + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipMemcpyAsync(d->d_pk_phase, pl->win_phase, nw, hipMemcpyHostToDevice, d->stream));
  }
  if (nb)
  {
    HIPCHK(hipMemcpyAsync(d->d_pk_nstart, pl->n_start, nb * sizeof(unsigned long long), hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipMemcpyAsync(d->d_pk_nlen, pl->n_len, nb * sizeof(unsigned), hipMemcpyHostToDevice, d->stream));
  }
  HIPCHK(hipStreamSynchronize(d->stream));
  d->lib_len = pl->length; d->pk_windows = pl->n_windows; d->pk_nblocks = pl->n_blocks;
  d->lib_packed = 1;
  return RAMX_OK;
}

// flank descriptors (already on the device) -> transposed, pre-oriented 4-bit windows + bounds, from either kind of library:
// words [k_lo, k_hi) of every flank's window, on stream `st`
// class table: tab[class][cand] = matrix[cand][code(class)], reference index order [cons][seq]
static void class_tab(const ramx_params *p, int (&tab)[RAMX_NCLASS][4])
{
  for (int c = 0; c < RAMX_NCLASS; c++)
  {
    const int code = (c == 8) ? RAMX_SYM_N : c;
    for (int k = 0; k < 4; k++) tab[c][k] = p->matrix[k * 100 + code];
  }
}

// words of a packed window: t'' = o + r + W + 8 runs over [7, L + 2W + 9]; + pad word in front, + lookahead words read by the kernels
static int window_words(int L, int W) { return (L + 2 * W + 2) / 8 + 12; }

static int launch_pack(ramx_dev *d, int Nx, int Np, int W, int k_lo, int k_hi, hipStream_t st)
{
  if (k_hi <= k_lo) return RAMX_OK;
  d->pk_last_lanes = Np; d->pk_last_words = k_hi;      // (a piece continues where the piece before ended: words [0, k_hi) are packed)
  if (!d->lib_packed)
  {
    dim3 grid((Np + 255) / 256, k_hi - k_lo);
    hipLaunchKernelGGL(ramx_pack_kernel, grid, dim3(256), 0, st, d->d_lib, (unsigned long long)d->lib_len,
                       d->d_flanks, Nx, Np, W, k_lo, d->d_bases, d->d_bounds);
    HIPCHK(hipGetLastError());
    return RAMX_OK;
  }
  PkLib L;
  L.bytes = d->d_pk_bytes; L.win_start = d->d_pk_wstart; L.win_byte = d->d_pk_wbyte; L.win_phase = d->d_pk_phase;
  L.n_start = d->d_pk_nstart; L.n_len = d->d_pk_nlen; L.length = d->lib_len; L.n_windows = d->pk_windows; L.n_blocks = d->pk_nblocks;
  if (k_lo == 0)
  {
    int rc;
    if ((rc = ensure(&d->d_flank_win, &d->cap_flank_win, (size_t)Np * sizeof(int)))) return rc;
    if (Nx > 0)
    {
      hipLaunchKernelGGL(ramx_flank_window_kernel, dim3((Nx + 255) / 256), dim3(256), 0, st, L, d->d_flanks, Nx, d->d_flank_win);
      HIPCHK(hipGetLastError());
    }
  }
  hipLaunchKernelGGL(ramx_pack2_kernel, dim3((Np + 255) / 256, (k_hi - k_lo + RAMX_PK_WORDS - 1) / RAMX_PK_WORDS), dim3(256), 0, st, L, d->d_flanks,
                     d->d_flank_win, Nx, Np, W, k_lo, k_hi, d->d_bases, d->d_bounds);
  HIPCHK(hipGetLastError());
  return RAMX_OK;
}

// A direction's windows are L + 2W columns long, and most runs stop after a fraction of them (the reference's default: 100 columns
// behind the end of the alignment): begin_direction packs the first RAMX_PK_SEGMENT columns, the packed-row route packs the
// following pieces on a second stream while the piece before them runs (prk_run), and every other route packs the rest here.
// prk_run counts a piece's words as packed (packed_kw) as soon as their pack is ENQUEUED on pack_stream, and a direction that
// stops early leaves that pack in flight.  Whoever next reads the windows, or rewrites or reallocates the flank and window
// buffers it reads and writes, settles it first: a wait on the library's stream, or on the host (before buffers are released).
static int pack_settle(ramx_dev *d, bool on_host = false)
{
  if (!d->pack_busy) return RAMX_OK;
  if (on_host) HIPCHK(hipEventSynchronize(d->pack_done));
  else HIPCHK(hipStreamWaitEvent(d->stream, d->pack_done, 0));
  d->pack_busy = 0;
  return RAMX_OK;
}
static int pack_rest(ramx_dev *d)
{
  { const int src = pack_settle(d); if (src != RAMX_OK) return src; }      // before the early return: "packed" may mean "enqueued"
  if (d->packed_kw >= d->KW) return RAMX_OK;
  const int rc = launch_pack(d, d->Nx, d->Np, d->p.bandwidth, d->packed_kw, d->KW, d->stream);
  d->packed_kw = d->KW;
  return rc;
}
static int pk_segment_columns(int L, int when_to_stop)
{
  const char *e = getenv("RAMX_PK_SEGMENT");
  // a direction whose stop rule cannot fire before its last column (-stopafter >= L: every column is wanted) reads its whole
  // window anyway: one piece
  const int v = e ? atoi(e) : (when_to_stop >= L ? 0 : 2048);
  return v < 0 ? 0 : v;          // 0: the whole direction in one piece (everything packed at once)
}

template <typename T>
static int ensure(T **p, size_t *cap, size_t need_bytes)
{
  if (need_bytes <= *cap && *p) return RAMX_OK;
  if (*p) HIPCHK(hipFree(*p));
  *p = NULL;
  HIPCHK(hipMalloc((void **)p, need_bytes ? need_bytes : 16));
  *cap = need_bytes;
  return RAMX_OK;
}

// a host vector into a device buffer of at least its size, on d->stream: the caller synchronises before the vector goes; an
// empty one leaves a buffer that exists
template <typename T>
static int upload(ramx_dev *d, T **p, size_t *cap, const std::vector<T> &v)
{
  int rc;
  if ((rc = ensure(p, cap, v.size() * sizeof(T)))) return rc;
  if (!v.empty()) HIPCHK(hipMemcpyAsync(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, d->stream));
  return RAMX_OK;
}

// flank descriptors, packed windows, bounds and trim records of Np flanks (kept between calls: a hipFree / hipMalloc pair costs
// ~0.5 ms of device sync per call)
static int ensure_windows(ramx_dev *d, int Np, int KW)
{
  int rc;
  if ((rc = ensure(&d->d_flanks, &d->cap_flanks, (size_t)Np * sizeof(ramx_flank)))) return rc;
  if ((rc = ensure(&d->d_bases, &d->cap_bases, (size_t)KW * Np * sizeof(unsigned)))) return rc;
  if ((rc = ensure(&d->d_bounds, &d->cap_bounds, (size_t)Np * sizeof(int2)))) return rc;
  return ensure(&d->d_trim, &d->cap_trim, (size_t)Np * sizeof(int2));
}

// The row buffer, 16 B x (W + 1) slots per flank.  The row is updated IN PLACE: a lane only ever touches its own 16-byte column
// of the tile, reads slot q+16 before it writes slot q, and launches are serialised, so one buffer serves as S(r-1) and S(r).
// Halving the footprint (65.6 MB at N = 100,000) keeps the whole row set inside the Infinity Cache.
static int ensure_rows(ramx_dev *d, size_t bytes, bool pingpong)
{
  if (bytes <= d->cap_state && d->d_state[0]) return RAMX_OK;
  if (d->d_state[0]) HIPCHK(hipFree(d->d_state[0]));
  if (d->d_state[1] && d->d_state[1] != d->d_state[0]) HIPCHK(hipFree(d->d_state[1]));
  d->d_state[0] = d->d_state[1] = NULL; d->cap_state = 0;
  HIPCHK(hipMalloc((void **)&d->d_state[0], bytes));
  if (pingpong) HIPCHK(hipMalloc((void **)&d->d_state[1], bytes));
  else d->d_state[1] = d->d_state[0];
  d->cap_state = bytes;
  return RAMX_OK;
}

// the cell-parallel kernels take flanks that are empty or start at or before the first base behind the core edge (t_lo <= 0: the
// masked band's carry argument needs the out-of-bounds prefix to end at or before the band centre)
static bool cp_flanks_fit(const ramx_flank *fl, int n)
{
  for (int i = 0; i < n; i++)
    if (fl[i].t_lo > 0 && fl[i].t_lo <= fl[i].t_hi) return false;
  return true;
}

extern "C" int ramx_dev_begin_direction(ramx_dev *d, const ramx_flank *flanks, int32_t n_flanks, const ramx_params *p)
{
  if (!d || !p || n_flanks < 0 || (n_flanks && !flanks)) { ramx_set_error("ramx_dev_begin_direction: bad argument"); return RAMX_ERR_ARG; }
  if (p->bandwidth < 0 || p->L < 0) { ramx_set_error("bandwidth and L must be >= 0"); return RAMX_ERR_ARG; }
  if (!p->matrix) { ramx_set_error("scoring matrix missing"); return RAMX_ERR_ARG; }
  HIPCHK(hipSetDevice(d->ordinal));
  rt_mark(NULL);
  const int W = p->bandwidth, Q = W + 1;
  const int Nx = n_flanks;
  const int Np = ((Nx + 63) / 64) * 64 > 0 ? ((Nx + 63) / 64) * 64 : 64;
  const int KW = window_words(p->L, W);
  d->Nx = Nx; d->Np = Np; d->KW = KW; d->p = *p;
  d->planes_ready = 0;        // the flank and window buffers the resident bit planes were made from are reused
  class_tab(p, d->tab);
  int rc;
  if ((rc = ensure_windows(d, Np, KW))) return rc;
  if ((rc = ensure_rows(d, (size_t)Np * Q * sizeof(int4), getenv("RAMX_PINGPONG") != NULL))) return rc;     // (A/B switch kept for profiling)
  if ((rc = ensure(&d->d_cons, &d->cap_cons, (size_t)p->L + 16))) return rc;
  rt_mark("begin: buffers");
  if ((rc = pack_settle(d)) != RAMX_OK) return rc;      // (a piece of the direction before still in flight: it reads d_flanks)
  if (Nx) HIPCHK(hipMemcpyAsync(d->d_flanks, flanks, (size_t)Nx * sizeof(ramx_flank), hipMemcpyHostToDevice, d->stream));
  rt_mark("begin: flanks to the device (enqueued)");
  {
    const int seg = pk_segment_columns(p->L, p->when_to_stop);
    const int first = seg > 0 ? ((seg + 8) >> 3) + 28 : KW;      // words the first piece's columns read (+ the widest band's window and look-ahead)
    d->packed_kw = first < KW ? first : KW;
    if ((rc = launch_pack(d, Nx, Np, W, 0, d->packed_kw, d->stream)) != RAMX_OK) return rc;
  }
  HIPCHK(hipMemsetAsync(d->d_sums, 0, 3 * NSHARD * 4 * sizeof(long long), d->stream));
  HIPCHK(hipMemsetAsync(d->d_cons, 0, (size_t)p->L + 16, d->stream));
  rt_mark("begin: pack of the first piece enqueued");
  HIPCHK(hipStreamSynchronize(d->stream));
  rt_mark("begin: synchronised");
  d->cp_flanks_ok = cp_flanks_fit(flanks, Nx) ? 1 : 0;
  // the packed-row kernel (ramx_kernels_packed.h) takes rows in which no flank has an out-of-bounds cell at the LOW end of the
  // band: cell 0 of row r is flank position t = r - W, so a non-empty flank is clear from row t_lo + W on
  d->pk_r0 = d->cp_flanks_ok ? 0 : -1;
  if (d->cp_flanks_ok)
    for (int i = 0; i < Nx; i++)
      if (flanks[i].t_lo <= flanks[i].t_hi && flanks[i].t_lo + W > d->pk_r0) d->pk_r0 = flanks[i].t_lo + W;
  d->ready = 1;
  return RAMX_OK;
}

template <bool INIT>
static void launch_column(ramx_dev *d, const KArgs &a)
{
  const int tiles = d->Np / 64;
  const dim3 grid((tiles + 3) / 4), block(256);
  // the chain-free candidate evaluation is exact iff neither gap penalty is positive (see the kernel header)
  if (a.go <= 0 && a.ge <= 0 && !d->force_chain)
    hipLaunchKernelGGL((ramx_column_kernel<INIT, false, 256>), grid, block, 0, d->stream, a);
  else
    hipLaunchKernelGGL((ramx_column_kernel<INIT, true, 256>), grid, block, 0, d->stream, a);
}

// -outmat trace: the DBG instantiation also writes the per-cell path codes and the row's best cell of every flank;
// -vvvv (a.dbg_cand != NULL): the full candidate recurrence, whose rows' best cells and end-cell gap states are written too
static void launch_column_trace(ramx_dev *d, const KArgs &a, bool init = false)
{
  const int tiles = d->Np / 64;
  const dim3 grid((tiles + 3) / 4), block(256);
  if (init) { hipLaunchKernelGGL((ramx_column_kernel<true, true, 256, true>), grid, block, 0, d->stream, a); return; }
  if (a.dbg_cand != NULL) { hipLaunchKernelGGL((ramx_column_kernel<false, true, 256, true>), grid, block, 0, d->stream, a); return; }
  if (a.go <= 0 && a.ge <= 0 && !d->force_chain)
    hipLaunchKernelGGL((ramx_column_kernel<false, false, 256, true>), grid, block, 0, d->stream, a);
  else
    hipLaunchKernelGGL((ramx_column_kernel<false, true, 256, true>), grid, block, 0, d->stream, a);
}

// does the vote of a column cross ranks?  (a communicator of ONE rank -- RAMX_COMM_SINGLE=1 at ramx_dev_comm_init -- counts with
// RAMX_FORCE_COLLECTIVE=1: the RCCL calls of the per-column route then run on a single GPU, tests/test_gpu_sharded.py)
static bool dev_is_multi(const ramx_dev *d)
{
  return (d->comm != NULL && (d->nranks > 1 || getenv("RAMX_FORCE_COLLECTIVE") != NULL)) || d->cb != NULL;
}

extern "C" int ramx_dev_is_multi(ramx_dev *d) { return d && dev_is_multi(d) ? 1 : 0; }

// ---- host-side collective on 4 x int64 in device memory (RCCL, or the test hook) ---------------
static int host_allreduce_shards(ramx_dev *d, long long *dptr)   // dptr: NSHARD x 4 int64, summed over ranks in place
{
  if (d->cb)
  {
    long long h[NSHARD * 4], h4[4] = { 0, 0, 0, 0 };
    HIPCHK(hipMemcpyAsync(h, dptr, sizeof(h), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    for (int i = 0; i < NSHARD * 4; i++) h4[i & 3] += h[i];
    d->cb(h4, d->cb_user);
    memset(h, 0, sizeof(h));
    memcpy(h, h4, sizeof(h4));
    HIPCHK(hipMemcpyAsync(dptr, h, sizeof(h), hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    return RAMX_OK;
  }
  ncclResult_t nr = ncclAllReduce(dptr, dptr, NSHARD * 4, ncclInt64, ncclSum, d->comm, d->stream);
  if (nr != ncclSuccess) { ramx_set_error("ncclAllReduce: %s", ncclGetErrorString(nr)); return RAMX_ERR_COMM; }
  return RAMX_OK;
}

// one small integer agreed over all ranks (max): used to agree on a fallback
static int host_allreduce_flag(ramx_dev *d, int *flag)
{
  if (d->cb)
  {
    long long h4[4] = { *flag ? 1 : 0, 0, 0, 0 };
    d->cb(h4, d->cb_user);
    *flag = h4[0] != 0;
    return RAMX_OK;
  }
  long long *tmp = d->d_sums + 3 * NSHARD * 4;   // spare 4 words behind the three vote slots
  long long h = *flag ? 1 : 0;
  HIPCHK(hipMemcpyAsync(tmp, &h, sizeof(h), hipMemcpyHostToDevice, d->stream));
  ncclResult_t nr = ncclAllReduce(tmp, tmp, 1, ncclInt64, ncclMax, d->comm, d->stream);
  if (nr != ncclSuccess) { ramx_set_error("ncclAllReduce: %s", ncclGetErrorString(nr)); return RAMX_ERR_COMM; }
  HIPCHK(hipMemcpyAsync(&h, tmp, sizeof(h), hipMemcpyDeviceToHost, d->stream));
  HIPCHK(hipStreamSynchronize(d->stream));
  *flag = h != 0;
  return RAMX_OK;
}

// ---- peer boxes ------------------------------------------------------------------------------------
extern "C" int ramx_dev_peer_export(ramx_dev *d, uint8_t handle[64])
{
  if (!d || !handle) { ramx_set_error("ramx_dev_peer_export: bad argument"); return RAMX_ERR_ARG; }
  HIPCHK(hipSetDevice(d->ordinal));
  if (!d->devbox)
  {
    hipError_t e = hipExtMallocWithFlags((void **)&d->devbox, sizeof(PeerBox), hipDeviceMallocFinegrained);
    if (e != hipSuccess) { d->devbox = NULL; ramx_set_error("fine-grained allocation for the peer box failed: %s", hipGetErrorString(e)); return RAMX_ERR_HIP; }
    HIPCHK(hipMemset(d->devbox, 0, sizeof(PeerBox)));
  }
  hipIpcMemHandle_t h;
  HIPCHK(hipIpcGetMemHandle(&h, d->devbox));
  static_assert(sizeof(hipIpcMemHandle_t) <= 64, "ipc handle size");
  memset(handle, 0, 64);
  memcpy(handle, &h, sizeof(h));
  return RAMX_OK;
}

__global__ void ramx_peer_token_kernel(PeerBox *const *peers, int rank, int nranks, unsigned long long token)
{
  if (threadIdx.x < nranks)
    __hip_atomic_store(&peers[threadIdx.x]->token[rank], token, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

extern "C" int ramx_dev_peer_import(ramx_dev *d, const uint8_t *handles, int rank, int nranks)
{
  if (!d || !handles || rank < 0 || rank >= nranks || nranks > RAMX_MAX_RANKS || !d->devbox)
  { ramx_set_error("ramx_dev_peer_import: bad argument (export first; at most %d ranks)", RAMX_MAX_RANKS); return RAMX_ERR_ARG; }
  HIPCHK(hipSetDevice(d->ordinal));
  d->peer_ready = 0;
  d->rank = rank; d->nranks = nranks;
  d->xbox = d->devbox; d->hostbox_host = NULL;
  for (int q = 0; q < RAMX_MAX_RANKS; q++)
    if (d->peer_ipc[q]) { (void)hipIpcCloseMemHandle(d->peer_ipc[q]); d->peer_ipc[q] = NULL; }
  for (int q = 0; q < nranks; q++)
  {
    if (q == rank) { d->peer[q] = d->xbox; continue; }
    hipIpcMemHandle_t h;
    memcpy(&h, handles + 64 * q, sizeof(h));
    void *ptr = NULL;
    hipError_t e = hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) { ramx_set_error("hipIpcOpenMemHandle(rank %d): %s", q, hipGetErrorString(e)); return RAMX_ERR_HIP; }
    d->peer[q] = (PeerBox *)ptr;
    d->peer_ipc[q] = ptr;
  }
  if (!d->d_peer) HIPCHK(hipMalloc((void **)&d->d_peer, RAMX_MAX_RANKS * sizeof(PeerBox *)));
  HIPCHK(hipMemcpy(d->d_peer, d->peer, nranks * sizeof(PeerBox *), hipMemcpyHostToDevice));
  return RAMX_OK;
}

/* Host-memory mailboxes: the same PeerBox protocol with every rank's box in ONE POSIX shared-memory segment that each
 * process registers with HIP (hipHostRegisterMapped).  Stores and polls cross PCIe instead of xGMI; no IPC handles,
 * no peer access between devices needed.  Used when the device-memory boxes cannot be mapped or fail their
 * self-test.  Every rank calls attach with the same name (ranks of one node); after a barrier rank 0 may unlink. */
extern "C" int ramx_dev_hostbox_attach(ramx_dev *d, const char *shm_name, int rank, int nranks)
{
  if (!d || !shm_name || rank < 0 || rank >= nranks || nranks > RAMX_MAX_RANKS)
  { ramx_set_error("ramx_dev_hostbox_attach: bad argument (at most %d ranks)", RAMX_MAX_RANKS); return RAMX_ERR_ARG; }
  HIPCHK(hipSetDevice(d->ordinal));
  d->peer_ready = 0;
  const size_t bytes = (((size_t)nranks * sizeof(PeerBox)) + 4095) & ~(size_t)4095;
  // rank 0 creates the segment exclusively (a leftover or pre-created segment of that name is an error, never silently
  // adopted) and sizes it; the other ranks open it -- the caller synchronises the ranks between rank 0's call and theirs
  int fd = rank == 0 ? shm_open(shm_name, O_CREAT | O_EXCL | O_RDWR, 0600) : shm_open(shm_name, O_RDWR, 0600);
  if (fd < 0) { ramx_set_error("shm_open(%s): %s", shm_name, strerror(errno)); return RAMX_ERR_COMM; }
  if (rank == 0 && ftruncate(fd, (off_t)bytes) != 0) { ramx_set_error("ftruncate(%s): %s", shm_name, strerror(errno)); close(fd); shm_unlink(shm_name); return RAMX_ERR_COMM; }
  void *map = mmap(NULL, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
  close(fd);
  if (map == MAP_FAILED) { ramx_set_error("mmap(%s): %s", shm_name, strerror(errno)); return RAMX_ERR_COMM; }
  hipError_t e = hipHostRegister(map, bytes, hipHostRegisterMapped | hipHostRegisterPortable);
  if (e != hipSuccess) { munmap(map, bytes); ramx_set_error("hipHostRegister(shared boxes): %s", hipGetErrorString(e)); return RAMX_ERR_HIP; }
  void *dptr = NULL;
  e = hipHostGetDevicePointer(&dptr, map, 0);
  if (e != hipSuccess) { (void)hipHostUnregister(map); munmap(map, bytes); ramx_set_error("hipHostGetDevicePointer: %s", hipGetErrorString(e)); return RAMX_ERR_HIP; }
  if (d->hostbox_map) { if (d->hostbox_registered) (void)hipHostUnregister(d->hostbox_map); munmap(d->hostbox_map, d->hostbox_bytes); }
  d->hostbox_map = map; d->hostbox_bytes = bytes; d->hostbox_registered = 1;
  d->hostbox_host = (PeerBox *)map + rank;
  memset(d->hostbox_host, 0, sizeof(PeerBox));          // my own box; the others clear theirs
  d->rank = rank; d->nranks = nranks;
  // the device-memory box (if any) is no longer the exchange target
  d->xbox = (PeerBox *)dptr + rank;
  for (int q = 0; q < nranks; q++) d->peer[q] = (PeerBox *)dptr + q;
  if (!d->d_peer) HIPCHK(hipMalloc((void **)&d->d_peer, RAMX_MAX_RANKS * sizeof(PeerBox *)));
  HIPCHK(hipMemcpy(d->d_peer, d->peer, nranks * sizeof(PeerBox *), hipMemcpyHostToDevice));
  return RAMX_OK;
}

extern "C" int ramx_hostbox_unlink(const char *shm_name)
{
  if (!shm_name) return RAMX_ERR_ARG;
  return shm_unlink(shm_name) == 0 ? RAMX_OK : RAMX_ERR_COMM;
}

/* self-test of the mapped boxes: write a token into every rank's box, then (after the caller has synchronised the
 * ranks) check that every rank's token arrived here.  phase 0 = write, phase 1 = check (returns 1 if all there). */
extern "C" int ramx_dev_peer_selftest(ramx_dev *d, int phase, unsigned long long token)
{
  if (!d || !d->d_peer) { ramx_set_error("ramx_dev_peer_selftest: import first"); return RAMX_ERR_ARG; }
  HIPCHK(hipSetDevice(d->ordinal));
  if (phase == 0)
  {
    hipLaunchKernelGGL(ramx_peer_token_kernel, dim3(1), dim3(64), 0, d->stream, (PeerBox *const *)d->d_peer, d->rank, d->nranks, token);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(d->stream));
    return RAMX_OK;
  }
  PeerBox h;
  for (int tries = 0; tries < 200; tries++)
  {
    if (d->hostbox_host) memcpy(&h, (const void *)d->hostbox_host, sizeof(h));
    else HIPCHK(hipMemcpy(&h, d->xbox, sizeof(h), hipMemcpyDeviceToHost));
    int ok = 1;
    for (int q = 0; q < d->nranks; q++) ok &= (h.token[q] == token);
    if (ok) return 1;
    struct timespec ts = { 0, 1000000 };
    nanosleep(&ts, NULL);
  }
  return 0;
}

extern "C" int ramx_dev_peer_enable(ramx_dev *d, int on)
{
  if (!d) return RAMX_ERR_ARG;
  d->peer_ready = (on && d->d_peer && d->xbox) ? 1 : 0;
  return RAMX_OK;
}

// The fast band packs (score << 4 | cell) keys: exact while every reachable |score| < 2^27 (a row-r cell is at most
// (r + W + 2) steps of at most max(|matrix|, |go| + |ge|) away from 0), and reads matrix entries as int8.  Scoring
// systems outside these bounds take the general (masked-path) band for every wave.
static int fast_pack_ok(const int (&tab)[RAMX_NCLASS][4], int go, int ge, int L, int W)
{
  long long mx = (long long)(go < 0 ? -go : go) + (long long)(ge < 0 ? -ge : ge);
  for (int c = 0; c < RAMX_NCLASS; c++)
    for (int k = 0; k < 4; k++)
    {
      const long long v = tab[c][k] < 0 ? -(long long)tab[c][k] : (long long)tab[c][k];
      if (v > mx) mx = v;
    }
  for (int c = 0; c < RAMX_NCLASS; c++)
    for (int k = 0; k < 4; k++)
      if (tab[c][k] < -128 || tab[c][k] > 127) return 0;       // the fast tables hold the candidates' scores as int8
  return ((long long)L + 2LL * W + 4) * mx < (1LL << 27) ? 1 : 0;
}

// P of the LEAN test of the register-resident bands (ramx_kernels_resident.h, prk_band_fast): max(0, largest matrix entry);
// -1 (never LEAN) with RAMX_NO_LEAN (A/B and tests) or when a gap penalty is positive
static int lean_p_of(const int (&tab)[RAMX_NCLASS][4], int go, int ge)
{
  if (getenv("RAMX_NO_LEAN") != NULL || go > 0 || ge > 0) return -1;
  int mx = 0;
  for (int c = 0; c < RAMX_NCLASS; c++)
    for (int k = 0; k < 4; k++) if (tab[c][k] > mx) mx = tab[c][k];
  return mx;
}

// ---- persistent path --------------------------------------------------------------------------
// Block shape of the persistent launch: at most ONE barrier participant per CU.
//   <= 4 tiles per CU (N <= 65,536): 256-thread blocks, one wave per SIMD, up to 256 blocks;
//   otherwise 512-thread blocks (two waves per SIMD), up to 256 blocks = 131,072 flanks.
template <int W, int BLOCK>
static int prk_capacity_blocks(int cus, int *out)
{
  static int cached = -1;              // (one device per process; the query is a runtime call per direction otherwise)
  if (cached >= 0) { *out = cached; return RAMX_OK; }
  int per_cu = 0;
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, ramx_persistent_kernel<W, BLOCK>, BLOCK, 0));
  if (per_cu > 1) per_cu = 1;          // one block per CU by design; never trust the API for more
  *out = per_cu * cus;
  cached = *out;
  return RAMX_OK;
}

static void test_delay_rank(const ramx_dev *d)
{
  // test hook: RAMX_TEST_DELAY_RANK="rank:milliseconds" holds that rank back just before its single launch, so that its
  // peers' kernels wait for its first words
  const char *e = getenv("RAMX_TEST_DELAY_RANK");
  int r = -1, ms = 0;
  if (e && sscanf(e, "%d:%d", &r, &ms) == 2 && r == d->rank && ms > 0) usleep((useconds_t)ms * 1000);
}

template <int W, int BLOCK>
static int prk_launch(ramx_dev *d, PArgs &pa, int blocks)
{
  // A PLAIN launch.  hipLaunchCooperativeKernel buys only the launch-time comparison of the grid with the occupancy query
  // (MI355X_MICROARCH.md, "coop-launch") -- prk_plan has made that comparison already (at most one workgroup per CU, never
  // more workgroups than CUs) -- and costs 15-19 us of host time per launch; the kernel has its own bounded barrier and
  // never calls grid.sync().  It also made every process that was profiled with rocprofv3 die with SIGSEGV inside exit():
  // the runtime's cooperative queue is torn down after the tool has finalised (tools/rocprof_exit_probe.sh isolates it:
  // streaming launches exit cleanly, one cooperative launch does not, with or without ramx_dev_destroy).
  // RAMX_COOP_LAUNCH=1 restores the cooperative launch.
  if (pa.nranks > 1) test_delay_rank(d);
  if (getenv("RAMX_COOP_LAUNCH") != NULL)
  {
    void *args[] = { (void *)&pa };
    HIPCHK(hipLaunchCooperativeKernel((const void *)ramx_persistent_kernel<W, BLOCK>, dim3(blocks), dim3(BLOCK), args, 0, d->stream));
    return RAMX_OK;
  }
  hipLaunchKernelGGL((ramx_persistent_kernel<W, BLOCK>), dim3(blocks), dim3(BLOCK), 0, d->stream, pa);
  HIPCHK(hipGetLastError());
  return RAMX_OK;
}

// block shape that keeps the whole flank set resident, or 0
template <int W>
static int prk_plan(int tiles, int cus, int *block, int *blocks)
{
  int cap = 0, rc;
  *block = 0; *blocks = 0;
  if ((rc = prk_capacity_blocks<W, 256>(cus, &cap)) != RAMX_OK) return rc;
  if ((tiles + 3) / 4 <= cap)
  {
    *block = 256; *blocks = (tiles + 3) / 4;
    return RAMX_OK;
  }
  if constexpr (W <= 40)     // wider bands have no two-waves-per-SIMD shape: the row needs more than 256 registers
  {
    if ((rc = prk_capacity_blocks<W, 512>(cus, &cap)) != RAMX_OK) return rc;
    if ((tiles + 7) / 8 <= cap) { *block = 512; *blocks = (tiles + 7) / 8; }
  }
  return RAMX_OK;
}

// which band widths have a register-resident instantiation
static bool prk_has_width(int W) { return W == 14 || W == 20 || W == 40 || W == 80; }
// ... and which have a one-workgroup-per-family instantiation (ramx_family_kernel: two waves per SIMD, 256 registers)
static bool fam_has_width(int W) { return W == 14 || W == 20 || W == 40; }

// A few words from device memory to the host at the end of a launch (control blocks, the error word, the consensus): written by
// a kernel into the session's pinned buffer.  hipMemcpy would do, but the first device-to-host copy of a process costs
// milliseconds of DMA set-up on this stack (6-10 ms of a 33 ms direction at N = 100,000), a store over the bus none.
// At most 64 KB (the tail of the staging buffer; the trim records use its head); the kernel moves whole 8-byte words (a source
// that is not a multiple of 8 bytes is over-read by up to 7 bytes, inside its allocation's granule).
static int d2h_small(ramx_dev *d, void *dst, const void *src, size_t bytes)
{
  const size_t off = d->cap_stage - ((size_t)64 << 10);
  if (bytes == 0) return RAMX_OK;
  if (bytes > ((size_t)64 << 10) || d->h_stage == NULL || d->cap_stage < ((size_t)128 << 10) || getenv("RAMX_DOWNLOAD_DMA") != NULL)
  {
    HIPCHK(hipStreamSynchronize(d->stream));
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return RAMX_OK;
  }
  int2 *stage = (int2 *)((char *)d->h_stage + off);
  const int n = (int)((bytes + 7) / 8);
  hipLaunchKernelGGL(ramx_to_host_kernel, dim3((n + 255) / 256), dim3(256), 0, d->stream, (const int2 *)src, stage, n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(d->stream));
  memcpy(dst, stage, bytes);
  return RAMX_OK;
}

#define RAMX_CP_MIN_K_OVER_PACKED 4      // the cell-parallel kernel goes first with at least this many lanes per flank
// ---- the route of a direction -------------------------------------------------------------------
// Decided once, at the top of ramx_dev_run_direction, and read by every later step.
struct DirRoute
{
  bool tracing, multi;
  bool mailbox_ok;                  // multi-rank: the vote can cross the devices through the mailboxes (true on one GPU)
  bool int32_can; int block, blocks;                          // the int32 persistent rows can run here, and their launch shape
  bool pk; int pk_r0, spread, rebase, pk_block, pk_blocks;    // the packed rows take the direction from row pk_r0 on
  bool cp_try;                      // the cell-parallel attempt is made (multi-rank: its agreement is held even with k == 0 here)
  int k, th, nb, vwf;               // its plan: lanes per flank (0: not on this rank), threads, workgroups, vote wave
  bool pack_now;                    // the kernel that goes first reads the whole window: pack the rest before anything else
};

// The switches that move a direction from one kernel to another.  Read once per direction and never kept: the tests flip them
// between two directions of one device.  (RAMX_NO_PK, RAMX_NO_CP and the value of RAMX_CP_K are read by the plans themselves.)
struct RouteEnv { bool no_persistent, no_peer, no_pk_multi, no_cp_device, cp_k; int cp_maxn; };      // cp_maxn: RAMX_CP_DEVICE_MAXN, most flanks of a device-wide launch
static RouteEnv route_env(void)
{
  const char *mx = getenv("RAMX_CP_DEVICE_MAXN");
  return { getenv("RAMX_NO_PERSISTENT") != NULL, getenv("RAMX_NO_PEER") != NULL, getenv("RAMX_NO_PK_MULTI") != NULL,
           getenv("RAMX_NO_CP_DEVICE") != NULL, getenv("RAMX_CP_K") != NULL, mx ? atoi(mx) : INT_MAX };
}

// Which kernels are admissible for this scoring system, band width, flank set, rank layout and these switches -- everything
// that can be said without asking the device (no HIP call, no session): int32_can / pk still await their occupancy answers,
// the cell-parallel plan the rule of RAMX_CP_MIN_K_OVER_PACKED (route_settle).
static DirRoute route_gates(const RouteEnv &e, int W, int go, int ge, const int (&tab)[RAMX_NCLASS][4], int L, int Nx, int pk_r0,
                            bool cp_flanks_ok, bool tracing, bool multi, bool peer_ready, int nranks, bool force_chain, int cus)
{
  DirRoute rt = {};
  rt.tracing = tracing; rt.multi = multi;
  rt.mailbox_ok = !multi || (peer_ready && nranks >= 2 && L < 65536 && !e.no_peer);
  // any kernel that runs the whole direction in one launch (a trace wants a launch per row)
  const bool single_launch = !tracing && !e.no_persistent && !force_chain && L > 0;
  rt.int32_can = single_launch && rt.mailbox_ok && go <= 0 && ge <= 0 && go + ge >= -32768 && prk_has_width(W);
  // The packed rows (ramx_kernels_packed.h): a scoring system whose rows fit int16 relative to a per-flank base.  (Multi-rank:
  // the packed kernel speaks the same mailbox protocol as the int32 one, ramx_kernels_vote.h; which of the two a rank runs, from
  // which row on and in how many pieces is that rank's own business.)
  rt.pk_r0 = single_launch ? pk_r0 : -1;
  rt.pk = rt.pk_r0 >= 0 && rt.pk_r0 < L && rt.mailbox_ok && !(multi && e.no_pk_multi) && ramx_pk_plan(W, go, ge, tab, &rt.spread, &rt.rebase) != 0;
  // The cell-parallel kernel in device-wide mode: at most one workgroup per CU.  Multi-rank: every rank takes this route or none,
  // so a rank with no flank of its own plans for one.
  rt.cp_try = single_launch && rt.mailbox_ok && !e.no_cp_device && (multi || Nx > 0);
  if (rt.cp_try && cp_flanks_ok && Nx <= e.cp_maxn && ramx_cp_max_family(W, go, ge, tab, L) > 0)
    ramx_cp_device_plan(W, Nx > 0 ? Nx : 1, cus, 0, &rt.k, &rt.th, &rt.nb, &rt.vwf);
  return rt;
}

// The rules that need the occupancy answers (rt.block / rt.pk_block of an admissible kernel; 0: its flank set is not co-resident).
static void route_settle(DirRoute &rt, const RouteEnv &e, int Nx)
{
  rt.int32_can = rt.int32_can && rt.block != 0;          // not co-resident: keep the streaming kernel
  // resident, and -- where flanks have low out-of-bounds cells in the first rows -- the int32 kernel for those rows
  rt.pk = rt.pk && rt.pk_block != 0 && (rt.pk_r0 == 0 || rt.int32_can);
  // Two lanes per flank (33,000-65,536 flanks at W = 40) against the packed-row kernel with one wave per SIMD, whole bench launch
  // at 50,000 / 65,000 flanks: 5.44 / 5.55 against 4.76 / 4.66 us per column (aligned phase alike, the capped tail is the packed
  // kernel's; profiles/r04_route_ab.log) -- where the packed rows can run they take those sets.
  if (rt.k > 0 && rt.k < RAMX_CP_MIN_K_OVER_PACKED && !e.cp_k && rt.pk) rt.k = 0;
  // Every route but the packed-row one reads base words of the whole window: it packs what begin_direction left (pack_rest).
  // Multi-rank the route is agreed later; whichever kernel then needs the whole window packs the rest first.
  rt.pack_now = rt.tracing || Nx <= 0 || !rt.pk || (!rt.multi && rt.k > 0);
}

// The route of the direction begun on d: the gates, then the occupancy questions of the admissible lane-per-flank kernels (each
// asked once per process), and the rules that need their answers.
static int direction_route(ramx_dev *d, const KArgs &a, int L, DirRoute *out)
{
  const RouteEnv e = route_env();
  DirRoute rt = route_gates(e, a.W, a.go, a.ge, a.tab, L, d->Nx, d->pk_r0, d->cp_flanks_ok != 0, d->trace_cb != NULL || d->verbose_cb != NULL,
                            dev_is_multi(d), d->peer_ready != 0, d->nranks, d->force_chain != 0, d->cus);
  const int W = a.W, tiles = d->Np / 64;
  if (rt.int32_can)
  {
    const int rc = (W == 14) ? prk_plan<14>(tiles, d->cus, &rt.block, &rt.blocks) : (W == 20) ? prk_plan<20>(tiles, d->cus, &rt.block, &rt.blocks) :
                   (W == 40) ? prk_plan<40>(tiles, d->cus, &rt.block, &rt.blocks) : prk_plan<80>(tiles, d->cus, &rt.block, &rt.blocks);
    if (rc != RAMX_OK) return rc;
  }
  if (rt.pk && ramx_pk_shape(W, tiles, &rt.pk_block, &rt.pk_blocks) != RAMX_OK) { ramx_set_error("packed-row kernel: occupancy query failed"); return RAMX_ERR_HIP; }
  route_settle(rt, e, d->Nx);
  *out = rt;
  return RAMX_OK;
}

// ---- multi-rank: this rank's mailbox before a launch ----------------------------------------------
// My box is cleared BEFORE the agreement that precedes the launch, which no remote launch can get past without my taking part:
// nobody writes a word of this run into it too early, and nothing of the last run survives.  Complete, not just enqueued: the
// agreement may be a host-only collective, and a peer that gets past it launches and writes into this box at once.
static int mailbox_clear(ramx_dev *d)
{
  if (!d->hostbox_host) HIPCHK(hipMemsetAsync(d->xbox, 0, sizeof(PeerBox), d->stream));
  HIPCHK(hipStreamSynchronize(d->stream));
  if (d->hostbox_host) { memset((void *)d->hostbox_host, 0, sizeof(PeerBox)); __sync_synchronize(); }
  return RAMX_OK;
}

// host-memory boxes: the zeroed device copy of my box (kept current by block 0, polled by the others); NULL with device boxes
static int mailbox_mirror(ramx_dev *d, PeerBox **mirror)
{
  *mirror = NULL;
  if (!d->hostbox_host) return RAMX_OK;
  if (!d->hostbox_mirror) HIPCHK(hipMalloc((void **)&d->hostbox_mirror, sizeof(PeerBox)));
  HIPCHK(hipMemsetAsync(d->hostbox_mirror, 0, sizeof(PeerBox), d->stream));
  *mirror = d->hostbox_mirror;
  return RAMX_OK;
}

// both control blocks (a direction that ran in pieces leaves its last one in either) and the error word (a refused entry check,
// a bounded spin that gave up) after a single-launch kernel
static int read_launch_state(ramx_dev *d, RamxCtl c[2], unsigned *errw)
{
  unsigned long long ew = 0;
  HIPCHK(hipStreamSynchronize(d->stream));
  int rc = d2h_small(d, c, d->d_ctl, 2 * sizeof(RamxCtl));
  if (rc == RAMX_OK) rc = d2h_small(d, &ew, d->d_err, sizeof(ew));
  *errw = (unsigned)ew;
  return rc;
}

#ifdef RAMX_PRK_TIMING
// -DRAMX_PRK_TIMING builds: phase breakdown per column of the launch that has just run, in ns (wall_clock64 ticks are 10 ns)
static int prk_timing_report(ramx_dev *d, unsigned long long *dbgbuf, size_t nw, bool pk, int block, int blocks, int L, int pk_r0)
{
  HIPCHK(hipStreamSynchronize(d->stream));
  unsigned long long *h = (unsigned long long *)malloc(nw * 8 * sizeof(unsigned long long));
  HIPCHK(hipMemcpy(h, dbgbuf, nw * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  static const char *nm[6] = { "wait vote", "block barrier 1", "band", pk ? "early arrival" : "reduce+barrier 2", pk ? "late arrival" : "issue atomics", "loop top" };
  const int wpb = block / 64;
  fprintf(stderr, "PRK_TIMING %s blocks %d x %d threads, L %d, first row %d (ns per column)\n", pk ? "packed rows" : "int32 rows", blocks, block, L, pk ? pk_r0 : 0);
  for (int k = 0; k < 6; k++)
  {
    double s0 = 0, sO = 0, mx = 0, mn = 1e30;
    for (size_t i = 0; i < nw; i++)
    {
      const double v = 10.0 * (double)h[i * 8 + k] / L;
      if ((int)(i % wpb) == 0) s0 += v; else sO += v;
      if (v > mx) mx = v;
      if (v < mn) mn = v;
    }
    fprintf(stderr, "PRK_TIMING %-18s wave0 avg %8.1f  other waves avg %8.1f  min %8.1f  max %8.1f\n", nm[k], s0 / blocks,
            wpb > 1 ? sO / (double)(nw - blocks) : 0.0, mn, mx);
  }
  fprintf(stderr, "PRK_TIMING band by wave index:");
  for (int wv = 0; wv < wpb; wv++)
  {
    double sw = 0;
    for (int b = 0; b < blocks - 1; b++) sw += 10.0 * (double)h[((size_t)b * wpb + wv) * 8 + 2] / L;
    fprintf(stderr, " w%d %.0f", wv, sw / (blocks > 1 ? blocks - 1 : 1));
  }
  fprintf(stderr, "\n");
  {
    // the workgroup everybody waits for: the one whose vote wave waits least for the vote
    int gb = 0;
    for (int b = 1; b < blocks; b++) if (h[(size_t)b * wpb * 8 + 0] < h[(size_t)gb * wpb * 8 + 0]) gb = b;
    fprintf(stderr, "PRK_TIMING workgroup %d (shortest vote wait), per wave: wait vote | barrier | band | early | late | top\n", gb);
    for (int wv = 0; wv < wpb; wv++)
    {
      const unsigned long long *q = h + ((size_t)gb * wpb + wv) * 8;
      fprintf(stderr, "PRK_TIMING   w%d %7.0f %7.0f %7.0f %7.0f %7.0f %7.0f   rows full %llu lean %llu\n", wv, 10.0 * q[0] / L, 10.0 * q[1] / L, 10.0 * q[2] / L,
              10.0 * q[3] / L, 10.0 * q[4] / L, 10.0 * q[5] / L, q[6], q[7]);
    }
  }
  {
    // second half of the run: waves that were kept from the LEAN band, and by how many lanes
    const double half = L - L / 2;
    size_t never = 0, always = 0, wg_any = 0;
    double lanes = 0, cols = 0;
    int hist[6] = { 0, 0, 0, 0, 0, 0 };       // waves by average number of such lanes in their non-lean columns: <=1, <=2, <=4, <=8, <=16, more
    for (int b = 0; b < blocks; b++)
    {
      bool any = false;
      for (int wv = 0; wv < wpb; wv++)
      {
        const size_t i = (size_t)b * wpb + wv;
        const double c = (double)h[i * 8 + 6], l = (double)h[i * 8 + 7];
        if (c == 0) { never++; continue; }
        any = any || c > 0.5 * half;
        if (c > 0.9 * half) always++;
        lanes += l; cols += c;
        const double avg = l / c;
        hist[avg <= 1 ? 0 : avg <= 2 ? 1 : avg <= 4 ? 2 : avg <= 8 ? 3 : avg <= 16 ? 4 : 5]++;
      }
      if (any) wg_any++;
    }
    fprintf(stderr, "PRK_LEANSTAT second half (%.0f columns): %zu of %zu waves always LEAN, %zu non-LEAN in > 90 %% of the columns; workgroups with a wave "
            "non-LEAN in > 50 %%: %zu of %d; lanes per non-LEAN wave-column %.2f; waves by that average <=1: %d <=2: %d <=4: %d <=8: %d <=16: %d more: %d\n",
            half, never, nw, always, wg_any, blocks, cols > 0 ? lanes / cols : 0.0, hist[0], hist[1], hist[2], hist[3], hist[4], hist[5]);
  }
  free(h);
  (void)hipFree(dbgbuf);
  return RAMX_OK;
}

// ... of the register-resident family kernel of a batch
static int fam_timing_report(const unsigned long long *dbg)
{
  unsigned long long h[64];
  HIPCHK(hipMemcpy(h, dbg, sizeof(h), hipMemcpyDeviceToHost));
  static const char *nm[6] = { "vote + stop rule", "winner table+barrier", "band + contrib", "wave reduce", "end barrier", "loop top" };
  const double cols = h[6] ? (double)h[6] : 1.0;
  fprintf(stderr, "FAM_TIMING family 0 (block 0), %.0f columns, ns per column per wave:\n", cols);
  for (int k = 0; k < 6; k++)
    fprintf(stderr, "FAM_TIMING %-22s w0 %7.1f  w1 %7.1f  w2 %7.1f  w3 %7.1f\n", nm[k], 10.0 * h[k] / cols, 10.0 * h[8 + k] / cols,
            10.0 * h[16 + k] / cols, 10.0 * h[24 + k] / cols);
  return RAMX_OK;
}
#endif

#ifdef RAMX_CP_TIMING
// -DRAMX_CP_TIMING builds: the cell-parallel launch of a batch whose block 0 wrote dbg (cp_timing_report: the whole-set direction's)
static int cp_family_timing_report(const unsigned long long *dbg)
{
  unsigned long long h[16 * 16 + 8];
  HIPCHK(hipMemcpy(h, dbg, sizeof(h), hipMemcpyDeviceToHost));
  static const char *nm[12] = { "vote read + stop rule", "(after speculative band)", "row update", "reductions", "records/slide/window",
                                "sum+atomics+barrier", "-", "loop top", "wait: drain", "wait: samples + polling", "wait: fold",
                                "wait: LDS + barrier" };
  const double cols = h[16 * 16] ? (double)h[16 * 16] : 1.0;
  fprintf(stderr, "CP_TIMING block 0, %.0f columns, shader clocks per column (waves 0, 1, last two):\n", cols);
  int nw = 0;
  for (int w = 0; w < 16; w++) if (h[w * 16 + 0]) nw = w + 1;
  for (int k = 0; k < 12; k++)
    if (k == 6) fprintf(stderr, "CP_TIMING mispredicted columns: %.0f of %.0f\n", (double)h[6], cols);
    else fprintf(stderr, "CP_TIMING %-24s w0 %7.1f  w1 %7.1f  w%d %7.1f  w%d %7.1f\n", nm[k], h[k] / cols, h[16 + k] / cols,
                        nw > 1 ? nw - 2 : 0, h[(nw > 1 ? nw - 2 : 0) * 16 + k] / cols, nw > 0 ? nw - 1 : 0, h[(nw > 0 ? nw - 1 : 0) * 16 + k] / cols);
  return RAMX_OK;
}
#endif

// The lane-per-flank persistent kernels on the route rt: the int32 rows, the packed rows, or the packed rows behind first rows
// on the int32 kernel.  Multi-rank only the agreement here can still turn the int32 rows off.
static int prk_run(ramx_dev *d, const KArgs &a, int L, DirRoute &rt, bool *used)
{
  *used = false;
  const int W = a.W;
  const bool multi = rt.multi;
  int rc;
  if (multi)
  {
    // every rank must take the same path: agree (max over ranks of "cannot")
    int cannot = rt.int32_can ? 0 : 1;
    if ((rc = host_allreduce_flag(d, &cannot)) != RAMX_OK) return rc;
    rt.int32_can = !cannot;
  }
  const bool pk = rt.pk;
  const int pk_r0 = rt.pk_r0, pk_block = rt.pk_block, pk_blocks = rt.pk_blocks;
  int block = rt.block, blocks = rt.blocks;
  if (!rt.int32_can && (multi || !pk)) return RAMX_OK;
  *used = true;        // agreed (multi-rank: by all ranks): from here on the caller handles a local failure collectively
  PArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.S = d->d_state[0]; pa.bases = d->d_bases; pa.bounds = d->d_bounds; pa.trim = d->d_trim;
  pa.sums0 = d->d_sums; pa.vote = d->d_vote; pa.ctl_out = d->d_ctl; pa.cons_out = d->d_cons; pa.err = d->d_err;
  pa.Np = d->Np; pa.Nx = d->Nx; pa.r0 = 0; pa.L = L; pa.go = a.go; pa.ge = a.ge; pa.cap = a.cap; pa.minimp = a.minimp;
  pa.when_to_stop = a.when_to_stop; pa.nblocks = blocks;
  pa.nranks = 1; pa.rank = 0; pa.peers = NULL; pa.box = NULL;
  if (multi)
  {
    pa.nranks = d->nranks; pa.rank = d->rank; pa.peers = (PeerBox *const *)d->d_peer; pa.box = d->xbox;
    // Rank-local steps first, WITHOUT leaving on an error: the collective below is executed by every rank in any case
    // (a rank that skipped it would pair its next collective with this one on the other ranks).
    int lrc = mailbox_mirror(d, &pa.mirror);
    if (lrc == RAMX_OK) lrc = mailbox_clear(d);
    if ((rc = host_allreduce_shards(d, d->d_sums)) != RAMX_OK) return rc;     // vote of row 0 (from K(-1)) over ranks
    if (lrc != RAMX_OK) return lrc;
    // test hook: RAMX_TEST_FAIL_PRK_RANK=<rank> makes that rank fail where a launch error would
    const char *tf = getenv("RAMX_TEST_FAIL_PRK_RANK");
    if (tf && atoi(tf) == d->rank) { ramx_set_error("test hook: forced failure of the persistent launch on rank %d", d->rank); return RAMX_ERR_HIP; }
  }
  memcpy(pa.tab, a.tab, sizeof(pa.tab));
  pa.pack_ok = getenv("RAMX_NO_FASTPACK") ? 0 : fast_pack_ok(pa.tab, a.go, a.ge, L, W);
  if (pa.pack_ok && getenv("RAMX_NO_MASKHI") == NULL) pa.pack_ok = 2;      // 2: the far-end-masked fast band may be used too
  pa.lean_p = lean_p_of(pa.tab, a.go, a.ge);
  // a leader costs its wave ~150 instructions in prk_leader_rows, the full band 640 more than LEAN; RAMX_LEADER_MAX=0 switches
  // the leader path off (A/B and tests), larger values exercise it on waves with many leaders
  { const char *lm = getenv("RAMX_LEADER_MAX"); pa.leader_max = lm ? atoi(lm) : 3; if (pa.leader_max < 0) pa.leader_max = 0; if (pa.leader_max > 64) pa.leader_max = 64; }
  // ---- the packed-row kernel (ramx_kernels_packed.h) takes the direction from row r0 = d->pk_r0 on when the scoring system's
  // rows fit int16 relative to a per-flank base; the rows before (flanks whose cores are shorter than the band have
  // out-of-bounds cells at the LOW end of the band there) stay on this kernel, which hands over the sums of row r0 --------
  PKArgs ka;
  memset(&ka, 0, sizeof(ka));
  ka.spread = rt.spread; ka.rebase = rt.rebase;
  if (!pk && (rc = pack_rest(d)) != RAMX_OK) return rc;        // the int32 kernel reads the whole window
  HIPCHK(hipMemsetAsync(d->d_vote, 0, PRK_NSETS * NSHARD * sizeof(PShard), d->stream));
  HIPCHK(hipMemsetAsync(d->d_err, 0, 64, d->stream));
  long long *sums_next = d->d_sums + (size_t)NSHARD * 4;        // slot 1: zeroed by K(-1)
  const bool head = !pk || pk_r0 > 0;                            // this kernel runs (all of the direction, or its first rows)
  if (pk && pk_r0 > 0) { pa.L = pk_r0; pa.sums_next = sums_next; }
#ifdef RAMX_PRK_TIMING
  const size_t nw = pk ? (size_t)pk_blocks * (pk_block / 64) : (size_t)blocks * (block / 64);
  unsigned long long *dbgbuf = NULL;
  HIPCHK(hipMalloc((void **)&dbgbuf, nw * 8 * sizeof(unsigned long long)));
  HIPCHK(hipMemset(dbgbuf, 0, nw * 8 * sizeof(unsigned long long)));
  if (pk) ka.dbg = dbgbuf; else pa.dbg = dbgbuf;                 // timing build: with a packed launch, its phases are the ones printed
#endif
  rc = RAMX_OK;
  const bool tmarks = getenv("RAMX_TIMING") != NULL;
  const double tm0 = now_ms();
  rt_mark("persistent route, memsets");
  if (head)
  {
    if (block == 256)
      rc = (W == 14) ? prk_launch<14, 256>(d, pa, blocks) : (W == 20) ? prk_launch<20, 256>(d, pa, blocks) :
           (W == 40) ? prk_launch<40, 256>(d, pa, blocks) : prk_launch<80, 256>(d, pa, blocks);
    else
      rc = (W == 14) ? prk_launch<14, 512>(d, pa, blocks) : (W == 20) ? prk_launch<20, 512>(d, pa, blocks) : prk_launch<40, 512>(d, pa, blocks);
  }
  rt_mark("first rows launched (int32 kernel)");
  if (rc == RAMX_OK && pk)
  {
    ka.S = d->d_state[0]; ka.bases = d->d_bases; ka.bounds = d->d_bounds; ka.trim = d->d_trim;
    ka.vote = d->d_vote; ka.cons_out = d->d_cons; ka.err = d->d_err;
    ka.peers = pa.peers; ka.box = pa.box; ka.mirror = pa.mirror; ka.rank = pa.rank; ka.nranks = pa.nranks;
    ka.xblock = 0;
    if (ka.nranks > 1 && getenv("RAMX_NO_PK_EXCHANGER") == NULL)
    {
      // a CU to spare: the device's exchange duties get a workgroup of their own (ramx_kernels_packed.h)
      int cap = 0;
      if (ramx_pk_capacity(W, pk_block, &cap) == RAMX_OK && pk_blocks + 1 <= cap) ka.xblock = pk_blocks;
    }
    ka.Np = d->Np; ka.Nx = d->Nx; ka.L = L; ka.go = a.go; ka.ge = a.ge; ka.cap = a.cap; ka.minimp = a.minimp;
    ka.when_to_stop = a.when_to_stop; ka.nblocks = pk_blocks;
    memcpy(ka.tab, a.tab, sizeof(ka.tab));
    ka.lean_p = pa.lean_p; ka.leader_max = pa.leader_max;
    ka.spec_on = getenv("RAMX_NO_PK_SPEC") == NULL ? 1 : 0;
    { const char *we = getenv("RAMX_TEST_PK_WRONG_EVERY"); ka.test_wrong_every = we ? atoi(we) : 0; }
    // distance between two checkpoints of a speculating workgroup: 1, 2, 4 or 8 columns; anything else: the kernel adapts it
    { const char *ck = getenv("RAMX_PK_CKPT"); const int v = ck ? atoi(ck) : 0; ka.ckpt = (v == 1 || v == 2 || v == 4 || v == 8) ? v : 0; }
    // test hook: a span smaller than the scoring system's makes the kernel's own checks (rows at entry, every 64th row) refuse
    { const char *ts = getenv("RAMX_TEST_PK_SPREAD"); if (ts) ka.spread = atoi(ts); }
    ka.spread_rows = ka.spread;
    { const char *ts = getenv("RAMX_TEST_PK_SPREAD_ROWS"); if (ts) ka.spread_rows = atoi(ts); }
    d->last_packed_r0 = pk_r0;
    // The direction runs in pieces of RAMX_PK_SEGMENT columns (one launch each: rows written back, sums of the next row handed
    // over as plain words, control block passed on), so that only the base words a run really reads are ever packed: the
    // next piece's words are packed on a second stream while this piece runs.
    const int seg = pk_segment_columns(L, a.when_to_stop);
    const int NWw = (2 * W + 1 + 8) / 8 + 2;
    long long *sbuf[2] = { d->d_sums + (size_t)NSHARD * 4, d->d_sums + (size_t)2 * NSHARD * 4 };     // slots 1 and 2
    const long long *sums_in = pk_r0 > 0 ? sbuf[0] : d->d_sums;
    int nextbuf = pk_r0 > 0 ? 1 : 0;
    int ctl_i = 0;                           // the control block of the launch before sits in d_ctl[ctl_i] (pk_r0 == 0: not read)
    auto words_for = [&](int r_end) { int wn = ((r_end + 7) >> 3) + NWw + 2; return wn < d->KW ? wn : d->KW; };
    if (ka.nranks > 1 && !head) test_delay_rank(d);
    for (int r = pk_r0, s_i = 0; r < L && rc == RAMX_OK; s_i++)
    {
      const int r1 = seg > 0 ? std::min(L, (r / seg + 1) * seg) : L;
      // this piece's words: normally packed already (begin_direction, or beside the piece before)
      if ((rc = pack_settle(d)) != RAMX_OK) return rc;
      if (d->packed_kw < words_for(r1))
      {
        if ((rc = launch_pack(d, d->Nx, d->Np, W, d->packed_kw, words_for(r1), d->stream)) != RAMX_OK) break;
        d->packed_kw = words_for(r1);
      }
      HIPCHK(hipMemsetAsync(d->d_vote, 0, PRK_NSETS * NSHARD * sizeof(PShard), d->stream));
      ka.r0 = r; ka.Lseg = r1; ka.sums_in = sums_in;
      ka.sums_next = r1 < L ? sbuf[nextbuf] : NULL;
      if (r1 < L) HIPCHK(hipMemsetAsync(sbuf[nextbuf], 0, (size_t)NSHARD * 4 * sizeof(long long), d->stream));
      ka.ctl_in = d->d_ctl + ctl_i; ka.ctl_out = d->d_ctl + (ctl_i ^ 1);
      if (r == 0) ka.ctl_out = d->d_ctl;     // (first launch of the direction: d_ctl[1] still holds K(-1)'s block, nothing is read)
      const double tm1 = now_ms();
      rc = ramx_pk_launch(d->stream, W, pk_block, pk_blocks, ka);
      if (rc != RAMX_OK) { ramx_set_error("packed-row kernel: launch failed (W %d, %d workgroups of %d threads)", W, pk_blocks, pk_block); break; }
      if (tmarks) fprintf(stderr, "RAMX_TIMING       run: piece %d (rows %d..%d, %d x %d threads) launched %.3f ms after the first launch (launch call %.3f ms)\n", s_i, r, r1, pk_blocks, pk_block, now_ms() - tm0, now_ms() - tm1);
      const int out_i = (r == 0) ? 0 : (ctl_i ^ 1);
      if (r1 >= L) break;
      // the next piece's words, beside this launch
      const int r2 = std::min(L, (r1 / seg + 1) * seg);
      if (d->packed_kw < words_for(r2))
      {
        if ((rc = launch_pack(d, d->Nx, d->Np, W, d->packed_kw, words_for(r2), d->pack_stream)) != RAMX_OK) break;
        HIPCHK(hipEventRecord(d->pack_done, d->pack_stream));
        d->pack_busy = 1;
        d->packed_kw = words_for(r2);
      }
      // did this piece end the direction?  (one synchronisation per piece: 2,048 columns)
      RamxCtl c2[2];
      unsigned errw = 0;
      HIPCHK(hipStreamSynchronize(d->stream));
      if (tmarks) fprintf(stderr, "RAMX_TIMING       run: piece %d complete %.3f ms after the first launch\n", s_i, now_ms() - tm0);
      if ((rc = read_launch_state(d, c2, &errw)) != RAMX_OK) break;
      rt_mark("piece: control block and error word read");
      const RamxCtl &hc = c2[out_i];
      if (hc.stopped || hc.pad != 0 || errw != 0 || hc.rows_done < r1) break;
      sums_in = sbuf[nextbuf]; nextbuf ^= 1; ctl_i = out_i; r = r1;
    }
    // (the caller reads both control blocks and takes the one with more rows)
    if (pk) { block = pk_block; blocks = pk_blocks; }
  }
  else d->last_packed_r0 = -1;
#ifdef RAMX_PRK_TIMING
  if (rc == RAMX_OK) rc = prk_timing_report(d, dbgbuf, nw, pk, block, blocks, L, pk_r0);
#endif
  return rc;
}

// test hooks of the vote-wave mode of the cell-parallel kernel (ramx_kernels_cp.h): RAMX_TEST_CP_WRONG_EVERY=n computes every
// n-th row on a deliberately wrong guess, RAMX_TEST_CP_VOTE_DELAY=units holds the vote wave back so that the band waves have
// finished their row on the guess when the decision arrives
static void cp_test_hooks(CPArgs &ca)
{
  const char *we = getenv("RAMX_TEST_CP_WRONG_EVERY"), *vd = getenv("RAMX_TEST_CP_VOTE_DELAY");
  ca.test_wrong_every = we ? atoi(we) : 0;
  ca.test_vote_delay = vd ? atoi(vd) : 0;
  ca.lean_p = lean_p_of(ca.tab, ca.go, ca.ge);
}

// What every cell-parallel launch is told -- a batch's classes, its device-wide families, the whole-set direction: windows,
// outputs and scoring system.  The caller adds its descriptors, its vote words and what else is its own.
static CPArgs cp_args(const ramx_dev *d, RamxCtl *ctl, int Np, int KW, const ramx_params &p, const int (&tab)[RAMX_NCLASS][4])
{
  CPArgs ca;
  memset(&ca, 0, sizeof(ca));
  ca.bases = d->d_bases; ca.bounds = d->d_bounds; ca.trim = d->d_trim; ca.ctl_out = ctl; ca.cons_out = d->d_cons;
  ca.Np = Np; ca.KW = KW; ca.L = p.L; ca.go = p.gapopen; ca.ge = p.gapextn; ca.cap = p.cappenalty; ca.minimp = p.minimprovement;
  ca.when_to_stop = p.when_to_stop;
  memcpy(ca.tab, tab, sizeof(ca.tab));
  cp_test_hooks(ca);
  return ca;
}

// ---- batch mode: the route of every family, decided once (family_plan) and read by every later step ----------------------
struct FamilyPlan
{
  bool resident, chain;      // the lane-per-flank families: register-resident kernel, else the streaming one (chain: full candidate recurrence)
  int n_cp, n_dev;           // families in the cell-parallel classes / in the device-wide launch
  std::vector<int> grp;      // per family: -1 device-wide, 0 .. RAMX_CP_NCLASS-1 cell-parallel class, above: lane-per-flank shape
  int cls_first[RAMX_NGROUP + 1], cls_count[RAMX_NGROUP], cp_k[RAMX_CP_NCLASS], cp_threads[RAMX_CP_NCLASS];
  std::vector<FamDesc> fam;  // the families of the groups >= 0, in group order (cls_first / cls_count)
  int dev_k, dev_threads, dev_vw;       // the device-wide launch: lanes per flank, threads, vote wave -- what its first family plans
  std::vector<CpDevDesc> dev;           // ... one descriptor per workgroup
  std::vector<int2> rounds;             // ... (first descriptor, workgroups): at most one workgroup per CU, one round after the other
  bool launched[RAMX_NGROUP];           // the group streams something is launched on (families_join)
};

// Which kernel takes which family -- no HIP call, no session.  Groups 0 .. RAMX_CP_NCLASS-1: the cell-parallel kernel (K lanes
// per flank, ramx_cp.hip) for families it can take: supported band width and scoring system, small enough for one workgroup at
// K lanes per flank, a flank set that fits (cp_flanks_fit).  Group -1: families above one such workgroup run on several, the
// family's vote through its own ticket words -- the device-wide mode of the same kernel, all of them in rounds of at most
// `cus` workgroups (every workgroup of a launch must be resident).  Groups RAMX_CP_NCLASS ..: one lane per flank, by workgroup
// shape (64, 128, 256, 512 threads = 1, 2, 4, 8 tiles).
static FamilyPlan family_plan(const RouteEnv &e, int W, int go, int ge, const int (&tab)[RAMX_NCLASS][4], int L, int cus, bool force_chain,
                              bool allow_dev, const ramx_flank *flanks, const int32_t *fam_first, const int32_t *fam_count, int n_families)
{
  FamilyPlan pl = {};
  pl.resident = fam_has_width(W) && go <= 0 && ge <= 0 && go + ge >= -32768 && !force_chain && !e.no_persistent;
  pl.chain = go > 0 || ge > 0 || force_chain;
  const int cp_max = force_chain ? 0 : ramx_cp_max_family(W, go, ge, tab, L);
  const bool dev_route = allow_dev && cp_max > 0 && cus > 0 && !e.no_cp_device && !e.no_persistent;
  // the device-wide plan of a set of nx flanks, asked once per size
  struct Shape { int k, th, nb, vw; bool known; };
  const int maxn = n_families > 0 ? *std::max_element(fam_count, fam_count + n_families) : 0;
  std::vector<Shape> memo[2] = { std::vector<Shape>((size_t)maxn + 1), std::vector<Shape>((size_t)maxn + 1) };
  auto shape_of = [&](int nx, int wide) -> const Shape &
  {
    Shape &s = memo[wide][nx];
    if (!s.known) { ramx_cp_device_plan(W, nx, cus, wide, &s.k, &s.th, &s.nb, &s.vw); s.known = true; }
    return s;
  };
  // small workgroups (four band waves, lowest latency) when all the multi-workgroup families then fit the CUs together
  int dev_wide = 0;
  if (dev_route)
  {
    long long need = 0;
    for (int f = 0; f < n_families; f++)
      if (fam_count[f] > cp_max && shape_of(fam_count[f], 0).k > 0) need += shape_of(fam_count[f], 0).nb;
    dev_wide = need > cus;
  }
  pl.grp.assign((size_t)n_families, 0);
  for (int f = 0; f < n_families; f++)
  {
    const int nx = fam_count[f];
    int g = RAMX_CP_NCLASS + (nx <= 64 ? 0 : nx <= 128 ? 1 : nx <= 256 ? 2 : 3);
    if (nx > 0 && cp_max > 0 && cp_flanks_fit(flanks + fam_first[f], nx))
    {
      int k = 0, th = 0;
      const int c = nx <= cp_max ? ramx_cp_class(W, nx, &k, &th) : -1;
      if (c >= 0) { g = c; pl.cp_k[c] = k; pl.cp_threads[c] = th; pl.n_cp++; }
      else if (dev_route)
      {
        // the first device-wide family fixes the launch's shape; a later family with another plan stays on its lane-per-flank shape
        const Shape &s = shape_of(nx, dev_wide);
        if (s.k > 0 && s.nb <= cus && (pl.dev_k == 0 || (s.k == pl.dev_k && s.th == pl.dev_threads && s.vw == pl.dev_vw)))
        {
          pl.dev_k = s.k; pl.dev_threads = s.th; pl.dev_vw = s.vw;
          if (pl.rounds.empty() || pl.rounds.back().y + s.nb > cus) pl.rounds.push_back(make_int2((int)pl.dev.size(), 0));
          pl.rounds.back().y += s.nb;
          for (int b = 0; b < s.nb; b++) pl.dev.push_back(CpDevDesc{ fam_first[f], nx, b, s.nb, f, pl.n_dev, { 0, 0 } });
          pl.n_dev++;
          g = -1;
        }
      }
    }
    pl.grp[f] = g;
    if (g >= 0) pl.cls_count[g]++;
  }
  for (int c = 0; c < RAMX_NGROUP; c++) pl.cls_first[c + 1] = pl.cls_first[c] + pl.cls_count[c];
  pl.fam.resize((size_t)pl.cls_first[RAMX_NGROUP]);
  int fill[RAMX_NGROUP];
  memcpy(fill, pl.cls_first, sizeof(fill));
  for (int f = 0; f < n_families; f++)
    if (pl.grp[f] >= 0) pl.fam[(size_t)fill[pl.grp[f]]++] = FamDesc{ fam_first[f] / 64, (fam_count[f] + 63) / 64, fam_count[f], f };
  // The streams launched on.  The register-resident kernel gains nothing from smaller workgroups (measured: 11.5 vs 10.3 ms): one
  // launch of 256 threads for the three smaller shapes -- adjacent in `fam` -- on the third one's stream.  The device-wide launch
  // shares the last shape's.
  const int g0 = RAMX_CP_NCLASS;
  for (int c = 0; c < RAMX_NGROUP; c++) pl.launched[c] = pl.cls_count[c] > 0;
  if (pl.resident) { pl.launched[g0 + 2] = pl.launched[g0] || pl.launched[g0 + 1] || pl.launched[g0 + 2]; pl.launched[g0] = pl.launched[g0 + 1] = false; }
  if (pl.n_dev > 0) pl.launched[RAMX_NGROUP - 1] = true;
  return pl;
}

// one pass over a batch: its arguments, and what its steps hand on
struct FamilyPass
{
  const ramx_flank *flanks; int32_t n_padded; const int32_t *fam_first, *fam_count; int32_t n_families; const ramx_params *p;
  int W, L, Np, KW, tab[RAMX_NCLASS][4];
  float ms;                                  // HIP-event time of the launches (families_join)
  unsigned long long *fam_dbg, *cp_dbg;      // -DRAMX_PRK_TIMING / -DRAMX_CP_TIMING builds: phase sums of block 0
};

static int families_check(const ramx_dev *d, const ramx_flank *flanks, int32_t n_padded, const int32_t *fam_first, const int32_t *fam_count,
                          int32_t n_families, const ramx_params *p)
{
  if (!d || !p || !p->matrix || n_families < 0 || n_padded < 0 || (n_padded & 63) || (n_families && (!fam_first || !fam_count || !flanks)))
  { ramx_set_error("ramx_dev_run_families: bad argument"); return RAMX_ERR_ARG; }
  if (p->bandwidth < 1 || p->L < 0) { ramx_set_error("ramx_dev_run_families: bad bandwidth / L"); return RAMX_ERR_ARG; }
  int maxn = 0;
  for (int f = 0; f < n_families; f++)
  {
    if (fam_count[f] < 0 || fam_first[f] < 0 || (fam_first[f] & 63) || (long long)fam_first[f] + fam_count[f] > n_padded) { ramx_set_error("ramx_dev_run_families: bad family layout"); return RAMX_ERR_ARG; }
    if (fam_count[f] > maxn) maxn = fam_count[f];
  }
  if (maxn > 512) { ramx_set_error("batch mode: a family has more than 512 flanks"); return RAMX_ERR_UNSUPPORTED; }
  return RAMX_OK;
}

// Buffers, then everything the launches read, on the library's stream: descriptors, flanks, their packed windows, the cleared
// consensus -- and, BEFORE the fork of the group streams, what the device-wide launch needs (descriptors, cleared vote / error
// words: one set per multi-workgroup family): that launch is then the first thing the idle device sees, and its workgroups are
// resident before any other group's.
static int families_upload(ramx_dev *d, FamilyPass &b, const FamilyPlan &pl)
{
  const size_t n = (size_t)b.n_families, cons_bytes = n * (b.L > 0 ? b.L : 1) + 16;
  int rc;
  // the process-wide session serves seam 1 too: a packed-rows direction that stopped early may still be packing beside us
  if ((rc = pack_settle(d)) != RAMX_OK) return rc;
  if ((rc = ensure_windows(d, b.Np, b.KW))) return rc;
  if ((rc = ensure(&d->d_cons, &d->cap_cons, cons_bytes))) return rc;
  if ((rc = ensure(&d->d_fam, &d->cap_fam, sizeof(FamDesc) * n))) return rc;
  if ((rc = ensure(&d->d_famctl, &d->cap_famctl, sizeof(RamxCtl) * n))) return rc;
  // the streaming kernel keeps the rows of every family in the row buffer
  if (!pl.resident && pl.n_cp + pl.n_dev < b.n_families && (rc = ensure_rows(d, (size_t)b.Np * (b.W + 1) * sizeof(int4), false))) return rc;
  if (pl.n_dev > 0)
  {
    if ((rc = ensure(&d->d_devdesc, &d->cap_devdesc, sizeof(CpDevDesc) * pl.dev.size()))) return rc;
    if ((rc = ensure(&d->d_vote_sets, &d->cap_vote_sets, sizeof(PShard) * RAMX_CP_NSETS * NSHARD * (size_t)pl.n_dev))) return rc;
    if ((rc = ensure(&d->d_err_sets, &d->cap_err_sets, 64 * (size_t)pl.n_dev))) return rc;
  }
  if (!pl.fam.empty()) HIPCHK(hipMemcpyAsync(d->d_fam, pl.fam.data(), sizeof(FamDesc) * pl.fam.size(), hipMemcpyHostToDevice, d->stream));
  if (b.n_padded) HIPCHK(hipMemcpyAsync(d->d_flanks, b.flanks, (size_t)b.n_padded * sizeof(ramx_flank), hipMemcpyHostToDevice, d->stream));
  if ((rc = launch_pack(d, b.n_padded, b.Np, b.W, 0, b.KW, d->stream)) != RAMX_OK) return rc;
  d->packed_kw = b.KW;
  HIPCHK(hipMemsetAsync(d->d_cons, 0, cons_bytes, d->stream));       // columns a family never ran read as 0
#ifdef RAMX_PRK_TIMING
  HIPCHK(hipMalloc((void **)&b.fam_dbg, 8 * 8 * sizeof(unsigned long long)));
  HIPCHK(hipMemset(b.fam_dbg, 0, 8 * 8 * sizeof(unsigned long long)));
#endif
#ifdef RAMX_CP_TIMING
  HIPCHK(hipMalloc((void **)&b.cp_dbg, (16 * 16 + 8) * sizeof(unsigned long long)));       // the classes', else the device-wide launch's
  HIPCHK(hipMemset(b.cp_dbg, 0, (16 * 16 + 8) * sizeof(unsigned long long)));
#endif
  HIPCHK(hipEventRecord(d->ev_begin, d->stream));
  // the groups run side by side: one stream per group, forked from / joined into the library's stream
  if (!d->cls_init)
  {
    for (int c = 0; c < RAMX_NGROUP; c++)
    {
      HIPCHK(hipStreamCreateWithFlags(&d->cls_stream[c], hipStreamNonBlocking));
      HIPCHK(hipEventCreateWithFlags(&d->cls_done[c], hipEventDisableTiming));
    }
    HIPCHK(hipEventCreateWithFlags(&d->cls_ready, hipEventDisableTiming));
    d->cls_init = 1;
  }
  if (pl.n_dev > 0)
  {
    HIPCHK(hipMemcpyAsync(d->d_devdesc, pl.dev.data(), sizeof(CpDevDesc) * pl.dev.size(), hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipMemsetAsync(d->d_vote_sets, 0, sizeof(PShard) * RAMX_CP_NSETS * NSHARD * (size_t)pl.n_dev, d->stream));
    HIPCHK(hipMemsetAsync(d->d_err_sets, 0, 64 * (size_t)pl.n_dev, d->stream));
  }
  // every group stream waits, whether the plan launches on it or not: uploads and the pack kernel run on the library's stream
  HIPCHK(hipEventRecord(d->cls_ready, d->stream));
  for (int c = 0; c < RAMX_NGROUP; c++) HIPCHK(hipStreamWaitEvent(d->cls_stream[c], d->cls_ready, 0));
  return RAMX_OK;
}

// families above one workgroup: the device-wide mode, enqueued first, on the stream of the last lane-per-flank shape
static int launch_dev_families(ramx_dev *d, FamilyPass &b, const FamilyPlan &pl)
{
  if (pl.n_dev == 0) return RAMX_OK;
  CPArgs ca = cp_args(d, d->d_famctl, b.Np, b.KW, *b.p, b.tab);
  ca.nranks = 1; ca.rank = 0;
  ca.vote = d->d_vote_sets; ca.err = d->d_err_sets; ca.vote_wave = pl.dev_vw;
  // test hooks: RAMX_TEST_CP_DROP_TICKET=row withholds one workgroup's words for that row, in every multi-workgroup family or
  // only in family RAMX_TEST_CP_DROP_FAMILY (index in the batch)
  const char *td = getenv("RAMX_TEST_CP_DROP_TICKET"), *tf = getenv("RAMX_TEST_CP_DROP_FAMILY");
  ca.test_drop_row = td ? atoi(td) : 0; ca.test_drop_id = tf ? atoi(tf) : -1;
  ca.dbg = pl.n_cp == 0 ? b.cp_dbg : NULL;
  for (const int2 &ro : pl.rounds)
  {
    ca.dev = d->d_devdesc + ro.x;
    const int rc = ramx_cp_launch_device(d->cls_stream[RAMX_NGROUP - 1], b.W, pl.dev_k, pl.dev_threads, ro.y, ca);
    if (rc != RAMX_OK) { ramx_set_error("cell-parallel multi-family device launch failed (W %d, %d workgroups)", b.W, ro.y); return rc; }
  }
  return RAMX_OK;
}

// the cell-parallel classes, each on its own stream
static int launch_cp_families(ramx_dev *d, FamilyPass &b, const FamilyPlan &pl)
{
  if (pl.n_cp == 0) return RAMX_OK;
  CPArgs ca = cp_args(d, d->d_famctl, b.Np, b.KW, *b.p, b.tab);
  if (getenv("RAMX_CP_PEEK") != NULL)
  {
    // test hook: keep the final rows of every flank, [flank][2W+1] (m, e), for ramx_dev_peek_family_state
    const size_t need = (size_t)b.Np * (2 * b.W + 1) * sizeof(int2);
    const int prc = ensure(&d->d_cpstate, &d->cap_cpstate, need);
    if (prc != RAMX_OK) return prc;
    HIPCHK(hipMemsetAsync(d->d_cpstate, 0, need, d->stream));
    HIPCHK(hipEventRecord(d->cls_ready, d->stream));
    for (int c = 0; c < RAMX_CP_NCLASS; c++) HIPCHK(hipStreamWaitEvent(d->cls_stream[c], d->cls_ready, 0));
    ca.state_out = (int2 *)d->d_cpstate;
    d->cpstate_W = b.W; d->cpstate_n = b.Np;
  }
  ca.dbg = b.cp_dbg;
  for (int c = 0; c < RAMX_CP_NCLASS; c++)
  {
    if (pl.cls_count[c] == 0) continue;
    ca.fam = (const FamDesc *)d->d_fam + pl.cls_first[c];
    const int rc = ramx_cp_launch_families(d->cls_stream[c], b.W, pl.cp_k[c], pl.cp_threads[c], pl.cls_count[c], ca);
    if (rc != RAMX_OK) { ramx_set_error("cell-parallel family kernel launch failed (W %d, %d lanes per flank)", b.W, pl.cp_k[c]); return rc; }
  }
  return RAMX_OK;
}

// one lane per flank, streaming: one launch per workgroup shape (BLOCK threads: 1, 2, 4 or 8 tiles)
template <bool CHAIN, int BLOCK>
static void fam_stream_launch(ramx_dev *d, const FamilyPlan &pl, FSArgs fs)
{
  const int g = RAMX_CP_NCLASS + (BLOCK == 64 ? 0 : BLOCK == 128 ? 1 : BLOCK == 256 ? 2 : 3);
  if (pl.cls_count[g] == 0) return;
  fs.fam = (const FamDesc *)d->d_fam + pl.cls_first[g];
  hipLaunchKernelGGL((ramx_family_stream_kernel<CHAIN, BLOCK>), dim3(pl.cls_count[g]), dim3(BLOCK), 0, d->cls_stream[g], fs);
}

// ... register-resident: F families of up to BLOCK flanks, at one of the widths of fam_has_width
template <int BLOCK>
static int fam_launch(int W, FArgs fa, const FamDesc *fam, int F, hipStream_t st)
{
  if (F == 0) return RAMX_OK;
  fa.fam = fam;
  if (W == 14) hipLaunchKernelGGL((ramx_family_kernel<14, BLOCK>), dim3(F), dim3(BLOCK), 0, st, fa);
  else if (W == 20) hipLaunchKernelGGL((ramx_family_kernel<20, BLOCK>), dim3(F), dim3(BLOCK), 0, st, fa);
  else hipLaunchKernelGGL((ramx_family_kernel<40, BLOCK>), dim3(F), dim3(BLOCK), 0, st, fa);
  HIPCHK(hipGetLastError());
  return RAMX_OK;
}

// the families no cell-parallel launch took: the streaming kernel, or the register-resident one where it applies
static int launch_lane_families(ramx_dev *d, FamilyPass &b, const FamilyPlan &pl)
{
  if (pl.n_cp + pl.n_dev == b.n_families) return RAMX_OK;
  const ramx_params &p = *b.p;
  const int g0 = RAMX_CP_NCLASS;
  const FamDesc *dfd = (const FamDesc *)d->d_fam;
  if (!pl.resident)
  {
    FSArgs fs;
    memset(&fs, 0, sizeof(fs));
    fs.k.bases = d->d_bases; fs.k.bounds = d->d_bounds; fs.k.trim = d->d_trim; fs.k.S_in = d->d_state[0]; fs.k.S_out = d->d_state[0];
    fs.k.Np = b.Np; fs.k.Nx = b.Np; fs.k.W = b.W; fs.k.go = p.gapopen; fs.k.ge = p.gapextn; fs.k.cap = p.cappenalty;
    fs.k.minimp = p.minimprovement; fs.k.when_to_stop = p.when_to_stop;
    memcpy(fs.k.tab, b.tab, sizeof(fs.k.tab));
    fs.fam = dfd; fs.ctl_out = d->d_famctl; fs.cons_out = d->d_cons; fs.L = b.L;
    if (pl.chain) { fam_stream_launch<true, 64>(d, pl, fs); fam_stream_launch<true, 128>(d, pl, fs); fam_stream_launch<true, 256>(d, pl, fs); fam_stream_launch<true, 512>(d, pl, fs); }
    else { fam_stream_launch<false, 64>(d, pl, fs); fam_stream_launch<false, 128>(d, pl, fs); fam_stream_launch<false, 256>(d, pl, fs); fam_stream_launch<false, 512>(d, pl, fs); }
    HIPCHK(hipGetLastError());
    return RAMX_OK;
  }
  FArgs fa;
  memset(&fa, 0, sizeof(fa));
  fa.bases = d->d_bases; fa.bounds = d->d_bounds; fa.fam = dfd; fa.trim = d->d_trim; fa.ctl_out = d->d_famctl; fa.cons_out = d->d_cons;
  fa.Np = b.Np; fa.L = b.L; fa.go = p.gapopen; fa.ge = p.gapextn; fa.cap = p.cappenalty; fa.minimp = p.minimprovement;
  fa.when_to_stop = p.when_to_stop;
  memcpy(fa.tab, b.tab, sizeof(fa.tab));
  fa.pack_ok = getenv("RAMX_NO_FASTPACK") ? 0 : fast_pack_ok(fa.tab, fa.go, fa.ge, b.L, b.W);
  if (fa.pack_ok && getenv("RAMX_NO_MASKHI") == NULL) fa.pack_ok = 2;
  fa.lean_p = lean_p_of(fa.tab, fa.go, fa.ge);
  fa.dbg = b.fam_dbg;
  // 256 threads up to 256 flanks (the three smaller shapes in one launch, see family_plan), 512 above
  const int n256 = pl.cls_count[g0] + pl.cls_count[g0 + 1] + pl.cls_count[g0 + 2];
  const int rc = fam_launch<256>(b.W, fa, dfd + pl.cls_first[g0], n256, d->cls_stream[g0 + 2]);
  return rc != RAMX_OK ? rc : fam_launch<512>(b.W, fa, dfd + pl.cls_first[g0 + 3], pl.cls_count[g0 + 3], d->cls_stream[g0 + 3]);
}

// every stream the plan launched on back into the library's stream; on return everything has run
static int families_join(ramx_dev *d, FamilyPass &b, const FamilyPlan &pl)
{
  for (int c = 0; c < RAMX_NGROUP; c++)
    if (pl.launched[c]) { HIPCHK(hipEventRecord(d->cls_done[c], d->cls_stream[c])); HIPCHK(hipStreamWaitEvent(d->stream, d->cls_done[c], 0)); }
  HIPCHK(hipEventRecord(d->ev_end, d->stream));
  HIPCHK(hipStreamSynchronize(d->stream));
  HIPCHK(hipEventElapsedTime(&b.ms, d->ev_begin, d->ev_end));
  return RAMX_OK;
}

// control blocks, consensus and trim records to the caller.  timed_out[f] != 0: that family's device-wide vote gave up -- its
// outputs are invalid; with timed_out == NULL such a family makes the whole call fail.
static int families_fetch(ramx_dev *d, const FamilyPass &b, const FamilyPlan &pl, ramx_run_info *infos, int8_t *cons, int32_t *trim_high,
                          int32_t *trim_pos, unsigned char *timed_out)
{
  const int n = b.n_families, L = b.L;
  std::vector<RamxCtl> hctl((size_t)n);
  HIPCHK(hipMemcpy(hctl.data(), d->d_famctl, sizeof(RamxCtl) * (size_t)n, hipMemcpyDeviceToHost));
  if (cons && L > 0) HIPCHK(hipMemcpy(cons, d->d_cons, (size_t)n * L, hipMemcpyDeviceToHost));
  if ((trim_high || trim_pos) && b.n_padded)
  {
    std::vector<int2> tmp((size_t)b.n_padded);
    HIPCHK(hipMemcpy(tmp.data(), d->d_trim, tmp.size() * sizeof(int2), hipMemcpyDeviceToHost));
    for (int i = 0; i < b.n_padded; i++) { if (trim_high) trim_high[i] = tmp[i].x; if (trim_pos) trim_pos[i] = tmp[i].y; }
  }
  for (int f = 0; f < n; f++)
  {
    const int g = pl.grp[f];
    const bool gave_up = g < 0 && hctl[f].pad != 0;
    if (timed_out) timed_out[f] = gave_up ? 1 : 0;
    if (gave_up && !timed_out) { ramx_set_error("batch mode: the vote of a multi-workgroup family timed out (bounded spin gave up)"); return RAMX_ERR_STATE; }
    if (!infos) continue;
    memset(&infos[f], 0, sizeof(ramx_run_info));
    infos[f].ret = hctl[f].max_row + 1;
    infos[f].rows_executed = hctl[f].rows_done;
    infos[f].limit_warning = (hctl[f].stopped && hctl[f].rows_done - 1 == L - 1) ? 1 : 0;
    infos[f].overflow32 = hctl[f].overflow;
    infos[f].n_extendable = b.fam_count[f];
    infos[f].launches = 1;
    infos[f].loop_ms = b.ms;
    /* 1: rows resident in registers (3: of K lanes per flank, the cell-parallel kernel); 2: streaming family kernel */
    infos[f].persistent = g < RAMX_CP_NCLASS ? 1 : (pl.resident ? 1 : 2);
    infos[f].lanes_per_flank = g < 0 ? pl.dev_k : (g < RAMX_CP_NCLASS ? pl.cp_k[g] : 1);
    infos[f].respeculated_rows = g < 0 ? hctl[f].besta : 0;
  }
  return RAMX_OK;
}

// One pass over a batch.  allow_dev: families above one cell-parallel workgroup may take the device-wide mode (several
// workgroups voting through ticket words with a bounded spin); a family whose vote gave up there (e.g. its workgroups were not
// all resident because a co-tenant held CUs) is reported in timed_out, and the caller repeats it with allow_dev = false.
static int run_families_pass(ramx_dev *d, const ramx_flank *flanks, int32_t n_padded, const int32_t *fam_first,
                             const int32_t *fam_count, int32_t n_families, const ramx_params *p,
                             ramx_run_info *infos, int8_t *cons, int32_t *trim_high, int32_t *trim_pos,
                             bool allow_dev, unsigned char *timed_out)
{
  int rc = families_check(d, flanks, n_padded, fam_first, fam_count, n_families, p);
  if (rc != RAMX_OK || n_families == 0) return rc;
  HIPCHK(hipSetDevice(d->ordinal));
  FamilyPass b = {};
  b.flanks = flanks; b.n_padded = n_padded; b.fam_first = fam_first; b.fam_count = fam_count; b.n_families = n_families; b.p = p;
  b.W = p->bandwidth; b.L = p->L; b.Np = n_padded > 0 ? n_padded : 64; b.KW = window_words(b.L, b.W);
  class_tab(p, b.tab);
  // (the plan and its host arrays live until everything enqueued from them has run: families_join synchronises)
  const FamilyPlan pl = family_plan(route_env(), b.W, p->gapopen, p->gapextn, b.tab, b.L, d->cus, d->force_chain != 0, allow_dev, flanks,
                                    fam_first, fam_count, n_families);
  rc = families_upload(d, b, pl);
  if (rc == RAMX_OK) rc = launch_dev_families(d, b, pl);
  if (rc == RAMX_OK) rc = launch_cp_families(d, b, pl);
  if (rc == RAMX_OK) rc = launch_lane_families(d, b, pl);
  if (rc == RAMX_OK) rc = families_join(d, b, pl);
#ifdef RAMX_PRK_TIMING
  if (rc == RAMX_OK && pl.resident && pl.n_cp + pl.n_dev < n_families) rc = fam_timing_report(b.fam_dbg);
  (void)hipFree(b.fam_dbg);
#endif
#ifdef RAMX_CP_TIMING
  if (rc == RAMX_OK && pl.n_cp + pl.n_dev > 0) rc = cp_family_timing_report(b.cp_dbg);
  (void)hipFree(b.cp_dbg);
#endif
  if (rc == RAMX_OK) rc = families_fetch(d, b, pl, infos, cons, trim_high, trim_pos, timed_out);
  d->ready = 0;       // the single-family buffers were reused: begin_direction must be called again before run_direction
  d->planes_ready = 0;
  return rc;
}

static ramx_flank empty_flank(void) { ramx_flank x; memset(&x, 0, sizeof(x)); x.t_lo = 1; x.t_hi = 0; x.step = 1; return x; }


extern "C" int ramx_dev_run_families(ramx_dev *d, const ramx_flank *flanks, int32_t n_padded, const int32_t *fam_first,
                                     const int32_t *fam_count, int32_t n_families, const ramx_params *p,
                                     ramx_run_info *infos, int8_t *cons, int32_t *trim_high, int32_t *trim_pos)
{
  std::vector<unsigned char> to((size_t)(n_families > 0 ? n_families : 1), 0);
  int rc = run_families_pass(d, flanks, n_padded, fam_first, fam_count, n_families, p, infos, cons, trim_high, trim_pos, true, to.data());
  if (rc != RAMX_OK) return rc;
  // Batch mode degrades, it does not fail: a multi-workgroup family whose device-wide vote gave up is repeated on the
  // one-lane-per-flank route (one workgroup per family, block-local vote: nothing to wait for), the other families'
  // results are kept.
  std::vector<int> redo;
  for (int f = 0; f < n_families; f++) if (to[f]) redo.push_back(f);
  if (redo.empty()) return RAMX_OK;
  fprintf(stderr, "ramx: batch mode: the device-wide vote of %zu multi-workgroup famil%s timed out (bounded spin); repeating "
                  "%s on the lane-per-flank route\n", redo.size(), redo.size() == 1 ? "y" : "ies", redo.size() == 1 ? "it" : "them");
  const int L = p->L;
  std::vector<ramx_flank> fl2;
  std::vector<int32_t> first2, count2;
  for (int f : redo)
  {
    first2.push_back((int32_t)fl2.size());
    count2.push_back(fam_count[f]);
    const int padded = ((fam_count[f] + 63) / 64) * 64;
    for (int i = 0; i < padded; i++) fl2.push_back(i < fam_count[f] ? flanks[fam_first[f] + i] : empty_flank());
  }
  const int n2 = (int)redo.size(), np2 = (int)fl2.size();
  std::vector<ramx_run_info> inf2((size_t)n2);
  std::vector<int8_t> cons2((size_t)n2 * (L > 0 ? L : 1));
  std::vector<int32_t> th2((size_t)np2 + 1), tp2((size_t)np2 + 1);
  rc = run_families_pass(d, fl2.data(), np2, first2.data(), count2.data(), n2, p, inf2.data(), cons2.data(), th2.data(), tp2.data(), false, NULL);
  if (rc != RAMX_OK) return rc;
  for (int k = 0; k < n2; k++)
  {
    const int f = redo[k];
    if (infos) infos[f] = inf2[k];
    if (cons && L > 0) memcpy(cons + (size_t)f * L, cons2.data() + (size_t)k * L, (size_t)L);
    for (int i = 0; i < fam_count[f]; i++)
    {
      if (trim_high) trim_high[fam_first[f] + i] = th2[first2[k] + i];
      if (trim_pos) trim_pos[fam_first[f] + i] = tp2[first2[k] + i];
    }
  }
  return RAMX_OK;
}

// ------------------------------------------------------------------------------------------
// replays along a given consensus: what ramx_dev_profile, ramx_dev_align, ramx_dev_pileup and ramx_dev_refine share on the host
// ------------------------------------------------------------------------------------------
struct ReplayPlan
{
  int tiles, maxrows;
  std::vector<int2> tile_fam;       // per tile: (family, flanks in the tile), (-1, 0) outside every family
  std::vector<int4> fam_desc;       // per family: (first tile, tiles, rows, 0)
};

// the checks of the family layout, the rows and the consensus (check), and the tile / family tables of the families with
// run[f] != 0 (run == NULL: all)
static int replay_plan(const char *who, int32_t n_padded, const int32_t *fam_first, const int32_t *fam_count, int32_t n_families,
                       int L, const int8_t *cons, const int32_t *rows, const char *run, bool check, ReplayPlan &pl)
{
  pl.tiles = n_padded / 64;
  pl.maxrows = 0;
  pl.tile_fam.assign((size_t)(pl.tiles > 0 ? pl.tiles : 1), make_int2(-1, 0));
  pl.fam_desc.assign((size_t)(n_families > 0 ? n_families : 1), make_int4(0, 0, 0, 0));
  for (int f = 0; f < n_families; f++)
  {
    if (check)
    {
      if (fam_count[f] < 0 || fam_first[f] < 0 || (fam_first[f] & 63) || (long long)fam_first[f] + fam_count[f] > n_padded)
      { ramx_set_error("%s: bad family layout", who); return RAMX_ERR_ARG; }
      if (rows[f] < 0 || rows[f] > L) { ramx_set_error("%s: rows[%d] = %d outside [0, L = %d]", who, f, rows[f], L); return RAMX_ERR_ARG; }
      if (rows[f] > 0 && !cons) { ramx_set_error("%s: cons missing", who); return RAMX_ERR_ARG; }
      for (int r = 0; r < rows[f]; r++)
        if (cons[(size_t)f * L + r] < 0 || cons[(size_t)f * L + r] > 3) { ramx_set_error("%s: consensus base outside A C G T (family %d, column %d)", who, f, r); return RAMX_ERR_ARG; }
    }
    const int t0 = fam_first[f] / 64, nt = (fam_count[f] + 63) / 64;
    if (check)
      for (int t = 0; t < nt; t++)
      {
        if (pl.tile_fam[t0 + t].x >= 0) { ramx_set_error("%s: families %d and %d overlap", who, pl.tile_fam[t0 + t].x, f); return RAMX_ERR_ARG; }
        pl.tile_fam[t0 + t].x = f;
      }
    if (run && !run[f]) continue;
    for (int t = 0; t < nt; t++)
    {
      const int left = fam_count[f] - 64 * t;
      pl.tile_fam[t0 + t] = make_int2(f, left < 64 ? left : 64);
    }
    pl.fam_desc[f] = make_int4(t0, nt, rows[f], 0);
    if (rows[f] > pl.maxrows) pl.maxrows = rows[f];
  }
  if (check && run)       // the overlap check marked every family's tiles: those that do not run belong to none
    for (int f = 0; f < n_families; f++)
      if (!run[f])
        for (int t = 0; t < (fam_count[f] + 63) / 64; t++) pl.tile_fam[fam_first[f] / 64 + t] = make_int2(-1, 0);
  return RAMX_OK;
}

// once per call: the flanks uploaded and their windows packed as Np flanks, the buffers of what replay_upload sends, and what
// run_band reads (k); need_state: the rows go through the global row buffer
static int replay_setup(ramx_dev *d, const ramx_flank *flanks, int32_t n_padded, int Np, int32_t n_families, const ramx_params *p,
                        bool need_state, KArgs &k, int *KW_out)
{
  HIPCHK(hipSetDevice(d->ordinal));
  const int W = p->bandwidth, L = p->L, KW = window_words(L, W);
  int rc;
  // a piece of the direction before may still be packing into d_bases on the second stream: it must have finished before the
  // buffer can be reallocated, let alone written
  if ((rc = pack_settle(d, true)) != RAMX_OK) return rc;
  if ((rc = ensure(&d->d_flanks, &d->cap_flanks, (size_t)Np * sizeof(ramx_flank)))) return rc;
  if ((rc = ensure(&d->d_bases, &d->cap_bases, (size_t)KW * Np * sizeof(unsigned)))) return rc;
  if ((rc = ensure(&d->d_bounds, &d->cap_bounds, (size_t)Np * sizeof(int2)))) return rc;
  if (need_state && (rc = ensure(&d->d_rp_state, &d->cap_rp_state, (size_t)Np * (W + 1) * sizeof(int4)))) return rc;
  if ((rc = ensure(&d->d_rp_cons, &d->cap_rp_cons, (size_t)n_families * L + 16))) return rc;
  if ((rc = ensure(&d->d_rp_rows, &d->cap_rp_rows, (size_t)n_families * sizeof(int)))) return rc;
  if ((rc = ensure(&d->d_rp_tile, &d->cap_rp_tile, (size_t)(Np / 64) * sizeof(int2)))) return rc;
  if ((rc = ensure(&d->d_rp_fam, &d->cap_rp_fam, (size_t)n_families * sizeof(int4)))) return rc;
  if (n_padded) HIPCHK(hipMemcpyAsync(d->d_flanks, flanks, (size_t)n_padded * sizeof(ramx_flank), hipMemcpyHostToDevice, d->stream));
  if ((rc = launch_pack(d, n_padded, Np, W, 0, KW, d->stream)) != RAMX_OK) return rc;
  d->packed_kw = KW;
  d->ready = 0;       // the direction's flank and window buffers were reused: begin_direction must be called again before run_direction
  d->planes_ready = 0;        // ... and the resident bit planes belong to the replay before this one
  memset(&k, 0, sizeof(k));
  k.bases = d->d_bases; k.bounds = d->d_bounds; k.S_in = d->d_rp_state; k.S_out = d->d_rp_state;
  k.Np = Np; k.Nx = Np; k.W = W; k.go = p->gapopen; k.ge = p->gapextn; k.cap = p->cappenalty;
  class_tab(p, k.tab);
  *KW_out = KW;
  return RAMX_OK;
}

// once per replay: the consensus, the rows and the plan's two tables
static int replay_upload(ramx_dev *d, const ReplayPlan &pl, int32_t n_families, int L, const int8_t *cons, const int32_t *rows)
{
  HIPCHK(hipMemcpyAsync(d->d_rp_cons, cons, (size_t)n_families * L, hipMemcpyHostToDevice, d->stream));
  HIPCHK(hipMemcpyAsync(d->d_rp_rows, rows, (size_t)n_families * sizeof(int), hipMemcpyHostToDevice, d->stream));
  HIPCHK(hipMemcpyAsync(d->d_rp_tile, pl.tile_fam.data(), pl.tile_fam.size() * sizeof(int2), hipMemcpyHostToDevice, d->stream));
  HIPCHK(hipMemcpyAsync(d->d_rp_fam, pl.fam_desc.data(), (size_t)n_families * sizeof(int4), hipMemcpyHostToDevice, d->stream));
  return RAMX_OK;
}

// the group of tiles whose `what` (tile_bytes per tile) fit the bytes the environment variable `env` allows (1 GiB unless it
// is set; read per call)
static int tile_group(const char *who, const char *env, const char *what, int tiles, size_t tile_bytes, int *group)
{
  size_t budget = (size_t)1 << 30;
  if (const char *e = getenv(env)) { const long long v = atoll(e); if (v > 0) budget = (size_t)v; }
  if (tile_bytes > budget)
  {
    ramx_set_error("%s: the %s (%zu bytes) do not fit %s = %zu", who, what, tile_bytes, env, budget);
    return RAMX_ERR_UNSUPPORTED;
  }
  *group = (int)(budget / tile_bytes < (size_t)tiles ? budget / tile_bytes : (size_t)tiles);
  return RAMX_OK;
}

// group after group on one stream: a group's later stages have read what its earlier ones wrote before the next group's kernels
// write it again.  body(tile0, nt, mark) launches the nstage stages of one group and calls mark() before the first and after
// each; with kernel_ms the marks are HIP events and stage i's time, summed over the groups, is added to kernel_ms[i].  With
// host_reuse the stream is synchronised after every group, because the next one fills the same host buffers; on return the
// stream is idle either way.
template <class Body>
static int tile_groups(ramx_dev *d, const char *who, int tiles, int group, int nstage, double *kernel_ms, bool host_reuse, Body body)
{
  const int ngroups = (tiles + group - 1) / group;
  std::vector<hipEvent_t> ev(kernel_ms ? (size_t)(nstage + 1) * ngroups : 0, (hipEvent_t)NULL);
  hipError_t he = hipSuccess;
  for (auto &e : ev) if (he == hipSuccess) he = hipEventCreate(&e);
  size_t marks = 0;
  auto mark = [&]() { if (marks < ev.size() && he == hipSuccess) he = hipEventRecord(ev[marks++], d->stream); };
  hipError_t se = hipSuccess;
  int rc = RAMX_OK;
  for (int g = 0; g < ngroups && rc == RAMX_OK && he == hipSuccess && se == hipSuccess; g++)
  {
    const int tile0 = g * group;
    rc = body(tile0, tiles - tile0 < group ? tiles - tile0 : group, mark);
    if (host_reuse && rc == RAMX_OK) se = hipStreamSynchronize(d->stream);
  }
  if (rc != RAMX_OK) ramx_set_error("%s: launch failed (%s)", who, hipGetErrorString(hipGetLastError()));
  if (!host_reuse || rc != RAMX_OK) se = hipStreamSynchronize(d->stream);
  for (size_t i = 0; i + 1 < ev.size() && rc == RAMX_OK && he == hipSuccess && se == hipSuccess; i++)
  {
    if ((int)(i % (nstage + 1)) == nstage) continue;       // from a group's last mark to the next group's first: no stage
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
    kernel_ms[i % (nstage + 1)] += ms;
  }
  for (auto &e : ev) if (e) (void)hipEventDestroy(e);
  if (rc != RAMX_OK) return rc;
  HIPCHK(he);
  HIPCHK(se);
  return RAMX_OK;
}

// what the kernels never reach is answered on the host: flanks [i0, i1) have no alignment (ends, col_idx / col_ins may be NULL)
static void replay_no_alignment(ramx_aln_end *ends, int32_t *col_idx, int32_t *col_ins, int i0, int i1, int maxrows, int32_t n_padded)
{
  const ramx_aln_end none = { -1, -1, 0, 0, 0 };
  if (ends) for (int i = i0; i < i1; i++) ends[i] = none;
  if (col_idx)
    for (int r = 0; r < maxrows; r++)
      for (int i = i0; i < i1; i++) { col_idx[(size_t)r * n_padded + i] = RAMX_ALN_NONE; col_ins[(size_t)r * n_padded + i] = 0; }
}

// what both alignment replays hand the forward kernel and the walk: run_band's arguments, the shared tables, the flanks' records
static int aln_args(ramx_dev *d, const KArgs &k, int L, AlnArgs &aa)
{
  int rc;
  if ((rc = ensure(&d->d_al_ends, &d->cap_al_ends, (size_t)k.Np * sizeof(ramx_aln_end)))) return rc;
  memset(&aa, 0, sizeof(aa));
  aa.k = k;
  aa.tile_fam = d->d_rp_tile; aa.cons = d->d_rp_cons; aa.rows = d->d_rp_rows; aa.ends = d->d_al_ends;
  aa.L = L; aa.nd = ramx_align_dwords(k.W);
  return RAMX_OK;
}

// ------------------------------------------------------------------------------------------
// support profile: every flank's band replayed along a given consensus (ramx_kernels_profile.h)
// ------------------------------------------------------------------------------------------
extern "C" int ramx_dev_profile(ramx_dev *d, const ramx_flank *flanks, int32_t n_padded, const int32_t *fam_first,
                                const int32_t *fam_count, int32_t n_families, const ramx_params *p,
                                const int8_t *cons, const int32_t *rows, ramx_col_profile *cols, int32_t *last_uncapped_row,
                                int32_t *row_best, int32_t *row_best_idx, double *kernel_ms)
{
  if (kernel_ms) *kernel_ms = 0;
  if (!d || !p || !p->matrix || n_families < 0 || n_padded < 0 || (n_padded & 63) || (n_padded && !flanks) ||
      (n_families && (!fam_first || !fam_count || !rows)))
  { ramx_set_error("ramx_dev_profile: bad argument"); return RAMX_ERR_ARG; }
  if ((row_best == NULL) != (row_best_idx == NULL)) { ramx_set_error("ramx_dev_profile: row_best and row_best_idx go together"); return RAMX_ERR_ARG; }
  const int W = p->bandwidth, L = p->L;
  if (W < 1 || L < 0) { ramx_set_error("ramx_dev_profile: bad bandwidth / L"); return RAMX_ERR_ARG; }
  ReplayPlan pl;
  int rc;
  if ((rc = replay_plan("ramx_dev_profile", n_padded, fam_first, fam_count, n_families, L, cons, rows, NULL, true, pl)) != RAMX_OK) return rc;
  const int tiles = pl.tiles, maxrows = pl.maxrows;
  if (maxrows > 0 && !cols) { ramx_set_error("ramx_dev_profile: cols missing"); return RAMX_ERR_ARG; }
  if (last_uncapped_row) for (int i = 0; i < n_padded; i++) last_uncapped_row[i] = -1;
  // no return on tiles == 0: a family without flanks still gets its bases from the sum kernel (align and pileup answer it on the host)
  if (n_families == 0 || maxrows == 0) return RAMX_OK;
  const int Np = n_padded > 0 ? n_padded : 64;        // ... and a set without flanks is packed and run as one tile of nothing
  // rows on chip for the band widths that have the instantiation (the conditions of the persistent kernel: no positive gap
  // penalty, e - m fits int16); RAMX_PROFILE_NO_RESIDENT sends them through the global row buffer like every other case (A/B)
  const bool chain = p->gapopen > 0 || p->gapextn > 0 || d->force_chain;
  const bool resident = !chain && ramx_profile_has_resident(W) && p->gapopen + p->gapextn >= -32768 && getenv("RAMX_PROFILE_NO_RESIDENT") == NULL;
  ProfArgs pa;
  memset(&pa, 0, sizeof(pa));
  int KW;
  if ((rc = replay_setup(d, flanks, n_padded, Np, n_families, p, !resident, pa.k, &KW)) != RAMX_OK) return rc;     // rows on chip need no row buffer
  if ((rc = ensure(&d->d_pf_slab, &d->cap_pf_slab, (size_t)(tiles > 0 ? tiles : 1) * maxrows * sizeof(ramx_col_profile)))) return rc;
  if ((rc = ensure(&d->d_pf_cols, &d->cap_pf_cols, (size_t)n_families * L * sizeof(ramx_col_profile)))) return rc;
  if ((rc = ensure(&d->d_pf_last, &d->cap_pf_last, (size_t)Np * sizeof(int)))) return rc;
  if (row_best)
  {
    if ((rc = ensure(&d->d_pf_best, &d->cap_pf_best, (size_t)maxrows * Np * sizeof(int)))) return rc;
    if ((rc = ensure(&d->d_pf_bidx, &d->cap_pf_bidx, (size_t)maxrows * Np * sizeof(int)))) return rc;
  }
  if ((rc = replay_upload(d, pl, n_families, L, cons, rows)) != RAMX_OK) return rc;
  HIPCHK(hipMemsetAsync(d->d_pf_last, 0xff, (size_t)Np * sizeof(int), d->stream));
  if (row_best)
  {
    // tiles outside every family and rows beyond a family's count are never written: they read as 0
    HIPCHK(hipMemsetAsync(d->d_pf_best, 0, (size_t)maxrows * Np * sizeof(int), d->stream));
    HIPCHK(hipMemsetAsync(d->d_pf_bidx, 0, (size_t)maxrows * Np * sizeof(int), d->stream));
  }
  // the profile kernels read the flank descriptors as well as their packed windows
  pa.flanks = d->d_flanks; pa.tile_fam = d->d_rp_tile; pa.cons = d->d_rp_cons; pa.rows = d->d_rp_rows; pa.slab = d->d_pf_slab;
  pa.last_uncapped = d->d_pf_last; pa.row_best = row_best ? d->d_pf_best : NULL; pa.row_best_idx = row_best ? d->d_pf_bidx : NULL;
  pa.L = L; pa.slab_rows = maxrows;
  ProfSumArgs sa;
  sa.slab = d->d_pf_slab; sa.fam = d->d_rp_fam; sa.cons = d->d_rp_cons; sa.cols = d->d_pf_cols; sa.L = L; sa.slab_rows = maxrows;
  if (resident)
  {
    pa.pack_ok = getenv("RAMX_NO_FASTPACK") ? 0 : fast_pack_ok(pa.k.tab, pa.k.go, pa.k.ge, L, W);
    if (pa.pack_ok && getenv("RAMX_NO_MASKHI") == NULL) pa.pack_ok = 2;
    pa.lean_p = lean_p_of(pa.k.tab, pa.k.go, pa.k.ge);
  }
  // one launch over all tiles, no groups: timed with the session's events
  HIPCHK(hipEventRecord(d->ev_begin, d->stream));
  if ((rc = ramx_profile_launch(d->stream, resident, chain, tiles, pa, n_families, sa)) != RAMX_OK)
  { ramx_set_error("ramx_dev_profile: launch failed (%s)", hipGetErrorString(hipGetLastError())); return rc; }
  HIPCHK(hipEventRecord(d->ev_end, d->stream));
  HIPCHK(hipStreamSynchronize(d->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, d->ev_begin, d->ev_end));
  if (kernel_ms) *kernel_ms = ms;
  // only rows[f] entries per family are written: one family comes straight into place, several come as one block that is
  // scattered here
  if (n_families == 1)
    HIPCHK(hipMemcpy(cols, d->d_pf_cols, (size_t)rows[0] * sizeof(ramx_col_profile), hipMemcpyDeviceToHost));
  else
  {
    std::vector<ramx_col_profile> stage((size_t)n_families * L);
    HIPCHK(hipMemcpy(stage.data(), d->d_pf_cols, stage.size() * sizeof(ramx_col_profile), hipMemcpyDeviceToHost));
    for (int f = 0; f < n_families; f++)
      if (rows[f] > 0) memcpy(cols + (size_t)f * L, stage.data() + (size_t)f * L, (size_t)rows[f] * sizeof(ramx_col_profile));
  }
  if (last_uncapped_row && n_padded) HIPCHK(hipMemcpy(last_uncapped_row, d->d_pf_last, (size_t)n_padded * sizeof(int), hipMemcpyDeviceToHost));
  if (row_best && n_padded)
  {
    HIPCHK(hipMemcpy(row_best, d->d_pf_best, (size_t)maxrows * n_padded * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(row_best_idx, d->d_pf_bidx, (size_t)maxrows * n_padded * sizeof(int), hipMemcpyDeviceToHost));
  }
  return RAMX_OK;
}

// ------------------------------------------------------------------------------------------
// per-copy alignments: the band replayed along a given consensus with every cell's decisions kept, then walked back
// (ramx_kernels_align.h)
// ------------------------------------------------------------------------------------------
extern "C" int ramx_dev_align(ramx_dev *d, const ramx_flank *flanks, int32_t n_padded, const int32_t *fam_first,
                              const int32_t *fam_count, int32_t n_families, const ramx_params *p,
                              const int8_t *cons, const int32_t *rows, ramx_aln_end *ends, int32_t *col_idx, int32_t *col_ins,
                              double *kernel_ms)
{
  if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0;
  // the records are the result: ends is required wherever there are flanks
  if (!d || !p || !p->matrix || n_families < 0 || n_padded < 0 || (n_padded & 63) || (n_padded && (!flanks || !ends)) ||
      (n_families && (!fam_first || !fam_count || !rows)))
  { ramx_set_error("ramx_dev_align: bad argument"); return RAMX_ERR_ARG; }
  if ((col_idx == NULL) != (col_ins == NULL)) { ramx_set_error("ramx_dev_align: col_idx and col_ins go together"); return RAMX_ERR_ARG; }
  const int W = p->bandwidth, L = p->L;
  if (W < 1 || L < 0) { ramx_set_error("ramx_dev_align: bad bandwidth / L"); return RAMX_ERR_ARG; }
  ReplayPlan pl;
  int rc;
  if ((rc = replay_plan("ramx_dev_align", n_padded, fam_first, fam_count, n_families, L, cons, rows, NULL, true, pl)) != RAMX_OK) return rc;
  const int tiles = pl.tiles, maxrows = pl.maxrows;
  auto no_alignment = [&](int f) {
    const int t0 = fam_first[f] / 64, nt = (fam_count[f] + 63) / 64;
    replay_no_alignment(ends, col_idx, col_ins, t0 * 64, (t0 + nt) * 64, maxrows, n_padded);
  };
  if (n_families == 0 || maxrows == 0 || tiles == 0)
  {
    for (int f = 0; f < n_families; f++) no_alignment(f);
    return RAMX_OK;
  }
  // the budget counts the decision codes only: the columns are whole-set [maxrows][Np] arrays of their own
  const size_t tile_bytes = (size_t)maxrows * ramx_align_dwords(W) * 64 * sizeof(unsigned);
  int group, KW;
  if ((rc = tile_group("ramx_dev_align", "RAMX_ALIGN_BYTES", "decision codes of one tile of 64 flanks", tiles, tile_bytes, &group)) != RAMX_OK) return rc;
  KArgs k;
  AlnArgs aa;
  if ((rc = replay_setup(d, flanks, n_padded, n_padded, n_families, p, true, k, &KW)) != RAMX_OK) return rc;
  if ((rc = aln_args(d, k, L, aa)) != RAMX_OK) return rc;
  if ((rc = ensure(&d->d_al_codes, &d->cap_al_codes, (size_t)group * tile_bytes))) return rc;
  const size_t ncol = (size_t)maxrows * n_padded;
  if (col_idx)
  {
    if ((rc = ensure(&d->d_al_idx, &d->cap_al_idx, ncol * sizeof(int)))) return rc;
    if ((rc = ensure(&d->d_al_ins, &d->cap_al_ins, ncol * sizeof(int)))) return rc;
  }
  if ((rc = replay_upload(d, pl, n_families, L, cons, rows)) != RAMX_OK) return rc;
  // the columns are preset once, for the whole set
  if (col_idx && (rc = ramx_align_launch_preset(d->stream, d->d_al_idx, d->d_al_ins, ncol)) != RAMX_OK) return rc;
  aa.codes = d->d_al_codes; aa.gn = group * 64;
  aa.col_idx = col_idx ? d->d_al_idx : NULL; aa.col_ins = col_idx ? d->d_al_ins : NULL;
  rc = tile_groups(d, "ramx_dev_align", tiles, group, 2, kernel_ms, false, [&](int tile0, int nt, auto &mark) {
    int lrc;
    aa.tile0 = tile0;
    mark();
    if ((lrc = ramx_align_launch_forward(d->stream, nt, aa)) != RAMX_OK) return lrc;
    mark();
    if ((lrc = ramx_align_launch_walk(d->stream, nt, aa)) != RAMX_OK) return lrc;
    mark();
    return RAMX_OK;
  });
  if (rc != RAMX_OK) return rc;
  // the tiles of every family, all rows, copied back per family; tiles outside every family keep what the caller has there
  for (int f = 0; f < n_families; f++)
  {
    const int t0 = fam_first[f] / 64, nt = (fam_count[f] + 63) / 64;
    if (nt == 0) continue;
    if (rows[f] == 0) { no_alignment(f); continue; }   // its tiles ran no row: the forward kernel still wrote their records
    HIPCHK(hipMemcpy(ends + (size_t)t0 * 64, d->d_al_ends + (size_t)t0 * 64, (size_t)nt * 64 * sizeof(ramx_aln_end), hipMemcpyDeviceToHost));
    if (col_idx)
    {
      HIPCHK(hipMemcpy2D(col_idx + (size_t)t0 * 64, (size_t)n_padded * sizeof(int), d->d_al_idx + (size_t)t0 * 64, (size_t)n_padded * sizeof(int),
                         (size_t)nt * 64 * sizeof(int), (size_t)maxrows, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy2D(col_ins + (size_t)t0 * 64, (size_t)n_padded * sizeof(int), d->d_al_ins + (size_t)t0 * 64, (size_t)n_padded * sizeof(int),
                         (size_t)nt * 64 * sizeof(int), (size_t)maxrows, hipMemcpyDeviceToHost));
    }
  }
  return RAMX_OK;
}

// ------------------------------------------------------------------------------------------
// pileup and consensus refinement: ramx_dev_align's forward pass and walk group after group, the group's columns counted on the
// device next to the walk (ramx_kernels_pileup.h); the re-call is host C (ramx_recall.c)
// ------------------------------------------------------------------------------------------
// once per call (not per replay): the shared setup, the walk's arguments and the families' summed columns
// (cols == false: the per-copy statistics, which have no columns)
static int pileup_setup(ramx_dev *d, const ramx_flank *flanks, int32_t n_padded, int32_t n_families, const ramx_params *p, AlnArgs &aa, int *KW,
                        bool cols = true)
{
  KArgs k;
  int rc;
  if ((rc = replay_setup(d, flanks, n_padded, n_padded, n_families, p, true, k, KW)) != RAMX_OK) return rc;
  if (cols && (rc = ensure(&d->d_pl_cols, &d->cap_pl_cols, (size_t)n_families * p->L * sizeof(ramx_col_pileup)))) return rc;
  return aln_args(d, k, p->L, aa);
}

// one replay of the plan's families along cons / rows: forward, walk and pileup per group of tiles, then the sum; on return
// the stream is idle, d_pl_cols holds the families' columns and d_al_ends their flanks' records.  pl.tiles > 0, pl.maxrows > 0.
// With cs (ramx_dev_copy_stats; its stats and reversed set by the caller) the third stage is the per-copy statistics kernel
// instead: it reads the same group's columns, needs no per-tile records and no sum, and leaves cs->stats filled.
// With lk (ramx_dev_planes; its planes and fam_base set by the caller, the buffer zeroed) a fourth stage follows the pileup's:
// the group's bit planes, written into the buffer of the whole flank set.
// With dn (ramx_dev_dinuc / ramx_dev_refine_cpg) a fourth stage follows the pileup's as well: the row-pair records of the group's
// tiles (ramx_kernels_dinuc.h) and, after the last group, their sum into d_dn_cols; pile == false leaves the pileup's stage
// empty (its mark stays, so that the fourth time is the fourth stage's).
static int pileup_replay(ramx_dev *d, const char *who, AlnArgs aa, int KW, const ReplayPlan &pl, int32_t n_families,
                         const int8_t *cons, const int32_t *rows, double *kernel_ms, const CopyStatsArgs *cs = NULL,
                         const PlanesArgs *lk = NULL, bool dn = false, bool pile = true)
{
  const int tiles = pl.tiles, maxrows = pl.maxrows, L = aa.L, W = aa.k.W;
  // the budget counts, per tile, the decision codes and the walked columns (col_idx, col_ins) of its 64 flanks: the columns
  // exist for one group at a time
  const size_t code_bytes = (size_t)maxrows * aa.nd * 64 * sizeof(unsigned), col_bytes = (size_t)maxrows * 64 * sizeof(int);
  int group, rc;
  if ((rc = tile_group(who, "RAMX_ALIGN_BYTES", "decision codes and columns of one tile of 64 flanks", tiles, code_bytes + 2 * col_bytes, &group)) != RAMX_OK)
    return rc;
  if ((rc = ensure(&d->d_al_codes, &d->cap_al_codes, (size_t)group * code_bytes))) return rc;
  if ((rc = ensure(&d->d_pl_idx, &d->cap_pl_idx, (size_t)group * col_bytes))) return rc;
  if ((rc = ensure(&d->d_pl_ins, &d->cap_pl_ins, (size_t)group * col_bytes))) return rc;
  if (!cs && pile && (rc = ensure(&d->d_pl_slab, &d->cap_pl_slab, (size_t)tiles * maxrows * sizeof(ramx_col_pileup)))) return rc;
  if (dn && (rc = ensure(&d->d_dn_slab, &d->cap_dn_slab, (size_t)tiles * maxrows * sizeof(ramx_col_dinuc)))) return rc;
  if ((rc = replay_upload(d, pl, n_families, L, cons, rows)) != RAMX_OK) return rc;
  const int gn = group * 64;
  aa.codes = d->d_al_codes; aa.gn = gn;
  CopyStatsArgs ca;
  memset(&ca, 0, sizeof(ca));
  if (cs)
  {
    ca = *cs;
    ca.bases = d->d_bases; ca.tile_fam = d->d_rp_tile; ca.cons = d->d_rp_cons; ca.rows = d->d_rp_rows; ca.ends = d->d_al_ends;
    ca.col_idx = d->d_pl_idx; ca.col_ins = d->d_pl_ins;
    ca.L = L; ca.Np = aa.k.Np; ca.W = W; ca.KW = KW; ca.gn = gn;
  }
  PlanesArgs la;
  memset(&la, 0, sizeof(la));
  if (lk)
  {
    la = *lk;
    la.bases = d->d_bases; la.tile_fam = d->d_rp_tile; la.fam = d->d_rp_fam; la.rows = d->d_rp_rows; la.ends = d->d_al_ends;
    la.col_idx = d->d_pl_idx; la.col_ins = d->d_pl_ins;
    la.Np = aa.k.Np; la.W = W; la.KW = KW; la.gn = gn;
  }
  PileArgs pa;
  pa.bases = d->d_bases; pa.tile_fam = d->d_rp_tile; pa.cons = d->d_rp_cons; pa.rows = d->d_rp_rows; pa.ends = d->d_al_ends;
  pa.col_idx = d->d_pl_idx; pa.col_ins = d->d_pl_ins; pa.slab = d->d_pl_slab;
  pa.L = L; pa.Np = aa.k.Np; pa.W = W; pa.KW = KW; pa.gn = gn; pa.slab_rows = maxrows;
  PileSumArgs sa;
  sa.slab = d->d_pl_slab; sa.fam = d->d_rp_fam; sa.cons = d->d_rp_cons; sa.cols = d->d_pl_cols; sa.L = L; sa.slab_rows = maxrows;
  DinucArgs da;
  da.bases = d->d_bases; da.tile_fam = d->d_rp_tile; da.cons = d->d_rp_cons; da.rows = d->d_rp_rows; da.ends = d->d_al_ends;
  da.col_idx = d->d_pl_idx; da.col_ins = d->d_pl_ins; da.slab = d->d_dn_slab;
  da.L = L; da.Np = aa.k.Np; da.W = W; da.KW = KW; da.gn = gn; da.tile0 = 0; da.slab_rows = maxrows;
  DinucSumArgs ds;
  ds.slab = d->d_dn_slab; ds.fam = d->d_rp_fam; ds.cons = d->d_rp_cons; ds.di = d->d_dn_cols; ds.L = L; ds.slab_rows = maxrows;
  return tile_groups(d, who, tiles, group, lk || dn ? 4 : 3, kernel_ms, false, [&](int tile0, int nt, auto &mark) {
    int lrc;
    aa.tile0 = pa.tile0 = da.tile0 = tile0;
    mark();
    // the walk addresses its columns as [r * k.Np + n] with n the flank's index in the whole set: given the group's width for
    // k.Np and the arrays' origin moved back by the group's first flank, it writes the group's own [maxrows][gn] arrays
    AlnArgs aw = aa;
    aw.k.Np = gn;
    aw.col_idx = d->d_pl_idx - (ptrdiff_t)tile0 * 64; aw.col_ins = d->d_pl_ins - (ptrdiff_t)tile0 * 64;
    if ((lrc = ramx_align_launch_forward(d->stream, nt, aa)) != RAMX_OK) return lrc;
    mark();
    if ((lrc = ramx_align_launch_preset(d->stream, d->d_pl_idx, d->d_pl_ins, (size_t)maxrows * gn)) != RAMX_OK) return lrc;     // per group
    if ((lrc = ramx_align_launch_walk(d->stream, nt, aw)) != RAMX_OK) return lrc;
    mark();
    if (cs)
    {
      ca.tile0 = tile0;
      if ((lrc = ramx_copystats_launch(d->stream, nt, ca)) != RAMX_OK) return lrc;
      mark();
      return RAMX_OK;
    }
    if (pile && (lrc = ramx_pileup_launch(d->stream, nt, pa)) != RAMX_OK) return lrc;
    // the last group's pileup stage ends with the sum over the tiles of every family
    if (pile && tile0 + nt == tiles && (lrc = ramx_pileup_launch_sum(d->stream, n_families, maxrows, sa)) != RAMX_OK) return lrc;
    mark();
    if (dn)
    {
      if ((lrc = ramx_dinuc_launch(d->stream, nt, da)) != RAMX_OK) return lrc;
      if (tile0 + nt == tiles && (lrc = ramx_dinuc_launch_sum(d->stream, n_families, maxrows, ds)) != RAMX_OK) return lrc;
      mark();
    }
    if (lk)
    {
      la.tile0 = tile0;
      if ((lrc = ramx_planes_launch(d->stream, nt, la)) != RAMX_OK) return lrc;
      mark();
    }
    return RAMX_OK;
  });
}

// the columns and flank records of the families with run[f] != 0 (NULL: all) after a replay, or answered here where nothing ran
static int pileup_fetch(ramx_dev *d, bool ran, int32_t n_padded, const int32_t *fam_first, const int32_t *fam_count, int32_t n_families,
                        int L, const int8_t *cons, const int32_t *rows, const char *run, ramx_col_pileup *cols, ramx_aln_end *ends)
{
  for (int f = 0; f < n_families; f++)
  {
    if (run && !run[f]) continue;
    const int t0 = fam_first[f] / 64, nt = (fam_count[f] + 63) / 64;
    if (rows[f] > 0 && cols)               // (cols is optional for ramx_dev_dinuc alone)
    {
      ramx_col_pileup *c = cols + (size_t)f * L;
      if (ran) HIPCHK(hipMemcpy(c, d->d_pl_cols + (size_t)f * L, (size_t)rows[f] * sizeof(ramx_col_pileup), hipMemcpyDeviceToHost));
      else
      {
        memset(c, 0, (size_t)rows[f] * sizeof(ramx_col_pileup));
        for (int r = 0; r < rows[f]; r++) c[r].base = cons[(size_t)f * L + r];
      }
    }
    if (!ends || nt == 0) continue;        // ends is optional here
    if (!ran || rows[f] == 0) replay_no_alignment(ends, NULL, NULL, t0 * 64, (t0 + nt) * 64, 0, n_padded);
    else HIPCHK(hipMemcpy(ends + (size_t)t0 * 64, d->d_al_ends + (size_t)t0 * 64, (size_t)nt * 64 * sizeof(ramx_aln_end), hipMemcpyDeviceToHost));
  }
  return RAMX_OK;
}

// the row-pair records of the families with run[f] != 0 (NULL: all) after a replay with dn, or answered here where nothing ran
static int dinuc_fetch(ramx_dev *d, bool ran, int32_t n_families, int L, const int8_t *cons, const int32_t *rows, const char *run,
                       ramx_col_dinuc *di)
{
  for (int f = 0; f < n_families; f++)
  {
    if ((run && !run[f]) || rows[f] <= 0) continue;
    ramx_col_dinuc *c = di + (size_t)f * L;
    if (ran) HIPCHK(hipMemcpy(c, d->d_dn_cols + (size_t)f * L, (size_t)rows[f] * sizeof(ramx_col_dinuc), hipMemcpyDeviceToHost));
    else
    {
      memset(c, 0, (size_t)rows[f] * sizeof(ramx_col_dinuc));
      for (int r = 0; r < rows[f]; r++) { c[r].base = cons[(size_t)f * L + r]; c[r].next = r + 1 < rows[f] ? cons[(size_t)f * L + r + 1] : -1; }
    }
  }
  return RAMX_OK;
}

extern "C" int ramx_dev_pileup(ramx_dev *d, const ramx_flank *flanks, int32_t n_padded, const int32_t *fam_first,
                               const int32_t *fam_count, int32_t n_families, const ramx_params *p,
                               const int8_t *cons, const int32_t *rows, ramx_col_pileup *cols, ramx_aln_end *ends, double *kernel_ms)
{
  if (kernel_ms) kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = 0;
  if (!d || !p || !p->matrix || n_families < 0 || n_padded < 0 || (n_padded & 63) || (n_padded && !flanks) ||
      (n_families && (!fam_first || !fam_count || !rows)))
  { ramx_set_error("ramx_dev_pileup: bad argument"); return RAMX_ERR_ARG; }
  if (p->bandwidth < 1 || p->L < 0) { ramx_set_error("ramx_dev_pileup: bad bandwidth / L"); return RAMX_ERR_ARG; }
  ReplayPlan pl;
  int rc;
  if ((rc = replay_plan("ramx_dev_pileup", n_padded, fam_first, fam_count, n_families, p->L, cons, rows, NULL, true, pl)) != RAMX_OK) return rc;
  if (pl.maxrows > 0 && !cols) { ramx_set_error("ramx_dev_pileup: cols missing"); return RAMX_ERR_ARG; }
  const bool run = n_families > 0 && pl.maxrows > 0 && pl.tiles > 0;
  if (run)
  {
    AlnArgs aa;
    int KW = 0;
    if ((rc = pileup_setup(d, flanks, n_padded, n_families, p, aa, &KW)) != RAMX_OK) return rc;
    if ((rc = pileup_replay(d, "ramx_dev_pileup", aa, KW, pl, n_families, cons, rows, kernel_ms)) != RAMX_OK) return rc;
  }
  return pileup_fetch(d, run, n_padded, fam_first, fam_count, n_families, p->L, cons, rows, NULL, cols, ends);
}

// ------------------------------------------------------------------------------------------
// dinucleotide pileup: the pileup's replay with the row-pair kernel as a fourth stage (ramx_kernels_dinuc.h)
// ------------------------------------------------------------------------------------------
extern "C" int ramx_dev_dinuc(ramx_dev *d, const ramx_flank *flanks, int32_t n_padded, const int32_t *fam_first,
                              const int32_t *fam_count, int32_t n_families, const ramx_params *p,
                              const int8_t *cons, const int32_t *rows, ramx_col_pileup *cols, ramx_col_dinuc *di, ramx_aln_end *ends,
                              double *kernel_ms)
{
  if (kernel_ms) kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = kernel_ms[3] = 0;
  if (!d || !p || !p->matrix || n_families < 0 || n_padded < 0 || (n_padded & 63) || (n_padded && !flanks) ||
      (n_families && (!fam_first || !fam_count || !rows)))
  { ramx_set_error("ramx_dev_dinuc: bad argument"); return RAMX_ERR_ARG; }
  if (p->bandwidth < 1 || p->L < 0) { ramx_set_error("ramx_dev_dinuc: bad bandwidth / L"); return RAMX_ERR_ARG; }
  ReplayPlan pl;
  int rc;
  if ((rc = replay_plan("ramx_dev_dinuc", n_padded, fam_first, fam_count, n_families, p->L, cons, rows, NULL, true, pl)) != RAMX_OK) return rc;
  if (pl.maxrows > 0 && !di) { ramx_set_error("ramx_dev_dinuc: di missing"); return RAMX_ERR_ARG; }
  const bool run = n_families > 0 && pl.maxrows > 0 && pl.tiles > 0;
  if (run)
  {
    AlnArgs aa;
    int KW = 0;
    if ((rc = pileup_setup(d, flanks, n_padded, n_families, p, aa, &KW, cols != NULL)) != RAMX_OK) return rc;
    if ((rc = ensure(&d->d_dn_cols, &d->cap_dn_cols, (size_t)n_families * p->L * sizeof(ramx_col_dinuc)))) return rc;
    if ((rc = pileup_replay(d, "ramx_dev_dinuc", aa, KW, pl, n_families, cons, rows, kernel_ms, NULL, NULL, true, cols != NULL)) != RAMX_OK) return rc;
    if (!cols && kernel_ms) kernel_ms[2] = 0;          // (two marks with nothing between them)
  }
  if ((rc = dinuc_fetch(d, run, n_families, p->L, cons, rows, NULL, di)) != RAMX_OK) return rc;
  return pileup_fetch(d, run, n_padded, fam_first, fam_count, n_families, p->L, cons, rows, NULL, cols, ends);
}

// ------------------------------------------------------------------------------------------
// per-copy statistics: the pileup's replay with the statistics kernel as its third stage (ramx_kernels_copystats.h)
// ------------------------------------------------------------------------------------------
extern "C" int ramx_dev_copy_stats(ramx_dev *d, const ramx_flank *flanks, int32_t n_padded, const int32_t *fam_first,
                                   const int32_t *fam_count, int32_t n_families, const ramx_params *p,
                                   const int8_t *cons, const int32_t *rows, int32_t rows_reversed,
                                   ramx_copy_stats *stats, ramx_aln_end *ends, double *kernel_ms)
{
  if (kernel_ms) kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = 0;
  // the records are the result: stats is required wherever there are flanks
  if (!d || !p || !p->matrix || n_families < 0 || n_padded < 0 || (n_padded & 63) || (n_padded && (!flanks || !stats)) ||
      (n_families && (!fam_first || !fam_count || !rows)))
  { ramx_set_error("ramx_dev_copy_stats: bad argument"); return RAMX_ERR_ARG; }
  if (p->bandwidth < 1 || p->L < 0) { ramx_set_error("ramx_dev_copy_stats: bad bandwidth / L"); return RAMX_ERR_ARG; }
  ReplayPlan pl;
  int rc;
  if ((rc = replay_plan("ramx_dev_copy_stats", n_padded, fam_first, fam_count, n_families, p->L, cons, rows, NULL, true, pl)) != RAMX_OK) return rc;
  const bool run = n_families > 0 && pl.maxrows > 0 && pl.tiles > 0;
  if (run)
  {
    AlnArgs aa;
    int KW = 0;
    if ((rc = pileup_setup(d, flanks, n_padded, n_families, p, aa, &KW, false)) != RAMX_OK) return rc;
    if ((rc = ensure(&d->d_cs_stats, &d->cap_cs_stats, (size_t)n_padded * sizeof(ramx_copy_stats)))) return rc;
    CopyStatsArgs cs;
    memset(&cs, 0, sizeof(cs));
    cs.stats = d->d_cs_stats; cs.reversed = rows_reversed != 0;
    if ((rc = pileup_replay(d, "ramx_dev_copy_stats", aa, KW, pl, n_families, cons, rows, kernel_ms, &cs)) != RAMX_OK) return rc;
  }
  // the tiles of every family, copied back per family; tiles outside every family keep what the caller has there
  for (int f = 0; f < n_families; f++)
  {
    const int t0 = fam_first[f] / 64, nt = (fam_count[f] + 63) / 64;
    if (nt == 0) continue;
    if (!run || rows[f] == 0)
    {
      memset(stats + (size_t)t0 * 64, 0, (size_t)nt * 64 * sizeof(ramx_copy_stats));
      replay_no_alignment(ends, NULL, NULL, t0 * 64, (t0 + nt) * 64, 0, n_padded);
      continue;
    }
    HIPCHK(hipMemcpy(stats + (size_t)t0 * 64, d->d_cs_stats + (size_t)t0 * 64, (size_t)nt * 64 * sizeof(ramx_copy_stats), hipMemcpyDeviceToHost));
    if (ends) HIPCHK(hipMemcpy(ends + (size_t)t0 * 64, d->d_al_ends + (size_t)t0 * 64, (size_t)nt * 64 * sizeof(ramx_aln_end), hipMemcpyDeviceToHost));
  }
  return RAMX_OK;
}

// ------------------------------------------------------------------------------------------
// the site-window analyses (target-site duplications, tandem periodicity, terminal repeats): sites or segments become windows
// clipped to their bounds, the windows are packed as flanks into the direction's own buffers, tile group after tile group, and
// one or two small kernels run over the packed windows
// ------------------------------------------------------------------------------------------
// The window of positions start + step * t, t = t_first .. t_last, as a flank: cut to the t whose position lies inside
// bound_lo..bound_hi, or the empty window t_lo = 1, t_hi = 0 where there is none (no base is read: the padding lanes of a tile
// are this one).  This is what keeps a batch's copies from reading a neighbouring family's bases in the concatenated library.
// Positions and bounds lie within +-RAMX_TSD_POS_MAX (checked before the first call) and |t| < 2^31: no difference overflows.
static void window_flank(ramx_flank &f, long long start, int step, bool compl_, long long t_first, long long t_last,
                         long long bound_lo, long long bound_hi)
{
  memset(&f, 0, sizeof(f));
  f.start = start; f.step = (int8_t)step; f.compl_ = compl_;
  const long long t_in = step > 0 ? bound_lo - start : start - bound_hi, t_out = step > 0 ? bound_hi - start : start - bound_lo;
  const long long a = t_in > t_first ? t_in : t_first, b = t_out < t_last ? t_out : t_last;
  if (a > b) { f.t_lo = 1; f.t_hi = 0; } else { f.t_lo = (int32_t)a; f.t_hi = (int32_t)b; }
}

static const ramx_tsd_site NO_SITE = { 0, -1, 0, -1 };         // the padding of a tile: an empty site in empty bounds

// the sites of ramx_dev_tsd and ramx_dev_term: seq_lo <= lo <= hi + 1, hi <= seq_hi, everything within +-RAMX_TSD_POS_MAX
static int check_sites(const char *who, const ramx_tsd_site *sites, int32_t n_sites)
{
  for (int i = 0; i < n_sites; i++)
    if (sites[i].seq_lo < -RAMX_TSD_POS_MAX || sites[i].seq_hi > RAMX_TSD_POS_MAX ||
        sites[i].seq_lo > sites[i].lo || sites[i].lo > sites[i].hi + 1 || sites[i].hi > sites[i].seq_hi)
    { ramx_set_error("%s: site %d: lo %lld hi %lld outside its bounds %lld..%lld, or lo > hi + 1", who, i, (long long)sites[i].lo,
                     (long long)sites[i].hi, (long long)sites[i].seq_lo, (long long)sites[i].seq_hi); return RAMX_ERR_ARG; }
  return RAMX_OK;
}

// the flank and window buffers of the direction are reused, as by the replays: room for `lanes` windows of KW words
static int site_windows_setup(ramx_dev *d, size_t lanes, int KW)
{
  int rc;
  HIPCHK(hipSetDevice(d->ordinal));
  if ((rc = pack_settle(d, true)) != RAMX_OK) return rc;
  if ((rc = ensure(&d->d_flanks, &d->cap_flanks, lanes * sizeof(ramx_flank)))) return rc;
  if ((rc = ensure(&d->d_bases, &d->cap_bases, (size_t)KW * lanes * sizeof(unsigned)))) return rc;
  if ((rc = ensure(&d->d_bounds, &d->cap_bounds, lanes * sizeof(int2)))) return rc;
  d->ready = 0;
  d->planes_ready = 0;
  d->packed_kw = KW;
  return RAMX_OK;
}

// target-site duplications: the two outside windows of every site packed as flanks, then one lane per site (ramx_kernels_tsd.h)
extern "C" int ramx_dev_tsd(ramx_dev *d, const ramx_tsd_site *sites, int32_t n_sites, const ramx_tsd_params *params, ramx_tsd *out,
                            double *kernel_ms)
{
  if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0;
  if (!d || n_sites < 0 || (n_sites && (!sites || !out))) { ramx_set_error("ramx_dev_tsd: bad argument"); return RAMX_ERR_ARG; }
  int rc;
  if ((rc = ramx_tsd_check_params(params)) != RAMX_OK) return rc;
  if ((rc = check_sites("ramx_dev_tsd", sites, n_sites)) != RAMX_OK) return rc;
  if (n_sites == 0) return RAMX_OK;
  if (n_sites > (1 << 29)) { ramx_set_error("ramx_dev_tsd: more than 2^29 sites in one call"); return RAMX_ERR_UNSUPPORTED; }
  const int n = n_sites, Np = (n + 63) & ~63, S = params->slack, t_last = params->kmax + S - 1;
  if ((rc = site_windows_setup(d, (size_t)2 * Np, RAMX_TSD_KW)) != RAMX_OK) return rc;
  if ((rc = ensure(&d->d_tsd_room, &d->cap_tsd_room, (size_t)Np * sizeof(int)))) return rc;
  if ((rc = ensure(&d->d_tsd_out, &d->cap_tsd_out, (size_t)Np * sizeof(ramx_tsd)))) return rc;
  // the windows: the left one runs down from lo - 1, the right one up from hi + 1, t = -slack .. kmax + slack - 1; the left
  // windows of all (padded) sites first, then the right ones
  // (every lane is written below: nothing is zeroed first)
  std::unique_ptr<ramx_flank[]> fl(new ramx_flank[(size_t)2 * Np]);
  std::unique_ptr<int[]> room(new int[(size_t)Np]);
  for (int i = 0; i < Np; i++)
  {
    const ramx_tsd_site &s = i < n ? sites[i] : NO_SITE;
    window_flank(fl[(size_t)i], s.lo - 1, -1, false, -S, t_last, s.seq_lo, s.seq_hi);
    window_flank(fl[(size_t)Np + i], s.hi + 1, 1, false, -S, t_last, s.seq_lo, s.seq_hi);
    room[(size_t)i] = s.hi + 1 - s.lo < 64 ? (int)(s.hi + 1 - s.lo) : 64;
  }
  TsdArgs ta;
  ta.bases = d->d_bases; ta.room = d->d_tsd_room; ta.out = d->d_tsd_out; ta.n = n; ta.Np = Np;
  ta.slack = S; ta.kmin = params->kmin; ta.kmax = params->kmax; ta.mm_div = params->mm_div;
  // one group of all the tiles
  return tile_groups(d, "ramx_dev_tsd", Np / 64, Np / 64, 2, kernel_ms, true, [&](int, int, auto &mark) {
    int lrc;
    HIPCHK(hipMemcpyAsync(d->d_flanks, fl.get(), (size_t)2 * Np * sizeof(ramx_flank), hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipMemcpyAsync(d->d_tsd_room, room.get(), (size_t)Np * sizeof(int), hipMemcpyHostToDevice, d->stream));
    mark();
    if ((lrc = launch_pack(d, 2 * Np, 2 * Np, RAMX_TSD_W, 0, RAMX_TSD_KW, d->stream)) != RAMX_OK) return lrc;
    mark();
    if ((lrc = ramx_tsd_launch(d->stream, ta)) != RAMX_OK) return lrc;
    mark();
    HIPCHK(hipMemcpyAsync(out, d->d_tsd_out, (size_t)n * sizeof(ramx_tsd), hipMemcpyDeviceToHost, d->stream));
    return RAMX_OK;
  });
}

// tandem periodicity: every segment packed as a flank, squeezed into a stream of its own, then one workgroup per segment and a
// lane per period (ramx_kernels_period.h)
extern "C" int ramx_dev_period_bounded(ramx_dev *d, const ramx_period_seg *segs, const ramx_period_seg *bounds, int32_t n_segs,
                                       const ramx_period_params *params, ramx_period *out, double *kernel_ms)
{
  if (kernel_ms) kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = 0;
  if (!d || n_segs < 0 || (n_segs && (!segs || !out))) { ramx_set_error("ramx_dev_period: bad argument"); return RAMX_ERR_ARG; }
  int rc;
  if ((rc = ramx_period_check_params(params)) != RAMX_OK) return rc;
  long long nmax = 0;
  for (int i = 0; i < n_segs; i++)
  {
    if (segs[i].lo < -RAMX_TSD_POS_MAX || segs[i].hi > RAMX_TSD_POS_MAX || segs[i].lo > segs[i].hi + 1)
    { ramx_set_error("ramx_dev_period: segment %d: lo %lld hi %lld: lo > hi + 1, or out of range", i, (long long)segs[i].lo, (long long)segs[i].hi); return RAMX_ERR_ARG; }
    if (bounds && (bounds[i].lo < -RAMX_TSD_POS_MAX || bounds[i].hi > RAMX_TSD_POS_MAX))
    { ramx_set_error("ramx_dev_period: segment %d: bounds out of range", i); return RAMX_ERR_ARG; }
    const long long len = (long long)(segs[i].hi + 1 - segs[i].lo);
    if (len > nmax) nmax = len;
  }
  if (nmax > RAMX_PERIOD_LEN_MAX)
  { ramx_set_error("ramx_dev_period: a segment of %lld bases, at most %d", nmax, RAMX_PERIOD_LEN_MAX); return RAMX_ERR_UNSUPPORTED; }
  if (n_segs == 0) return RAMX_OK;
  if (n_segs > (1 << 29)) { ramx_set_error("ramx_dev_period: more than 2^29 segments in one call"); return RAMX_ERR_UNSUPPORTED; }
  // the windows and streams of one tile of 64 segments, at the length of the call's longest segment
  const int KW = period_window_words((int)nmax), SW = period_stream_words((int)nmax) > 0 ? period_stream_words((int)nmax) : 1;
  const size_t tile_bytes = (size_t)64 * ((size_t)KW * sizeof(unsigned) + (size_t)SW * (sizeof(unsigned long long) + sizeof(unsigned)));
  const int tiles = (n_segs + 63) / 64;
  int group;
  if ((rc = tile_group("ramx_dev_period", "RAMX_PERIOD_BYTES", "windows and streams of one tile of 64 segments", tiles, tile_bytes, &group)) != RAMX_OK)
    return rc;
  const size_t Gp = (size_t)group * 64;
  if ((rc = site_windows_setup(d, Gp, KW)) != RAMX_OK) return rc;
  if ((rc = ensure(&d->d_per_bases, &d->cap_per_bases, Gp * SW * sizeof(unsigned long long)))) return rc;
  if ((rc = ensure(&d->d_per_valid, &d->cap_per_valid, Gp * SW * sizeof(unsigned)))) return rc;
  if ((rc = ensure(&d->d_per_len, &d->cap_per_len, Gp * sizeof(int)))) return rc;
  if ((rc = ensure(&d->d_per_out, &d->cap_per_out, Gp * sizeof(ramx_period)))) return rc;
  // (a group writes every lane it sends: nothing is zeroed first)
  std::unique_ptr<ramx_flank[]> fl(new ramx_flank[Gp]);
  std::unique_ptr<int[]> len(new int[Gp]);
  PeriodArgs pa;
  pa.win = d->d_bases; pa.bases = d->d_per_bases; pa.valid = d->d_per_valid; pa.len = d->d_per_len; pa.out = d->d_per_out;
  pa.KW = KW; pa.SW = SW;
  pa.pmax = params->pmax; pa.mm = params->mm; pa.min_score = params->min_score;
  return tile_groups(d, "ramx_dev_period", tiles, group, 3, kernel_ms, true, [&](int tile0, int nt, auto &mark) {
    const int Np = nt * 64, s0 = tile0 * 64, n = n_segs - s0 < Np ? n_segs - s0 : Np;
    int lrc;
    // the window of a segment: all of it, or with bounds what of it lies inside them; its length stays the segment's
    // (the arrays through pointers of the loop's own: the flanks' byte stores would have the captured ones read again per lane)
    const ramx_period_seg none = { 0, -1 }, all = { -RAMX_TSD_POS_MAX, RAMX_TSD_POS_MAX };
    const ramx_period_seg *const sg = segs + s0, *const bd = bounds ? bounds + s0 : NULL;
    ramx_flank *const f = fl.get();
    int *const ln = len.get();
    for (int i = 0; i < Np; i++)
    {
      const ramx_period_seg &s = i < n ? sg[i] : none, &b = i < n && bd ? bd[i] : all;
      window_flank(f[i], s.lo, 1, false, 0, (long long)(s.hi - s.lo), b.lo, b.hi);
      ln[i] = (int)(s.hi + 1 - s.lo);
    }
    HIPCHK(hipMemcpyAsync(d->d_flanks, f, (size_t)Np * sizeof(ramx_flank), hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipMemcpyAsync(d->d_per_len, ln, (size_t)Np * sizeof(int), hipMemcpyHostToDevice, d->stream));
    mark();
    if ((lrc = launch_pack(d, Np, Np, RAMX_PERIOD_W, 0, KW, d->stream)) != RAMX_OK) return lrc;
    mark();
    pa.n = n; pa.Np = Np;
    if ((lrc = ramx_period_squeeze_launch(d->stream, pa)) != RAMX_OK) return lrc;
    mark();
    if ((lrc = ramx_period_scan_launch(d->stream, pa)) != RAMX_OK) return lrc;
    mark();
    HIPCHK(hipMemcpyAsync(out + s0, d->d_per_out, (size_t)n * sizeof(ramx_period), hipMemcpyDeviceToHost, d->stream));
    return RAMX_OK;      // (the next group writes the host and device buffers of this one again: host_reuse)
  });
}

extern "C" int ramx_dev_period(ramx_dev *d, const ramx_period_seg *segs, int32_t n_segs, const ramx_period_params *params, ramx_period *out,
                               double *kernel_ms)
{
  return ramx_dev_period_bounded(d, segs, NULL, n_segs, params, out, kernel_ms);
}

// terminal repeats: the three windows of every site packed as flanks and squeezed into streams by the period's kernel, then one
// wave per (site, orientation) (ramx_kernels_term.h)
extern "C" int ramx_dev_term(ramx_dev *d, const ramx_tsd_site *sites, int32_t n_sites, const ramx_term_params *params, ramx_term *out,
                             double *kernel_ms)
{
  if (kernel_ms) kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = 0;
  if (!d || n_sites < 0 || (n_sites && (!sites || !out))) { ramx_set_error("ramx_dev_term: bad argument"); return RAMX_ERR_ARG; }
  int rc;
  if ((rc = ramx_term_check_params(params)) != RAMX_OK) return rc;
  if ((rc = check_sites("ramx_dev_term", sites, n_sites)) != RAMX_OK) return rc;
  // the length of a site's windows: half the site, at most tmax
  auto window_len = [](const ramx_tsd_site &s, int tmax) {
    const long long half = (long long)(s.hi + 1 - s.lo) / 2;
    return (int)(half < tmax ? half : tmax);
  };
  int Tmax = 0;
  for (int i = 0; i < n_sites; i++) if (window_len(sites[i], params->tmax) > Tmax) Tmax = window_len(sites[i], params->tmax);
  if (n_sites == 0) return RAMX_OK;
  if (n_sites > (1 << 29)) { ramx_set_error("ramx_dev_term: more than 2^29 sites in one call"); return RAMX_ERR_UNSUPPORTED; }
  // the three windows and streams of one tile of 64 sites, at the length of the call's longest window
  const int KW = period_window_words(Tmax), SW = period_stream_words(Tmax) > 0 ? period_stream_words(Tmax) : 1;
  const size_t tile_bytes = (size_t)3 * 64 * ((size_t)KW * sizeof(unsigned) + (size_t)SW * (sizeof(unsigned long long) + sizeof(unsigned)));
  const int tiles = (n_sites + 63) / 64;
  int group;
  if ((rc = tile_group("ramx_dev_term", "RAMX_TERM_BYTES", "windows and streams of one tile of 64 sites", tiles, tile_bytes, &group)) != RAMX_OK) return rc;
  const size_t Gp = (size_t)group * 64;
  if ((rc = site_windows_setup(d, 3 * Gp, KW)) != RAMX_OK) return rc;
  if ((rc = ensure(&d->d_per_bases, &d->cap_per_bases, 3 * Gp * SW * sizeof(unsigned long long)))) return rc;
  if ((rc = ensure(&d->d_per_valid, &d->cap_per_valid, 3 * Gp * SW * sizeof(unsigned)))) return rc;
  if ((rc = ensure(&d->d_per_len, &d->cap_per_len, Gp * sizeof(int)))) return rc;
  if ((rc = ensure(&d->d_term_out, &d->cap_term_out, 2 * Gp * sizeof(ramx_term)))) return rc;
  // (a group writes every lane it sends: nothing is zeroed first)
  std::unique_ptr<ramx_flank[]> fl(new ramx_flank[3 * Gp]);
  std::unique_ptr<int[]> len(new int[Gp]);
  PeriodArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.win = d->d_bases; pa.bases = d->d_per_bases; pa.valid = d->d_per_valid; pa.len = d->d_per_len;
  pa.KW = KW; pa.SW = SW;
  TermArgs ta;
  ta.bases = d->d_per_bases; ta.valid = d->d_per_valid; ta.T = d->d_per_len; ta.out = d->d_term_out; ta.SW = SW;
  ta.match = params->match; ta.mismatch = params->mismatch; ta.gap = params->gap; ta.min_score = params->min_score;
  return tile_groups(d, "ramx_dev_term", tiles, group, 3, kernel_ms, true, [&](int tile0, int nt, auto &mark) {
    const int Np = nt * 64, s0 = tile0 * 64, n = n_sites - s0 < Np ? n_sites - s0 : Np;
    int lrc, Tgroup = 0;
    // the windows of T bases: the 5' one up from lo, the 3' one up from hi + 1 - T, and the 3' one down from hi, complemented;
    // the first of all (padded) sites first, then the second, then the third
    // (the arrays through pointers of the loop's own, as in ramx_dev_period_bounded)
    const ramx_tsd_site *const st = sites + s0;
    ramx_flank *const f = fl.get();
    int *const ln = len.get();
    const int tmax = params->tmax;
    for (int i = 0; i < Np; i++)
    {
      const ramx_tsd_site &s = i < n ? st[i] : NO_SITE;
      const int T = window_len(s, tmax);
      window_flank(f[i], s.lo, 1, false, 0, T - 1, s.seq_lo, s.seq_hi);
      window_flank(f[(size_t)Np + i], s.hi + 1 - T, 1, false, 0, T - 1, s.seq_lo, s.seq_hi);
      window_flank(f[(size_t)2 * Np + i], s.hi, -1, true, 0, T - 1, s.seq_lo, s.seq_hi);
      ln[i] = T;
      if (T > Tgroup) Tgroup = T;
    }
    HIPCHK(hipMemcpyAsync(d->d_flanks, f, (size_t)3 * Np * sizeof(ramx_flank), hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipMemcpyAsync(d->d_per_len, ln, (size_t)Np * sizeof(int), hipMemcpyHostToDevice, d->stream));
    mark();
    if ((lrc = launch_pack(d, 3 * Np, 3 * Np, RAMX_PERIOD_W, 0, KW, d->stream)) != RAMX_OK) return lrc;
    mark();
    pa.n = 3 * Np; pa.Np = 3 * Np;
    if ((lrc = ramx_period_squeeze_launch(d->stream, pa)) != RAMX_OK) return lrc;
    mark();
    ta.n = n; ta.Np = Np;
    if ((lrc = ramx_term_align_launch(d->stream, ta, Tgroup)) != RAMX_OK) return lrc;
    mark();
    HIPCHK(hipMemcpyAsync(out + (size_t)2 * s0, d->d_term_out, (size_t)2 * n * sizeof(ramx_term), hipMemcpyDeviceToHost, d->stream));
    return RAMX_OK;      // (the next group writes the host and device buffers of this one again: host_reuse)
  });
}

// ------------------------------------------------------------------------------------------
// cross-family overlap (include/ramx_xfam.h): pairs of sequences of any two lengths, one wave a pair (ramx_kernels_xfam.h)
// ------------------------------------------------------------------------------------------
// what a pair adds to its group: its strip border, its descriptor and its record; and what a sequence adds
static size_t xfam_pair_bytes(long long na) { return (size_t)16 * (size_t)na + sizeof(XfamPair) + sizeof(ramx_term) + 8; }
static size_t xfam_seq_bytes(long long n) { return ((size_t)n + 15) & ~(size_t)15; }
static_assert(sizeof(XfamPair) + sizeof(ramx_term) + 8 == 80, "the 80 bytes a pair of include/ramx_xfam.h");

extern "C" int ramx_dev_seq_pairs(ramx_dev *d, const int8_t *codes, const int64_t *seq_off, int32_t n_seqs, const ramx_seq_pair *pairs,
                                  int32_t n_pairs, const ramx_pair_params *pp, ramx_term *out, double *kernel_ms)
{
  if (kernel_ms) *kernel_ms = 0;
  int rc;
  if ((rc = ramx_pair_check_params(pp)) != RAMX_OK) return rc;
  if (n_seqs < 0 || n_pairs < 0 || !seq_off || (n_pairs && (!pairs || !out)))
  { ramx_set_error("ramx_dev_seq_pairs: bad argument"); return RAMX_ERR_ARG; }
  for (int s = 0; s < n_seqs; s++)
    if (seq_off[s] < 0 || seq_off[s + 1] < seq_off[s] || (seq_off[s + 1] > seq_off[s] && !codes))
    { ramx_set_error("ramx_dev_seq_pairs: seq_off decreases at sequence %d, or codes missing", s); return RAMX_ERR_ARG; }
  for (int p = 0; p < n_pairs; p++)
    if (pairs[p].a < 0 || pairs[p].a >= n_seqs || pairs[p].b < 0 || pairs[p].b >= n_seqs || pairs[p].a == pairs[p].b ||
        pairs[p].inverted < 0 || pairs[p].inverted > 1 || pairs[p].reserved)
    { ramx_set_error("ramx_dev_seq_pairs: pair %d: a %d b %d (two different sequences of 0..%d), inverted %d (0, 1), reserved %d (0)", p,
                     pairs[p].a, pairs[p].b, n_seqs - 1, pairs[p].inverted, pairs[p].reserved); return RAMX_ERR_ARG; }
  auto len_of = [&](int s) { return (long long)(seq_off[s + 1] - seq_off[s]); };
  for (int p = 0; p < n_pairs; p++)
    if (len_of(pairs[p].a) > RAMX_XFAM_MAXLEN || len_of(pairs[p].b) > RAMX_XFAM_MAXLEN)
    { ramx_set_error("ramx_dev_seq_pairs: pair %d: %lld and %lld bases, at most %d", p, len_of(pairs[p].a), len_of(pairs[p].b), RAMX_XFAM_MAXLEN);
      return RAMX_ERR_UNSUPPORTED; }
  if (n_pairs == 0) return RAMX_OK;
  if (!d) d = ramx_default_device();      // seam 1's process-wide session
  if (!d) return RAMX_ERR_NO_DEVICE;
  size_t budget = (size_t)1 << 30;
  if (const char *e = getenv("RAMX_XFAM_BYTES")) { const long long v = atoll(e); if (v > 0) budget = (size_t)v; }
  int force_cols = 0;                     // RAMX_XFAM_COLS = 4, 8, 16: that specialisation for every pair (the tests' way to each of them)
  if (const char *e = getenv("RAMX_XFAM_COLS")) { const int v = atoi(e); if (v == 4 || v == 8 || v == 16) force_cols = v; }
  // consecutive pairs in groups that fit: a group's sequences once each, and every pair's border, descriptor and record
  auto empty = [&](int p) { return len_of(pairs[p].a) == 0 || len_of(pairs[p].b) == 0; };
  std::vector<int> gfirst;                // the first pair of every group, and n_pairs at the end
  std::vector<int> stamp((size_t)n_seqs, -1);
  size_t need_codes = 0, need_border = 0, need_pairs = 0;
  {
    size_t bytes = 0, cbytes = 0, bbytes = 0;
    int g = 0;
    gfirst.push_back(0);
    for (int p = 0; p < n_pairs; p++)
    {
      if (empty(p)) continue;
      const int sa = pairs[p].a, sb = pairs[p].b;
      auto add_of = [&]() {
        return xfam_pair_bytes(len_of(sa)) + (stamp[(size_t)sa] == g ? 0 : xfam_seq_bytes(len_of(sa))) + (stamp[(size_t)sb] == g ? 0 : xfam_seq_bytes(len_of(sb)));
      };
      if (bytes && bytes + add_of() > budget) { g++; gfirst.push_back(p); bytes = cbytes = bbytes = 0; }
      const size_t add = add_of();
      if (add > budget)
      { ramx_set_error("ramx_dev_seq_pairs: pair %d alone (%zu bytes) does not fit RAMX_XFAM_BYTES = %zu", p, add, budget); return RAMX_ERR_UNSUPPORTED; }
      if (stamp[(size_t)sa] != g) { stamp[(size_t)sa] = g; cbytes += xfam_seq_bytes(len_of(sa)); }
      if (stamp[(size_t)sb] != g) { stamp[(size_t)sb] = g; cbytes += xfam_seq_bytes(len_of(sb)); }
      bytes += add; bbytes += (size_t)16 * (size_t)len_of(sa);
      if (cbytes > need_codes) need_codes = cbytes;
      if (bbytes > need_border) need_border = bbytes;
      if ((size_t)(p + 1 - gfirst.back()) > need_pairs) need_pairs = (size_t)(p + 1 - gfirst.back());
    }
    gfirst.push_back(n_pairs);
    // (a group's records are copied back in one piece, the empty pairs at its end included)
    for (size_t k = 0; k + 1 < gfirst.size(); k++)
      if ((size_t)(gfirst[k + 1] - gfirst[k]) > need_pairs) need_pairs = (size_t)(gfirst[k + 1] - gfirst[k]);
  }
  // self-contained, as the site-window analyses: a direction begun before is over, resident planes are dropped
  HIPCHK(hipSetDevice(d->ordinal));
  if ((rc = pack_settle(d, true)) != RAMX_OK) return rc;
  d->ready = 0;
  d->planes_ready = 0;
  if ((rc = ensure(&d->d_xf_codes, &d->cap_xf_codes, need_codes))) return rc;
  if ((rc = ensure(&d->d_xf_border, &d->cap_xf_border, need_border))) return rc;
  if ((rc = ensure(&d->d_xf_pairs, &d->cap_xf_pairs, need_pairs * sizeof(XfamPair)))) return rc;
  if ((rc = ensure(&d->d_xf_out, &d->cap_xf_out, need_pairs * sizeof(ramx_term)))) return rc;
  std::vector<signed char> hcodes(need_codes ? need_codes : 1);
  std::vector<XfamPair> hpairs(need_pairs ? need_pairs : 1);
  std::vector<long long> where((size_t)n_seqs, 0);
  std::fill(stamp.begin(), stamp.end(), -1);
  XfamArgs xa;
  memset(&xa, 0, sizeof(xa));
  xa.codes = d->d_xf_codes; xa.border = d->d_xf_border; xa.out = d->d_xf_out;
  xa.match = pp->match; xa.mismatch = pp->mismatch; xa.gap = pp->gap; xa.min_score = pp->min_score;
  const int ngroups = (int)gfirst.size() - 1;
  return tile_groups(d, "ramx_dev_seq_pairs", ngroups, 1, 1, kernel_ms, true, [&](int g, int, auto &mark) {
    const int p0 = gfirst[(size_t)g], p1 = gfirst[(size_t)g + 1];
    size_t cat = 0;
    long long bat = 0;
    int m = 0;
    for (int p = p0; p < p1; p++)
    {
      if (empty(p)) { memset(&out[p], 0, sizeof(ramx_term)); continue; }
      const int two[2] = { pairs[p].a, pairs[p].b };
      for (int s : two)
        if (stamp[(size_t)s] != g)
        {
          stamp[(size_t)s] = g; where[(size_t)s] = (long long)cat;
          memcpy(hcodes.data() + cat, codes + seq_off[s], (size_t)len_of(s));
          cat += xfam_seq_bytes(len_of(s));
        }
      XfamPair &x = hpairs[(size_t)m++];
      x.a_off = where[(size_t)two[0]]; x.b_off = where[(size_t)two[1]]; x.border_off = bat;
      x.na = (int)len_of(two[0]); x.nb = (int)len_of(two[1]); x.inverted = pairs[p].inverted; x.out_index = p - p0;
      bat += x.na;                                            // (in records of 16 bytes)
    }
    if (m == 0) { mark(); mark(); return RAMX_OK; }
    // pairs differ by orders of magnitude in cells: by specialisation, then the largest first; the kernel writes a pair's record
    // at its place in the group, whatever its place in the launch
    auto cols_of = [&](const XfamPair &x) { return force_cols ? force_cols : ramx_xfam_cols(x.nb); };
    std::sort(hpairs.begin(), hpairs.begin() + m, [&](const XfamPair &x, const XfamPair &y) {
      const int cx = cols_of(x), cy = cols_of(y);
      if (cx != cy) return cx < cy;
      const long long wx = (long long)x.na * x.nb, wy = (long long)y.na * y.nb;
      return wx != wy ? wx > wy : x.out_index < y.out_index;
    });
    HIPCHK(hipMemcpyAsync(d->d_xf_codes, hcodes.data(), cat, hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipMemcpyAsync(d->d_xf_pairs, hpairs.data(), (size_t)m * sizeof(XfamPair), hipMemcpyHostToDevice, d->stream));
    mark();
    for (int lo = 0; lo < m;)
    {
      int hi = lo, na_max = 0;
      while (hi < m && cols_of(hpairs[(size_t)hi]) == cols_of(hpairs[(size_t)lo])) { if (hpairs[(size_t)hi].na > na_max) na_max = hpairs[(size_t)hi].na; hi++; }
      xa.pairs = d->d_xf_pairs + lo; xa.n = hi - lo;
      const int lrc = ramx_xfam_align_launch(d->stream, xa, cols_of(hpairs[(size_t)lo]), na_max);
      if (lrc != RAMX_OK) return lrc;
      lo = hi;
    }
    mark();
    // (an empty pair's record in between is copied as the device left it and written again below, after the copy)
    HIPCHK(hipMemcpyAsync(out + p0, d->d_xf_out, (size_t)(p1 - p0) * sizeof(ramx_term), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    for (int p = p0; p < p1; p++) if (empty(p)) memset(&out[p], 0, sizeof(ramx_term));
    return RAMX_OK;      // (the next group writes the host and device buffers of this one again: host_reuse)
  });
}

// ------------------------------------------------------------------------------------------
// co-segregation of variants: the pileup's replay with the bit planes as a fourth stage, kept resident, and the Gram matrix of
// chosen planes (ramx_kernels_linkage.h)
// ------------------------------------------------------------------------------------------
static size_t linkage_budget(void)
{
  size_t budget = (size_t)2 << 30;
  if (const char *e = getenv("RAMX_LINKAGE_BYTES")) { const long long v = atoll(e); if (v > 0) budget = (size_t)v; }
  return budget;
}

extern "C" int ramx_dev_planes(ramx_dev *d, const ramx_flank *flanks, int32_t n_padded, const int32_t *fam_first,
                               const int32_t *fam_count, int32_t n_families, const ramx_params *p,
                               const int8_t *cons, const int32_t *rows, ramx_col_pileup *cols, ramx_aln_end *ends, double *kernel_ms)
{
  if (kernel_ms) kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = kernel_ms[3] = 0;
  if (!d || !p || !p->matrix || n_families < 0 || n_padded < 0 || (n_padded & 63) || (n_padded && !flanks) ||
      (n_families && (!fam_first || !fam_count || !rows)))
  { ramx_set_error("ramx_dev_planes: bad argument"); return RAMX_ERR_ARG; }
  if (p->bandwidth < 1 || p->L < 0) { ramx_set_error("ramx_dev_planes: bad bandwidth / L"); return RAMX_ERR_ARG; }
  ReplayPlan pl;
  int rc;
  if ((rc = replay_plan("ramx_dev_planes", n_padded, fam_first, fam_count, n_families, p->L, cons, rows, NULL, true, pl)) != RAMX_OK) return rc;
  if (pl.maxrows > 0 && !cols) { ramx_set_error("ramx_dev_planes: cols missing"); return RAMX_ERR_ARG; }
  d->planes_ready = 0;
  // where every family's planes lie: rows * 8 planes of its tiles' words each, family after family
  const size_t nf1 = (size_t)(n_families > 0 ? n_families : 1);
  std::vector<ResidentFam> fam(nf1);
  std::vector<long long> base(nf1, 0);
  size_t words = 0;
  const size_t budget = linkage_budget();
  for (int f = 0; f < n_families; f++)
  {
    const size_t nt = (size_t)((fam_count[f] + 63) / 64), need = (size_t)rows[f] * RAMX_PLANE_CLASSES * nt;
    fam[f] = ResidentFam{ rows[f], (int)nt, fam_first[f], fam_count[f], (long long)words };
    base[f] = fam[f].base;
    words += need;
    if (words * sizeof(unsigned long long) > budget)
    {
      ramx_set_error("ramx_dev_planes: the bit planes of families 0..%d (family %d: %d rows x 8 classes x %zu tiles; %zu bytes so far) do not fit RAMX_LINKAGE_BYTES = %zu",
                     f, f, rows[f], nt, words * sizeof(unsigned long long), budget);
      return RAMX_ERR_UNSUPPORTED;
    }
  }
  const bool run = n_families > 0 && pl.maxrows > 0 && pl.tiles > 0;
  if (run)
  {
    AlnArgs aa;
    int KW = 0;
    if ((rc = pileup_setup(d, flanks, n_padded, n_families, p, aa, &KW)) != RAMX_OK) return rc;
    if ((rc = ensure(&d->d_lk_planes, &d->cap_lk_planes, (words ? words : 1) * sizeof(unsigned long long)))) return rc;
    if ((rc = ensure(&d->d_lk_base, &d->cap_lk_base, (size_t)n_families * sizeof(long long)))) return rc;
    HIPCHK(hipMemsetAsync(d->d_lk_planes, 0, (words ? words : 1) * sizeof(unsigned long long), d->stream));
    // a blocking copy: `base` is a local, and pileup_replay may return on an error before it has synchronised
    HIPCHK(hipMemcpy(d->d_lk_base, base.data(), (size_t)n_families * sizeof(long long), hipMemcpyHostToDevice));
    PlanesArgs lk;
    memset(&lk, 0, sizeof(lk));
    lk.planes = d->d_lk_planes; lk.fam_base = d->d_lk_base;
    if ((rc = pileup_replay(d, "ramx_dev_planes", aa, KW, pl, n_families, cons, rows, kernel_ms, NULL, &lk)) != RAMX_OK) return rc;
  }
  if ((rc = pileup_fetch(d, run, n_padded, fam_first, fam_count, n_families, p->L, cons, rows, NULL, cols, ends)) != RAMX_OK) return rc;
  // resident from here on (where nothing ran there is no plane a Gram could be asked for)
  ResidentFam *keep = (ResidentFam *)realloc(d->res_fam, nf1 * sizeof(ResidentFam));
  if (!keep) { ramx_set_error("ramx_dev_planes: out of memory"); return RAMX_ERR_ARG; }
  memcpy(keep, fam.data(), nf1 * sizeof(ResidentFam));
  d->res_fam = keep; d->res_families = n_families; d->res_npadded = n_padded;
  d->planes_ready = 1;
  return RAMX_OK;
}

// the shared host path of the calls that answer from the resident planes: Gram, pair matrix, split
static int resident_check(const char *who, const ramx_dev *d, int32_t n_families)
{
  if (!d->planes_ready)
  { ramx_set_error("%s: no resident bit planes (ramx_dev_planes has not run on this device, or a later call dropped them)", who); return RAMX_ERR_STATE; }
  if (n_families != d->res_families)
  { ramx_set_error("%s: %d families, the resident replay has %d", who, n_families, d->res_families); return RAMX_ERR_ARG; }
  return RAMX_OK;
}

// family f's list of P planes (pp == NULL: the caller has found an argument of this family wrong; that is reported behind the
// count's range): in [0, RAMX_LINKAGE_MAX_PLANES], every plane inside the resident replay, strictly increasing in (row, class).
// at != NULL: the planes' first words are appended to it.  No HIP call.
static int plane_list(const char *who, int f, const ResidentFam &rf, const ramx_plane *pp, int P, std::vector<long long> *at)
{
  if (P < 0 || P > RAMX_LINKAGE_MAX_PLANES)
  { ramx_set_error("%s: family %d: %d planes outside [0, %d]", who, f, P, RAMX_LINKAGE_MAX_PLANES); return RAMX_ERR_ARG; }
  if (P > 0 && !pp) { ramx_set_error("%s: family %d: bad argument", who, f); return RAMX_ERR_ARG; }
  for (int i = 0; i < P; i++)
  {
    if (pp[i].row < 0 || pp[i].row >= rf.rows || pp[i].cls < 0 || pp[i].cls >= RAMX_PLANE_CLASSES)
    { ramx_set_error("%s: family %d, plane %d: (row %d, class %d) outside the resident replay (%lld rows, classes 0..7)", who, f, i, pp[i].row, pp[i].cls, (long long)rf.rows); return RAMX_ERR_ARG; }
    if (i > 0 && (pp[i].row < pp[i - 1].row || (pp[i].row == pp[i - 1].row && pp[i].cls <= pp[i - 1].cls)))
    { ramx_set_error("%s: family %d, plane %d: the planes are not strictly increasing in (row, class)", who, f, i); return RAMX_ERR_ARG; }
    if (at) at->push_back(rf.base + ((long long)pp[i].row * RAMX_PLANE_CLASSES + pp[i].cls) * rf.tiles);
  }
  return RAMX_OK;
}

// the blocks (f, bi, bj, 0), bi <= bj, of family f's n x n matrix in blocks of `side`: the upper triangle with the diagonal
static void upper_blocks(std::vector<int4> &block, int f, int n, int side)
{
  const int nb = (n + side - 1) / side;
  for (int bi = 0; bi < nb; bi++)
    for (int bj = bi; bj < nb; bj++) block.push_back(make_int4(f, bi, bj, 0));
}

// k <= 2 launches in a row on d->stream between k + 1 events, and one synchronisation behind them (which the uploads before
// need too: they read the caller's vectors).  The event interval of launch i is added to ms[i] when all went well; *failed: the
// launch that was refused, -1 if none was
template <typename F>
static int timed_launches(ramx_dev *d, int k, F launch, double *ms, int *failed)
{
  hipEvent_t ev[3] = { NULL, NULL, NULL };
  bool timed = true;
  for (int i = 0; i <= k; i++) timed = timed && hipEventCreate(&ev[i]) == hipSuccess;
  if (timed) (void)hipEventRecord(ev[0], d->stream);
  int rc = RAMX_OK;
  *failed = -1;
  for (int i = 0; i < k && rc == RAMX_OK; i++)
    if ((rc = launch(i)) != RAMX_OK) *failed = i;
    else if (timed) (void)hipEventRecord(ev[i + 1], d->stream);
  const hipError_t se = hipStreamSynchronize(d->stream);
  float t = 0;
  for (int i = 0; i < k; i++)
    if (timed && rc == RAMX_OK && se == hipSuccess && hipEventElapsedTime(&t, ev[i], ev[i + 1]) == hipSuccess) ms[i] += t;
  for (int i = 0; i <= k; i++) if (ev[i]) (void)hipEventDestroy(ev[i]);
  if (rc != RAMX_OK) return rc;
  HIPCHK(se);
  return RAMX_OK;
}

extern "C" int ramx_dev_plane_gram(ramx_dev *d, int32_t n_families, const ramx_plane *planes, const int32_t *plane_first,
                                   const int32_t *plane_count, int32_t *co, const int64_t *co_first, uint64_t *bits, const int64_t *bits_first)
{
  if (!d || n_families < 0 || (n_families && (!plane_first || !plane_count)))
  { ramx_set_error("ramx_dev_plane_gram: bad argument"); return RAMX_ERR_ARG; }
  int rc;
  if ((rc = resident_check("ramx_dev_plane_gram", d, n_families)) != RAMX_OK) return rc;
  // everything is checked before anything is launched or written
  std::vector<long long> at, co_at((size_t)(n_families > 0 ? n_families : 1), 0);
  std::vector<int4> gfam((size_t)(n_families > 0 ? n_families : 1), make_int4(0, 0, 0, 0)), block;
  size_t co_words = 0;
  for (int f = 0; f < n_families; f++)
  {
    const int P = plane_count[f];
    const ResidentFam &rf = d->res_fam[f];
    const ramx_plane *pp = P > 0 && plane_first[f] >= 0 && planes && co && co_first && co_first[f] >= 0 &&
                           (!bits || (bits_first && bits_first[f] >= 0)) ? planes + plane_first[f] : NULL;
    const int at0 = (int)at.size();
    // a family without tiles writes nothing: its planes are checked, their words are not listed
    if ((rc = plane_list("ramx_dev_plane_gram", f, rf, pp, P, rf.tiles ? &at : NULL)) != RAMX_OK) return rc;
    if (P == 0 || rf.tiles == 0) continue;
    gfam[f] = make_int4(at0, P, rf.tiles, 0);
    co_at[f] = (long long)co_words;
    co_words += (size_t)P * P;
    upper_blocks(block, f, P, RAMX_GRAM_BLOCK);
  }
  if (block.empty()) return RAMX_OK;
  // a plane to count has passed row < rows[f] of a family with tiles: that replay has run and its buffer exists
  HIPCHK(hipSetDevice(d->ordinal));
  if ((rc = upload(d, &d->d_lk_at, &d->cap_lk_at, at))) return rc;
  if ((rc = upload(d, &d->d_lk_coat, &d->cap_lk_coat, co_at))) return rc;
  if ((rc = upload(d, &d->d_lk_gfam, &d->cap_lk_gfam, gfam))) return rc;
  if ((rc = upload(d, &d->d_lk_block, &d->cap_lk_block, block))) return rc;
  if ((rc = ensure(&d->d_lk_co, &d->cap_lk_co, co_words * sizeof(int)))) return rc;
  GramArgs ga;
  ga.planes = d->d_lk_planes; ga.block = d->d_lk_block; ga.fam = d->d_lk_gfam; ga.at = d->d_lk_at; ga.co_at = d->d_lk_coat; ga.co = d->d_lk_co;
  int failed;
  d->lk_gram_ms = 0;
  rc = timed_launches(d, 1, [&](int) { return ramx_plane_gram_launch(d->stream, (int)block.size(), ga); }, &d->lk_gram_ms, &failed);
  if (failed >= 0) ramx_set_error("ramx_dev_plane_gram: the launch of %d workgroups failed", (int)block.size());
  if (rc != RAMX_OK) return rc;
  for (int f = 0; f < n_families; f++)
  {
    const int P = gfam[f].y, T = gfam[f].z;
    if (P == 0) continue;
    HIPCHK(hipMemcpy(co + co_first[f], d->d_lk_co + co_at[f], (size_t)P * P * sizeof(int), hipMemcpyDeviceToHost));
    // the chosen planes' own words, plane after plane (a diagnostic: one copy a plane)
    for (int i = 0; bits && i < P; i++)
      HIPCHK(hipMemcpy(bits + bits_first[f] + (size_t)i * T, d->d_lk_planes + at[(size_t)gfam[f].x + i], (size_t)T * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  }
  return RAMX_OK;
}

extern "C" double ramx_dev_plane_gram_ms(ramx_dev *d) { return d ? d->lk_gram_ms : 0; }

// pairwise divergence between chosen copies of the resident replay (ramx_dist.h, ramx_kernels_dist.h): the planes transposed
// into bit streams over the rows, then the pair matrix of the streams
extern "C" int ramx_dev_copy_dist(ramx_dev *d, int32_t n_families, const int32_t *copies, const int32_t *copy_first,
                                  const int32_t *copy_count, ramx_copy_dist *out, const int64_t *out_first)
{
  if (d) d->lk_dist_ms[0] = d->lk_dist_ms[1] = 0;
  if (!d || n_families < 0 || (n_families && (!copy_first || !copy_count)))
  { ramx_set_error("ramx_dev_copy_dist: bad argument"); return RAMX_ERR_ARG; }
  int rc;
  if ((rc = resident_check("ramx_dev_copy_dist", d, n_families)) != RAMX_OK) return rc;
  // everything is checked before anything is launched or written
  std::vector<DistFam> dfam((size_t)(n_families > 0 ? n_families : 1));
  std::vector<int4> item, block;
  std::vector<int> slot;
  size_t stream_words = 0, records = 0;
  memset(dfam.data(), 0, dfam.size() * sizeof(DistFam));
  for (int f = 0; f < n_families; f++)
  {
    const int C = copy_count[f];
    const ResidentFam &rf = d->res_fam[f];
    if (C < 0 || C > RAMX_DIST_MAX_COPIES)
    { ramx_set_error("ramx_dev_copy_dist: family %d: %d copies outside [0, %d]", f, C, RAMX_DIST_MAX_COPIES); return RAMX_ERR_ARG; }
    if (C == 0) continue;
    if (copy_first[f] < 0 || !copies || !out || !out_first || out_first[f] < 0)
    { ramx_set_error("ramx_dev_copy_dist: family %d: bad argument", f); return RAMX_ERR_ARG; }
    const int32_t *cp = copies + copy_first[f];
    for (int i = 0; i < C; i++)
    {
      if (cp[i] < 0 || cp[i] >= rf.count)
      { ramx_set_error("ramx_dev_copy_dist: family %d, entry %d: copy %d outside the family's %d flanks", f, i, cp[i], rf.count); return RAMX_ERR_ARG; }
      if (i > 0 && cp[i] <= cp[i - 1])
      { ramx_set_error("ramx_dev_copy_dist: family %d, entry %d: the copies are not strictly increasing", f, i); return RAMX_ERR_ARG; }
    }
    if (rf.rows == 0) continue;                       // all-zero records, written below on the host
    DistFam &fd = dfam[f];
    fd.plane_base = rf.base; fd.stream_base = (long long)stream_words; fd.out_base = (long long)records;
    fd.T = rf.tiles; fd.rows = rf.rows; fd.RW = (rf.rows + 63) / 64; fd.C = C;
    stream_words += (size_t)C * RAMX_DIST_STREAMS * fd.RW;
    records += (size_t)C * C;
    // one wave per tile that holds a chosen copy and per block of 64 rows (the list is ascending: a tile's copies are adjacent)
    for (int i = 0; i < C; )
    {
      const int tile = cp[i] >> 6, s0 = (int)slot.size();
      slot.resize(slot.size() + 64, -1);
      for (; i < C && (cp[i] >> 6) == tile; i++) slot[(size_t)s0 + (cp[i] & 63)] = i;
      for (int rb = 0; rb < fd.RW; rb++) item.push_back(make_int4(f, tile, s0, rb));
    }
    upper_blocks(block, f, C, RAMX_DIST_BLOCK);
  }
  if (!block.empty())
  {
    // a copy to count has passed rows[f] > 0 of a family with flanks: that replay has run and its buffer exists
    HIPCHK(hipSetDevice(d->ordinal));
    if ((rc = ensure(&d->d_lk_streams, &d->cap_lk_streams, stream_words * sizeof(unsigned long long)))) return rc;
    if ((rc = upload(d, &d->d_lk_dfam, &d->cap_lk_dfam, dfam))) return rc;
    if ((rc = upload(d, &d->d_lk_ditem, &d->cap_lk_ditem, item))) return rc;
    if ((rc = upload(d, &d->d_lk_dslot, &d->cap_lk_dslot, slot))) return rc;
    if ((rc = upload(d, &d->d_lk_dblock, &d->cap_lk_dblock, block))) return rc;
    if ((rc = ensure(&d->d_lk_dist, &d->cap_lk_dist, records * sizeof(ramx_copy_dist)))) return rc;
    DistArgs da;
    da.planes = d->d_lk_planes; da.fam = d->d_lk_dfam; da.item = d->d_lk_ditem; da.slot = d->d_lk_dslot; da.block = d->d_lk_dblock;
    da.streams = d->d_lk_streams; da.out = d->d_lk_dist;
    // the pair kernel goes behind the transposition without a round trip to the host
    int failed;
    rc = timed_launches(d, 2, [&](int i) { return i == 0 ? ramx_dist_transpose_launch(d->stream, (int)item.size(), da)
                                                         : ramx_dist_pairs_launch(d->stream, (int)block.size(), da); }, d->lk_dist_ms, &failed);
    if (failed >= 0) ramx_set_error("ramx_dev_copy_dist: the launch of %d waves and %d workgroups failed", (int)item.size(), (int)block.size());
    if (rc != RAMX_OK) return rc;
  }
  for (int f = 0; f < n_families; f++)
  {
    const size_t C = (size_t)copy_count[f];
    if (C == 0) continue;
    if (dfam[f].C == 0) memset(out + out_first[f], 0, C * C * sizeof(ramx_copy_dist));     // rows == 0
    else HIPCHK(hipMemcpy(out + out_first[f], d->d_lk_dist + dfam[f].out_base, C * C * sizeof(ramx_copy_dist), hipMemcpyDeviceToHost));
  }
  return RAMX_OK;
}

extern "C" void ramx_dev_copy_dist_ms(ramx_dev *d, double ms[2])
{
  if (!ms) return;
  ms[0] = d ? d->lk_dist_ms[0] : 0; ms[1] = d ? d->lk_dist_ms[1] : 0;
}

extern "C" int ramx_dev_subfamilies(ramx_dev *d, int32_t n_families, const ramx_plane *planes, const int32_t *plane_first,
                                    const int32_t *plane_count, const uint8_t *init, int32_t K, int32_t max_iter, int32_t *labels,
                                    uint8_t *patterns_out, int32_t *cnt_out, int32_t *size_out, int32_t *iterations, int32_t *converged)
{
  if (!d || n_families < 0 || (n_families && (!plane_first || !plane_count || !size_out || !iterations || !converged)))
  { ramx_set_error("ramx_dev_subfamilies: bad argument"); return RAMX_ERR_ARG; }
  if (K < 1 || K > RAMX_SUBFAM_K) { ramx_set_error("ramx_dev_subfamilies: K = %d outside [1, %d]", K, RAMX_SUBFAM_K); return RAMX_ERR_ARG; }
  if (max_iter < 1) { ramx_set_error("ramx_dev_subfamilies: max_iter = %d below 1", max_iter); return RAMX_ERR_ARG; }
  int rc;
  if ((rc = resident_check("ramx_dev_subfamilies", d, n_families)) != RAMX_OK) return rc;
  if (d->res_npadded > 0 && !labels) { ramx_set_error("ramx_dev_subfamilies: labels missing"); return RAMX_ERR_ARG; }
  // everything is checked before anything is launched or written
  const size_t nf1 = (size_t)(n_families > 0 ? n_families : 1);
  std::vector<SubfamFam> fam(nf1);
  std::vector<long long> at;
  std::vector<longlong2> var;
  std::vector<int> cov;                               // per variant: its cover plane's index in the family's list
  std::vector<int> vidx;                              // per variant: its own index in the family's list
  std::vector<unsigned char> pat;
  std::vector<int> count(nf1, 0);
  size_t mask_words = 0, cnt_words = 0;
  for (int f = 0; f < n_families; f++)
  {
    const int P = plane_count[f];
    const ResidentFam &rf = d->res_fam[f];
    const int T = rf.tiles;
    const ramx_plane *pp = P > 0 && plane_first[f] >= 0 && planes && cnt_out ? planes + plane_first[f] : NULL;
    SubfamFam &fd = fam[f];
    fd.var0 = (int)var.size(); fd.at0 = (int)at.size(); fd.P = P; fd.T = T; fd.flank0 = rf.first;
    fd.mask0 = (long long)mask_words; fd.cnt0 = (long long)cnt_words;
    count[f] = rf.count;
    // the words of every family's planes are listed, those of a family without tiles too: cnt_out is laid out by at0
    if ((rc = plane_list("ramx_dev_subfamilies", f, rf, pp, P, &at)) != RAMX_OK) return rc;
    for (int i = 0; i < P; i++)
    {
      if (pp[i].cls == RAMX_PLANE_COVER) continue;
      int c = -1;
      for (int j = i; j >= 0 && pp[j].row == pp[i].row; j--) if (pp[j].cls == RAMX_PLANE_COVER) c = j;
      for (int j = i + 1; j < P && pp[j].row == pp[i].row; j++) if (pp[j].cls == RAMX_PLANE_COVER) c = j;
      if (c < 0)
      { ramx_set_error("ramx_dev_subfamilies: family %d, plane %d: the cover plane (%d, %d) of the variant (%d, %d) is not in the list", f, i, pp[i].row, RAMX_PLANE_COVER, pp[i].row, pp[i].cls); return RAMX_ERR_ARG; }
      longlong2 vr; vr.x = at[(size_t)fd.at0 + i]; vr.y = at[(size_t)fd.at0 + c];
      var.push_back(vr); cov.push_back(c); vidx.push_back(i);
    }
    fd.V = (int)var.size() - fd.var0;
    if (fd.V > 0 && (!init || !patterns_out)) { ramx_set_error("ramx_dev_subfamilies: family %d: init / patterns_out missing", f); return RAMX_ERR_ARG; }
    for (int v = 0; v < fd.V; v++)
    {
      unsigned char b = 0;
      for (int k = 0; k < K; k++) if (init[((size_t)fd.var0 + v) * K + k]) b |= (unsigned char)(1u << k);
      pat.push_back(b);
    }
    mask_words += (size_t)K * T;
    cnt_words += (size_t)K * (P + 1);
  }
  {
    SubfamLay *lay = (SubfamLay *)realloc(d->sf_lay, nf1 * sizeof(SubfamLay));
    if (!lay) { ramx_set_error("ramx_dev_subfamilies: out of memory"); return RAMX_ERR_ARG; }
    for (int f = 0; f < n_families; f++) lay[f] = SubfamLay{ fam[f].mask0, fam[f].T };
    d->sf_lay = lay; d->sf_families = 0; d->sf_K = K;       // no result until the call has succeeded
  }
  // the answers of a family that never reaches the device (no tile): one assignment of nobody
  for (int i = 0; i < d->res_npadded; i++) labels[i] = -1;
  std::vector<char> active(nf1, 0);
  int n_active = 0;
  for (int f = 0; f < n_families; f++)
  {
    iterations[f] = 1; converged[f] = 1;
    for (int k = 0; k < K; k++) size_out[(size_t)f * K + k] = 0;
    for (size_t i = 0; i < (size_t)K * fam[f].P; i++) cnt_out[(size_t)K * fam[f].at0 + i] = 0;
    for (size_t i = 0; i < (size_t)K * fam[f].V; i++) patterns_out[(size_t)K * fam[f].var0 + i] = init[(size_t)K * fam[f].var0 + i] ? 1 : 0;
    if (fam[f].T == 0) continue;
    active[f] = 1; n_active++;
  }
  d->sf_ms[0] = d->sf_ms[1] = 0;
  if (n_active == 0) { d->sf_families = n_families; return RAMX_OK; }
  HIPCHK(hipSetDevice(d->ordinal));
  if ((rc = upload(d, &d->d_sf_fam, &d->cap_sf_fam, fam))) return rc;
  if ((rc = upload(d, &d->d_sf_at, &d->cap_sf_at, at))) return rc;
  if ((rc = upload(d, &d->d_sf_var, &d->cap_sf_var, var))) return rc;
  if ((rc = upload(d, &d->d_sf_count, &d->cap_sf_count, count))) return rc;
  if ((rc = ensure(&d->d_sf_labels, &d->cap_sf_labels, (size_t)d->res_npadded * sizeof(int)))) return rc;
  if ((rc = ensure(&d->d_sf_cnt, &d->cap_sf_cnt, cnt_words * sizeof(int)))) return rc;
  if ((rc = ensure(&d->d_sf_mask, &d->cap_sf_mask, mask_words * sizeof(unsigned long long)))) return rc;
  HIPCHK(hipMemsetAsync(d->d_sf_labels, 0xff, (size_t)d->res_npadded * sizeof(int), d->stream));     // no label yet: -1
  HIPCHK(hipMemsetAsync(d->d_sf_cnt, 0, cnt_words * sizeof(int), d->stream));
  SubfamArgs sa;
  memset(&sa, 0, sizeof(sa));
  sa.planes = d->d_lk_planes; sa.fam = d->d_sf_fam; sa.at = d->d_sf_at; sa.var = d->d_sf_var;
  sa.count = d->d_sf_count; sa.labels = d->d_sf_labels; sa.mask = d->d_sf_mask;
  sa.cnt = d->d_sf_cnt; sa.K = K;
  std::vector<int2> tile, item;
  std::vector<int> changed, cnt(cnt_words, 0);
  // between two assignments only the per-tile change counts and the counts come to the host: the update rule runs here
  for (int it = 1; n_active > 0; it++)
  {
    tile.clear(); item.clear();
    for (int f = 0; f < n_families; f++)
    {
      if (!active[f]) continue;
      for (int t = 0; t < fam[f].T; t++) tile.push_back(make_int2(f, t));
      for (int i = 0; i <= fam[f].P; i++) item.push_back(make_int2(f, i));
    }
    changed.assign(tile.size(), 0);
    // (the lists only shrink: the first iteration's buffers serve the later ones)
    if ((rc = upload(d, &d->d_sf_pat, &d->cap_sf_pat, pat))) return rc;
    if ((rc = upload(d, &d->d_sf_tile, &d->cap_sf_tile, tile))) return rc;
    if ((rc = upload(d, &d->d_sf_item, &d->cap_sf_item, item))) return rc;
    if ((rc = ensure(&d->d_sf_changed, &d->cap_sf_changed, tile.size() * sizeof(int)))) return rc;
    sa.pat = d->d_sf_pat; sa.tile = d->d_sf_tile; sa.item = d->d_sf_item; sa.changed = d->d_sf_changed;
    int failed;
    if ((rc = timed_launches(d, 1, [&](int) { return ramx_subfam_assign_launch(d->stream, (int)tile.size(), sa); }, &d->sf_ms[0], &failed)) != RAMX_OK)
    { if (rc == RAMX_ERR_HIP) ramx_set_error("ramx_dev_subfamilies: the assign launch of %d waves failed", (int)tile.size()); return rc; }
    if ((rc = timed_launches(d, 1, [&](int) { return ramx_subfam_count_launch(d->stream, (int)item.size(), sa); }, &d->sf_ms[1], &failed)) != RAMX_OK)
    { if (rc == RAMX_ERR_HIP) ramx_set_error("ramx_dev_subfamilies: the count launch of %d waves failed", (int)item.size()); return rc; }
    HIPCHK(hipMemcpy(changed.data(), d->d_sf_changed, tile.size() * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cnt.data(), d->d_sf_cnt, cnt_words * sizeof(int), hipMemcpyDeviceToHost));
    size_t w = 0;
    for (int f = 0; f < n_families; f++)
    {
      if (!active[f]) continue;
      const SubfamFam &fd = fam[f];
      long long nchanged = 0;
      for (int t = 0; t < fd.T; t++) nchanged += changed[w++];
      iterations[f] = it;
      // the first assignment has no label to agree with; with one pattern no later one could differ from it
      const bool stable = K == 1 || (it > 1 && nchanged == 0);
      if (stable || it == max_iter)
      {
        converged[f] = stable ? 1 : 0;
        active[f] = 0; n_active--;
        for (int k = 0; k < K; k++)
        {
          const int *row = cnt.data() + fd.cnt0 + (size_t)k * (fd.P + 1);
          size_out[(size_t)f * K + k] = row[fd.P];
          for (int i = 0; i < fd.P; i++) cnt_out[(size_t)K * fd.at0 + (size_t)k * fd.P + i] = row[i];
        }
        for (int v = 0; v < fd.V; v++)
          for (int k = 0; k < K; k++) patterns_out[((size_t)fd.var0 + v) * K + k] = (pat[(size_t)fd.var0 + v] >> k) & 1;
        continue;
      }
      for (int k = 0; k < K; k++)
      {
        const int *row = cnt.data() + fd.cnt0 + (size_t)k * (fd.P + 1);
        if (row[fd.P] == 0) continue;                 // an empty group keeps its pattern
        for (int v = 0; v < fd.V; v++)
        {
          const size_t g = (size_t)fd.var0 + v;
          const bool on = 2LL * row[vidx[g]] > (long long)row[cov[g]];          // exactly half is not a majority
          pat[g] = (unsigned char)(on ? pat[g] | (1u << k) : pat[g] & ~(1u << k));
        }
      }
    }
  }
  for (int f = 0; f < n_families; f++)
    if (fam[f].T > 0 && count[f] > 0)
      HIPCHK(hipMemcpy(labels + fam[f].flank0, d->d_sf_labels + fam[f].flank0, (size_t)count[f] * sizeof(int), hipMemcpyDeviceToHost));
  d->sf_families = n_families;
  return RAMX_OK;
}

extern "C" int ramx_dev_subfam_masks(ramx_dev *d, int32_t family, uint64_t *mask)
{
  if (!d || !mask || family < 0) { ramx_set_error("ramx_dev_subfam_masks: bad argument"); return RAMX_ERR_ARG; }
  if (!d->planes_ready || !d->sf_lay || family >= d->sf_families)
  { ramx_set_error("ramx_dev_subfam_masks: no ramx_dev_subfamilies result of family %d on the resident planes", family); return RAMX_ERR_STATE; }
  const SubfamLay &lay = d->sf_lay[family];
  if (lay.tiles > 0) HIPCHK(hipMemcpy(mask, d->d_sf_mask + lay.mask0, (size_t)d->sf_K * lay.tiles * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return RAMX_OK;
}

extern "C" void ramx_dev_subfam_ms(ramx_dev *d, double ms[2]) { ms[0] = d ? d->sf_ms[0] : 0; ms[1] = d ? d->sf_ms[1] : 0; }

// the loop of ramx_dev_refine and ramx_dev_refine_cpg: with cpg the replay counts the row pairs as well and the re-call is the
// CpG-aware one (di, n_cpg as ramx_dev_refine_cpg's)
struct CpgRecall { int32_t rows_reversed, cpg_ts; };

static int refine_loop(ramx_dev *d, const char *who, const ramx_flank *flanks, int32_t n_padded, const int32_t *fam_first,
                       const int32_t *fam_count, int32_t n_families, const ramx_params *p,
                       const int8_t *cons_in, const int32_t *rows_in, int32_t max_replays,
                       int8_t *cons_out, int32_t *rows_out, int32_t *replays, int32_t *converged,
                       ramx_col_pileup *cols, ramx_aln_end *ends, double *kernel_ms,
                       const CpgRecall *cpg, ramx_col_dinuc *di, int32_t *n_cpg)
{
  if (kernel_ms) { kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = 0; if (cpg) kernel_ms[3] = 0; }
  if (!d || !p || !p->matrix || n_families < 0 || n_padded < 0 || (n_padded & 63) || (n_padded && !flanks) ||
      (n_families && (!fam_first || !fam_count || !rows_in || !rows_out || !replays || !converged)) || max_replays < 1 ||
      (cpg && n_families && !n_cpg))
  { ramx_set_error("%s: bad argument", who); return RAMX_ERR_ARG; }
  if (p->bandwidth < 1 || p->L < 0) { ramx_set_error("%s: bad bandwidth / L", who); return RAMX_ERR_ARG; }
  if (dev_is_multi(d))
  { ramx_set_error("%s: not with a communicator or mailbox route active (the re-call needs the counts of every rank)", who); return RAMX_ERR_UNSUPPORTED; }
  const int L = p->L;
  ReplayPlan pl;
  int rc;
  if ((rc = replay_plan(who, n_padded, fam_first, fam_count, n_families, L, cons_in, rows_in, NULL, true, pl)) != RAMX_OK) return rc;
  if (pl.maxrows > 0 && (!cols || !cons_out || (cpg && !di))) { ramx_set_error("%s: cons_out / cols%s missing", who, cpg ? " / di" : ""); return RAMX_ERR_ARG; }
  std::vector<int8_t> cur((size_t)(n_families > 0 ? n_families : 1) * (L > 0 ? L : 1), 0), next((size_t)(L > 0 ? L : 1));
  std::vector<int32_t> rows(rows_in, rows_in + n_families);
  std::vector<char> active((size_t)n_families, 1);
  for (int f = 0; f < n_families; f++)
  {
    if (rows[f] > 0) memcpy(cur.data() + (size_t)f * L, cons_in + (size_t)f * L, (size_t)rows[f]);
    replays[f] = 0; converged[f] = 0;
    if (cpg) n_cpg[f] = 0;
  }
  AlnArgs aa;
  int KW = 0, left = n_families;
  bool set_up = false;
  for (int it = 0; it < max_replays && left > 0; it++)
  {
    // only the families that have not converged replay: the tiles of the others belong to none in this replay's table
    if ((rc = replay_plan(who, n_padded, fam_first, fam_count, n_families, L, cur.data(), rows.data(), active.data(), false, pl)) != RAMX_OK) return rc;
    const bool run = pl.maxrows > 0 && pl.tiles > 0;
    if (run)
    {
      // once per call, not per replay: the flanks and their windows do not change
      if (!set_up && (rc = pileup_setup(d, flanks, n_padded, n_families, p, aa, &KW)) != RAMX_OK) return rc;
      if (!set_up && cpg && (rc = ensure(&d->d_dn_cols, &d->cap_dn_cols, (size_t)n_families * L * sizeof(ramx_col_dinuc)))) return rc;
      set_up = true;
      if ((rc = pileup_replay(d, who, aa, KW, pl, n_families, cur.data(), rows.data(), kernel_ms, NULL, NULL, cpg != NULL)) != RAMX_OK) return rc;
    }
    if (cpg && (rc = dinuc_fetch(d, run, n_families, L, cur.data(), rows.data(), active.data(), di)) != RAMX_OK) return rc;
    if ((rc = pileup_fetch(d, run, n_padded, fam_first, fam_count, n_families, L, cur.data(), rows.data(), active.data(), cols, ends)) != RAMX_OK) return rc;
    for (int f = 0; f < n_families; f++)
    {
      if (!active[f]) continue;
      int8_t *c = cur.data() + (size_t)f * L;
      const int32_t n = cpg ? ramx_recall_cpg(c, rows[f], cols + (size_t)f * L, di + (size_t)f * L, cpg->rows_reversed, p->matrix, cpg->cpg_ts, L,
                                              next.data(), &n_cpg[f])
                            : ramx_recall_consensus(c, rows[f], cols + (size_t)f * L, L, next.data());
      replays[f] = it + 1;
      if (n == rows[f] && (n == 0 || memcmp(c, next.data(), (size_t)n) == 0)) { converged[f] = 1; active[f] = 0; left--; }
      else if (it + 1 == max_replays) { active[f] = 0; left--; }
      else { memcpy(c, next.data(), (size_t)n); rows[f] = n; }
    }
  }
  for (int f = 0; f < n_families; f++)
  {
    rows_out[f] = rows[f];
    if (rows[f] > 0) memcpy(cons_out + (size_t)f * L, cur.data() + (size_t)f * L, (size_t)rows[f]);
  }
  return RAMX_OK;
}

extern "C" int ramx_dev_refine(ramx_dev *d, const ramx_flank *flanks, int32_t n_padded, const int32_t *fam_first,
                               const int32_t *fam_count, int32_t n_families, const ramx_params *p,
                               const int8_t *cons_in, const int32_t *rows_in, int32_t max_replays,
                               int8_t *cons_out, int32_t *rows_out, int32_t *replays, int32_t *converged,
                               ramx_col_pileup *cols, ramx_aln_end *ends, double *kernel_ms)
{
  return refine_loop(d, "ramx_dev_refine", flanks, n_padded, fam_first, fam_count, n_families, p, cons_in, rows_in, max_replays,
                     cons_out, rows_out, replays, converged, cols, ends, kernel_ms, NULL, NULL, NULL);
}

extern "C" int ramx_dev_refine_cpg(ramx_dev *d, const ramx_flank *flanks, int32_t n_padded, const int32_t *fam_first,
                                   const int32_t *fam_count, int32_t n_families, const ramx_params *p,
                                   const int8_t *cons_in, const int32_t *rows_in, int32_t max_replays, int32_t rows_reversed, int32_t cpg_ts,
                                   int8_t *cons_out, int32_t *rows_out, int32_t *replays, int32_t *converged,
                                   ramx_col_pileup *cols, ramx_col_dinuc *di, int32_t *n_cpg, ramx_aln_end *ends, double *kernel_ms)
{
  const CpgRecall cpg = { rows_reversed != 0, cpg_ts };
  return refine_loop(d, "ramx_dev_refine_cpg", flanks, n_padded, fam_first, fam_count, n_families, p, cons_in, rows_in, max_replays,
                     cons_out, rows_out, replays, converged, cols, ends, kernel_ms, &cpg, di, n_cpg);
}

// ---- ramx_dev_run_direction and its steps -----------------------------------------------------------
static long long *sums_slot(ramx_dev *d, int r) { return d->d_sums + (size_t)(((r % 3) + 3) % 3) * NSHARD * 4; }

// -outmat / -vvvv: the DBG buffers a traced column launch writes
static int trace_buffers(ramx_dev *d, KArgs &ka)
{
  const int Bt = 2 * d->p.bandwidth + 1;
  int trc;
  if ((trc = ensure(&d->d_dbg_best, &d->cap_dbg_best, (size_t)d->Np * sizeof(int2))) != RAMX_OK) return trc;
  ka.dbg_best = d->d_dbg_best;
  ka.dbg_codes = NULL; ka.dbg_cand = NULL; ka.dbg_gap = NULL; ka.dbg_band = NULL;
  if (d->trace_cb)
  {
    if ((trc = ensure(&d->d_dbg_codes, &d->cap_dbg_codes, (size_t)d->Np * Bt)) != RAMX_OK) return trc;
    ka.dbg_codes = d->d_dbg_codes;
  }
  if (d->verbose_cb)
  {
    if ((trc = ensure(&d->d_dbg_cand, &d->cap_dbg_cand, (size_t)d->Np * 16 * sizeof(int))) != RAMX_OK) return trc;
    if ((trc = ensure(&d->d_dbg_gap, &d->cap_dbg_gap, (size_t)d->Np * sizeof(int2))) != RAMX_OK) return trc;
    ka.dbg_cand = d->d_dbg_cand; ka.dbg_gap = d->d_dbg_gap;
    if (d->verbose_band)
    {
      if ((trc = ensure(&d->d_dbg_band, &d->cap_dbg_band, (size_t)d->Np * 8 * Bt * sizeof(int))) != RAMX_OK) return trc;
      ka.dbg_band = d->d_dbg_band;
    }
  }
  return RAMX_OK;
}

// hands the DBG buffers of the launch that has just completed to the callbacks
static int deliver_trace(ramx_dev *d, int r, int besta)
{
  const int Bt = 2 * d->p.bandwidth + 1;
  std::vector<int8_t> codes;
  std::vector<int2> best((size_t)d->Nx + 1), gaps((size_t)d->Nx + 1);
  std::vector<int32_t> bs((size_t)d->Nx + 1), bi((size_t)d->Nx + 1), gfl(2 * (size_t)d->Nx + 2), cand(16 * (size_t)d->Nx + 16);
  if (d->Nx && r >= 0) HIPCHK(hipMemcpy(best.data(), d->d_dbg_best, (size_t)d->Nx * sizeof(int2), hipMemcpyDeviceToHost));
  for (int i = 0; i < d->Nx; i++) { bs[i] = best[i].x; bi[i] = best[i].y; }
  if (d->trace_cb && r >= 0)
  {
    codes.resize((size_t)d->Nx * Bt + 1);
    if (d->Nx) HIPCHK(hipMemcpy(codes.data(), d->d_dbg_codes, (size_t)d->Nx * Bt, hipMemcpyDeviceToHost));
    d->trace_cb(r, besta, codes.data(), bs.data(), bi.data(), d->trace_user);
  }
  if (d->verbose_cb)
  {
    if (d->Nx)
    {
      HIPCHK(hipMemcpy(cand.data(), d->d_dbg_cand, (size_t)d->Nx * 16 * sizeof(int), hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(gaps.data(), d->d_dbg_gap, (size_t)d->Nx * sizeof(int2), hipMemcpyDeviceToHost));
    }
    for (int i = 0; i < d->Nx; i++) { gfl[2 * i] = gaps[i].x; gfl[2 * i + 1] = gaps[i].y; }
    std::vector<int32_t> band;
    if (d->verbose_band && d->Nx)
    {
      band.resize((size_t)d->Nx * 8 * Bt);
      HIPCHK(hipMemcpy(band.data(), d->d_dbg_band, band.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    d->verbose_cb(r, besta, d->Nx, bs.data(), bi.data(), gfl.data(), cand.data(), band.empty() ? NULL : band.data(), d->verbose_user);
  }
  return RAMX_OK;
}

// K(-1): the boundary row and the candidates of row 0 -- how every direction but a cell-parallel one begins, and (again) how a
// direction starts over on the per-column route after a single-launch kernel gave up: d_ctl[1] then holds the initial control
// block again, and d_ctl[0], where that kernel left its last one, is cleared.
static int boundary_row(ramx_dev *d, KArgs &a, bool again)
{
  HIPCHK(hipMemsetAsync(d->d_sums, 0, 3 * NSHARD * 4 * sizeof(long long), d->stream));
  if (!again) HIPCHK(hipEventRecord(d->ev_begin, d->stream));
  a.r = -1; a.S_in = d->d_state[0]; a.S_out = d->d_state[1]; a.ctl_in = d->d_ctl; a.ctl_out = d->d_ctl + 1;
  a.sums_in = sums_slot(d, 0); a.sums_out = sums_slot(d, 0); a.sums_zero = sums_slot(d, 1); a.nshards_in = NSHARD;
  if (!again && d->verbose_cb != NULL)
  {
    int trc = trace_buffers(d, a);
    if (trc != RAMX_OK) return trc;
    launch_column_trace(d, a, true);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(d->stream));
    if ((trc = deliver_trace(d, -1, 0)) != RAMX_OK) return trc;
  }
  else launch_column<true>(d, a);
  if (again) HIPCHK(hipMemsetAsync(d->d_ctl, 0, sizeof(RamxCtl), d->stream));
  else HIPCHK(hipGetLastError());
  return RAMX_OK;
}

#ifdef RAMX_CP_TIMING
static int cp_timing_report(const CPArgs &ca, const DirRoute &rt)
{
  unsigned long long h[16 * 16 + 8];
  HIPCHK(hipMemcpy(h, ca.dbg, sizeof(h), hipMemcpyDeviceToHost));
  const double cols = h[16 * 16] ? (double)h[16 * 16] : 1.0;
  fprintf(stderr, "SP_TIMING workgroup 0, %d workgroups x %d threads, K %d, %.0f rows; shader clocks (100 MHz) per row\n", rt.nb, rt.th, rt.k, cols);
  fprintf(stderr, "SP_TIMING vote wave: tickets wait+fold %.1f | winner+forward %.1f | stop rule, decision %.1f | loop %.1f | waiting for band sums %.1f | forwarded at once %.0f %%\n",
          h[0] / cols, h[1] / cols, h[2] / cols, h[3] / cols, h[4] / cols, 100.0 * h[5] / cols);
  for (int wv = 1; wv < rt.th / 64; wv++)
    fprintf(stderr, "SP_TIMING band wave %d: idle %.1f | planning %.1f | rows %.1f\n", wv, h[wv * 16 + 0] / cols, h[wv * 16 + 1] / cols, h[wv * 16 + 2] / cols);
  return RAMX_OK;
}
#endif

// The device-wide cell-parallel launch of the plan in rt: boundary row and every column inside the kernel.  *accepted: the launch
// call went through -- from there on an error is the kernel's (an execution error: not something another route can serve).
static int cp_device_launch(ramx_dev *d, const KArgs &a, const DirRoute &rt, bool *accepted)
{
  const int nb = rt.nb;
  { const int prc = pack_rest(d); if (prc != RAMX_OK) return prc; }      // this kernel reads the whole window
  CPArgs ca = cp_args(d, d->d_ctl, d->Np, d->KW, d->p, d->tab);       // (a's scalars are d->p's)
  {
    std::vector<CpDevDesc> hd((size_t)nb);
    for (int i = 0; i < nb; i++) { memset(&hd[i], 0, sizeof(CpDevDesc)); hd[i].first = 0; hd[i].nx = d->Nx; hd[i].b = i; hd[i].nb = nb; hd[i].id = 0; }
    int drc = ensure(&d->d_devdesc, &d->cap_devdesc, sizeof(CpDevDesc) * (size_t)nb);
    if (drc != RAMX_OK) return drc;
    HIPCHK(hipMemcpyAsync(d->d_devdesc, hd.data(), sizeof(CpDevDesc) * (size_t)nb, hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));       // hd goes out of scope
  }
  ca.dev = d->d_devdesc; ca.vote = d->d_vote; ca.err = d->d_err; ca.S = d->d_state[0]; ca.vote_wave = rt.vwf;
  { const char *td = getenv("RAMX_TEST_CP_DROP_TICKET"); ca.test_drop_row = td ? atoi(td) : 0; ca.test_drop_id = -1; }
  ca.nranks = 1; ca.rank = 0;
  if (rt.multi)
  {
    ca.nranks = d->nranks; ca.rank = d->rank; ca.peers = (PeerBox *const *)d->d_peer; ca.box = d->xbox;
    { const int mrc = mailbox_mirror(d, &ca.mirror); if (mrc != RAMX_OK) return mrc; }
    const char *tf = getenv("RAMX_TEST_FAIL_PRK_RANK");      // test hook: this rank fails where a launch error would
    if (tf && atoi(tf) == d->rank) { ramx_set_error("test hook: forced failure of the cell-parallel launch on rank %d", d->rank); return RAMX_ERR_HIP; }
  }
  HIPCHK(hipMemsetAsync(d->d_vote, 0, RAMX_CP_NSETS * NSHARD * sizeof(PShard), d->stream));
  HIPCHK(hipMemsetAsync(d->d_err, 0, 64, d->stream));
  HIPCHK(hipMemsetAsync(d->d_ctl, 0, 2 * sizeof(RamxCtl), d->stream));
#ifdef RAMX_CP_TIMING
  HIPCHK(hipMalloc((void **)&ca.dbg, (16 * 16 + 8) * sizeof(unsigned long long)));
  HIPCHK(hipMemset(ca.dbg, 0, (16 * 16 + 8) * sizeof(unsigned long long)));
#endif
  HIPCHK(hipEventRecord(d->ev_begin, d->stream));
  if (rt.multi) test_delay_rank(d);
  int crc = ramx_cp_launch_device(d->stream, a.W, rt.k, rt.th, nb, ca);
  if (crc != RAMX_OK)
  {
#ifdef RAMX_CP_TIMING
    (void)hipFree(ca.dbg);
#endif
    ramx_set_error("cell-parallel device launch failed (W %d, %d lanes per flank, %d workgroups)", a.W, rt.k, nb);
    return crc;
  }
  *accepted = true;
  HIPCHK(hipEventRecord(d->ev_end, d->stream));
  HIPCHK(hipStreamSynchronize(d->stream));
#ifdef RAMX_CP_TIMING
  if (rt.vwf) { const int trc = cp_timing_report(ca, rt); if (trc != RAMX_OK) return trc; }
  (void)hipFree(ca.dbg);
#endif
  return RAMX_OK;
}

// The cell-parallel route: K lanes per flank, the whole direction in one launch of at most one workgroup per CU.  *lanes > 0 on
// return: the direction has run.  Multi-rank: the vote crosses the devices through the mailboxes (ramx_dev_peer_* set-up),
// exactly as in the lane-per-flank persistent kernels; every rank takes this route or none: one agreement before, one after.
static int cp_attempt(ramx_dev *d, const KArgs &a, int L, DirRoute &rt, int *lanes)
{
  *lanes = 0;
  if (!rt.cp_try) return RAMX_OK;
  int k = rt.k, rc;
  if (rt.multi)
  {
    if ((rc = mailbox_clear(d)) != RAMX_OK) return rc;
    int cannot = k > 0 ? 0 : 1;
    if ((rc = host_allreduce_flag(d, &cannot)) != RAMX_OK) return rc;
    if (cannot) k = 0;
  }
  if (k <= 0) return RAMX_OK;
  // from here on a multi-rank run never leaves before the second agreement (a rank that did would leave the others'
  // kernels spinning to their limit and then waiting in a collective it never joins)
  bool accepted = false;
  const int lrc = cp_device_launch(d, a, rt, &accepted);
  RamxCtl c0;
  memset(&c0, 0, sizeof(c0));
  int bad = lrc != RAMX_OK;
  if (!bad && hipMemcpy(&c0, d->d_ctl, sizeof(c0), hipMemcpyDeviceToHost) != hipSuccess) bad = 1;
  bad = bad || c0.pad != 0;
  if (rt.multi)
  {
    if (lrc != RAMX_OK) (void)hipStreamSynchronize(d->stream);
    if ((rc = host_allreduce_flag(d, &bad)) != RAMX_OK) return rc;
    if (bad)
    {
      fprintf(stderr, "ramx: cross-device cell-parallel launch gave up or failed on some rank; repeating the direction with per-column "
                      "launches and leaving the mailbox path off for the rest of this process\n");
      d->peer_ready = 0;        // agreed by all ranks (the flag above is reduced)
      rt.mailbox_ok = rt.int32_can = rt.pk = false;      // ... and with the mailboxes go this direction's other single-launch kernels
    }
  }
  else if (lrc != RAMX_OK && accepted)
    return lrc;               // the kernel ran and failed (a fault is sticky: the context is gone): the error as it was reported
  else if (lrc != RAMX_OK)
  {
    // single GPU: the other routes can serve the same flank set -- an occupancy query that says no, a launch configuration
    // this one instantiation refuses -- so a refusal here is not the direction's failure
    (void)hipStreamSynchronize(d->stream);
    (void)hipGetLastError();
    fprintf(stderr, "ramx: cell-parallel device launch not possible (%s); continuing on the lane-per-flank route\n", ramx_last_error());
  }
  else if (bad)
    fprintf(stderr, "ramx: device-wide vote of the cell-parallel launch timed out (bounded spin); repeating the direction with "
                    "per-column launches\n");
  if (!bad) *lanes = k;
  return RAMX_OK;
}

// The lane-per-flank persistent kernels behind K(-1): the in-place row buffer holds S(-1), d_ctl[1] the initial control block,
// and the kernel writes its final one to d_ctl[0].  A launch that gave up -- a bounded spin that ran out (e.g. a co-tenant
// holding CUs), a row the packed kernel refused -- is not fatal: the direction starts over on the per-column route.
static int prk_attempt(ramx_dev *d, KArgs &a, int L, DirRoute &rt, bool *persistent)
{
  if (d->d_state[0] != d->d_state[1]) { ramx_set_error("persistent path needs the in-place row buffer"); return RAMX_OK; }
  if (rt.tracing) return RAMX_OK;
  // Single GPU: a failure is simply returned.  Multi-rank: once the ranks have agreed on the persistent path (prk_run sets
  // `persistent` after that agreement) a rank-local failure -- an allocation, a memset, the launch itself -- must NOT leave
  // before the agreement below, or the other ranks' kernels spin to their limit and then wait in a collective this rank
  // never joins.
  const int lrc = prk_run(d, a, L, rt, persistent);
  if (lrc != RAMX_OK && !(rt.multi && *persistent)) return lrc;
  if (!*persistent) return RAMX_OK;
  RamxCtl c0[2];
  unsigned errw = 0;
  int bad = lrc != RAMX_OK, rc;
  memset(c0, 0, sizeof(c0));
  if (rt.multi)
  {
    // agree over all ranks whether the cross-device launch went through; if any rank gave up or failed locally, every rank
    // repeats the direction with the per-column launches and the host collective
    if (bad) (void)hipStreamSynchronize(d->stream);
    else if (read_launch_state(d, c0, &errw) != RAMX_OK) bad = 1;
    bad = bad || c0[0].pad != 0 || c0[1].pad != 0 || errw != 0;
    if ((rc = host_allreduce_flag(d, &bad)) != RAMX_OK) return rc;
    if (!bad) return RAMX_OK;
    fprintf(stderr, "ramx: cross-device persistent launch gave up on some rank; repeating the direction with per-column launches "
                    "and leaving the mailbox path off for the rest of this process\n");
    d->peer_ready = 0;          // agreed by all ranks (the flag above is reduced): nobody tries the mailboxes again
  }
  else
  {
    if ((rc = read_launch_state(d, c0, &errw)) != RAMX_OK) return rc;
    rt_mark("after the launch: control blocks, error word");
    if (c0[0].pad == 0 && c0[1].pad == 0 && errw == 0) return RAMX_OK;
    if (errw == 2 || errw == 3)
      fprintf(stderr, "ramx: the packed-row kernel refused %s (a cell outside the span computed for this scoring system); repeating "
                      "the direction with per-column launches\n", errw == 3 ? "the rows it was handed" : "a row it computed");
    else
      fprintf(stderr, "ramx: device-wide barrier of the persistent launch timed out (bounded spin); repeating the direction with "
                      "per-column launches\n");
  }
  *persistent = false;
  return boundary_row(d, a, true);
}

// The per-column route: K(0 .. L-1) back to back on one stream, no host synchronisation per column -- the stop decision lives
// in the control blocks on the device, a stopped launch returns at once; the host looks at a pinned copy every 64 columns, one
// checkpoint behind, and stops launching.  A trace runs one row at a time instead.
static int column_loop(ramx_dev *d, KArgs &a, int L, const DirRoute &rt, int *launches, int *nsamp)
{
  const int CHUNK = 64;
  const int stride = L > MAX_SAMPLES * 4 ? L / MAX_SAMPLES : 4;
  int pending = -1, chk = 0;
  bool stopped = false;
  memset(d->h_ctl, 0, 4 * sizeof(RamxCtl));
  for (int r = 0; r < L && !stopped; r++)
  {
    if (rt.multi)
    {
      // the vote shards of row r (32 x 4 x int64 = 1 KB) are summed across ranks in place; the column kernel then
      // folds them exactly as in the single-GPU case.  One collective per column, no extra kernel.
      int hrc = host_allreduce_shards(d, sums_slot(d, r));
      if (hrc != RAMX_OK) return hrc;
    }
    a.sums_in = sums_slot(d, r); a.nshards_in = NSHARD;
    a.r = r; a.S_in = d->d_state[(r + 1) & 1]; a.S_out = d->d_state[r & 1];
    a.ctl_in = d->d_ctl + ((r + 1) & 1); a.ctl_out = d->d_ctl + (r & 1);
    a.sums_out = sums_slot(d, r + 1); a.sums_zero = sums_slot(d, r + 2);
    if (rt.tracing)
    {
      // one row at a time: launch, wait, hand the row's trace to the caller (debugging aid, no attempt at speed)
      int trc = trace_buffers(d, a);
      if (trc != RAMX_OK) return trc;
      launch_column_trace(d, a);
      (*launches)++;
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(d->stream));
      RamxCtl c;
      HIPCHK(hipMemcpy(&c, a.ctl_out, sizeof(c), hipMemcpyDeviceToHost));
      if (c.rows_done == r + 1)      // the launch ran (a stopped predecessor makes the kernel return at once)
        if ((trc = deliver_trace(d, r, c.besta)) != RAMX_OK) return trc;
      if (c.stopped) stopped = true;
      continue;
    }
    const bool sample = (r % stride) == (stride / 2) && *nsamp < MAX_SAMPLES;
    if (sample) HIPCHK(hipEventRecord(d->ev_s0[*nsamp], d->stream));
    launch_column<false>(d, a);
    if (sample) { HIPCHK(hipEventRecord(d->ev_s1[*nsamp], d->stream)); (*nsamp)++; }
    (*launches)++;
    if (((r + 1) % CHUNK) == 0 || r == L - 1)
    {
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(d->h_ctl + 2 * chk, d->d_ctl, 2 * sizeof(RamxCtl), hipMemcpyDeviceToHost, d->stream));
      HIPCHK(hipEventRecord(d->ev_chk[chk], d->stream));
      if (pending >= 0)
      {
        HIPCHK(hipEventSynchronize(d->ev_chk[pending]));
        const RamxCtl *h = d->h_ctl + 2 * pending;
        if (h[0].stopped || h[1].stopped) stopped = true;
      }
      pending = chk;
      chk ^= 1;
    }
  }
  return RAMX_OK;
}

// f: the direction's final control block (its besta word carries the single-launch kernels' row counts)
static int fill_run_info(ramx_dev *d, ramx_run_info *info, const RamxCtl &f, int L, int launches, int nsamp, bool persistent, bool cp_done, int lanes)
{
  const bool packed = persistent && !cp_done && d->last_packed_r0 >= 0;
  info->ret = f.max_row + 1;
  info->rows_executed = f.rows_done;
  info->limit_warning = (f.stopped && f.rows_done - 1 == L - 1) ? 1 : 0;   // ram_extend.c:1225-1231
  info->overflow32 = f.overflow;
  info->n_extendable = d->Nx;
  info->launches = launches;
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, d->ev_begin, d->ev_end));
  info->loop_ms = ms;
  double acc = 0; int cnt = 0;
  for (int i = 0; i < nsamp; i++)
  {
    float t = 0;
    if (hipEventElapsedTime(&t, d->ev_s0[i], d->ev_s1[i]) == hipSuccess) { acc += t; cnt++; }
  }
  info->kernel_ms_avg = cnt ? acc / cnt : 0.0;
  info->kernel_samples = cnt;
  info->persistent = persistent ? 1 : 0;
  info->lanes_per_flank = lanes;
  info->respeculated_rows = cp_done ? f.besta : packed ? (f.besta >> 16) & 0xffff : 0;
  info->packed_rows = (packed && f.rows_done > d->last_packed_r0) ? f.rows_done - d->last_packed_r0 : 0;
  info->lean_rows = packed ? (f.besta & 0xffff) : 0;
  return RAMX_OK;
}

extern "C" int ramx_dev_run_direction(ramx_dev *d, ramx_run_info *info)
{
  if (!d || !d->ready) { ramx_set_error("ramx_dev_run_direction: begin_direction has not been called"); return RAMX_ERR_STATE; }
  HIPCHK(hipSetDevice(d->ordinal));
  const ramx_params &p = d->p;
  const int L = p.L;
  KArgs a;
  memset(&a, 0, sizeof(a));
  a.bases = d->d_bases; a.bounds = d->d_bounds; a.trim = d->d_trim; a.cons_out = d->d_cons;
  a.Np = d->Np; a.Nx = d->Nx; a.W = p.bandwidth; a.go = p.gapopen; a.ge = p.gapextn; a.cap = p.cappenalty;
  a.minimp = p.minimprovement; a.when_to_stop = p.when_to_stop;
  memcpy(a.tab, d->tab, sizeof(a.tab));
  int launches = 0, nsamp = 0, lanes = 0, rc;
  bool persistent = false;
  DirRoute rt;
  rt_mark(NULL);
  if ((rc = direction_route(d, a, L, &rt)) != RAMX_OK) return rc;
  if (rt.pack_now && (rc = pack_rest(d)) != RAMX_OK) return rc;
  rt_mark("route (occupancy answers)");
  if ((rc = cp_attempt(d, a, L, rt, &lanes)) != RAMX_OK) return rc;
  const bool cp_done = lanes > 0;
  rt_mark("cell-parallel plan / launch");
  if (cp_done) persistent = true;
  else
  {
    lanes = 1;
    if ((rc = boundary_row(d, a, false)) != RAMX_OK) return rc;
    rt_mark("boundary row launched");
    if ((rc = prk_attempt(d, a, L, rt, &persistent)) != RAMX_OK) return rc;
  }
  d->last_persistent = persistent ? 1 : 0;
  if (!persistent)
  {
    if ((rc = pack_rest(d)) != RAMX_OK) return rc;      // the column launches read the whole window
    if ((rc = column_loop(d, a, L, rt, &launches, &nsamp)) != RAMX_OK) return rc;
  }
  if (!cp_done) HIPCHK(hipEventRecord(d->ev_end, d->stream));
  rt_mark("loop enqueued / pieces run");
  HIPCHK(hipStreamSynchronize(d->stream));
  RamxCtl h[2];
  if ((rc = d2h_small(d, h, d->d_ctl, sizeof(h))) != RAMX_OK) return rc;
  rt_mark("final synchronisation, control blocks");
  const RamxCtl &f = (L == 0) ? h[1] : ((h[0].rows_done > h[1].rows_done) ? h[0] : h[1]);
  d->final_ctl = f;
  if (persistent)
  {
    launches = 1;
    if (f.pad != 0) { ramx_set_error("persistent kernel: device-wide barrier timed out (bounded spin gave up)"); return RAMX_ERR_STATE; }
  }
  return info ? fill_run_info(d, info, f, L, launches, nsamp, persistent, cp_done, lanes) : RAMX_OK;
}

extern "C" int ramx_dev_download(ramx_dev *d, int8_t *cons, int32_t cons_cap, int32_t *trim_high, int32_t *trim_pos)
{
  if (!d || !d->ready) { ramx_set_error("ramx_dev_download: nothing to download"); return RAMX_ERR_STATE; }
  HIPCHK(hipSetDevice(d->ordinal));
  const int rows = d->final_ctl.rows_done;
  const bool timing = getenv("RAMX_TIMING") != NULL;
  const double td0 = now_ms();
  if (cons)
  {
    if (cons_cap < rows) { ramx_set_error("cons buffer too small (%d < %d)", cons_cap, rows); return RAMX_ERR_ARG; }
    if (rows) { const int drc = d2h_small(d, cons, d->d_cons, (size_t)rows); if (drc != RAMX_OK) return drc; }
  }
  if ((trim_high || trim_pos) && d->Nx)
  {
    // through a pinned buffer kept with the session: the copy into pageable memory pins the caller's pages on the fly (8 ms for
    // 800 KB at N = 100,000)
    const size_t need = (size_t)d->Nx * sizeof(int2);
    if (need > d->cap_stage)
    {
      if (d->h_stage) HIPCHK(hipHostFree(d->h_stage));
      d->h_stage = NULL; d->cap_stage = 0;
      HIPCHK(hipHostMalloc(&d->h_stage, need + need / 2, hipHostMallocDefault));
      d->cap_stage = need + need / 2;
    }
    int2 *tmp = (int2 *)d->h_stage;
    const double td1 = now_ms();
    if (getenv("RAMX_DOWNLOAD_DMA"))
      HIPCHK(hipMemcpyAsync(tmp, d->d_trim, need, hipMemcpyDeviceToHost, d->stream));
    else
    {
      hipLaunchKernelGGL(ramx_to_host_kernel, dim3((d->Nx + 255) / 256), dim3(256), 0, d->stream, (const int2 *)d->d_trim, tmp, d->Nx);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(d->stream));
    if (timing) fprintf(stderr, "RAMX_TIMING       download: consensus %.3f ms, trim copy %.3f ms\n", td1 - td0, now_ms() - td1);
    for (int i = 0; i < d->Nx; i++)
    {
      if (trim_high) trim_high[i] = tmp[i].x;
      if (trim_pos) trim_pos[i] = tmp[i].y;
    }
  }
  return RAMX_OK;
}

extern "C" int ramx_dev_peek_state(ramx_dev *d, int32_t flank, int32_t *cells, int32_t *high, int32_t *pos)
{
  if (!d || !d->ready || flank < 0 || flank >= d->Nx) { ramx_set_error("ramx_dev_peek_state: bad argument"); return RAMX_ERR_ARG; }
  HIPCHK(hipSetDevice(d->ordinal));
  const int W = d->p.bandwidth, Q = W + 1, B = 2 * W + 1;
  const int rows = d->final_ctl.rows_done;
  const int4 *S = d->d_state[(rows - 1) & 1];   // K(r) wrote state[r & 1]; rows == 0 -> boundary row in slot 1
  const int tile = flank / 64, lane = flank % 64;
  for (int q = 0; q < Q; q++)
  {
    int4 v;
    HIPCHK(hipMemcpy(&v, S + ((size_t)tile * Q + q) * 64 + lane, sizeof(v), hipMemcpyDeviceToHost));
    cells[4 * q] = v.x; cells[4 * q + 1] = v.y;
    if (2 * q + 1 < B) { cells[4 * q + 2] = v.z; cells[4 * q + 3] = v.w; }
    else { if (high) *high = v.z; if (pos) *pos = v.w; }
  }
  return RAMX_OK;
}

extern "C" int ramx_dev_peek_windows(ramx_dev *d, uint32_t *words, int64_t words_cap, int32_t *bounds, int64_t lanes_cap,
                                     int32_t *packed_words, int32_t *lanes)
{
  if (!d || !packed_words || !lanes || words_cap < 0 || lanes_cap < 0 || d->pk_last_words <= 0 || d->pk_last_lanes <= 0 || !d->d_bases || !d->d_bounds)
  { ramx_set_error("ramx_dev_peek_windows: bad argument, or nothing has been packed on this device"); return RAMX_ERR_ARG; }
  const int KW = d->pk_last_words, Np = d->pk_last_lanes;
  *packed_words = KW; *lanes = Np;
  if (!words || !bounds || words_cap < (int64_t)KW * Np || lanes_cap < Np)
  { ramx_set_error("ramx_dev_peek_windows: %d words of %d lanes do not fit the caller's buffers", KW, Np); return RAMX_ERR_ARG; }
  HIPCHK(hipSetDevice(d->ordinal));
  { const int src = pack_settle(d, true); if (src != RAMX_OK) return src; }     // a piece still being packed on the second stream
  HIPCHK(hipStreamSynchronize(d->stream));
  HIPCHK(hipMemcpy(words, d->d_bases, (size_t)KW * Np * sizeof(unsigned), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(bounds, d->d_bounds, (size_t)Np * sizeof(int2), hipMemcpyDeviceToHost));
  return RAMX_OK;
}

extern "C" int ramx_dev_peek_family_state(ramx_dev *d, int32_t flank, int32_t *cells)
{
  if (!d) d = ramx_default_device();      // seam 1 runs on the process-wide session
  if (!d || !d->d_cpstate || flank < 0 || flank >= d->cpstate_n || !cells)
  { ramx_set_error("ramx_dev_peek_family_state: nothing kept (set RAMX_CP_PEEK=1 before the batch call)"); return RAMX_ERR_ARG; }
  HIPCHK(hipSetDevice(d->ordinal));
  const int B = 2 * d->cpstate_W + 1;
  HIPCHK(hipMemcpy(cells, d->d_cpstate + (size_t)flank * B, (size_t)B * sizeof(int2), hipMemcpyDeviceToHost));
  return RAMX_OK;
}

// Largest family (extendable cores in one direction) that seam 1 should hand to the one-workgroup-per-family route; larger
// sets go through ramx_dev_run_direction, whose device-wide cell-parallel kernel beats the lane-per-flank family kernel
// (W = 40, 500 flanks: 2.6 vs 7.3 us per column).  512 where the cell-parallel kernel does not apply.
extern "C" int ramx_dev_family_route_max(ramx_dev *d, const ramx_params *p)
{
  if (!d || !p || !p->matrix) return 512;
  int tab9[RAMX_NCLASS][4];
  class_tab(p, tab9);
  if (d->force_chain || getenv("RAMX_NO_CP_DEVICE") != NULL || getenv("RAMX_NO_PERSISTENT") != NULL) return 512;
  const int m = ramx_cp_max_family(p->bandwidth, p->gapopen, p->gapextn, tab9, p->L);
  if (m <= 0) return 512;
  const int s1 = ramx_cp_single_family_max(p->bandwidth);
  return s1 < m ? s1 : m;
}

extern "C" int ramx_dev_set_row_trace(ramx_dev *d, ramx_row_trace_cb cb, void *user)
{
  if (!d) d = ramx_default_device();
  if (!d) return RAMX_ERR_NO_DEVICE;
  d->trace_cb = cb;
  d->trace_user = user;
  return RAMX_OK;
}

extern "C" int ramx_dev_set_row_verbose(ramx_dev *d, ramx_row_verbose_cb cb, void *user)
{
  if (!d) d = ramx_default_device();
  if (!d) return RAMX_ERR_NO_DEVICE;
  d->verbose_cb = cb;
  d->verbose_user = user;
  return RAMX_OK;
}

extern "C" int ramx_dev_set_verbose_band(ramx_dev *d, int on)
{
  if (!d) d = ramx_default_device();
  if (!d) return RAMX_ERR_NO_DEVICE;
  d->verbose_band = on ? 1 : 0;
  return RAMX_OK;
}

extern "C" int ramx_dev_set_allreduce_cb(ramx_dev *d, ramx_allreduce_cb cb, void *user)
{
  if (!d) { ramx_set_error("ramx_dev_set_allreduce_cb: bad argument"); return RAMX_ERR_ARG; }
  d->cb = cb;
  d->cb_user = user;
  return RAMX_OK;
}

extern "C" int ramx_comm_unique_id(uint8_t id[128])
{
  ncclUniqueId u;
  ncclResult_t r = ncclGetUniqueId(&u);
  if (r != ncclSuccess) { ramx_set_error("ncclGetUniqueId: %s", ncclGetErrorString(r)); return RAMX_ERR_COMM; }
  memcpy(id, &u, 128);
  return RAMX_OK;
}

extern "C" int ramx_dev_comm_init(ramx_dev *d, const uint8_t id[128], int rank, int nranks)
{
  if (!d || rank < 0 || rank >= nranks) { ramx_set_error("ramx_dev_comm_init: bad argument"); return RAMX_ERR_ARG; }
  HIPCHK(hipSetDevice(d->ordinal));
  d->rank = rank; d->nranks = nranks;
  if (nranks == 1 && getenv("RAMX_COMM_SINGLE") == NULL) return RAMX_OK;       // one rank: nothing to exchange (RAMX_COMM_SINGLE=1: make the communicator all the same)
  ncclUniqueId u;
  memcpy(&u, id, 128);
  ncclResult_t r = ncclCommInitRank(&d->comm, nranks, u, rank);
  if (r != ncclSuccess) { ramx_set_error("ncclCommInitRank: %s", ncclGetErrorString(r)); d->comm = NULL; return RAMX_ERR_COMM; }
  return RAMX_OK;
}

extern "C" int ramx_dev_comm_size(ramx_dev *d)
{
  if (!d) { ramx_set_error("ramx_dev_comm_size: bad argument"); return RAMX_ERR_ARG; }
  if (!d->comm) return 1;
  int n = 0;
  ncclResult_t r = ncclCommCount(d->comm, &n);
  if (r != ncclSuccess) { ramx_set_error("ncclCommCount: %s", ncclGetErrorString(r)); return RAMX_ERR_COMM; }
  return n;
}
