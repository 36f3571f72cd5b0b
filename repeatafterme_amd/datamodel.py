"""Flat host-side mirror of the reference's in-memory data model.

``CoreSet``  <-> linked list of ``struct coreAlignment`` (reference common.h:80-98)
``FlankSet`` <-> ``struct sequenceLibrary`` + the core list (reference sequence.h:36-46)
``ExtendParams`` <-> the arguments / globals of ``extend_alignment`` (reference
ram_extend.c:859-864, globals :40,:52,:61) plus the scoring system
(score_system.h:7-17).

Base codes are the reference's (sequence.h:7-15): A,C,G,T = 0..3, a,c,g,t = 4..7, N = 99.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

SYM_N = 99
MSIZE = 100  # scoring matrix is [100][100], index [consensus][sequence]


@dataclass
class CoreSet:
    left_pos: np.ndarray      # leftSeqPos   (index into FlankSet.sequence, 0-based closed)
    right_pos: np.ndarray     # rightSeqPos
    lower: np.ndarray         # lowerSeqBound
    upper: np.ndarray         # upperSeqBound
    orient: np.ndarray        # 1 = reverse strand
    left_ext: np.ndarray      # leftExtendable
    right_ext: np.ndarray     # rightExtendable
    seq_idx: Optional[np.ndarray] = None
    left_len: Optional[np.ndarray] = None    # leftExtensionLen  (out)
    right_len: Optional[np.ndarray] = None   # rightExtensionLen (out)
    score: Optional[np.ndarray] = None       # score (accumulates over both directions)
    lower_flag: Optional[np.ndarray] = None  # enum CoreBoundFlag (common.h:10)
    upper_flag: Optional[np.ndarray] = None

    def __post_init__(self):
        n = len(self.left_pos)
        for k in ("left_pos", "right_pos", "lower", "upper"):
            setattr(self, k, np.ascontiguousarray(getattr(self, k), dtype=np.int64))
        for k in ("orient", "left_ext", "right_ext"):
            setattr(self, k, np.ascontiguousarray(getattr(self, k), dtype=np.int8))
        if self.seq_idx is None:
            self.seq_idx = np.arange(n, dtype=np.int32)
        for k in ("seq_idx", "left_len", "right_len", "score", "lower_flag", "upper_flag"):
            v = getattr(self, k)
            setattr(self, k, np.zeros(n, np.int32) if v is None else np.ascontiguousarray(v, dtype=np.int32))

    @property
    def n(self) -> int:
        return len(self.left_pos)

    def copy(self) -> "CoreSet":
        return CoreSet(**{k: getattr(self, k).copy() for k in self.__dataclass_fields__})

    def subset(self, sl) -> "CoreSet":
        return CoreSet(**{k: getattr(self, k)[sl].copy() for k in self.__dataclass_fields__})


@dataclass
class FlankSet:
    sequence: np.ndarray                 # int8 codes, all windows concatenated
    boundaries: np.ndarray               # uint64 cumulative ends, 0-terminated (sequence.h:24-31)
    cores: CoreSet
    offsets: Optional[np.ndarray] = None  # genomic start of each window
    identifiers: Optional[List[str]] = None

    def __post_init__(self):
        self.sequence = np.ascontiguousarray(self.sequence, dtype=np.int8)
        self.boundaries = np.ascontiguousarray(self.boundaries, dtype=np.uint64)
        nseq = len(self.boundaries) - 1
        if self.offsets is None:
            self.offsets = np.zeros(nseq + 1, np.uint64)
        self.offsets = np.ascontiguousarray(self.offsets, dtype=np.uint64)
        if self.identifiers is None:
            self.identifiers = ["s%06d" % i for i in range(nseq)]


@dataclass
class ExtendParams:
    bandwidth: int = 14          # -bandwidth  (ram_extend.c:247)
    cappenalty: int = -90        # per-matrix default (ram_extend.c:301-344)
    minimprovement: int = 27
    L: int = 10000               # -L (ram_extend.c:246)
    when_to_stop: int = 100      # -stopafter (ram_extend.c:249)
    l: int = 1                   # ram_extend.c:40
    gapopen: int = -28
    gapextn: int = -5
    matrix: np.ndarray = field(default=None)   # int32 [100*100] row-major [cons][base]
    matrix_name: str = ""


def new_master(L: int, l: int = 1) -> np.ndarray:
    """master = malloc(2L+l+1) with the l-long N spacer at master[L] (ram_extend.c:347-353,415-416)."""
    m = np.zeros(2 * L + l + 1, np.int8)
    m[L:L + l] = SYM_N
    return m


# one column of a support profile: C-ABI ramx_col_profile (include/ramx.h), 48 bytes
COL_PROFILE_DTYPE = np.dtype([("total", np.int64, (4,)), ("base", np.int32), ("n_capped", np.int32),
                              ("n_new_high", np.int32), ("n_out_of_seq", np.int32)], align=True)
assert COL_PROFILE_DTYPE.itemsize == 48


# per-flank record of an alignment: C-ABI ramx_aln_end (include/ramx.h), 20 bytes
ALN_END_DTYPE = np.dtype([("end_row", np.int32), ("end_idx", np.int32), ("score", np.int32), ("start_idx", np.int32),
                          ("tail_ins", np.int32)])
assert ALN_END_DTYPE.itemsize == 20
ALN_DELETED = -2 ** 31           # RAMX_ALN_DELETED: the column is deleted in this flank
ALN_NONE = -2 ** 31 + 1          # RAMX_ALN_NONE: a column above end_row, or a flank without an alignment


@dataclass
class Alignment:
    """Per-copy alignments of one direction of one family to its kept consensus (C-ABI ramx_alignment / ramx_dev_align)."""
    direction: int
    family: int                      # index in a batch, else 0
    cons: np.ndarray                 # int8 [rows]: the kept consensus (rows = ret)
    flanks: np.ndarray               # FLANK_DTYPE [n_flanks]
    core_index: np.ndarray           # position in the core list of every flank
    ends: np.ndarray                 # ALN_END_DTYPE [n_flanks]
    col_idx: np.ndarray              # int32 [rows][n_flanks]: matched flank position, ALN_DELETED or ALN_NONE
    col_ins: np.ndarray              # int32 [rows][n_flanks]: bases inserted before the column's move


# one column of a pileup: C-ABI ramx_col_pileup (include/ramx.h), 128 bytes
PILEUP_INS = 4                   # RAMX_PILEUP_INS: inserted-base slots kept per column
PILEUP_DTYPE = np.dtype([("base", np.int32), ("cover", np.int32), ("match", np.int32, (5,)), ("del", np.int32),
                         ("ins_open", np.int32), ("ins_long", np.int32), ("ins_bases", np.int64),
                         ("ins", np.int32, (PILEUP_INS, 5))], align=True)
assert PILEUP_DTYPE.itemsize == 128 and PILEUP_DTYPE.fields["ins_bases"][1] == 40


# one pair of adjacent columns (rows r, r + 1) of a dinucleotide pileup: C-ABI ramx_col_dinuc (include/ramx.h), 128 bytes
DINUC_DTYPE = np.dtype([("base", np.int32), ("next", np.int32), ("both", np.int32), ("adjacent", np.int32), ("split", np.int32),
                        ("gapped", np.int32), ("di", np.int32, (5, 5)), ("reserved", np.int32)])
assert DINUC_DTYPE.itemsize == 128


# per-copy statistics of an alignment: C-ABI ramx_copy_stats (include/ramx.h), 48 bytes
COPY_STATS_FIELDS = ("cols", "match", "ts", "tv", "n_match", "del", "del_open", "ins", "ins_open", "cpg_cols", "cpg_ts", "score")
COPY_STATS_DTYPE = np.dtype([(k, np.int32) for k in COPY_STATS_FIELDS])
assert COPY_STATS_DTYPE.itemsize == 48


# co-segregation of variants: C-ABI ramx_plane (8 bytes) and ramx_link (40 bytes), include/ramx.h
PLANE_DTYPE = np.dtype([("row", np.int32), ("cls", np.int32)])
LINK_DTYPE = np.dtype([(k, np.int32) for k in ("p", "q", "n", "n_p", "n_q", "n_pq")] + [("expected", np.float64), ("mlog10p", np.float64)])
assert PLANE_DTYPE.itemsize == 8 and LINK_DTYPE.itemsize == 40
PLANE_COVER = 6                      # RAMX_PLANE_COVER
LINKAGE_MAX_PLANES = 2048            # RAMX_LINKAGE_MAX_PLANES
PLANE_NAMES = ("A", "C", "G", "T", "N", "del", "cover", "ins")


@dataclass
class Linkage:
    """Variants of one direction of one family along its kept consensus and their Gram matrix (C-ABI ramx_linkage)."""
    direction: int
    family: int                      # index in a batch, else 0
    cons: np.ndarray                 # int8 [rows]: the kept consensus (rows = ret)
    cols: np.ndarray                 # PILEUP_DTYPE [rows]
    planes: np.ndarray               # PLANE_DTYPE [P]: the selected variants and their rows' cover planes
    co: np.ndarray                   # int32 [P][P]


# pairwise divergence between copies: C-ABI ramx_copy_dist (24 bytes), include/ramx_dist.h
COPY_DIST_FIELDS = ("cover", "sites", "ts", "tv", "del_one", "del_both")
COPY_DIST_DTYPE = np.dtype([(k, np.int32) for k in COPY_DIST_FIELDS])
assert COPY_DIST_DTYPE.itemsize == 24
DIST_MAX_COPIES = 2048               # RAMX_DIST_MAX_COPIES


@dataclass
class DistSummary:
    """What a pair matrix says together (C-ABI ramx_dist_family)."""
    n: int
    pairs: int
    used: int
    medoid: int                      # place in the list, -1: none
    mean: float
    medoid_mean: float


@dataclass
class Dist:
    """Pairwise divergence between selected copies of one direction of one family along its kept consensus (C-ABI ramx_dist)."""
    direction: int
    family: int                      # index in a batch, else 0
    cons: np.ndarray                 # int8 [rows]: the kept consensus (rows = ret)
    core_index: np.ndarray           # position in the core list of every flank
    ends: np.ndarray                 # ALN_END_DTYPE [n_flanks]
    copies: np.ndarray               # int32 [C]: the selected flanks, ascending
    dist: np.ndarray                 # COPY_DIST_DTYPE [C][C]


SUBFAM_MAX = 8                       # RAMX_SUBFAM_MAX


@dataclass
class SubfamGroup:
    """One kept group of a split: its own refined consensus and pileup (C-ABI ramx_subfam_group)."""
    group: int
    size: int
    refined_cons: np.ndarray         # int8 [refined rows]
    refined_cols: np.ndarray         # PILEUP_DTYPE [refined rows]
    replays: int
    converged: int


@dataclass
class Subfamilies:
    """The copies of one direction of one family split by the linked variants they carry (C-ABI ramx_subfamilies)."""
    direction: int
    family: int                      # index in a batch, else 0
    cons: np.ndarray                 # int8 [rows]: the kept consensus (rows = ret)
    flanks: np.ndarray               # FLANK_DTYPE [n_flanks]
    core_index: np.ndarray           # position in the core list of every flank
    planes: np.ndarray               # PLANE_DTYPE [P]
    labels: np.ndarray               # int32 [n_flanks]
    patterns: np.ndarray             # uint8 [V][K]
    cnt: np.ndarray                  # int32 [K][P]
    size: np.ndarray                 # int32 [K]
    dist: np.ndarray                 # int32 [n_flanks][K]
    iterations: int
    converged: int
    groups: list                     # SubfamGroup, ascending in group: those of at least min_members copies


@dataclass
class Copies:
    """Per-copy statistics of one direction of one family along its kept consensus (C-ABI ramx_copies / ramx_dev_copy_stats)."""
    direction: int
    family: int                      # index in a batch, else 0
    cons: np.ndarray                 # int8 [rows]: the kept consensus (rows = ret)
    flanks: np.ndarray               # FLANK_DTYPE [n_flanks]
    core_index: np.ndarray           # position in the core list of every flank
    ends: np.ndarray                 # ALN_END_DTYPE [n_flanks]
    stats: np.ndarray                # COPY_STATS_DTYPE [n_flanks]


@dataclass
class Refinement:
    """Pileup and refinement of one direction of one family (C-ABI ramx_refinement / ramx_dev_pileup / ramx_dev_refine)."""
    direction: int
    family: int                      # index in a batch, else 0
    cons: np.ndarray                 # int8 [ret]: the kept consensus
    cols: np.ndarray                 # PILEUP_DTYPE [ret]: its pileup
    refined_cons: np.ndarray         # int8 [refined rows]
    refined_cols: np.ndarray         # PILEUP_DTYPE [refined rows]
    replays: int
    converged: int


@dataclass
class CpgRefinement:
    """CpG-aware refinement of one direction of one family (C-ABI ramx_cpg_refinement / ramx_dev_refine_cpg)."""
    direction: int
    family: int                      # index in a batch, else 0
    cons: np.ndarray                 # int8 [ret]: the kept consensus
    refined_cons: np.ndarray         # int8 [refined rows]
    refined_cols: np.ndarray         # PILEUP_DTYPE [refined rows]
    refined_di: np.ndarray           # DINUC_DTYPE [refined rows]
    replays: int
    converged: int
    n_cpg: int                       # row pairs the last re-call called CG


# target-site duplications: C-ABI ramx_tsd_site (32 bytes), ramx_tsd (16 bytes), ramx_tsd_params
TSD_SITE_DTYPE = np.dtype([("lo", np.int64), ("hi", np.int64), ("seq_lo", np.int64), ("seq_hi", np.int64)])
TSD_DTYPE = np.dtype([("k", np.int32), ("mm", np.int32), ("dl", np.int32), ("dr", np.int32)])
assert TSD_SITE_DTYPE.itemsize == 32 and TSD_DTYPE.itemsize == 16


@dataclass
class TsdParams:
    slack: int = 3
    kmin: int = 4
    kmax: int = 20
    mm_div: int = 10


@dataclass
class TsdSummary:
    """What a family's records say together (C-ABI ramx_tsd_hist)."""
    hist: np.ndarray                 # int32 [33]: records by k
    mode: int                        # the k >= 1 with the largest count, ties to the larger k; 0: none
    mode_count: int
    null: np.ndarray                 # float64 [33]: copies expected to show a word of that length by chance


# tandem periodicity: C-ABI ramx_period_seg (16 bytes), ramx_period (32 bytes), ramx_period_params
PERIOD_SEG_DTYPE = np.dtype([("lo", np.int64), ("hi", np.int64)])
PERIOD_DTYPE = np.dtype([("period", np.int32), ("score", np.int32), ("start", np.int32), ("end", np.int32), ("agree", np.int32),
                         ("disagree", np.int32), ("reserved", np.int32, (2,))])
assert PERIOD_SEG_DTYPE.itemsize == 16 and PERIOD_DTYPE.itemsize == 32


@dataclass
class PeriodParams:
    pmax: int = 1024
    mm: int = 3
    min_score: int = 16


@dataclass
class PeriodSummary:
    """What a family's records say together (C-ABI ramx_period_hist)."""
    n: int
    n_tract: int                     # records with a period
    n_mono: int                      # period 1
    n_simple: int                    # period 2..6
    n_tandem: int                    # period >= 7
    at_lo: int                       # tracts that begin at the segment's first base
    at_hi: int                       # tracts that reach its last base
    mode: int                        # the most frequent period, ties to the smaller; 0: none
    mode_count: int


# terminal repeats: C-ABI ramx_term (32 bytes), ramx_term_params, ramx_term_family; the sites are TSD_SITE_DTYPE
TERM_DTYPE = np.dtype([(k, np.int32) for k in ("score", "a_start", "a_end", "b_start", "b_end", "matches", "columns", "T")])
assert TERM_DTYPE.itemsize == 32
TERM_VERDICTS = ("none", "LTR", "TIR")


@dataclass
class TermParams:
    tmax: int = 512
    match: int = 2
    mismatch: int = 3
    gap: int = 5
    min_score: int = 40
    slack: int = 3


@dataclass
class TermSummary:
    """What a family's records say together (C-ABI ramx_term_family)."""
    n: int
    n_direct: int                    # records with a score
    n_inverted: int
    direct_anchored: int             # ... that begin at the 5' terminus and end at the 3' terminus
    inverted_anchored: int           # ... that begin at both termini
    direct_median: int               # lower median of the 5' lengths of the anchored records
    inverted_median: int
    verdict: int                     # 0 none, 1 LTR, 2 TIR (TERM_VERDICTS)
    direct_matches: int
    direct_columns: int
    inverted_matches: int
    inverted_columns: int


# cross-family overlap (include/ramx_xfam.h): C-ABI ramx_seq_pair (16 bytes), ramx_pair_params, ramx_xfam_link_params; the
# records are TERM_DTYPE
SEQ_PAIR_FIELDS = ("a", "b", "inverted", "reserved")
SEQ_PAIR_DTYPE = np.dtype([(k, np.int32) for k in SEQ_PAIR_FIELDS])
assert SEQ_PAIR_DTYPE.itemsize == 16
XFAM_MAXLEN = 32767                  # RAMX_XFAM_MAXLEN


@dataclass
class PairParams:
    match: int = 2
    mismatch: int = 3
    gap: int = 5
    min_score: int = 80


@dataclass
class XfamLinkParams:
    min_columns: int = 80
    min_permille: int = 800


FLANK_DTYPE = np.dtype([("start", np.int64), ("t_lo", np.int32), ("t_hi", np.int32), ("step", np.int8), ("compl_", np.int8),
                        ("pad_", np.int8, (6,))])
assert FLANK_DTYPE.itemsize == 24


@dataclass
class Profile:
    """Per-column support of one direction of one family (C-ABI ramx_profile / ramx_dev_profile)."""
    direction: int
    family: int                      # index in a batch, else 0
    ret: int                         # columns [0, ret) are the kept ones
    cols: np.ndarray                 # COL_PROFILE_DTYPE [n_cols]
    core_index: np.ndarray           # position in the core list of every flank
    last_uncapped_row: np.ndarray    # per flank: last row at which it was not capped under the column's base, -1: none

    @property
    def score(self) -> np.ndarray:
        """curr_extension_score of every column (ram_extend.c:1064-1086): max(0, max_a total[a])."""
        return np.maximum(self.cols["total"].max(axis=1), 0) if len(self.cols) else np.zeros(0, np.int64)
