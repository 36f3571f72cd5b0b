"""Thin Python handle on seam 2 of include/ramx.h (ramx_dev_*): init / upload / run_direction /
download / destroy.  Used by bench.py and the parity tests that want to look below
``extend_alignment`` (state peeks, repeated runs on resident data, the multi-GPU communicator)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from .datamodel import (ALN_END_DTYPE, ALN_NONE, COL_PROFILE_DTYPE, COPY_DIST_DTYPE, COPY_STATS_DTYPE, DistSummary, DINUC_DTYPE, LINK_DTYPE, PILEUP_DTYPE, PILEUP_INS, PLANE_DTYPE,
                        TSD_DTYPE, TSD_SITE_DTYPE, PERIOD_DTYPE, PERIOD_SEG_DTYPE, TERM_DTYPE, CoreSet, ExtendParams, PeriodParams, TermParams, TsdParams)
from .extend import RunInfo, _info, _params


def resolve_flanks(direction: int, cores: CoreSet, bandwidth: int, L: int):
    """-> (flank descriptor array, core index of every flank); C-ABI ramx_resolve_flanks."""
    L_ = _lib.lib()
    fc = _lib.FlatCores(cores.n, *[getattr(cores, k).ctypes.data for k in
                                   ("left_pos", "right_pos", "lower", "upper", "orient", "left_ext",
                                    "right_ext", "left_len", "right_len", "score")])
    flanks = (_lib.Flank * max(cores.n, 1))()
    idx = np.zeros(max(cores.n, 1), np.int32)
    nx = L_.ramx_resolve_flanks(int(direction), C.byref(fc), bandwidth, L, flanks, idx.ctypes.data)
    return (flanks, nx), idx[:nx].copy()


@dataclass
class ProfileResult:
    cols: np.ndarray                       # COL_PROFILE_DTYPE [n_families][L]; only rows[f] entries per family are written
    last_uncapped_row: np.ndarray          # [n_padded]
    row_best: Optional[np.ndarray]         # [max rows][n_padded], or None
    row_best_idx: Optional[np.ndarray]
    kernel_ms: float


@dataclass
class AlignResult:
    ends: np.ndarray                       # ALN_END_DTYPE [n_padded]
    col_idx: Optional[np.ndarray]          # int32 [max rows][n_padded], or None
    col_ins: Optional[np.ndarray]
    forward_ms: float                      # HIP-event time of the forward kernels
    walk_ms: float                         # ... and of the walk kernels


@dataclass
class PileupResult:
    cols: np.ndarray                       # PILEUP_DTYPE [n_families][L]; only rows[f] entries per family are written
    ends: np.ndarray                       # ALN_END_DTYPE [n_padded]
    forward_ms: float                      # HIP-event times of the forward kernels, the walk kernels, the pileup kernels + sum
    walk_ms: float
    pileup_ms: float


@dataclass
class RefineResult:
    cons: np.ndarray                       # int8 [n_families][L]: the refined consensus, rows[f] entries per family
    rows: np.ndarray                       # int32 [n_families]
    replays: np.ndarray                    # int32 [n_families]
    converged: np.ndarray                  # int32 [n_families]
    cols: np.ndarray                       # PILEUP_DTYPE [n_families][L]: the pileup of `cons`
    ends: np.ndarray                       # ALN_END_DTYPE [n_padded]: the alignments along `cons`
    forward_ms: float                      # summed over the replays
    walk_ms: float
    pileup_ms: float


@dataclass
class DinucResult:
    di: np.ndarray                         # DINUC_DTYPE [n_families][L]; only rows[f] entries per family are written
    cols: Optional[np.ndarray]             # PILEUP_DTYPE [n_families][L], or None (pileup=False)
    ends: np.ndarray                       # ALN_END_DTYPE [n_padded]
    kernel_ms: tuple                       # HIP-event times: forward, walk, pileup + sum, dinucleotide kernel + sum


@dataclass
class RefineCpgResult:
    cons: np.ndarray                       # int8 [n_families][L]: the refined consensus, rows[f] entries per family
    rows: np.ndarray                       # int32 [n_families]
    replays: np.ndarray                    # int32 [n_families]
    converged: np.ndarray                  # int32 [n_families]
    n_cpg: np.ndarray                      # int32 [n_families]: row pairs the last re-call called CG
    cols: np.ndarray                       # PILEUP_DTYPE [n_families][L]: the pileup of `cons`
    di: np.ndarray                         # DINUC_DTYPE [n_families][L]: its dinucleotide pileup
    ends: np.ndarray                       # ALN_END_DTYPE [n_padded]: the alignments along `cons`
    kernel_ms: tuple                       # as DinucResult's, summed over the replays


@dataclass
class CopyStatsResult:
    stats: np.ndarray                      # COPY_STATS_DTYPE [n_padded]
    ends: np.ndarray                       # ALN_END_DTYPE [n_padded]
    kernel_ms: tuple                       # HIP-event times of the forward kernels, the walk kernels, the statistics kernel


@dataclass
class PlanesResult:
    cols: np.ndarray                       # PILEUP_DTYPE [n_families][L], as PileupResult
    ends: np.ndarray                       # ALN_END_DTYPE [n_padded]
    kernel_ms: tuple                       # HIP-event times: forward, walk, pileup + sum, planes
    fam_count: np.ndarray                  # int32 [n_families]: what plane_gram sizes `bits` with


def select_planes(cons, cols, min_count: int = 4, min_permille: int = 100, max_variants: int = 1024) -> np.ndarray:
    """The variants of a pileup and their rows' cover planes (C-ABI ramx_select_planes, host C): -> PLANE_DTYPE [P]."""
    c = np.ascontiguousarray(cons, np.int8)
    pl = np.ascontiguousarray(cols, PILEUP_DTYPE).reshape(-1)
    assert len(pl) >= len(c)
    out = np.zeros(max(2 * max(int(max_variants), 0), 1), PLANE_DTYPE)
    n = _lib.lib().ramx_select_planes(c.ctypes.data, len(c), pl.ctypes.data, int(min_count), int(min_permille), int(max_variants),
                                      out.ctypes.data)
    return out[:n].copy()


def link_pairs(planes, co, min_mlog10p: float = 0.0, cap: Optional[int] = None):
    """The pair statistic on a Gram matrix (C-ABI ramx_link_pairs, host C): -> (LINK_DTYPE [min(found, cap)], found)."""
    pl = np.ascontiguousarray(planes, PLANE_DTYPE).reshape(-1)
    P = len(pl)
    m = np.ascontiguousarray(co, np.int32)
    assert m.size == P * P
    if cap is None:
        cap = P * (P - 1) // 2
    out = np.zeros(max(cap, 1), LINK_DTYPE)
    n = _lib.lib().ramx_link_pairs(pl.ctypes.data, P, m.ctypes.data, float(min_mlog10p), out.ctypes.data, int(cap))
    return out[:min(n, cap)].copy(), int(n)


def link_components(planes, links, K: int = 4):
    """The initial patterns of a split into subfamilies from the linked pairs (C-ABI ramx_link_components, host C).  links:
    LINK_DTYPE records as link_pairs returns them at the caller's threshold.  -> (init uint8 [V][K'], component int32 [V]), K' = 1 +
    the components kept."""
    pl = np.ascontiguousarray(planes, PLANE_DTYPE).reshape(-1)
    lk = np.ascontiguousarray(links, LINK_DTYPE).reshape(-1)
    V = int((pl["cls"] != 6).sum())
    init = np.zeros(max(V * max(int(K), 1), 1), np.uint8)
    comp = np.zeros(max(V, 1), np.int32)
    kp = _lib.lib().ramx_link_components(pl.ctypes.data, len(pl), lk.ctypes.data, len(lk), int(K), init.ctypes.data, comp.ctypes.data)
    if kp < 1:
        raise _lib.RamxError(f"ramx_link_components: K = {K} outside 1..8, or a link outside the list")
    return init[:V * kp].reshape(V, kp).copy(), comp[:V].copy()


@dataclass
class SubfamResult:
    labels: np.ndarray                     # int32 [flanks of the family]: the group of every copy
    patterns: np.ndarray                   # uint8 [V][K]: the patterns of the last assignment
    cnt: np.ndarray                        # int32 [K][P]: copies of group k with the listed plane's bit set
    size: np.ndarray                       # int32 [K]
    iterations: int                        # assignments made
    converged: int
    masks: Optional[np.ndarray]            # uint64 [K][T]: the groups as bit planes, or None


def select_copies(ends, rows: int, min_cols: int = 1, max_copies: int = 256) -> np.ndarray:
    """Which copies to compare (C-ABI ramx_select_copies, host C): those of at least min_cols columns along `rows` rows, the
    longest max_copies of them.  -> int32 [C], ascending."""
    e = np.ascontiguousarray(ends, ALN_END_DTYPE).reshape(-1)
    out = np.zeros(max(len(e), 1), np.int32)
    n = _lib.lib().ramx_select_copies(e.ctypes.data if len(e) else None, len(e), int(rows), int(min_cols), int(max_copies), out.ctypes.data)
    return out[:n].copy()


def dist_kimura(rec) -> float:
    """Kimura two-parameter distance (percent) of one COPY_DIST_DTYPE record (C-ABI ramx_dist_kimura); < 0: undefined."""
    r = np.ascontiguousarray(rec, COPY_DIST_DTYPE).reshape(-1)
    assert len(r) == 1
    return float(_lib.lib().ramx_dist_kimura(r.ctypes.data))


def dist_summary(m, min_sites: int = 1) -> DistSummary:
    """Mean Kimura distance and medoid of a COPY_DIST_DTYPE [n][n] matrix (C-ABI ramx_dist_summary, host C)."""
    a = np.ascontiguousarray(m, COPY_DIST_DTYPE)
    n = int(round(a.size ** 0.5))
    assert n * n == a.size
    out = _lib.DistFamily()
    _lib.check(_lib.lib().ramx_dist_summary(a.ctypes.data if n else None, n, int(min_sites), C.byref(out)), "ramx_dist_summary")
    return DistSummary(int(out.n), int(out.pairs), int(out.used), int(out.medoid), float(out.mean), float(out.medoid_mean))


def copy_kimura(stats) -> float:
    """Kimura two-parameter divergence (percent) of one COPY_STATS_DTYPE record (C-ABI ramx_copy_kimura); < 0: undefined."""
    s = np.ascontiguousarray(stats, COPY_STATS_DTYPE).reshape(-1)
    assert len(s) == 1
    return float(_lib.lib().ramx_copy_kimura(s.ctypes.data))


def family_divergence_of(stats, min_sites: int = 1):
    """Mean Kimura divergence over the records with at least min_sites sites and a defined value (C-ABI
    ramx_family_divergence): -> (percent, number of records used)."""
    s = np.ascontiguousarray(stats, COPY_STATS_DTYPE).reshape(-1)
    used = C.c_int32()
    div = _lib.lib().ramx_family_divergence(s.ctypes.data if len(s) else None, len(s), int(min_sites), C.byref(used))
    return float(div), int(used.value)


def recall_consensus(cons, cols, L: int) -> np.ndarray:
    """Re-call a consensus from its pileup (C-ABI ramx_recall_consensus, host C): -> the new consensus, at most L columns."""
    c = np.ascontiguousarray(cons, np.int8)
    cols = np.ascontiguousarray(cols, PILEUP_DTYPE)
    assert len(cols) >= len(c)
    out = np.zeros(max(L, 1), np.int8)
    n = _lib.lib().ramx_recall_consensus(c.ctypes.data, len(c), cols.ctypes.data, int(L), out.ctypes.data)
    return out[:n].copy()


def recall_cpg(cons, cols, di, matrix, rows_reversed: bool = False, cpg_ts: int = 0, L: Optional[int] = None):
    """CpG-aware re-call of a consensus from its pileup and dinucleotide pileup (C-ABI ramx_recall_cpg, host C); matrix as
    ExtendParams.matrix.  -> (the new consensus, at most L columns, and the row pairs it called CG)."""
    c = np.ascontiguousarray(cons, np.int8)
    cols = np.ascontiguousarray(cols, PILEUP_DTYPE)
    di = np.ascontiguousarray(di, DINUC_DTYPE)
    m = np.ascontiguousarray(matrix, np.int32)
    assert len(cols) >= len(c) and len(di) >= len(c) and m.size == 100 * 100
    L = len(c) + PILEUP_INS * len(c) if L is None else int(L)
    out = np.zeros(max(L, 1), np.int8)
    n_cpg = C.c_int32()
    n = _lib.lib().ramx_recall_cpg(c.ctypes.data, len(c), cols.ctypes.data, di.ctypes.data, int(bool(rows_reversed)), m.ctypes.data,
                                   int(cpg_ts), L, out.ctypes.data, C.byref(n_cpg))
    return out[:n].copy(), int(n_cpg.value)


def pad_flanks(flanks):
    """(flank array, n) -> the same flanks padded to a multiple of 64 with empty flanks (t_lo = 1, t_hi = 0)."""
    arr, nx = flanks
    npad = max((nx + 63) // 64 * 64, 64)
    out = (_lib.Flank * npad)()
    for i in range(npad):
        if i < nx:
            out[i] = arr[i]
        else:
            out[i].t_lo, out[i].t_hi, out[i].step = 1, 0, 1
    return out, npad


def _flatten(lists, dtype):
    """Per-family arrays as the C-ABI takes them -> (all of them in one array, which is never empty; first and count per family,
    int32)."""
    cnt = np.array([len(x) for x in lists], np.int32)
    return np.concatenate(list(lists) + [np.zeros(1, dtype)]), (np.cumsum(cnt) - cnt).astype(np.int32), cnt


def _starts(sizes):
    """int64 sizes per family -> where each family begins in one array of them all"""
    return (np.cumsum(sizes) - sizes).astype(np.int64)


class Device:
    def __init__(self, ordinal: int = 0):
        self._L = _lib.lib()
        h = C.c_void_p()
        _lib.check(self._L.ramx_dev_create(ordinal, C.byref(h)), "ramx_dev_create")
        self._h = h
        self._keep = None
        self.nx = 0
        self.p = None

    def close(self):
        if self._h:
            self._L.ramx_dev_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_library(self, sequence: np.ndarray):
        assert sequence.dtype == np.int8 and sequence.flags.c_contiguous
        _lib.check(self._L.ramx_dev_load_library(self._h, sequence.ctypes.data, len(sequence)), "ramx_dev_load_library")

    def load_library_packed(self, tables: dict):
        """The packed form of a library (C-ABI ramx_dev_load_library_packed); tables as loader.pack_library makes them."""
        from .loader import _Packed
        keep = {k: np.ascontiguousarray(tables[k], dt) for k, dt in
                (("win_start", np.uint64), ("win_byte", np.uint64), ("win_phase", np.uint8), ("bytes", np.uint8),
                 ("n_start", np.uint64), ("n_len", np.uint32))}
        ptr = lambda k, ct: keep[k].ctypes.data_as(C.POINTER(ct))       # noqa: E731
        pk = _Packed(int(tables["length"]), len(keep["win_phase"]), ptr("win_start", C.c_uint64), ptr("win_byte", C.c_uint64),
                     ptr("win_phase", C.c_uint8), ptr("bytes", C.c_uint8), len(keep["bytes"]), ptr("n_start", C.c_uint64),
                     ptr("n_len", C.c_uint32), len(keep["n_len"]))
        self._L.ramx_dev_load_library_packed.argtypes = [C.c_void_p, C.POINTER(_Packed)]
        _lib.check(self._L.ramx_dev_load_library_packed(self._h, C.byref(pk)), "ramx_dev_load_library_packed")

    def tsd(self, sites, tp: Optional[TsdParams] = None, timing: bool = False):
        """The target-site duplication of every site on the library this device holds (C-ABI ramx_dev_tsd): -> TSD_DTYPE
        [n_sites]; timing=True: (records, [pack ms, kernel ms])."""
        s = np.ascontiguousarray(sites, TSD_SITE_DTYPE).reshape(-1)
        tp = TsdParams() if tp is None else tp
        cp = _lib.TsdParams(int(tp.slack), int(tp.kmin), int(tp.kmax), int(tp.mm_div))
        out = np.zeros(len(s), TSD_DTYPE)
        ms = (C.c_double * 2)()
        _lib.check(self._L.ramx_dev_tsd(self._h, s.ctypes.data if len(s) else None, len(s), C.byref(cp),
                                        out.ctypes.data if len(s) else None, ms), "ramx_dev_tsd")
        return (out, [ms[0], ms[1]]) if timing else out

    def period(self, segs, pp: Optional[PeriodParams] = None, timing: bool = False):
        """The tandem periodicity of every segment (lo, hi) on the library this device holds (C-ABI ramx_dev_period): ->
        PERIOD_DTYPE [n_segs]; timing=True: (records, [pack ms, squeeze ms, scan ms])."""
        s = np.ascontiguousarray(segs, PERIOD_SEG_DTYPE).reshape(-1)
        pp = PeriodParams() if pp is None else pp
        cp = _lib.PeriodParams(int(pp.pmax), int(pp.mm), int(pp.min_score), 0)
        out = np.zeros(len(s), PERIOD_DTYPE)
        ms = (C.c_double * 3)()
        _lib.check(self._L.ramx_dev_period(self._h, s.ctypes.data if len(s) else None, len(s), C.byref(cp),
                                           out.ctypes.data if len(s) else None, ms), "ramx_dev_period")
        return (out, [ms[0], ms[1], ms[2]]) if timing else out

    def term(self, sites, tp: Optional[TermParams] = None, timing: bool = False):
        """The terminal repeats of every site on the library this device holds (C-ABI ramx_dev_term): -> TERM_DTYPE [n_sites][2],
        direct and inverted; timing=True: (records, [pack ms, squeeze ms, align ms])."""
        s = np.ascontiguousarray(sites, TSD_SITE_DTYPE).reshape(-1)
        tp = TermParams() if tp is None else tp
        cp = _lib.TermParams(int(tp.tmax), int(tp.match), int(tp.mismatch), int(tp.gap), int(tp.min_score), int(tp.slack))
        out = np.zeros((len(s), 2), TERM_DTYPE)
        ms = (C.c_double * 3)()
        _lib.check(self._L.ramx_dev_term(self._h, s.ctypes.data if len(s) else None, len(s), C.byref(cp),
                                         out.ctypes.data if len(s) else None, ms), "ramx_dev_term")
        return (out, [ms[0], ms[1], ms[2]]) if timing else out

    def begin_direction(self, flanks, p: ExtendParams):
        arr, nx = flanks
        cp, keep = _params(p)
        self._keep = keep
        _lib.check(self._L.ramx_dev_begin_direction(self._h, arr, nx, C.byref(cp)), "ramx_dev_begin_direction")
        self.nx, self.p = nx, p

    def run_direction(self) -> RunInfo:
        ci = _lib.RunInfo()
        _lib.check(self._L.ramx_dev_run_direction(self._h, C.byref(ci)), "ramx_dev_run_direction")
        self.last = _info(ci)
        return self.last

    def download(self):
        rows = self.last.rows_executed
        cons = np.zeros(max(rows, 1), np.int8)
        th = np.zeros(max(self.nx, 1), np.int32)
        tp = np.zeros(max(self.nx, 1), np.int32)
        _lib.check(self._L.ramx_dev_download(self._h, cons.ctypes.data, len(cons), th.ctypes.data, tp.ctypes.data),
                   "ramx_dev_download")
        return cons[:rows], th[:self.nx], tp[:self.nx]

    def _families(self, flanks, p, cons, rows, fam_first, fam_count):
        """The argument forms of profile() -> (flank array, n_padded, first, count, cons [nf][L], rows)."""
        L = p.L
        if fam_first is None:
            n = flanks[1]
            arr, npad = pad_flanks(flanks)
            fam_first, fam_count = [0], [n]
            c1 = np.asarray(cons, np.int8).ravel()
            rows = [len(c1) if rows is None else int(rows)]
            cons = np.zeros((1, max(L, 1)), np.int8)
            cons[0, :min(len(c1), L)] = c1[:L]
        else:
            arr, npad = flanks
        nf = len(fam_first)
        first = np.ascontiguousarray(fam_first, np.int32)
        count = np.ascontiguousarray(fam_count, np.int32)
        rows_a = np.ascontiguousarray(rows, np.int32)
        cons = np.ascontiguousarray(cons, np.int8)
        assert cons.size >= nf * L and len(rows_a) == nf
        return arr, npad, first, count, cons, rows_a

    @staticmethod
    def _no_ends(npad):
        ends = np.zeros(max(npad, 1), ALN_END_DTYPE)
        ends["end_row"] = ends["end_idx"] = -1
        return ends

    def profile(self, flanks, p: ExtendParams, cons, rows=None, fam_first=None, fam_count=None, row_best: bool = False,
                out: Optional[np.ndarray] = None) -> ProfileResult:
        """Replay flanks along a given consensus (C-ABI ramx_dev_profile).  One family: `flanks` = (array, n) as
        resolve_flanks returns it (padded here), `cons` a 1-D int8 array, `rows` its length unless given.  Several families:
        `flanks` = (array, n_padded) already laid out in tiles of 64, fam_first / fam_count per family, `cons`
        [n_families][L], `rows` per family.  `out`: a COL_PROFILE_DTYPE array [n_families][L] to write into (entries beyond
        rows[f] are left alone)."""
        cp, keep = _params(p)
        arr, npad, first, count, cons, rows_a = self._families(flanks, p, cons, rows, fam_first, fam_count)
        nf, L = len(first), p.L
        cols = out if out is not None else np.zeros((nf, max(L, 1)), COL_PROFILE_DTYPE)
        assert cols.dtype == COL_PROFILE_DTYPE and cols.flags.c_contiguous and cols.size >= nf * L
        last = np.full(max(npad, 1), -1, np.int32)
        rb = rbi = None
        if row_best:
            mr = int(rows_a.max()) if nf else 0
            rb = np.zeros((max(mr, 1), max(npad, 1)), np.int32)
            rbi = np.zeros((max(mr, 1), max(npad, 1)), np.int32)
        ms = C.c_double()
        _lib.check(self._L.ramx_dev_profile(self._h, arr, npad, first.ctypes.data, count.ctypes.data, nf, C.byref(cp),
                                            cons.ctypes.data, rows_a.ctypes.data, cols.ctypes.data, last.ctypes.data,
                                            rb.ctypes.data if row_best else None, rbi.ctypes.data if row_best else None,
                                            C.byref(ms)), "ramx_dev_profile")
        return ProfileResult(cols, last[:npad], rb, rbi, ms.value)

    def align(self, flanks, p: ExtendParams, cons, rows=None, fam_first=None, fam_count=None, columns: bool = True,
              out: Optional[AlignResult] = None) -> AlignResult:
        """Align every flank to a given consensus (C-ABI ramx_dev_align): arguments as profile().  columns=False: only the
        per-flank records.  `out`: a result to write into (entries of tiles outside every family are left alone)."""
        cp, keep = _params(p)
        arr, npad, first, count, cons, rows_a = self._families(flanks, p, cons, rows, fam_first, fam_count)
        nf = len(first)
        mr = max(int(rows_a.max()) if nf else 0, 0)
        if out is not None:
            ends, idx, ins = out.ends, out.col_idx, out.col_ins
            assert ends.dtype == ALN_END_DTYPE and ends.flags.c_contiguous and len(ends) >= npad
            assert not columns or (idx.shape == ins.shape and idx.shape[0] >= mr and idx.shape[1] == npad and
                                   idx.flags.c_contiguous and ins.flags.c_contiguous)
        else:
            ends = self._no_ends(npad)
            idx = np.full((max(mr, 1), max(npad, 1)), ALN_NONE, np.int32) if columns else None
            ins = np.zeros((max(mr, 1), max(npad, 1)), np.int32) if columns else None
        ms = (C.c_double * 2)()
        _lib.check(self._L.ramx_dev_align(self._h, arr, npad, first.ctypes.data, count.ctypes.data, nf, C.byref(cp),
                                          cons.ctypes.data, rows_a.ctypes.data, ends.ctypes.data,
                                          idx.ctypes.data if columns else None, ins.ctypes.data if columns else None, ms),
                   "ramx_dev_align")
        return AlignResult(ends, idx if columns else None, ins if columns else None, ms[0], ms[1])

    def pileup(self, flanks, p: ExtendParams, cons, rows=None, fam_first=None, fam_count=None) -> PileupResult:
        """Pileup of every family along a given consensus (C-ABI ramx_dev_pileup): arguments as profile()."""
        cp, keep = _params(p)
        arr, npad, first, count, cons, rows_a = self._families(flanks, p, cons, rows, fam_first, fam_count)
        nf = len(first)
        cols = np.zeros((nf, max(p.L, 1)), PILEUP_DTYPE)
        ends = self._no_ends(npad)
        ms = (C.c_double * 3)()
        _lib.check(self._L.ramx_dev_pileup(self._h, arr, npad, first.ctypes.data, count.ctypes.data, nf, C.byref(cp),
                                           cons.ctypes.data, rows_a.ctypes.data, cols.ctypes.data, ends.ctypes.data, ms),
                   "ramx_dev_pileup")
        return PileupResult(cols, ends, ms[0], ms[1], ms[2])

    def dinuc(self, flanks, p: ExtendParams, cons, rows=None, fam_first=None, fam_count=None, pileup: bool = True) -> DinucResult:
        """Dinucleotide pileup of every family along a given consensus, and its pileup from the same walk unless pileup=False
        (C-ABI ramx_dev_dinuc): arguments as profile()."""
        cp, keep = _params(p)
        arr, npad, first, count, cons, rows_a = self._families(flanks, p, cons, rows, fam_first, fam_count)
        nf = len(first)
        di = np.zeros((nf, max(p.L, 1)), DINUC_DTYPE)
        cols = np.zeros((nf, max(p.L, 1)), PILEUP_DTYPE) if pileup else None
        ends = self._no_ends(npad)
        ms = (C.c_double * 4)()
        _lib.check(self._L.ramx_dev_dinuc(self._h, arr, npad, first.ctypes.data, count.ctypes.data, nf, C.byref(cp),
                                          cons.ctypes.data, rows_a.ctypes.data, cols.ctypes.data if pileup else None, di.ctypes.data,
                                          ends.ctypes.data, ms), "ramx_dev_dinuc")
        return DinucResult(di, cols, ends, tuple(ms))

    def refine_cpg(self, flanks, p: ExtendParams, cons, rows=None, fam_first=None, fam_count=None, max_replays: int = 10,
                   rows_reversed: bool = False, cpg_ts: int = 0) -> RefineCpgResult:
        """refine() with the CpG-aware re-call (C-ABI ramx_dev_refine_cpg): arguments as profile(); rows_reversed: the rows run
        against the reading order (a left extension)."""
        cp, keep = _params(p)
        arr, npad, first, count, cons, rows_a = self._families(flanks, p, cons, rows, fam_first, fam_count)
        nf = len(first)
        out = np.zeros((nf, max(p.L, 1)), np.int8)
        rows_out, replays, conv, n_cpg = (np.zeros(max(nf, 1), np.int32) for _ in range(4))
        cols = np.zeros((nf, max(p.L, 1)), PILEUP_DTYPE)
        di = np.zeros((nf, max(p.L, 1)), DINUC_DTYPE)
        ends = self._no_ends(npad)
        ms = (C.c_double * 4)()
        _lib.check(self._L.ramx_dev_refine_cpg(self._h, arr, npad, first.ctypes.data, count.ctypes.data, nf, C.byref(cp),
                                               cons.ctypes.data, rows_a.ctypes.data, int(max_replays), int(bool(rows_reversed)),
                                               int(cpg_ts), out.ctypes.data, rows_out.ctypes.data, replays.ctypes.data,
                                               conv.ctypes.data, cols.ctypes.data, di.ctypes.data, n_cpg.ctypes.data,
                                               ends.ctypes.data, ms), "ramx_dev_refine_cpg")
        return RefineCpgResult(out, rows_out[:nf], replays[:nf], conv[:nf], n_cpg[:nf], cols, di, ends, tuple(ms))

    def copy_stats(self, flanks, p: ExtendParams, cons, rows=None, fam_first=None, fam_count=None, rows_reversed: bool = False,
                   out: Optional[np.ndarray] = None) -> CopyStatsResult:
        """Per-copy statistics of every family along a given consensus (C-ABI ramx_dev_copy_stats): arguments as profile().
        rows_reversed: the rows run against the reading order (a left extension).  `out`: a COPY_STATS_DTYPE array [n_padded]
        to write into (records of tiles outside every family are left alone)."""
        cp, keep = _params(p)
        arr, npad, first, count, cons, rows_a = self._families(flanks, p, cons, rows, fam_first, fam_count)
        nf = len(first)
        stats = out if out is not None else np.zeros(max(npad, 1), COPY_STATS_DTYPE)
        assert stats.dtype == COPY_STATS_DTYPE and stats.flags.c_contiguous and len(stats) >= npad
        ends = self._no_ends(npad)
        ms = (C.c_double * 3)()
        _lib.check(self._L.ramx_dev_copy_stats(self._h, arr, npad, first.ctypes.data, count.ctypes.data, nf, C.byref(cp),
                                               cons.ctypes.data, rows_a.ctypes.data, int(bool(rows_reversed)), stats.ctypes.data,
                                               ends.ctypes.data, ms), "ramx_dev_copy_stats")
        return CopyStatsResult(stats, ends, (ms[0], ms[1], ms[2]))

    def planes(self, flanks, p: ExtendParams, cons, rows=None, fam_first=None, fam_count=None) -> PlanesResult:
        """The pileup of every family along a given consensus, and its bit planes left resident on the device for plane_gram()
        (C-ABI ramx_dev_planes): arguments as profile()."""
        cp, keep = _params(p)
        arr, npad, first, count, cons, rows_a = self._families(flanks, p, cons, rows, fam_first, fam_count)
        nf = len(first)
        cols = np.zeros((nf, max(p.L, 1)), PILEUP_DTYPE)
        ends = self._no_ends(npad)
        ms = (C.c_double * 4)()
        _lib.check(self._L.ramx_dev_planes(self._h, arr, npad, first.ctypes.data, count.ctypes.data, nf, C.byref(cp),
                                           cons.ctypes.data, rows_a.ctypes.data, cols.ctypes.data, ends.ctypes.data, ms),
                   "ramx_dev_planes")
        self._resident = ((count + 63) // 64, first.copy(), count.copy(), npad)
        return PlanesResult(cols, ends, tuple(ms), count)

    def _resident_families(self, nf):
        """(tiles, first flank, flanks) of nf families and n_padded of the last planes(); zeros before any, and for the families
        it did not have (the library refuses such a call)."""
        tiles, first, count, npad = getattr(self, "_resident", (np.zeros(0, np.int32),) * 3 + (0,))
        return tuple([int(a[f]) if f < len(a) else 0 for f in range(nf)] for a in (tiles, first, count)) + (npad,)

    def plane_gram(self, planes, bits: bool = False):
        """The Gram matrix of chosen planes of the resident replay (C-ABI ramx_dev_plane_gram).  `planes`: one PLANE_DTYPE
        array (one family), or a list of them, one per family of the planes() call.  -> co (int32 [P][P]), or (co, bits) with
        bits uint64 [P][T]; lists of them for a list."""
        one = not isinstance(planes, (list, tuple))
        lists = [np.ascontiguousarray(x, PLANE_DTYPE).reshape(-1) for x in ([planes] if one else planes)]
        nf = len(lists)
        tiles = self._resident_families(nf)[0]
        allp, first, cnt = _flatten(lists, PLANE_DTYPE)
        cells = cnt.astype(np.int64) ** 2
        co_first = _starts(cells)
        co = np.full(max(int(cells.sum()), 1), -1, np.int32)
        bsz = cnt.astype(np.int64) * np.array(tiles, np.int64)
        b_first = _starts(bsz)
        bw = np.zeros(max(int(bsz.sum()), 1), np.uint64) if bits else None
        _lib.check(self._L.ramx_dev_plane_gram(self._h, nf, allp.ctypes.data, first.ctypes.data, cnt.ctypes.data, co.ctypes.data,
                                               co_first.ctypes.data, bw.ctypes.data if bits else None,
                                               b_first.ctypes.data if bits else None), "ramx_dev_plane_gram")
        cos = [co[co_first[f]:co_first[f] + int(cnt[f]) ** 2].reshape(int(cnt[f]), int(cnt[f])) for f in range(nf)]
        if not bits:
            return cos[0] if one else cos
        bws = [bw[b_first[f]:b_first[f] + bsz[f]].reshape(int(cnt[f]), tiles[f]) for f in range(nf)]
        return (cos[0], bws[0]) if one else (cos, bws)

    def copy_dist(self, copies, fill=None):
        """The pair matrix of chosen copies of the resident replay (C-ABI ramx_dev_copy_dist).  `copies`: one int32 array of
        flank indices within the family (one family), or a list of them, one per family of the planes() call.  -> COPY_DIST_DTYPE
        [C][C]; a list of them for a list.  fill: the byte the result buffer holds before the call (tests)."""
        one = not isinstance(copies, (list, tuple))
        lists = [np.ascontiguousarray(x, np.int32).reshape(-1) for x in ([copies] if one else copies)]
        nf = len(lists)
        allc, first, cnt = _flatten(lists, np.int32)
        cells = cnt.astype(np.int64) ** 2
        o_first = _starts(cells)
        out = np.zeros(max(int(cells.sum()), 1), COPY_DIST_DTYPE)
        if fill is not None:
            out.view(np.uint8)[:] = fill
        _lib.check(self._L.ramx_dev_copy_dist(self._h, nf, allc.ctypes.data, first.ctypes.data, cnt.ctypes.data, out.ctypes.data,
                                              o_first.ctypes.data), "ramx_dev_copy_dist")
        ms = [out[o_first[f]:o_first[f] + int(cells[f])].reshape(int(cnt[f]), int(cnt[f])) for f in range(nf)]
        return ms[0] if one else ms

    def copy_dist_ms(self):
        """HIP-event times of the transposition and the pair kernel of the last copy_dist() (C-ABI ramx_dev_copy_dist_ms)."""
        ms = (C.c_double * 2)()
        self._L.ramx_dev_copy_dist_ms(self._h, ms)
        return float(ms[0]), float(ms[1])

    def subfamilies(self, planes, init, max_iter: int = 8, masks: bool = False, K: Optional[int] = None):
        """The copies of every family of the resident replay split by the variants they carry (C-ABI ramx_dev_subfamilies).
        `planes` as plane_gram(); `init`: uint8 [V][K] per family (link_components), the same K for all.  -> SubfamResult, or a
        list of them for a list."""
        one = not isinstance(planes, (list, tuple))
        lists = [np.ascontiguousarray(x, PLANE_DTYPE).reshape(-1) for x in ([planes] if one else planes)]
        inits = [np.ascontiguousarray(x, np.uint8) for x in ([init] if one else init)]
        nf = len(lists)
        V = [int((x["cls"] != 6).sum()) for x in lists]
        if K is None:
            K = next((int(x.shape[1]) for x in inits if x.ndim == 2), 1)
        for f in range(nf):
            assert not 1 <= K <= 8 or inits[f].size == V[f] * K, (f, inits[f].shape, V[f], K)     # another K: the library refuses it
        tiles, first_f, count_f, npad = self._resident_families(nf)
        allp, first, cnt = _flatten(lists, PLANE_DTYPE)
        alli = np.concatenate([x.reshape(-1) for x in inits] + [np.zeros(1, np.uint8)])
        labels = np.full(max(npad, 1), -2, np.int32)
        pats = np.full(max(sum(V) * max(K, 1), 1), 255, np.uint8)
        counts = np.full(max(int(cnt.sum()) * max(K, 1), 1), -1, np.int32)
        size = np.full(max(nf * max(K, 1), 1), -1, np.int32)
        its, conv = np.full(max(nf, 1), -1, np.int32), np.full(max(nf, 1), -1, np.int32)
        _lib.check(self._L.ramx_dev_subfamilies(self._h, nf, allp.ctypes.data, first.ctypes.data, cnt.ctypes.data, alli.ctypes.data,
                                                int(K), int(max_iter), labels.ctypes.data, pats.ctypes.data, counts.ctypes.data,
                                                size.ctypes.data, its.ctypes.data, conv.ctypes.data), "ramx_dev_subfamilies")
        out, v0 = [], 0
        for f in range(nf):
            P, T = int(cnt[f]), tiles[f]
            mk = None
            if masks:
                mk = np.zeros((K, T), np.uint64)
                buf = np.zeros(max(K * T, 1), np.uint64)
                _lib.check(self._L.ramx_dev_subfam_masks(self._h, f, buf.ctypes.data), "ramx_dev_subfam_masks")
                mk = buf[:K * T].reshape(K, T)
            out.append(SubfamResult(labels[first_f[f]:first_f[f] + count_f[f]].copy(),
                                    pats[K * v0:K * (v0 + V[f])].reshape(V[f], K).copy(),
                                    counts[K * int(first[f]):K * (int(first[f]) + P)].reshape(K, P).copy(),
                                    size[f * K:(f + 1) * K].copy(), int(its[f]), int(conv[f]), mk))
            v0 += V[f]
        self._subfam_labels = labels[:npad]
        return out[0] if one else out

    def subfam_ms(self):
        """HIP-event times of the assign and the count kernels of the last subfamilies(), summed over its iterations."""
        ms = (C.c_double * 2)()
        self._L.ramx_dev_subfam_ms(self._h, ms)
        return float(ms[0]), float(ms[1])

    def plane_gram_ms(self) -> float:
        """HIP-event time of the Gram kernel of the last plane_gram() (C-ABI ramx_dev_plane_gram_ms)."""
        return float(self._L.ramx_dev_plane_gram_ms(self._h))

    def refine(self, flanks, p: ExtendParams, cons, rows=None, fam_first=None, fam_count=None,
               max_replays: int = 10) -> RefineResult:
        """Replay -> re-call -> replay until the consensus is stable or max_replays replays have run (C-ABI ramx_dev_refine):
        arguments as profile()."""
        cp, keep = _params(p)
        arr, npad, first, count, cons, rows_a = self._families(flanks, p, cons, rows, fam_first, fam_count)
        nf = len(first)
        out = np.zeros((nf, max(p.L, 1)), np.int8)
        rows_out, replays, conv = (np.zeros(max(nf, 1), np.int32) for _ in range(3))
        cols = np.zeros((nf, max(p.L, 1)), PILEUP_DTYPE)
        ends = self._no_ends(npad)
        ms = (C.c_double * 3)()
        _lib.check(self._L.ramx_dev_refine(self._h, arr, npad, first.ctypes.data, count.ctypes.data, nf, C.byref(cp),
                                           cons.ctypes.data, rows_a.ctypes.data, int(max_replays), out.ctypes.data,
                                           rows_out.ctypes.data, replays.ctypes.data, conv.ctypes.data, cols.ctypes.data,
                                           ends.ctypes.data, ms), "ramx_dev_refine")
        return RefineResult(out, rows_out[:nf], replays[:nf], conv[:nf], cols, ends, ms[0], ms[1], ms[2])

    def peek_state(self, flank: int):
        B = 2 * self.p.bandwidth + 1
        cells = np.zeros(4 * (self.p.bandwidth + 1), np.int32)
        hi, po = C.c_int32(), C.c_int32()
        _lib.check(self._L.ramx_dev_peek_state(self._h, flank, cells.ctypes.data, C.byref(hi), C.byref(po)),
                   "ramx_dev_peek_state")
        return cells[:2 * B].reshape(B, 2).copy(), hi.value, po.value

    def peek_windows(self):
        """Debug / test hook (C-ABI ramx_dev_peek_windows): what the last pack call on this device left -- a direction's, a
        replay's or tsd()'s.  -> (words uint32 [packed_words][lanes], bounds int32 [lanes][2]); nothing is packed here."""
        kw, lanes = C.c_int32(), C.c_int32()
        rc = self._L.ramx_dev_peek_windows(self._h, None, 0, None, 0, C.byref(kw), C.byref(lanes))     # sizes the buffers
        if kw.value <= 0 or lanes.value <= 0:
            _lib.check(rc, "ramx_dev_peek_windows")
        words = np.zeros((kw.value, lanes.value), np.uint32)
        bounds = np.zeros((lanes.value, 2), np.int32)
        _lib.check(self._L.ramx_dev_peek_windows(self._h, words.ctypes.data, words.size, bounds.ctypes.data, lanes.value,
                                                 C.byref(kw), C.byref(lanes)), "ramx_dev_peek_windows")
        assert words.shape == (kw.value, lanes.value)
        return words, bounds

    def unique_id(self) -> np.ndarray:
        uid = np.zeros(128, np.uint8)
        _lib.check(self._L.ramx_comm_unique_id(uid.ctypes.data), "ramx_comm_unique_id")
        return uid

    def comm_init(self, uid: np.ndarray, rank: int, nranks: int):
        uid = np.ascontiguousarray(uid, dtype=np.uint8)
        _lib.check(self._L.ramx_dev_comm_init(self._h, uid.ctypes.data, rank, nranks), "ramx_dev_comm_init")

    def comm_size(self) -> int:
        return _lib.check(self._L.ramx_dev_comm_size(self._h), "ramx_dev_comm_size")

    def set_allreduce_callback(self, fn):
        """Test hook (ramx_dev_set_allreduce_cb): fn(list of 4 ints) -> list of 4 ints summed over ranks."""
        def _cb(ptr, _user):
            vals = fn([ptr[i] for i in range(4)])
            for i in range(4):
                ptr[i] = int(vals[i])
        self._cb = _lib.ALLREDUCE_CB(_cb)      # keep the trampoline alive
        _lib.check(self._L.ramx_dev_set_allreduce_cb(self._h, self._cb, None), "ramx_dev_set_allreduce_cb")

    def peer_setup(self, rank: int, world: int, all_gather_bytes, all_reduce_min, barrier) -> bool:
        """In-kernel vote exchange for the cross-device persistent path.  Two tiers, each enabled only if it works on
        every rank (self-test), tried in this order:
          "device": every rank's mailbox in fine-grained device memory, mapped into the others over hipIpc (xGMI);
          "host":   the mailboxes in one POSIX shared-memory segment registered with HIP (PCIe; ranks of one node).
        RAMX_PEER_KIND=device|host restricts the choice (tests).  all_gather_bytes(bytes64) -> list of world bytes
        objects; all_reduce_min(int) -> int; barrier() -> None.  Returns whether a tier is enabled; `peer_kind` names
        it ("device", "host" or None)."""
        import os
        only = os.environ.get("RAMX_PEER_KIND", "")
        token = 0x52414D58000000 + world
        self.peer_kind = None

        def selftest(ok):
            if all_reduce_min(ok) == 1:
                if self._L.ramx_dev_peer_selftest(self._h, 0, token) < 0:
                    ok = 0
                barrier()
                if ok and self._L.ramx_dev_peer_selftest(self._h, 1, token) != 1:
                    ok = 0
            return all_reduce_min(ok)

        if only in ("", "device"):
            ok = 1
            h = np.zeros(64, np.uint8)
            if self._L.ramx_dev_peer_export(self._h, h.ctypes.data) < 0:
                ok = 0
            handles = all_gather_bytes(h.tobytes())
            if all_reduce_min(ok) == 1:
                allh = np.frombuffer(b"".join(handles), np.uint8).copy()
                if self._L.ramx_dev_peer_import(self._h, allh.ctypes.data, rank, world) < 0:
                    ok = 0
            if selftest(ok) == 1:
                self._L.ramx_dev_peer_enable(self._h, 1)
                self.peer_kind = "device"
                return True
        if only in ("", "host"):
            # one name for the job: rank 0's pid + a random nonce, spread through the same all-gather; rank 0 creates the
            # segment exclusively, the others open it after a barrier; the name is unlinked in any case
            mine = np.zeros(64, np.uint8)
            tag = (b"/ramx_box_%d_%s" % (os.getpid(), os.urandom(8).hex().encode()))[:63]
            mine[:len(tag)] = np.frombuffer(tag, np.uint8)
            name = bytes(all_gather_bytes(mine.tobytes())[0]).split(b"\0", 1)[0]
            ok = 1
            try:
                if rank == 0:
                    ok = 1 if self._L.ramx_dev_hostbox_attach(self._h, name, rank, world) >= 0 else 0
                barrier()                   # the segment exists (or rank 0 failed: the others then fail to open it)
                if rank != 0:
                    ok = 1 if self._L.ramx_dev_hostbox_attach(self._h, name, rank, world) >= 0 else 0
                barrier()                   # every box has been cleared by its owner
                ok = selftest(ok)
            finally:
                if rank == 0:
                    self._L.ramx_hostbox_unlink(name)
            if ok == 1:
                self._L.ramx_dev_peer_enable(self._h, 1)
                self.peer_kind = "host"
                return True
        self._L.ramx_dev_peer_enable(self._h, 0)
        return False
