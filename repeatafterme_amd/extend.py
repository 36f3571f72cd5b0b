"""Python host-side mirror of the reference's extension-loop interface, bound to libramx.so.

``extend_alignment`` has the argument meaning, return value and side effects of the reference's
``extend_alignment`` (ram_extend.c:859-1258): it updates ``master`` and the cores' extension
lengths / scores in place and returns ``max_extension_score_row_idx + 1``.  All computation runs
in the HIP kernels behind the C-ABI; a missing library or GPU raises ``RamxError``.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from .datamodel import (ALN_END_DTYPE, COL_PROFILE_DTYPE, COPY_DIST_DTYPE, COPY_STATS_DTYPE, Dist, DINUC_DTYPE, FLANK_DTYPE, PILEUP_DTYPE, PLANE_DTYPE, Alignment, Copies, SubfamGroup, Subfamilies,
                        CoreSet, CpgRefinement, ExtendParams, Linkage, Profile, Refinement, TSD_DTYPE, TSD_SITE_DTYPE, TsdParams, TsdSummary,
                        PERIOD_DTYPE, PERIOD_SEG_DTYPE, PeriodParams, PeriodSummary, TERM_DTYPE, TermParams, TermSummary)


@dataclass
class RunInfo:
    ret: int
    rows_executed: int
    limit_warning: int
    overflow32: int
    n_extendable: int
    launches: int
    loop_ms: float
    kernel_ms_avg: float
    kernel_samples: int
    prep_ms: float
    persistent: int = 0
    lanes_per_flank: int = 1
    respeculated_rows: int = 0
    packed_rows: int = 0
    lean_rows: int = 0


def _params(p: ExtendParams):
    mat = np.ascontiguousarray(p.matrix, dtype=np.int32)
    assert mat.size == 100 * 100
    cp = _lib.Params(p.bandwidth, p.cappenalty, p.minimprovement, p.L, p.when_to_stop, p.l, p.gapopen,
                     p.gapextn, mat.ctypes.data)
    return cp, mat


def _info(ci: _lib.RunInfo) -> RunInfo:
    return RunInfo(**{k: getattr(ci, k) for k, _ in _lib.RunInfo._fields_})


class _ProfileSink:
    """Collects what seam 1 hands to the profile sink (ramx_set_profile_sink) while the block runs."""

    def __init__(self):
        self.got = []

        def _cb(ptr, _user):
            pr = ptr.contents
            cols = np.zeros(pr.n_cols, COL_PROFILE_DTYPE)
            if pr.n_cols:
                C.memmove(cols.ctypes.data, pr.cols, pr.n_cols * COL_PROFILE_DTYPE.itemsize)
            idx = np.zeros(pr.n_flanks, np.int32)
            last = np.full(pr.n_flanks, -1, np.int32)
            if pr.n_flanks:
                C.memmove(idx.ctypes.data, pr.core_index, 4 * pr.n_flanks)
                C.memmove(last.ctypes.data, pr.last_uncapped_row, 4 * pr.n_flanks)
            self.got.append(Profile(pr.direction, pr.family, pr.ret, cols, idx, last))
        self._cb = _lib.PROFILE_CB(_cb)

    def __enter__(self):
        _lib.lib().ramx_set_profile_sink(self._cb, None)
        return self

    def __exit__(self, *exc):
        _lib.lib().ramx_set_profile_sink(_lib.PROFILE_CB(), None)
        return False


class _AlignSink:
    """Collects what seam 1 hands to the alignment sink (ramx_set_align_sink) while the block runs."""

    def __init__(self):
        self.got = []

        def _cb(ptr, _user):
            al = ptr.contents
            n, rows = al.n_flanks, al.rows

            def grab(src, count, dtype):
                out = np.zeros(count, dtype)
                if count and src:
                    C.memmove(out.ctypes.data, src, count * out.dtype.itemsize)
                return out
            idx = np.full((rows, n), -2 ** 31 + 1, np.int32)
            ins = np.zeros((rows, n), np.int32)
            if rows and n and al.col_idx:
                full = grab(al.col_idx, (rows - 1) * al.stride + n, np.int32)
                full_i = grab(al.col_ins, (rows - 1) * al.stride + n, np.int32)
                for r in range(rows):
                    idx[r] = full[r * al.stride:r * al.stride + n]
                    ins[r] = full_i[r * al.stride:r * al.stride + n]
            self.got.append(Alignment(al.direction, al.family, grab(al.cons, rows, np.int8), grab(al.flanks, n, FLANK_DTYPE),
                                      grab(al.core_index, n, np.int32), grab(al.ends, n, ALN_END_DTYPE), idx, ins))
        self._cb = _lib.ALIGN_CB(_cb)

    def __enter__(self):
        _lib.lib().ramx_set_align_sink(self._cb, None)
        return self

    def __exit__(self, *exc):
        _lib.lib().ramx_set_align_sink(_lib.ALIGN_CB(), None)
        return False


class _RefineSink:
    """Collects what seam 1 hands to the refinement sink (ramx_set_refine_sink) while the block runs."""

    def __init__(self, max_replays):
        self.got = []
        self.max_replays = int(max_replays)

        def _cb(ptr, _user):
            rf = ptr.contents

            def grab(src, count, dtype):
                out = np.zeros(count, dtype)
                if count and src:
                    C.memmove(out.ctypes.data, src, count * out.dtype.itemsize)
                return out
            self.got.append(Refinement(rf.direction, rf.family, grab(rf.cons, rf.rows, np.int8), grab(rf.cols, rf.rows, PILEUP_DTYPE),
                                       grab(rf.refined_cons, rf.refined_rows, np.int8),
                                       grab(rf.refined_cols, rf.refined_rows, PILEUP_DTYPE), rf.replays, rf.converged))
        self._cb = _lib.REFINE_CB(_cb)

    def __enter__(self):
        _lib.lib().ramx_set_refine_sink(self._cb, None, self.max_replays)
        return self

    def __exit__(self, *exc):
        _lib.lib().ramx_set_refine_sink(_lib.REFINE_CB(), None, 1)
        return False


class _CpgSink:
    """Collects what seam 1 hands to the CpG sink (ramx_set_cpg_sink) while the block runs."""

    def __init__(self, max_replays, cpg_ts=0):
        self.got = []
        self.args = (int(max_replays), int(cpg_ts))

        def _cb(ptr, _user):
            cr = ptr.contents

            def grab(src, count, dtype):
                out = np.zeros(count, dtype)
                if count and src:
                    C.memmove(out.ctypes.data, src, count * out.dtype.itemsize)
                return out
            self.got.append(CpgRefinement(cr.direction, cr.family, grab(cr.cons, cr.rows, np.int8),
                                          grab(cr.refined_cons, cr.refined_rows, np.int8),
                                          grab(cr.refined_cols, cr.refined_rows, PILEUP_DTYPE),
                                          grab(cr.refined_di, cr.refined_rows, DINUC_DTYPE), cr.replays, cr.converged, cr.n_cpg))
        self._cb = _lib.CPG_CB(_cb)

    def __enter__(self):
        _lib.lib().ramx_set_cpg_sink(self._cb, None, *self.args)
        return self

    def __exit__(self, *exc):
        _lib.lib().ramx_set_cpg_sink(_lib.CPG_CB(), None, 1, 0)
        return False


class _CopiesSink:
    """Collects what seam 1 hands to the copies sink (ramx_set_copies_sink) while the block runs."""

    def __init__(self):
        self.got = []

        def _cb(ptr, _user):
            cp = ptr.contents
            n = cp.n_flanks

            def grab(src, count, dtype):
                out = np.zeros(count, dtype)
                if count and src:
                    C.memmove(out.ctypes.data, src, count * out.dtype.itemsize)
                return out
            self.got.append(Copies(cp.direction, cp.family, grab(cp.cons, cp.rows, np.int8), grab(cp.flanks, n, FLANK_DTYPE),
                                   grab(cp.core_index, n, np.int32), grab(cp.ends, n, ALN_END_DTYPE),
                                   grab(cp.stats, n, COPY_STATS_DTYPE)))
        self._cb = _lib.COPIES_CB(_cb)

    def __enter__(self):
        _lib.lib().ramx_set_copies_sink(self._cb, None)
        return self

    def __exit__(self, *exc):
        _lib.lib().ramx_set_copies_sink(_lib.COPIES_CB(), None)
        return False


class _LinkageSink:
    """Collects what seam 1 hands to the linkage sink (ramx_set_linkage_sink) while the block runs.  select: (min_count,
    min_permille, max_variants)."""

    def __init__(self, select=(4, 100, 1024)):
        self.got = []
        self.select = tuple(int(x) for x in select)

        def _cb(ptr, _user):
            lk = ptr.contents

            def grab(src, count, dtype):
                out = np.zeros(count, dtype)
                if count and src:
                    C.memmove(out.ctypes.data, src, count * out.dtype.itemsize)
                return out
            P = lk.n_planes
            self.got.append(Linkage(lk.direction, lk.family, grab(lk.cons, lk.rows, np.int8), grab(lk.cols, lk.rows, PILEUP_DTYPE),
                                    grab(lk.planes, P, PLANE_DTYPE), grab(lk.co, P * P, np.int32).reshape(P, P)))
        self._cb = _lib.LINKAGE_CB(_cb)

    def __enter__(self):
        _lib.lib().ramx_set_linkage_sink(self._cb, None, *self.select)
        return self

    def __exit__(self, *exc):
        _lib.lib().ramx_set_linkage_sink(_lib.LINKAGE_CB(), None, 4, 100, 1024)
        return False


class _SubfamSink:
    """Collects what seam 1 hands to the subfamily sink (ramx_set_subfam_sink) while the block runs.  args: (min_count,
    min_permille, max_variants, min_mlog10p, K, max_iter, min_members, max_replays)."""
    DEFAULT = (4, 100, 1024, 3.0, 4, 8, 4, 10)

    def __init__(self, args=DEFAULT):
        self.got = []
        a = tuple(args)
        self.args = tuple(int(x) for x in a[:3]) + (float(a[3]),) + tuple(int(x) for x in a[4:])
        assert len(self.args) == 8

        def _cb(ptr, _user):
            sf = ptr.contents

            def grab(src, count, dtype):
                out = np.zeros(count, dtype)
                if count and src:
                    C.memmove(out.ctypes.data, src, count * out.dtype.itemsize)
                return out
            n, P, V, K = sf.n_flanks, sf.n_planes, sf.n_variants, sf.K
            groups = []
            for g in range(sf.n_groups):
                gr = sf.groups[g]
                groups.append(SubfamGroup(gr.group, gr.size, grab(gr.refined_cons, gr.refined_rows, np.int8),
                                          grab(gr.refined_cols, gr.refined_rows, PILEUP_DTYPE), gr.replays, gr.converged))
            self.got.append(Subfamilies(sf.direction, sf.family, grab(sf.cons, sf.rows, np.int8), grab(sf.flanks, n, FLANK_DTYPE),
                                        grab(sf.core_index, n, np.int32), grab(sf.planes, P, PLANE_DTYPE), grab(sf.labels, n, np.int32),
                                        grab(sf.patterns, V * K, np.uint8).reshape(V, K), grab(sf.cnt, K * P, np.int32).reshape(K, P),
                                        grab(sf.size, K, np.int32), grab(sf.dist, n * K, np.int32).reshape(n, K), sf.iterations,
                                        sf.converged, groups))
        self._cb = _lib.SUBFAM_CB(_cb)

    def __enter__(self):
        _lib.lib().ramx_set_subfam_sink(self._cb, None, *self.args)
        return self

    def __exit__(self, *exc):
        _lib.lib().ramx_set_subfam_sink(_lib.SUBFAM_CB(), None, *self.DEFAULT)
        return False


class _DistSink:
    """Collects what seam 1 hands to the distance sink (ramx_set_dist_sink) while the block runs.  select: (min_cols,
    max_copies)."""
    DEFAULT = (1, 256)

    def __init__(self, select=DEFAULT):
        self.got = []
        self.select = tuple(int(x) for x in select)
        assert len(self.select) == 2

        def _cb(ptr, _user):
            ds = ptr.contents

            def grab(src, count, dtype):
                out = np.zeros(count, dtype)
                if count and src:
                    C.memmove(out.ctypes.data, src, count * out.dtype.itemsize)
                return out
            n, c = ds.n_flanks, ds.n_copies
            self.got.append(Dist(ds.direction, ds.family, grab(ds.cons, ds.rows, np.int8), grab(ds.core_index, n, np.int32),
                                 grab(ds.ends, n, ALN_END_DTYPE), grab(ds.copies, c, np.int32),
                                 grab(ds.dist, c * c, COPY_DIST_DTYPE).reshape(c, c)))
        self._cb = _lib.DIST_CB(_cb)

    def __enter__(self):
        _lib.lib().ramx_set_dist_sink(self._cb, None, *self.select)
        return self

    def __exit__(self, *exc):
        _lib.lib().ramx_set_dist_sink(_lib.DIST_CB(), None, *self.DEFAULT)
        return False


def extend_alignment(direction: int, cores: CoreSet, sequence: np.ndarray, master: np.ndarray,
                     p: ExtendParams, profile: bool = False, align: bool = False, refine: int = 0, copies: bool = False,
                     linkage=None, subfam=None, cpg=None, period=None, dist=None):
    """direction: 1 = right, 0 = left (reference ram_extend.c:424,506).  profile=True: returns (RunInfo, Profile) -- the
    direction is replayed along the consensus it chose (C-ABI ramx_dev_profile) after the loop.  align=True: returns
    (RunInfo, Alignment), or (RunInfo, Profile, Alignment) with both -- every flank aligned to the kept consensus (C-ABI
    ramx_dev_align).  refine=n > 0: a Refinement comes last in the tuple -- the kept consensus' pileup and its refinement over at
    most n replays (C-ABI ramx_dev_pileup / ramx_dev_refine).  copies=True: a Copies comes last of all -- every copy's
    statistics along the kept consensus (C-ABI ramx_dev_copy_stats).  linkage=True or (min_count, min_permille, max_variants): a
    Linkage comes behind everything else -- the variants of the kept consensus and their Gram matrix (C-ABI ramx_dev_planes,
    ramx_select_planes, ramx_dev_plane_gram).  subfam=True or the eight arguments of ramx_set_subfam_sink behind its callback: a
    Subfamilies comes behind those -- the copies split by their linked variants, every kept group with its own consensus.
    cpg=n > 0 or (n, cpg_ts): a CpgRefinement comes last of all -- the kept consensus refined over at most n replays with the
    CpG-aware re-call (C-ABI ramx_dev_refine_cpg).  period=True or a PeriodParams: the tandem periodicity of every core's
    extension in this direction, PERIOD_DTYPE [cores.n], comes behind everything (C-ABI ramx_period_flat with which = direction,
    on the library the call left on the device).  dist=True or (min_cols, max_copies): a Dist comes last of all, behind the
    periodicity -- the pairwise divergence between the selected copies along the kept consensus (C-ABI ramx_dev_planes,
    ramx_select_copies, ramx_dev_copy_dist; include/ramx_dist.h)."""
    if dist:
        with _DistSink(_DistSink.DEFAULT if dist is True else dist) as dsink:
            res = extend_alignment(direction, cores, sequence, master, p, profile=profile, align=align, refine=refine, copies=copies,
                                   linkage=linkage, subfam=subfam, cpg=cpg, period=period)
        assert len(dsink.got) == 1
        return (res + (dsink.got[0],)) if isinstance(res, tuple) else (res, dsink.got[0])
    if period:
        res = extend_alignment(direction, cores, sequence, master, p, profile=profile, align=align, refine=refine, copies=copies,
                               linkage=linkage, subfam=subfam, cpg=cpg)
        rec = period_flat(cores, sequence, 1 if direction else 0, None if period is True else period)
        return (res + (rec,)) if isinstance(res, tuple) else (res, rec)
    if cpg:
        with _CpgSink(*((cpg,) if isinstance(cpg, int) else cpg)) as gsink:
            res = extend_alignment(direction, cores, sequence, master, p, profile=profile, align=align, refine=refine, copies=copies,
                                   linkage=linkage, subfam=subfam)
        assert len(gsink.got) == 1
        return (res + (gsink.got[0],)) if isinstance(res, tuple) else (res, gsink.got[0])
    if subfam:
        with _SubfamSink(_SubfamSink.DEFAULT if subfam is True else subfam) as ssink:
            res = extend_alignment(direction, cores, sequence, master, p, profile=profile, align=align, refine=refine, copies=copies,
                                   linkage=linkage)
        assert len(ssink.got) == 1
        return (res + (ssink.got[0],)) if isinstance(res, tuple) else (res, ssink.got[0])
    if linkage:
        with _LinkageSink((4, 100, 1024) if linkage is True else linkage) as lsink:
            res = extend_alignment(direction, cores, sequence, master, p, profile=profile, align=align, refine=refine, copies=copies)
        assert len(lsink.got) == 1
        return (res + (lsink.got[0],)) if isinstance(res, tuple) else (res, lsink.got[0])
    if copies:
        with _CopiesSink() as csink:
            res = extend_alignment(direction, cores, sequence, master, p, profile=profile, align=align, refine=refine)
        assert len(csink.got) == 1
        return (res + (csink.got[0],)) if isinstance(res, tuple) else (res, csink.got[0])
    if refine:
        with _RefineSink(refine) as rsink:
            res = extend_alignment(direction, cores, sequence, master, p, profile=profile, align=align)
        assert len(rsink.got) == 1
        return (res + (rsink.got[0],)) if isinstance(res, tuple) else (res, rsink.got[0])
    if align:
        with _AlignSink() as asink:
            res = extend_alignment(direction, cores, sequence, master, p, profile=profile)
        assert len(asink.got) == 1
        return (res + (asink.got[0],)) if profile else (res, asink.got[0])
    if profile:
        with _ProfileSink() as sink:
            info = extend_alignment(direction, cores, sequence, master, p)
        assert len(sink.got) == 1
        return info, sink.got[0]
    L = _lib.lib()
    assert sequence.dtype == np.int8 and sequence.flags.c_contiguous
    assert master.dtype == np.int8 and len(master) >= 2 * p.L + p.l + 1
    fc = _lib.FlatCores(cores.n, *[getattr(cores, k).ctypes.data for k in
                                   ("left_pos", "right_pos", "lower", "upper", "orient", "left_ext",
                                    "right_ext", "left_len", "right_len", "score")])
    cp, _keep = _params(p)
    ci = _lib.RunInfo()
    rc = L.ramx_extend_flat(int(direction), C.byref(fc), sequence.ctypes.data, len(sequence),
                            master.ctypes.data, C.byref(cp), C.byref(ci))
    _lib.check(rc, "ramx_extend_flat")
    return _info(ci)


def extend_batch(direction: int, families, p: ExtendParams, profile: bool = False, align: bool = False, copies: bool = False,
                 linkage=None, subfam=None, period=None, dist=None):
    """Many families in one launch (C-ABI ramx_extend_batch).  `families` is a list of (cores, sequence, master);
    every family is updated in place exactly like extend_alignment does for one.  Returns one RunInfo per family;
    profile=True: (RunInfos, Profiles), one Profile per family in the order of `families`; align=True: (RunInfos,
    Alignments), or (RunInfos, Profiles, Alignments) with both.  copies=True: the families' Copies come last in the tuple.
    linkage (as extend_alignment): the families' Linkages come behind everything else; subfam (as extend_alignment): their
    Subfamilies last of all.  period (as extend_alignment): one PERIOD_DTYPE array per family behind everything (C-ABI
    ramx_period_batch with which = direction).  dist (as extend_alignment): the families' Dists last of all."""
    if dist:
        with _DistSink(_DistSink.DEFAULT if dist is True else dist) as dsink:
            res = extend_batch(direction, families, p, profile=profile, align=align, copies=copies, linkage=linkage, subfam=subfam,
                               period=period)
        by_family = {ds.family: ds for ds in dsink.got}
        assert len(by_family) == len(dsink.got) == len(families)
        dss = [by_family[i] for i in range(len(families))]
        return (res + (dss,)) if isinstance(res, tuple) else (res, dss)
    if period:
        res = extend_batch(direction, families, p, profile=profile, align=align, copies=copies, linkage=linkage, subfam=subfam)
        recs = period_batch(families, 1 if direction else 0, None if period is True else period)
        return (res + (recs,)) if isinstance(res, tuple) else (res, recs)
    if subfam:
        with _SubfamSink(_SubfamSink.DEFAULT if subfam is True else subfam) as ssink:
            res = extend_batch(direction, families, p, profile=profile, align=align, copies=copies, linkage=linkage)
        by_family = {sf.family: sf for sf in ssink.got}
        assert len(by_family) == len(ssink.got) == len(families)
        sfs = [by_family[i] for i in range(len(families))]
        return (res + (sfs,)) if isinstance(res, tuple) else (res, sfs)
    if linkage:
        with _LinkageSink((4, 100, 1024) if linkage is True else linkage) as lsink:
            res = extend_batch(direction, families, p, profile=profile, align=align, copies=copies)
        by_family = {lk.family: lk for lk in lsink.got}
        assert len(by_family) == len(lsink.got) == len(families)
        lks = [by_family[i] for i in range(len(families))]
        return (res + (lks,)) if isinstance(res, tuple) else (res, lks)
    if copies:
        with _CopiesSink() as csink:
            res = extend_batch(direction, families, p, profile=profile, align=align)
        by_family = {cp.family: cp for cp in csink.got}
        assert len(by_family) == len(csink.got) == len(families)
        cps = [by_family[i] for i in range(len(families))]
        return (res + (cps,)) if isinstance(res, tuple) else (res, cps)
    if align:
        with _AlignSink() as asink:
            res = extend_batch(direction, families, p, profile=profile)
        by_family = {al.family: al for al in asink.got}
        assert len(by_family) == len(asink.got) == len(families)
        als = [by_family[i] for i in range(len(families))]
        return (res + (als,)) if profile else (res, als)
    if profile:
        with _ProfileSink() as sink:
            infos = extend_batch(direction, families, p)
        by_family = {pr.family: pr for pr in sink.got}
        assert len(by_family) == len(sink.got) == len(families)
        return infos, [by_family[i] for i in range(len(families))]
    L = _lib.lib()
    n = len(families)
    arr = (_lib.Family * max(n, 1))()
    keep = []
    for i, (cores, sequence, master) in enumerate(families):
        assert sequence.dtype == np.int8 and sequence.flags.c_contiguous and master.dtype == np.int8
        arr[i].cores = _lib.FlatCores(cores.n, *[getattr(cores, k).ctypes.data for k in
                                                 ("left_pos", "right_pos", "lower", "upper", "orient", "left_ext",
                                                  "right_ext", "left_len", "right_len", "score")])
        arr[i].sequence = sequence.ctypes.data
        arr[i].seq_len = len(sequence)
        arr[i].master = master.ctypes.data
        keep.append((cores, sequence, master))
    cp, _keep = _params(p)
    infos = (_lib.RunInfo * max(n, 1))()
    _lib.check(L.ramx_extend_batch(int(direction), arr, n, C.byref(cp), infos), "ramx_extend_batch")
    return [_info(infos[i]) for i in range(n)]


# ---- target-site duplications (include/ramx.h, ramx_tsd): after both extension calls ----

def _tsd_params(tp):
    tp = TsdParams() if tp is None else tp
    return _lib.TsdParams(int(tp.slack), int(tp.kmin), int(tp.kmax), int(tp.mm_div))


def _flat_cores(cores: CoreSet):
    return _lib.FlatCores(cores.n, *[getattr(cores, k).ctypes.data for k in
                                     ("left_pos", "right_pos", "lower", "upper", "orient", "left_ext",
                                      "right_ext", "left_len", "right_len", "score")])


def tsd_sites(cores: CoreSet) -> np.ndarray:
    """One site per core from the extents both directions left in the cores (C-ABI ramx_tsd_sites, host C)."""
    out = np.zeros(cores.n, TSD_SITE_DTYPE)
    fc = _flat_cores(cores)
    _lib.check(_lib.lib().ramx_tsd_sites(C.byref(fc), out.ctypes.data if cores.n else None), "ramx_tsd_sites")
    return out


def tsd_summary(records, tp: TsdParams = None) -> TsdSummary:
    """Histogram, modal length and chance expectation of a family's records (C-ABI ramx_tsd_summary, host C)."""
    r = np.ascontiguousarray(records, TSD_DTYPE).reshape(-1)
    h = _lib.TsdHist()
    cp = _tsd_params(tp)
    _lib.check(_lib.lib().ramx_tsd_summary(r.ctypes.data if len(r) else None, len(r), C.byref(cp), C.byref(h)), "ramx_tsd_summary")
    return TsdSummary(np.array(h.hist[:], np.int32), int(h.mode), int(h.mode_count), np.array(h.null[:], np.float64))


def termini(cons_left, cons_right, T: int = 32):
    """-> (first bases, last bases, terminal-inverted-repeat length) of the extended consensus, from the kept columns of the two
    directions as the loop hands them over -- the left rows run outward from the core (C-ABI ramx_termini, host C)."""
    cl, cr = np.ascontiguousarray(cons_left, np.int8), np.ascontiguousarray(cons_right, np.int8)
    five, three = C.create_string_buffer(max(T, 0) + 1), C.create_string_buffer(max(T, 0) + 1)
    tir = C.c_int32()
    _lib.check(_lib.lib().ramx_termini(cl.ctypes.data if len(cl) else None, len(cl), cr.ctypes.data if len(cr) else None, len(cr),
                                       int(T), five, three, C.byref(tir)), "ramx_termini")
    return five.value.decode(), three.value.decode(), int(tir.value)


def tsd_flat(cores: CoreSet, sequence: np.ndarray, tp: TsdParams = None) -> np.ndarray:
    """The target-site duplication of every core after both extension calls, on the library they left on the session's device
    (C-ABI ramx_tsd_flat): -> TSD_DTYPE [cores.n]."""
    assert sequence.dtype == np.int8 and sequence.flags.c_contiguous
    out = np.zeros(cores.n, TSD_DTYPE)
    fc = _flat_cores(cores)
    cp = _tsd_params(tp)
    _lib.check(_lib.lib().ramx_tsd_flat(C.byref(fc), sequence.ctypes.data, len(sequence), C.byref(cp), out.ctypes.data if cores.n else None),
               "ramx_tsd_flat")
    return out


def tsd_alignment(core_list, seq_lib, n: int, tp: TsdParams = None) -> np.ndarray:
    """The same on the reference's data model: core_list / seq_lib are pointers to a struct coreAlignment list of n nodes and its
    struct sequenceLibrary, as the loader returns them -- packed twin included (C-ABI ramx_tsd_alignment)."""
    out = np.zeros(n, TSD_DTYPE)
    cp = _tsd_params(tp)
    _lib.check(_lib.lib().ramx_tsd_alignment(C.cast(core_list, C.c_void_p), C.cast(seq_lib, C.c_void_p), C.byref(cp),
                                             out.ctypes.data if n else None), "ramx_tsd_alignment")
    return out


def tsd_batch(families, tp: TsdParams = None):
    """The same for the families of an extend_batch, in one launch on the concatenated library it leaves on the device (C-ABI
    ramx_tsd_batch).  `families` as extend_batch takes them; -> one TSD_DTYPE array per family."""
    n = len(families)
    arr = (_lib.Family * max(n, 1))()
    for i, (cores, sequence, master) in enumerate(families):
        assert sequence.dtype == np.int8 and sequence.flags.c_contiguous
        arr[i].cores = _flat_cores(cores)
        arr[i].sequence = sequence.ctypes.data
        arr[i].seq_len = len(sequence)
        arr[i].master = master.ctypes.data if master is not None else None
    total = sum(f[0].n for f in families)
    out = np.zeros(total, TSD_DTYPE)
    cp = _tsd_params(tp)
    _lib.check(_lib.lib().ramx_tsd_batch(arr, n, C.byref(cp), out.ctypes.data if total else None), "ramx_tsd_batch")
    ends = np.cumsum([0] + [f[0].n for f in families])
    return [out[ends[i]:ends[i + 1]].copy() for i in range(n)]


# ---- tandem periodicity (include/ramx.h, ramx_period): after the extension calls ----

def _period_params(pp):
    pp = PeriodParams() if pp is None else pp
    return _lib.PeriodParams(int(pp.pmax), int(pp.mm), int(pp.min_score), 0)


def period_sequence(codes, pp: PeriodParams = None) -> np.ndarray:
    """The record of an array of library codes, e.g. the kept consensus of a direction (C-ABI ramx_period_sequence, host C):
    -> one PERIOD_DTYPE record."""
    c = np.ascontiguousarray(codes, np.int8).reshape(-1)
    out = np.zeros(1, PERIOD_DTYPE)
    cp = _period_params(pp)
    _lib.check(_lib.lib().ramx_period_sequence(c.ctypes.data if len(c) else None, len(c), C.byref(cp), out.ctypes.data), "ramx_period_sequence")
    return out[0]


def period_segments(cores: CoreSet, which: int) -> np.ndarray:
    """One segment per core: which = 0 the left extension, 1 the right one, 2 the whole element (C-ABI ramx_period_segments)."""
    out = np.zeros(cores.n, PERIOD_SEG_DTYPE)
    fc = _flat_cores(cores)
    _lib.check(_lib.lib().ramx_period_segments(C.byref(fc), int(which), out.ctypes.data if cores.n else None), "ramx_period_segments")
    return out


def period_summary(records, segs, pp: PeriodParams = None) -> PeriodSummary:
    """What a family's records say together (C-ABI ramx_period_summary, host C)."""
    r = np.ascontiguousarray(records, PERIOD_DTYPE).reshape(-1)
    s = np.ascontiguousarray(segs, PERIOD_SEG_DTYPE).reshape(-1)
    assert len(r) == len(s)
    h = _lib.PeriodHist()
    cp = _period_params(pp)
    _lib.check(_lib.lib().ramx_period_summary(r.ctypes.data if len(r) else None, s.ctypes.data if len(s) else None, len(r), C.byref(cp),
                                              C.byref(h)), "ramx_period_summary")
    return PeriodSummary(*[int(getattr(h, k)) for k in ("n", "n_tract", "n_mono", "n_simple", "n_tandem", "at_lo", "at_hi", "mode", "mode_count")])


def period_flat(cores: CoreSet, sequence: np.ndarray, which: int, pp: PeriodParams = None) -> np.ndarray:
    """The tandem periodicity of every core's left extension (which = 0), right extension (1) or whole element (2) after the
    extension calls, on the library they left on the session's device (C-ABI ramx_period_flat): -> PERIOD_DTYPE [cores.n]."""
    assert sequence.dtype == np.int8 and sequence.flags.c_contiguous
    out = np.zeros(cores.n, PERIOD_DTYPE)
    fc = _flat_cores(cores)
    cp = _period_params(pp)
    _lib.check(_lib.lib().ramx_period_flat(C.byref(fc), sequence.ctypes.data, len(sequence), int(which), C.byref(cp),
                                           out.ctypes.data if cores.n else None), "ramx_period_flat")
    return out


def period_alignment(core_list, seq_lib, n: int, which: int, pp: PeriodParams = None) -> np.ndarray:
    """The same on the reference's data model, as tsd_alignment takes it (C-ABI ramx_period_alignment)."""
    out = np.zeros(n, PERIOD_DTYPE)
    cp = _period_params(pp)
    _lib.check(_lib.lib().ramx_period_alignment(C.cast(core_list, C.c_void_p), C.cast(seq_lib, C.c_void_p), int(which), C.byref(cp),
                                                out.ctypes.data if n else None), "ramx_period_alignment")
    return out


def period_batch(families, which: int, pp: PeriodParams = None):
    """The same for the families of an extend_batch, in one call on the concatenated library it leaves on the device (C-ABI
    ramx_period_batch).  `families` as extend_batch takes them; -> one PERIOD_DTYPE array per family."""
    n = len(families)
    arr = (_lib.Family * max(n, 1))()
    for i, (cores, sequence, master) in enumerate(families):
        assert sequence.dtype == np.int8 and sequence.flags.c_contiguous
        arr[i].cores = _flat_cores(cores)
        arr[i].sequence = sequence.ctypes.data
        arr[i].seq_len = len(sequence)
        arr[i].master = master.ctypes.data if master is not None else None
    total = sum(f[0].n for f in families)
    out = np.zeros(total, PERIOD_DTYPE)
    cp = _period_params(pp)
    _lib.check(_lib.lib().ramx_period_batch(arr, n, int(which), C.byref(cp), out.ctypes.data if total else None), "ramx_period_batch")
    ends = np.cumsum([0] + [f[0].n for f in families])
    return [out[ends[i]:ends[i + 1]].copy() for i in range(n)]


# ---- terminal repeats (include/ramx.h, ramx_term): after both extension calls, on the sites of tsd_sites ----

def _term_params(tp):
    tp = TermParams() if tp is None else tp
    return _lib.TermParams(int(tp.tmax), int(tp.match), int(tp.mismatch), int(tp.gap), int(tp.min_score), int(tp.slack))


def term_pair(a, b, tp: TermParams = None) -> np.ndarray:
    """The record of two arrays of library codes, b as given (C-ABI ramx_term_pair, host C): -> one TERM_DTYPE record."""
    a = np.ascontiguousarray(a, np.int8).reshape(-1)
    b = np.ascontiguousarray(b, np.int8).reshape(-1)
    out = np.zeros(1, TERM_DTYPE)
    cp = _term_params(tp)
    _lib.check(_lib.lib().ramx_term_pair(a.ctypes.data if len(a) else None, len(a), b.ctypes.data if len(b) else None, len(b), C.byref(cp),
                                         out.ctypes.data), "ramx_term_pair")
    return out[0]


def term_summary(records, tp: TermParams = None) -> TermSummary:
    """What a family's records [n][2] say together (C-ABI ramx_term_summary, host C)."""
    r = np.ascontiguousarray(records, TERM_DTYPE).reshape(-1)
    assert len(r) % 2 == 0
    h = _lib.TermFamily()
    cp = _term_params(tp)
    _lib.check(_lib.lib().ramx_term_summary(r.ctypes.data if len(r) else None, len(r) // 2, C.byref(cp), C.byref(h)), "ramx_term_summary")
    return TermSummary(*[int(getattr(h, k)) for k, _ in _lib.TermFamily._fields_])


def term_flat(cores: CoreSet, sequence: np.ndarray, tp: TermParams = None) -> np.ndarray:
    """The terminal repeats of every core's element after both extension calls, on the library they left on the session's device
    (C-ABI ramx_term_flat): -> TERM_DTYPE [cores.n][2], direct and inverted."""
    assert sequence.dtype == np.int8 and sequence.flags.c_contiguous
    out = np.zeros((cores.n, 2), TERM_DTYPE)
    fc = _flat_cores(cores)
    cp = _term_params(tp)
    _lib.check(_lib.lib().ramx_term_flat(C.byref(fc), sequence.ctypes.data, len(sequence), C.byref(cp), out.ctypes.data if cores.n else None),
               "ramx_term_flat")
    return out


def term_alignment(core_list, seq_lib, n: int, tp: TermParams = None) -> np.ndarray:
    """The same on the reference's data model, as tsd_alignment takes it (C-ABI ramx_term_alignment)."""
    out = np.zeros((n, 2), TERM_DTYPE)
    cp = _term_params(tp)
    _lib.check(_lib.lib().ramx_term_alignment(C.cast(core_list, C.c_void_p), C.cast(seq_lib, C.c_void_p), C.byref(cp),
                                              out.ctypes.data if n else None), "ramx_term_alignment")
    return out


def term_batch(families, tp: TermParams = None):
    """The same for the families of an extend_batch, in one call on the concatenated library it leaves on the device (C-ABI
    ramx_term_batch).  `families` as extend_batch takes them; -> one TERM_DTYPE [n][2] array per family."""
    n = len(families)
    arr = (_lib.Family * max(n, 1))()
    for i, (cores, sequence, master) in enumerate(families):
        assert sequence.dtype == np.int8 and sequence.flags.c_contiguous
        arr[i].cores = _flat_cores(cores)
        arr[i].sequence = sequence.ctypes.data
        arr[i].seq_len = len(sequence)
        arr[i].master = master.ctypes.data if master is not None else None
    total = sum(f[0].n for f in families)
    out = np.zeros((total, 2), TERM_DTYPE)
    cp = _term_params(tp)
    _lib.check(_lib.lib().ramx_term_batch(arr, n, C.byref(cp), out.ctypes.data if total else None), "ramx_term_batch")
    ends = np.cumsum([0] + [f[0].n for f in families])
    return [out[ends[i]:ends[i + 1]].copy() for i in range(n)]
