"""The inputs of tests/test_gpu_session_reuse.py, built here so that tests/test_session_cases.py can vouch for them on the CPU:
two worlds, BIG and SMALL, that go through one device session one after the other.  A session keeps its device buffers between
calls and reallocates only to grow, so a SMALL call after a BIG one finds every buffer holding BIG's rows, tiles, window words
and stream words behind (and between) its own.  SMALL is smaller than BIG in every extent a buffer is sized or strided by, and
BIG's numbers differ from SMALL's where they would show: stale data cannot equal the truth by accident.

BIG needs the oracle's loop only (the GPU tests assert of a BIG call no more than that it answered); SMALL's expectations are the
restatements of tests/*_ref.py.  Nothing here needs a GPU."""
import functools
import types

import numpy as np

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import PERIOD_SEG_DTYPE, TSD_SITE_DTYPE, new_master
from repeatafterme_amd.synth import synth_family

import copystats_ref as cr
import dinuc_ref as dr
import linkage_ref as lr
import period_ref as per
import pileup_ref as pr
import subfam_ref as sr
import term_ref as tr
import tsd_ref as ts
import window_ref as wr

BIG_N, BIG_W, BIG_L, BIG_K, BIG_SEED, BIG_MATRIX = 300, 40, 300, 280, 97, "14p43g"
BIG_VARIANTS = 200                       # the variants of BIG's plane list (with their rows' cover planes)
SMALL_W, SMALL_L, SMALL_MATRIX = 5, 30, "14p43g"
SMALL_FAMILIES = ((70, 24, 62), (0, 0, 0), (3, 24, 63))          # (flanks, K, seed); the second has no flank at all
SMALL_ROWS_C = 17                        # columns of the 3-flank family's consensus
SUBFAM_K = 3
SELECT = dict(min_count=2, min_permille=50, max_variants=1024)
# site-window parameters of the SMALL calls: short windows need a lower bar than the defaults' 40
TERM = dict(tmax=512, match=2, mismatch=3, gap=5, min_score=30, slack=3)
PERIOD = dict(pmax=1024, mm=3, min_score=16)
TSD = dict(slack=3, kmin=4, kmax=20, mm_div=10)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


def _clipped(fs, lo, hi, seed):
    """Every copy's window cut to lo..hi bases beyond its core: the copies end at different columns."""
    cores = fs.cores.copy()
    q = np.random.default_rng(seed).integers(lo, hi + 1, cores.n)
    cores.upper = np.minimum(cores.upper, cores.right_pos + q)
    cores.lower = np.maximum(cores.lower, cores.left_pos - q)
    return cores


def foreign(cons, at, k):
    """Every seventh base changed (the consensus of test_gpu_replay_corners.family) and k columns dropped at `at`."""
    c = np.array(cons, np.int8)
    c[::7] = (c[::7] + 1) & 3
    return np.delete(c, slice(at, at + k))


def lay_out(parts, hole_before):
    from test_gpu_replay_long import lay_out as _lay_out
    return _lay_out(parts, hole_before)


# ---------------------------------------------------------------------------------------------------- BIG

@functools.lru_cache(maxsize=None)
def big():
    """Four families in nine tiles (576 padded flanks), W = 40, L = 300.  The first has 300 flanks (five tiles, the last with
    44), both strands, runs of N, copies cut at 150..300 bases so that the loop runs past row 256, along the loop's own consensus
    with every seventh base changed; three families of 5 flanks follow, a tile of no family before the last, along 40 random
    columns each.  130 sites lie behind the families in the same library (those of tests/test_gpu_term.py: windows up to 1,024
    bases, segments up to 2,049).  -> namespace(lib, fams, offs, p, loop, cons, rows, sites, segs, planes, ...)"""
    import test_gpu_term as tgt
    rng = np.random.default_rng(BIG_SEED)
    fs = synth_family(BIG_N, BIG_L, BIG_W, K=BIG_K, seed=BIG_SEED, both_sides=True, minus_frac=0.4, n_run_frac=0.1)
    cores = _clipped(fs, 150, BIG_L, BIG_SEED)
    p = po.Params.named(BIG_MATRIX, bandwidth=BIG_W, L=BIG_L, when_to_stop=1000)
    fams = [(np.ascontiguousarray(fs.sequence, np.int8), cores)]
    for k in range(3):
        m = synth_family(5, BIG_L, BIG_W, K=60, seed=BIG_SEED + 1 + k, both_sides=True, minus_frac=0.4)
        fams.append((np.ascontiguousarray(m.sequence, np.int8), m.cores.copy()))
    loop = {d: po.oracle_extend(d, cores.copy(), fams[0][0], new_master(BIG_L), p, trace=True, row_trace=True) for d in (1, 0)}
    rows = [loop[1].rows_executed, 40, 40, 40]
    cons = rng.integers(0, 4, (4, BIG_L)).astype(np.int8)
    cons[0, :rows[0]] = loop[1].col_base[:rows[0]]
    cons[0, :rows[0]:7] = (cons[0, :rows[0]:7] + 1) & 3
    site_lib, sites = tgt.make_library()
    sites = sites.copy()
    offs = [int(v) for v in np.cumsum([0] + [len(x[0]) for x in fams])]
    for k in sites.dtype.names:
        sites[k] += offs[-1]
    lib = np.ascontiguousarray(np.concatenate([x[0] for x in fams] + [site_lib]), np.int8)
    segs = np.zeros(len(sites), PERIOD_SEG_DTYPE)
    segs["lo"], segs["hi"] = sites["lo"], sites["hi"]
    planes = [sr.list_with(rows[0], BIG_VARIANTS)] + [sr.list_with(40, 5, first_row=3 * k) for k in range(3)]
    _frozen(lib, cons, sites, segs)
    return types.SimpleNamespace(lib=lib, fams=fams, offs=offs[:4], p=p, loop=loop, cons=cons, rows=rows, sites=sites, segs=segs,
                                 planes=planes, n_families=4, tiles=9, n_padded=576)


def big_layout():
    """-> ((flank array, 576), first, count) of BIG"""
    from repeatafterme_amd.device import resolve_flanks
    b = big()
    parts = []
    for (seq, cores), off in zip(b.fams, b.offs):
        fl, nx = resolve_flanks(1, cores, BIG_W, BIG_L)[0]
        assert nx == cores.n
        parts.append((fl, nx, off))
    flanks, first, count = lay_out(parts, hole_before=3)
    assert flanks[1] == b.n_padded and first == [0, 320, 384, 512] and count == [BIG_N, 5, 5, 5]
    return flanks, first, count


# ---------------------------------------------------------------------------------------------------- SMALL

def _site_element(rng, n, T, inverted, skip):
    """n bases whose last T repeat the first T (directly, or as their reverse complement), but for `skip` bases at the end that
    falls outside the library."""
    x = rng.integers(0, 4, n).astype(np.int8)
    if inverted:
        x[n - T:n - skip] = tr.revcomp(x[skip:T])
    else:
        x[n - T + skip:] = x[skip:T]
    return x


@functools.lru_cache(maxsize=None)
def small():
    """Three families in four tiles -- 70 flanks in two tiles, a family without flanks, a tile of no family, 3 flanks in the last
    -- on a short library of its own, W = 5, L = 30, rows = (28, 0, 17); three sites: one of length 0 inside the library (two
    equal 6-mers meet there), one that begins 3 bases in front of the library (a direct terminal repeat, windows of 27), one that
    ends 3 bases behind it (an inverted one, windows of 21).  -> namespace with the inputs and, per family, what the restatements
    need (cores, sequence, consensus)."""
    rng = np.random.default_rng(2024)
    p = po.Params.named(SMALL_MATRIX, bandwidth=SMALL_W, L=SMALL_L, cappenalty=-10, when_to_stop=1000)       # (a cap that flanks do reach)
    fams = []
    for n, K, seed in SMALL_FAMILIES:
        if n == 0:
            fams.append(None)
            continue
        fs = synth_family(n, SMALL_L, SMALL_W, K=K, seed=seed, both_sides=True, minus_frac=0.4, n_run_frac=0.1)
        fams.append((np.ascontiguousarray(fs.sequence, np.int8), _clipped(fs, 6, SMALL_L + 8, seed) if n > 3 else fs.cores.copy()))
    front = _site_element(rng, 55, 27, False, 3)
    back = _site_element(rng, 42, 21, True, 3)
    word = rng.integers(0, 4, 6).astype(np.int8)
    mid = np.concatenate((rng.integers(0, 4, 23).astype(np.int8), [99], word, word, [99], rng.integers(0, 4, 23).astype(np.int8)))
    seqA, seqC = fams[0][0], fams[2][0]
    parts = [front[3:], seqA, mid, seqC, back[:-3]]
    lib = np.ascontiguousarray(np.concatenate(parts), np.int8)
    at = np.cumsum([0] + [len(x) for x in parts])
    offs = [int(at[1]), 0, int(at[3])]
    n = len(lib)
    junction = int(at[2]) + 23 + 1 + 6
    sites = np.array([(junction, junction - 1, 0, n - 1), (-3, 51, -3, n - 1), (n - 39, n + 2, 0, n + 7)], np.int64).view(TSD_SITE_DTYPE).reshape(-1)
    segs = np.zeros(3, PERIOD_SEG_DTYPE)
    segs["lo"], segs["hi"] = sites["lo"], sites["hi"]
    # the consensus of every family: the loop's own, changed (and two columns dropped, so that copies insert there)
    cons = np.zeros((3, SMALL_L), np.int8)
    rows, loops = [], []
    for f, fam in enumerate(fams):
        if fam is None:
            rows.append(0)
            loops.append(None)
            continue
        o = po.oracle_extend(1, fam[1].copy(), fam[0], new_master(SMALL_L), p, trace=True, row_trace=True)
        c = foreign(o.col_base[:o.rows_executed], at=9, k=2)[:SMALL_ROWS_C if f == 2 else SMALL_L]
        cons[f, :len(c)] = c
        rows.append(len(c))
        loops.append(o)
    _frozen(lib, cons, sites, segs)
    return types.SimpleNamespace(lib=lib, p=p, fams=fams, offs=offs, cons=cons, rows=rows, loops=loops, sites=sites, segs=segs,
                                 n_families=3, tiles=4, n_padded=256, hole_tile=2)


def small_layout():
    """-> ((flank array, 256), first, count) of SMALL: lay_out of the linkage tests with the tile of no family before family 1,
    the family without flanks (it takes no tile: its first is the next family's)."""
    from repeatafterme_amd import _lib
    from repeatafterme_amd.device import resolve_flanks
    s = small()
    parts = []
    for f, fam in enumerate(s.fams):
        if fam is None:
            parts.append(((_lib.Flank * 1)(), 0, 0))
        else:
            fl, nx = resolve_flanks(1, fam[1], SMALL_W, SMALL_L)[0]
            assert nx == fam[1].n
            parts.append((fl, nx, s.offs[f]))
    flanks, first, count = lay_out(parts, hole_before=1)
    assert flanks[1] == s.n_padded and first == [0, 192, 192] and count == [70, 0, 3]
    return flanks, first, count


def plane_lists(w):
    """The plane list of every family of a world: BIG's are given, SMALL's are selected from its pileups."""
    return w.planes if hasattr(w, "planes") else small_truth()["planes"]


def extents(w, W, L):
    """The extents a buffer is sized or strided by, of one world; the site windows' words as csrc/ramx_period_api.h counts them."""
    T = max(int(min(TERM["tmax"], (s["hi"] + 1 - s["lo"]) // 2)) for s in w.sites)
    seg = max(int(s["hi"] + 1 - s["lo"]) for s in w.segs)
    lists = plane_lists(w)
    return dict(padded_flanks=w.n_padded, tiles=w.tiles, maxrows=max(w.rows), L=L, KW=wr.window_words(L, W), library=len(w.lib),
                families=w.n_families, consensus_bytes=w.n_families * L, sites=len(w.sites),
                term_KW=(T + 7) // 8 + 1, term_SW=max((T + 31) // 32, 1), period_KW=(seg + 7) // 8 + 1, period_SW=max((seg + 31) // 32, 1),
                planes=max(len(x) for x in lists), planes_in_all=sum(len(x) for x in lists),
                plane_words=sum(r * 8 * ((len(c) + 63) // 64 if c is not None else 0) for r, c in zip(w.rows, _counts(w))),
                variants=max(len(sr.variants_of(x)[0]) for x in lists))


def _counts(w):
    return [None if fam is None else range(fam[1].n) for fam in w.fams]


# ---------------------------------------------------------------------------------------------------- SMALL's truth

def _profile_reference(cores, seq, p, cons):
    from test_gpu_profile import replay_reference
    return replay_reference(1, cores, seq, p, cons)


@functools.lru_cache(maxsize=None)
def small_truth():
    """Everything a SMALL call returns, from the restatements alone; per family f (None where the family has no flank or no row):
    profile (totals, counts, row_best, row_best_idx, last), walks (core indices, results), cols (pileup), di, refine, refine_cpg,
    stats / stats_reversed, planes (the selected list), pl (the bit sets), gram, init, subfam; and the three site-window
    answers."""
    s = small()
    t = dict(profile=[], walks=[], cols=[], di=[], refine=[], refine_cpg=[], stats=[], stats_reversed=[], planes=[], pl=[], gram=[],
             init=[], subfam=[])
    for f, fam in enumerate(s.fams):
        rows = s.rows[f]
        if fam is None or rows == 0:
            for k in t:
                t[k].append(None)
            t["planes"][-1] = lr.as_planes([])
            continue
        seq, cores = fam
        cons = s.cons[f, :rows]
        t["profile"].append(_profile_reference(cores, seq, s.p, cons))
        cols, di, idx, results = dr.pileups(1, cores, seq, s.p, cons, with_walks=True)
        t["walks"].append((idx, results))
        t["cols"].append(cols)
        t["di"].append(di)
        t["refine"].append(pr.refine(1, cores, seq, s.p, cons, 3))
        t["refine_cpg"].append(dr.refine_cpg(1, cores, seq, s.p, cons, 3))
        for key, rev in (("stats", False), ("stats_reversed", True)):
            t[key].append(cr.stats_of(1, cores, idx, results, seq, SMALL_W, cons, rev))
        pl = lr.planes_of(1, cores, idx, results, seq, SMALL_W, cons)
        planes = lr.select(cons, cols, **SELECT)
        t["pl"].append(pl)
        t["planes"].append(planes)
        t["gram"].append(lr.gram(pl, planes))
        init = sr.copy_init(pl, planes, SUBFAM_K, len(idx), 5 + f)
        t["init"].append(init)
        t["subfam"].append(sr.iterate(pl, planes, init, len(idx), max_iter=8))
    lib = s.lib
    t["tsd"] = ts.tsd_all(lib, [tuple(int(v) for v in x) for x in s.sites], **TSD)
    t["period"] = per.records(lib, [(int(x["lo"]), int(x["hi"])) for x in s.segs], **PERIOD)
    t["term"] = [tr.site_records(lib, tuple(int(v) for v in x), **TERM) for x in s.sites]
    return t


def small_windows():
    """(words, bounds) of SMALL's packed flank windows from tests/window_ref.py."""
    flanks, _, _ = small_layout()
    s = small()
    return wr.windows(s.lib, wr.descriptors(flanks), s.n_padded, SMALL_W, wr.window_words(SMALL_L, SMALL_W))


# ---------------------------------------------------------------------------------------------------- the loop's two worlds

LOOP_BIG = dict(n=700, W=40, L=200, K=150, seed=71)
LOOP_SMALL = dict(n=70, W=14, L=40, K=30, seed=72)


@functools.lru_cache(maxsize=None)
def loop_world(which):
    """One direction of the loop: -> namespace(seq, cores, p, oracle result of direction 1 from the untouched cores)"""
    c = LOOP_BIG if which == "big" else LOOP_SMALL
    fs = synth_family(c["n"], c["L"], c["W"], K=c["K"], seed=c["seed"], both_sides=True, minus_frac=0.4, n_run_frac=0.1)
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    p = po.Params.named("14p43g", bandwidth=c["W"], L=c["L"], when_to_stop=30)
    o = po.oracle_extend(1, fs.cores.copy(), seq, new_master(c["L"]), p, trace=True)
    _frozen(seq)
    return types.SimpleNamespace(seq=seq, cores=fs.cores, p=p, o=o, **c)


def extents_of_loop(which):
    c = LOOP_BIG if which == "big" else LOOP_SMALL
    return dict(padded_flanks=wr.padded_lanes(c["n"]), L=c["L"], W=c["W"], KW=wr.window_words(c["L"], c["W"]),
                state_bytes=wr.padded_lanes(c["n"]) * (c["W"] + 1) * 16)
