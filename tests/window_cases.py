"""The inputs of tests/test_gpu_windows.py, built here so that tests/test_window_ref.py can vouch for them on the CPU: every
case is a one-byte-per-base library, flank descriptors, W and L, and the packed tables the device is fed (several sets where a
test runs the same flanks over other window layouts).  Nothing here needs a GPU: the flanks come from ramx_resolve_flanks (host
C) or are written out by hand."""
from dataclasses import dataclass, field

import numpy as np

import window_ref as wr

SWEEP_SEEDS = (300, 301, 302)
SWEEP_W = (0, 3, 14, 40, 80)
SWEEP_L = (50, 600)
LOOP_W = (0, 14, 40, 80)
FLANK_COUNTS = (1, 63, 64, 65, 130, 256, 257, 321)


@dataclass
class Case:
    name: str
    lib: np.ndarray                 # one byte per base, lower case and N included
    descs: list                     # [(start, t_lo, t_hi, step, compl)]
    W: int
    L: int
    tables: dict = field(default_factory=dict)     # name -> packed tables of wr.fold(lib)
    flanks: tuple = None            # (ctypes flank array, n) for the device
    extra: dict = field(default_factory=dict)

    @property
    def KW(self):
        return wr.window_words(self.L, self.W)


def flank_array(descs):
    from repeatafterme_amd import _lib
    arr = (_lib.Flank * max(len(descs), 1))()
    for i, (start, t_lo, t_hi, step, compl) in enumerate(descs):
        arr[i].start, arr[i].t_lo, arr[i].t_hi, arr[i].step, arr[i].compl_ = start, t_lo, t_hi, step, compl
    return arr, len(descs)


def split_runs_at_windows(tables):
    """A run of N that crosses a window's first base becomes two runs that touch there: what a loader makes of two records that
    end and begin with N, and what the diff in pack_library never produces."""
    starts = set(int(s) for s in tables["win_start"][1:-1])
    ns, nl = [], []
    for s, ln in zip(tables["n_start"], tables["n_len"]):
        s, e = int(s), int(s) + int(ln)
        for c in sorted(x for x in starts if s < x < e):
            ns.append(s); nl.append(c - s)
            s = c
        ns.append(s); nl.append(e - s)
    out = dict(tables)
    out["n_start"], out["n_len"] = np.array(ns, np.uint64), np.array(nl, np.uint32)
    return out


def packed_tables(lib, starts):
    """pack_library of the folded library with the phases cycling 0..3 over the windows."""
    from repeatafterme_amd.loader import pack_library
    starts = sorted(set(int(s) for s in starts) | {0})
    return pack_library(wr.fold(lib), starts, [i % 4 for i in range(len(starts))])


def _starts_of(boundaries):
    return [0] + [int(b) for b in boundaries[:-2]]       # FlankSet.boundaries: every window's end, then a 0


def _inside_starts(descs, lib_len, seed):
    """Extra window starts inside flanks: for two flanks in three a position 9..70 bases into the flank (mid-word for most W)."""
    rng = np.random.default_rng(seed)
    out = []
    for i, (start, t_lo, t_hi, step, _) in enumerate(descs):
        if i % 3 == 2 or t_hi < 12:
            continue
        t = int(rng.integers(9, min(t_hi, 70) + 1))
        p = start + step * t
        if 0 < p < lib_len:
            out.append(p)
    return out


_memo = {}


def _memoised(fn):
    def wrapped(*a):
        key = (fn.__name__,) + a
        if key not in _memo:
            _memo[key] = fn(*a)
        return _memo[key]
    return wrapped


def _adversarial(seed, direction, W, L, n_windows=40):
    from repeatafterme_amd.device import resolve_flanks
    from repeatafterme_amd.synth import synth_adversarial
    fs = synth_adversarial(seed, n_windows=n_windows, L=L, W=W, lowercase=True)
    lib = np.ascontiguousarray(fs.sequence, np.int8)
    flanks, idx = resolve_flanks(direction, fs.cores, W, L)
    descs = wr.descriptors(flanks)
    at = _starts_of(fs.boundaries)
    c = Case(f"adversarial seed {seed} dir {direction} W {W} L {L}", lib, descs, W, L, flanks=flanks,
             tables={"bounds": packed_tables(lib, at), "inside": packed_tables(lib, at + _inside_starts(descs, len(lib), seed))},
             extra=dict(fs=fs, idx=idx, direction=direction, seed=seed))
    return c


@_memoised
def sweep_cases(W, L):
    """synth_adversarial (truncated flanks, N runs, both strands, tightened bounds, lower case), both directions; the windows
    begin at the set's own boundaries ("bounds") and also inside flanks ("inside").  Twice as many windows at the short L, where
    a window holds few words for the N runs to fall into."""
    return [_adversarial(seed, d, W, L, n_windows=80 if L < 100 else 40) for seed in SWEEP_SEEDS for d in (1, 0)]


@_memoised
def loop_cases(W):
    """The same sets at the L of a short direction, for the loop on the packed form."""
    return [_adversarial(seed, d, W, 120) for seed in SWEEP_SEEDS for d in (1, 0)]


@_memoised
def count_cases(n):
    """n flanks exactly, both strands, N runs, a window of the packed form per copy."""
    from repeatafterme_amd.device import resolve_flanks
    from repeatafterme_amd.synth import synth_family
    W, L = 14, 100
    fs = synth_family(n, L, W, K=90, seed=500 + n, both_sides=True, minus_frac=0.4, n_run_frac=0.3)
    lib = np.ascontiguousarray(fs.sequence, np.int8)
    out = []
    for d in (1, 0):
        flanks, idx = resolve_flanks(d, fs.cores, W, L)
        assert flanks[1] == n
        out.append(Case(f"{n} flanks dir {d}", lib, wr.descriptors(flanks), W, L, flanks=flanks,
                        tables={"bounds": packed_tables(lib, _starts_of(fs.boundaries))}))
    return out


NMASK_W = 3
RUN_LENGTHS = (1, 7, 8, 9, 16, 300)


@_memoised
def nmask_case():
    """A library written for the N mask of the fast path.  Runs of length 1, 7, 8, 9, 16 at every alignment mod 8 and of length
    300 at two; a run of 1 at position 0 and a run of 9 that ends at the last position; pairs and triples of runs within eight
    bases at every alignment; runs that cross a window's first base (split into two touching runs in the "windows" tables).
    Flanks: forward and reverse complemented over the whole library from all eight alignments (they run off position 0 and off
    the last position), and shorter ones with t_lo > 0, bounds that cut words, and an empty one.  Tables: one window, several
    windows, and "clean": the same flanks over a copy of the library without any N (n_blocks = 0)."""
    rng = np.random.default_rng(77)
    parts, marks = [], []             # marks: positions at which a window is to begin

    def clean(k):
        parts.append(rng.integers(0, 4, k).astype(np.int8))

    def run(k):
        parts.append(np.full(k, 99, np.int8))

    def at():
        return sum(len(p) for p in parts)

    def align(a):                      # clean bases up to the next position = a mod 8, at least 17 of them
        clean(17)
        clean((a - at()) % 8)

    run(1)
    for ln in RUN_LENGTHS[:5]:
        for a in range(8):
            align(a)
            run(ln)
    for a in (3, 0):
        align(a)
        run(300)
    for a in range(8):                 # pairs: N x N N
        align(a)
        run(1); clean(1); run(2)
    for a in range(8):                 # triples: N x N x x N N   (seven bases)
        align(a)
        run(1); clean(1); run(1); clean(2); run(2)
    for a in range(8):                 # a run across a window's first base, three bases before it and four behind
        align(a)
        run(3); marks.append(at()); run(4)
    for a in (1, 6):                   # ... and windows that begin on clean ground, mid-word
        align(a)
        marks.append(at())
    align(5)
    run(9)
    lib = np.concatenate(parts)
    n = len(lib)
    assert lib[0] == 99 and lib[1] != 99 and (lib[n - 9:] == 99).all() and lib[n - 10] != 99
    W, L = NMASK_W, n
    far = L + W + 2
    descs = []
    for a in range(8):
        for t_lo in (-W - 2, -2):
            descs.append((a, t_lo, far, 1, 0))
            descs.append((n - 1 - a, t_lo, far, -1, 1))
    for i, (t_lo, ln) in enumerate(((1, 90), (5, 300), (8, 61), (13, 700), (29, 33), (2, 450), (40, 41))):
        descs.append((100 + 37 * i, t_lo, t_lo + ln, 1, i % 2))
        descs.append((n - 90 - 41 * i, t_lo, t_lo + ln, -1, 1 - i % 2))
    descs.append((500, 1, 0, 1, 0))    # empty
    nolib = lib.copy()
    isn = nolib == 99
    nolib[isn] = rng.integers(0, 4, int(isn.sum()))
    c = Case("N mask", lib, descs, W, L, flanks=flank_array(descs),
             tables={"one": packed_tables(lib, [0]), "windows": split_runs_at_windows(packed_tables(lib, marks))},
             extra=dict(clean_lib=nolib, clean_tables=packed_tables(nolib, marks), marks=marks))
    assert len(c.extra["clean_tables"]["n_len"]) == 0
    return c


def loader_case(tmp):
    """A genome whose records have lengths 4k + 1, 4k + 2, 4k + 3 and 4k, written as .2bit and loaded with the packed loader:
    ranges at a record's first and last base, both strands, N runs at both ends of a record and inside.  -> Case whose tables
    are the loader's own, and the loader's FlankSet."""
    import os
    from repeatafterme_amd.device import resolve_flanks
    from repeatafterme_amd.loader import load_sequence_subset_packed, write_ranges, write_twobit
    rng = np.random.default_rng(123)
    recs = []
    for name, ln in (("r1", 1001), ("r2", 802), ("r3", 1311), ("r4", 76), ("r5", 333)):
        a = rng.integers(0, 4, ln).astype(np.int8)
        for _ in range(ln // 40):
            s = int(rng.integers(0, ln - 1))
            a[s:s + int(rng.integers(1, 20))] = 99
        recs.append((name, a))
    recs[1][1][:5] = 99
    recs[1][1][-3:] = 99
    recs[2][1][-1] = 99
    rows = [("r1", 0, 6, 1, 1, "+"), ("r1", 995, 1001, 1, 1, "-"), ("r1", 400, 420, 1, 1, "-"), ("r1", 130, 141, 1, 1, "+"),
            ("r2", 0, 9, 1, 1, "-"), ("r2", 795, 802, 1, 1, "+"), ("r2", 300, 310, 1, 1, "+"),
            ("r3", 1300, 1311, 1, 1, "+"), ("r3", 0, 3, 1, 1, "-"), ("r3", 650, 655, 1, 1, "-"), ("r3", 901, 927, 1, 1, "+"),
            ("r4", 0, 76, 1, 1, "+"), ("r4", 30, 40, 1, 1, "-"), ("r5", 1, 5, 1, 1, "+"), ("r5", 329, 332, 1, 1, "-"),
            ("r5", 150, 170, 1, 1, "+")]
    tb, bed = os.path.join(str(tmp), "w.2bit"), os.path.join(str(tmp), "w.tsv")
    write_twobit(tb, recs)
    write_ranges(bed, rows)
    fs, tables = load_sequence_subset_packed(tb, bed, 200)
    W, L = 14, 150
    out = []
    for d in (1, 0):
        flanks, _ = resolve_flanks(d, fs.cores, W, L)
        out.append(Case(f"loader dir {d}", np.ascontiguousarray(fs.sequence, np.int8), wr.descriptors(flanks), W, L, flanks=flanks,
                        tables={"loader": tables}, extra=dict(fs=fs, recs=recs)))
    return out


PIECES_W, PIECES_L, PIECES_N = 40, 760, 300


@_memoised
def pieces_case():
    """The family of test_gpu_persistent.py's pieces test at 300 flanks: two shared copies with a gap between, some flanks that
    end early; one window of the packed form per copy."""
    from repeatafterme_amd.device import resolve_flanks
    import test_gpu_persistent as tgp
    fs = tgp._two_copy_family(PIECES_N, PIECES_L, PIECES_W, 100, seed=6100, short_frac=0.05)
    lib = np.ascontiguousarray(fs.sequence, np.int8)
    flanks, idx = resolve_flanks(1, fs.cores, PIECES_W, PIECES_L)
    assert flanks[1] == PIECES_N
    return Case("two-copy family", lib, wr.descriptors(flanks), PIECES_W, PIECES_L, flanks=flanks,
                tables={"bounds": packed_tables(lib, _starts_of(fs.boundaries))}, extra=dict(fs=fs))


@_memoised
def replay_case():
    """Two families on one library, laid out in tiles with a tile that belongs to neither between them (the layout of
    test_gpu_linkage.py): -> Case over the padded flank array, with first / count of the families."""
    from repeatafterme_amd.device import resolve_flanks
    from repeatafterme_amd.synth import synth_family
    import test_gpu_replay_long as rl
    W, L = 14, 120
    fams = [synth_family(n, L, W, K=100, seed=s, both_sides=True, minus_frac=0.4, n_run_frac=0.3) for n, s in ((70, 31), (100, 32))]
    lib = np.ascontiguousarray(np.concatenate([fs.sequence for fs in fams]), np.int8)
    offs = [0, len(fams[0].sequence)]
    parts, starts = [], []
    for fs, off in zip(fams, offs):
        fl, nx = resolve_flanks(1, fs.cores, W, L)[0]
        parts.append((fl, nx, off))
        starts += [off + s for s in _starts_of(fs.boundaries)]
    flanks, first, count = rl.lay_out(parts, hole_before=1)
    return Case("two families and a hole", lib, wr.descriptors(flanks), W, L, flanks=flanks,
                tables={"bounds": packed_tables(lib, starts)}, extra=dict(first=first, count=count))
