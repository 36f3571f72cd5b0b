"""Column sums past 2^31 (tests only; no kernel code): the identity the wide-sum tests stand on, the vote and stop rule restated
on a table of sums, and the families and scoring systems those tests share.

The reference keeps the four column sums of a row in `int` (ram_extend.c:874-878) and so does the oracle; the library keeps them in
int64 and raises `overflow32` where the reference would have wrapped.  Nothing int32 can therefore say what the library must compute
past 2^31 -- but a small family can.  Repeat every core of a family of m copies r times (the same windows of the same sequence: only
the core arrays grow).  Every copy's DP rows are those of the copy it repeats, so every column sum of the big family is exactly r
times the small family's; the cap rule (ram_extend.c:1052-1062) is per copy and does not change; and the stop rule
curr >= max + dist * minimprovement (:1194-1196) scales exactly when the big family runs with r times the minimprovement.  On int64
sums the big family therefore goes where the small one goes: same return value, rows, consensus, the per-copy results tiled r
times -- and `overflow32` is set exactly when r * max(S[:rows_executed]) > 2^31 - 1, S being the small run's traced sums.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import CoreSet
from repeatafterme_amd.synth import synth_family

import score_gates as sg

INT32_MAX = 2 ** 31 - 1


def replicate(cores, r):
    """The family of `cores` with every core repeated r times: copy i of the result is copy i % n of `cores`."""
    return CoreSet(**{k: np.tile(getattr(cores, k), r) for k in cores.__dataclass_fields__})


def _int32(v):
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def vote(sums, minimprovement, when_to_stop, wrap=False):
    """The vote (ram_extend.c:1081-1085) and the stop rule (:1194-1216) on a table of sums [L][4], as the loop applies them row by
    row -> (ret, rows_executed, limit_warning, consensus of the executed rows).  wrap: every sum, and the right-hand side of the stop
    rule, reduced to int32 the way the reference's `int` holds them.  (The sums of a row depend on the consensus of the rows
    before it: where a wrapped vote leaves the path the sums were traced on, its later rows mean nothing -- but it has left.)"""
    L = len(sums)
    max_ext, max_row, cons = 0, -1, []
    for r in range(L):
        curr, besta = 0, 0
        for a in range(4):
            s = _int32(sums[r][a]) if wrap else int(sums[r][a])
            if s > curr:
                curr, besta = s, a
        cons.append(besta)
        bar = max_ext + abs(max_row - r) * int(minimprovement)
        if curr >= (_int32(bar) if wrap else bar):
            max_row, max_ext = r, curr
        if abs(r - max_row) >= when_to_stop:
            break
    else:
        r = L                                       # ran out of rows: no warning (ram_extend.c:1225 compares after the last r++)
    rows = min(r + 1, L)
    return max_row + 1, rows, int(r == L - 1), np.array(cons[:rows], np.int8)


def edge_replications(S, rows):
    """(r_lo, r_lo + 1): the most repetitions that keep every sum of the executed rows within int32, and the fewest that do not."""
    r_lo = INT32_MAX // int(np.max(S[:rows]))
    return r_lo, r_lo + 1


def deep_replication(S, rows, at=0.25):
    """The fewest repetitions that put the first sum above int32 into the first `at` of the executed rows (a quarter): most votes,
    every later new maximum and the stop decision then happen above 2^31."""
    return INT32_MAX // int(np.max(S[:max(int(rows * at), 1)])) + 1


def first_wide_row(S, rows, r):
    """The first executed row in which r * S leaves int32, or None."""
    over = np.flatnonzero(np.max(S[:rows], axis=1) * int(r) > INT32_MAX)
    return int(over[0]) if len(over) else None


# ---- the configurations of tests/test_gpu_wide_sums.py (pinned on the CPU by tests/test_wide_sums_ref.py) -------------------------

@dataclass(frozen=True)
class Config:
    W: int
    P: int                  # score of a match; cappenalty = -5 max(P, mn)
    mn: int                 # magnitude of the score of a mismatch
    go: int
    ge: int
    m: int                  # copies of the small family
    L: int
    K: int                  # aligned columns of the family
    stop: int = 30          # when_to_stop
    q: int = 0              # minimprovement of the small family (0: 2 P, as tests/score_gates.py has it)
    seed: int = 5
    both_sides: bool = True
    core_len: int = 10
    deep_at: float = 0.25   # deep_replication puts the first sum above int32 into this part of the executed rows
    max_copies: int = 0     # a limit of the route on the size of the big family (0: none)


# The register-resident kernels (int32 rows, family kernel, resident profile replay) take gapopen + gapextn >= -32768 only
# (score_gates.go_ge_ok), so their system is a tenth of the streaming kernel's, with more columns or copies to make up for it.
_BIG = (100000, 80000, -250000, -50000)
_ROWS = (10000, 8000, -25000, -5000)
CONFIGS = {
    "stream14": Config(14, *_BIG, 60, 120, 70),
    "stream9": Config(9, *_BIG, 60, 120, 70),                       # no kernel is specialised for this band width
    "rows14": Config(14, *_ROWS, 60, 200, 150),
    "rows80": Config(80, *_ROWS, 60, 200, 150),
    # the family kernel takes up to 512 copies: few copies in the small family, many columns
    "family14": Config(14, *_ROWS, 4, 1100, 1000, q=10000, deep_at=0.6, max_copies=512),
    "family14_a": Config(14, *_ROWS, 4, 1100, 300, q=10000, seed=6, max_copies=512),      # the neighbours of the batch: a third of the columns
    "family14_b": Config(14, *_ROWS, 4, 1100, 350, q=10000, seed=7, max_copies=512),
    # admitted to the packed int16 rows; the stop rule fires in the last rows, so that the packed kernel runs L - W rows or more
    "packed14": Config(14, 200, 150, -450, -75, 64, 2000, 1962, q=2000),
    "packed14_short": Config(14, 200, 150, -450, -75, 64, 2000, 1962, q=2000, both_sides=False),
    # int8 scores for the cell-parallel kernel
    "cells40": Config(40, 127, 100, -300, -50, 64, 2000, 1900, q=1270),
    # the profile replay: more than 256 columns
    "profile14": Config(14, *_ROWS, 60, 300, 280),
}


BATCH_MIDDLE, BATCH_NEIGHBOURS = "family14", ("family14_a", "family14_b")      # the batch seam: only the middle family crosses


def family(cfg):
    return synth_family(cfg.m, cfg.L, cfg.W, cfg.K, seed=cfg.seed, both_sides=cfg.both_sides, minus_frac=0.3, n_run_frac=0.2, div=0.05,
                        core_len=cfg.core_len)


def params(cfg, r=1):
    """The scoring system of a configuration, for the family repeated r times."""
    return po.Params(bandwidth=cfg.W, cappenalty=-5 * max(cfg.P, cfg.mn), minimprovement=(cfg.q or 2 * cfg.P) * r, L=cfg.L, when_to_stop=cfg.stop,
                     l=1, gapopen=cfg.go, gapextn=cfg.ge, matrix=sg.shape_matrix(cfg.P, cfg.mn))


@dataclass
class SmallRun:
    cfg: Config
    fs: object              # the FlankSet of the small family
    cores: object           # its cores after both directions (right, then left, as main() runs them)
    master: np.ndarray
    res: tuple              # the oracle's traced results (right, left)

    @property
    def directions(self):
        return (1, 0) if self.cfg.both_sides else (1,)

    def direction(self, d):
        return self.res[0 if d else 1]

    def S(self, d):
        return self.direction(d).col_sums

    def top(self, d):
        o = self.direction(d)
        return int(np.max(o.col_sums[:o.rows_executed])) if o.rows_executed else 0

    def overflows(self, d, r):
        return int(r * self.top(d) > INT32_MAX)

    def replications(self, deep=True):
        """Both sides of the edge of either direction, and (deep) the repetitions that put the crossing early in both."""
        rs = set()
        for d in self.directions:
            o = self.direction(d)
            if o.rows_executed and self.top(d) > 0:
                rs.update(edge_replications(o.col_sums, o.rows_executed))
                if deep:
                    rs.add(deep_replication(o.col_sums, o.rows_executed, self.cfg.deep_at))
        return sorted(rs)


@lru_cache(maxsize=None)
def small_run(name):
    """The oracle on the small family of a configuration, both directions, traced.  Computed once per process; do not change it."""
    cfg = CONFIGS[name]
    fs = family(cfg)
    p = params(cfg)
    c, m = fs.cores.copy(), po.new_master(cfg.L)
    right = po.oracle_extend(1, c, fs.sequence, m, p, trace=True)
    left = po.oracle_extend(0, c, fs.sequence, m, p, trace=True) if cfg.both_sides else None
    return SmallRun(cfg, fs, c, m, (right, left))


def check_premises(run, d, r):
    """The conditions under which the identity says what the big family must compute, and under which a kernel that truncated could
    not pass by luck; asserted wherever a configuration is used.  -> the first row above int32 (None below the edge)."""
    cfg, o = run.cfg, run.direction(d)
    S, rows = o.col_sums, o.rows_executed
    q = params(cfg).minimprovement
    assert 0 <= S.min() and S.max() <= INT32_MAX, "the small run itself must stay within int32"
    assert cfg.L * r * q <= INT32_MAX, "the reference's own int product abs(..) * MINIMPROVEMENT must not be what wraps"
    assert cfg.max_copies == 0 or cfg.m * r <= cfg.max_copies, (cfg.m * r, cfg.max_copies)
    wide = vote(r * S, r * q, cfg.stop)
    assert wide[:3] == (o.ret, rows, o.limit_warning) and np.array_equal(wide[3], o.col_base[:rows])
    first = first_wide_row(S, rows, r)
    if first is not None:
        wrapped = vote(r * S, r * q, cfg.stop, wrap=True)
        assert wrapped[:2] != wide[:2] or not np.array_equal(wrapped[3], wide[3]), "the case must tell int64 sums from wrapped ones"
    return first


def pk_first_row(direction, cores, W, L):
    """The row from which the packed-row kernel takes a direction (csrc/ramx_device.hip, ramx_dev_begin_direction): the first in
    which no flank has an out-of-bounds cell at the low end of the band; the int32 rows run before it."""
    from repeatafterme_amd.device import resolve_flanks
    (fl, nx), _ = resolve_flanks(direction, cores, W, L)
    return max([0] + [fl[i].t_lo + W for i in range(nx) if fl[i].t_lo <= fl[i].t_hi])
