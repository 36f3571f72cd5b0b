"""The score-range gates of the kernel routes, restated in plain Python (tests only; no kernel code), and the scoring systems
and families the gate tests share.

Each fast route decides on the host whether a user's scoring system -- a 100 x 100 int32 matrix, gapopen, gapextn -- fits its
narrow arithmetic.  This module says, independently of the library, which side of each gate a system is on:

  pk_plan            csrc/ramx_packed.hip ramx_pk_plan          packed int16 rows of the lane-per-flank kernel
  fast_pack_ok       csrc/ramx_device.hip fast_pack_ok          fast band of the int32-row kernels, family kernel, profile replay
  cp_value_range_ok  csrc/ramx_cp.hip ramx_cp_max_family        cell-parallel kernel (the value-range part of it)
  go_ge_ok           csrc/ramx_device.hip route_gates           int32-row persistent kernel (e - m as int16 in LDS)

All of them look at the scores through the class table the device layer builds (ramx_dev_begin_direction): the matrix entries
[a][b] with a = 0..3 (the four candidate consensus bases) and b = 0..7 and 99 (A C G T, their soft-masked codes, N).
"""
from dataclasses import dataclass

import numpy as np

from oracle import pyoracle as po
from repeatafterme_amd.synth import synth_family

PK_WIDTHS = (14, 20, 40, 80)
PK_REBASE = 6000            # the base of a flank's packed row follows its best cell once that is further away (every 16th row)
PK_LIMIT = 32000            # what the plan lets an int16 intermediate reach
PK_MARGIN = 64
CLASS_CODES = tuple(range(8)) + (99,)


def class_table(matrix):
    """[9][4]: tab[class][candidate] = matrix[candidate][code(class)]."""
    m = np.asarray(matrix, np.int64).reshape(100, 100)
    return np.array([[m[a, b] for a in range(4)] for b in CLASS_CODES], np.int64)


def p_mn(matrix):
    """(P, mn): the largest class-table entry and the largest magnitude of a negative one, both >= 0."""
    t = class_table(matrix)
    return max(int(t.max()), 0), max(int(-t.min()), 0)


def pk_drift16(P, mn, GO, GE):
    """How far a flank's best cell can move over at most 16 rows.  Up: P per row (a substitution; gaps only lose).  Down: the
    best cell of row r, cell j, is followed to row r + k by d deletions first (cell j - d of row r + d: always in bounds while
    the flank has bases left) and k - d substitutions, where d > 0 only if the flank's end has come closer than cell j; that
    path costs at most GO + d GE + (k - d) mn, linear in d, so its maximum is at d = 1 or d = k."""
    return max(16 * P, 16 * mn, GO + GE + 15 * max(mn, GE))


@dataclass
class PkPlan:
    admitted: bool
    spread: int             # an in-bounds cell lies at most this far below its row's best cell
    lag: int                # the base lags the best cell by at most this
    total: int              # the larger of the two sums compared with PK_LIMIT (reported for both sides of the edge)


def pk_plan(W, gapopen, gapextn, matrix):
    P, mn = p_mn(matrix)
    GO, GE = -int(gapopen), -int(gapextn)
    if W not in PK_WIDTHS or gapopen > 0 or gapextn > 0:
        return PkPlan(False, 0, 0, 0)
    sp = 3 * W * (P + mn + GE) + GO + W * GE
    lag = PK_REBASE + pk_drift16(P, mn, GO, GE)
    total = max(sp + lag + mn + GO + GE, lag + P) + PK_MARGIN
    return PkPlan(total <= PK_LIMIT, sp, lag, total)


def _mx(gapopen, gapextn, matrix):
    return max(abs(int(gapopen)) + abs(int(gapextn)), int(np.abs(class_table(matrix)).max()))


def _int8(matrix):
    t = class_table(matrix)
    return bool(t.min() >= -128 and t.max() <= 127)


def fast_pack_ok(W, L, gapopen, gapextn, matrix):
    return _int8(matrix) and (L + 2 * W + 4) * _mx(gapopen, gapextn, matrix) < (1 << 27)


def cp_value_range_ok(W, L, gapopen, gapextn, matrix):
    if W not in PK_WIDTHS or gapopen > 0 or gapextn > 0 or L <= 0:
        return False
    return _int8(matrix) and (L + 2 * W + 4) * _mx(gapopen, gapextn, matrix) < (1 << 23) and 200 * -int(gapextn) < (1 << 23)


def go_ge_ok(gapopen, gapextn):
    return gapopen <= 0 and gapextn <= 0 and gapopen + gapextn >= -32768


# ---- scoring systems of a given shape ----------------------------------------------------------------------------------------

def shape_matrix(P, mn):
    """+P where the candidate equals the base (soft-masked or not), -mn everywhere else (N included)."""
    m = np.zeros((100, 100), np.int32)
    for a in range(4):
        for b in CLASS_CODES:
            m[a, b] = P if b < 8 and (b & 3) == a else -mn
    return m.reshape(-1)


def scale_system(matrix, gapopen, gapextn, s):
    """(matrix, gapopen, gapextn) with every class-table entry and both gap penalties multiplied by s."""
    m = np.asarray(matrix, np.int64).reshape(100, 100).copy()
    for a in range(4):
        for b in CLASS_CODES:
            m[a, b] *= s
    return m.reshape(-1).astype(np.int32), int(gapopen) * s, int(gapextn) * s


def largest_scale(admits, hi=1 << 20):
    """The largest integer s in [1, hi] with admits(s), for a gate that is monotone in s (admitted up to some s, refused
    above); 0 if s = 1 is refused, hi if the gate has no edge below it (a system of zeros: every scale is the same system)."""
    if not admits(1):
        return 0
    if admits(hi):
        return hi
    lo = 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if admits(mid):
            lo = mid
        else:
            hi = mid
    return lo


def largest_pk_scale(W, matrix, gapopen, gapextn):
    def admits(s):
        m, go, ge = scale_system(matrix, gapopen, gapextn, s)
        return pk_plan(W, go, ge, m).admitted
    return largest_scale(admits)


# ---- the six shapes of scoring system of the packed-row tests, and their families ---------------------------------------------

SHAPES = {                   # (P, mn, GO, GE) at scale 1; "a" is the built-in 14p43g with its own gap penalties
    "a": None,
    "b": (1, 1, 0, 10),      # gap-extension-heavy
    "c": (1, 1, 60, 2),      # gap-open-heavy: GO in the thousands at the admitted scale
    "d": (20, 1, 3, 1),      # match-heavy
    "e": (1, 20, 3, 1),      # mismatch-heavy
    "f": (5, 4, 0, 0),       # free gaps
}


def shape_system(shape):
    """(matrix, gapopen, gapextn, cappenalty, minimprovement) of a shape at scale 1."""
    if SHAPES[shape] is None:
        p = po.Params.named("14p43g")
        return p.matrix, p.gapopen, p.gapextn, p.cappenalty, p.minimprovement
    P, mn, GO, GE = SHAPES[shape]
    return shape_matrix(P, mn), -GO, -GE, -5 * max(P, mn), 2 * P


def shape_params(shape, s, W, L, **kw):
    m, go, ge, cap, mini = shape_system(shape)
    m, go, ge = scale_system(m, go, ge, s)
    return po.Params(bandwidth=W, cappenalty=cap * s, minimprovement=mini * s, L=L, when_to_stop=kw.pop("when_to_stop", L),
                     l=1, gapopen=go, gapextn=ge, matrix=m, **kw)


def edge_scale(shape, W):
    m, go, ge = shape_system(shape)[:3]
    return largest_pk_scale(W, m, go, ge)


def gate_family(n, L, W, seed, cut=(40, 250), K=150):
    """Aligned copies (K columns, then unrelated sequence), N runs in a fifth of the flanks, every third flank ending `cut`
    bases past the core -- most of them while still aligned."""
    fs = synth_family(n, L, W, K=K, seed=seed, core_len=12, n_run_frac=0.2)
    rng = np.random.default_rng(seed + 1)
    short = np.arange(0, n, 3)
    fs.cores.upper[short] = fs.cores.right_pos[short] + rng.integers(cut[0], cut[1] + 1, size=len(short))
    return fs
