"""The 9 x 4 class table (tests only; no kernel code): scoring systems in which every entry of the table can be told from every
other, families that carry soft-masked bases and N into every column a kernel executes, and the confusions a restated table can
suffer, as functions from matrix to matrix.

Every kernel scores a base through tab[class][candidate] = matrix[candidate][code(class)], the classes being A C G T a c g t N
(csrc/ramx_device.hip class_tab); the library restates that table about ten times, each in its own layout.  The built-in systems
hold ONE constant in the 20 entries of the classes 4..8, so no test on them can see a confusion among those classes, a wrong
lower-case complement, a wrong candidate index or an N score taken for padding.  The systems here differ from 14p43g only on
[0..3] x [0..7, 99]; what a family must give under them comes from the oracle on the family itself (oracle_run), and the oracle is
pinned to the reference on these very systems by tests/test_class_table_ref.py.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import SYM_N
from repeatafterme_amd.synth import synth_family

import score_gates as sg
from score_gates import CLASS_CODES

LOWER = (4, 5, 6, 7)
WHEN_TO_STOP = 20

# ---- scoring systems ---------------------------------------------------------------------------------------------------------------

# DISTINCT[candidate][class]: 36 pairwise distinct entries.  Matches 12..9 in upper case and 8..5 in lower case, N small with both
# signs, the 24 mismatches are -3..-26, each once.
#               A    C    G    T    a    c    g    t    N
DISTINCT = ((  12, -18, -10, -21,   8, -16,  -8, -24,  -1),
            ( -19,  11, -20,  -7, -14,   7, -22,  -5,   2),
            (  -6, -17,  10, -15,  -4, -25,   6, -12,  -2),
            ( -23,  -9, -13,   9, -26, -11,  -3,   5,   1))
N_PAYS = (-4, -4, 4, -4)                # the score of N per candidate

SYSTEMS = ("distinct", "nocase", "n_pays", "distinct_go", "distinct_x11")


def _base():
    p = po.Params.named("14p43g")
    return p.matrix.reshape(100, 100).copy(), p.gapopen, p.gapextn


def _with_table(table):
    m, _, _ = _base()
    for a in range(4):
        for k, b in enumerate(CLASS_CODES):
            m[a, b] = table[a][k]
    return m.reshape(-1).astype(np.int32)


def matrix_of(name):
    """(matrix int32[100*100], gapopen, gapextn) of a named system."""
    m, go, ge = _base()
    if name == "distinct":
        return _with_table(DISTINCT), go, ge
    if name == "nocase":
        m[:4, 4:8] = m[:4, 0:4]
        m[:4, SYM_N] = -1
        return m.reshape(-1), go, ge
    if name == "n_pays":
        m[:4, SYM_N] = N_PAYS
        return m.reshape(-1), go, ge
    if name == "distinct_go":
        return _with_table(DISTINCT), 3, ge
    if name == "distinct_x11":
        return _with_table([[11 * v for v in row] for row in DISTINCT]), 11 * go, 11 * ge
    if name == "14p43g":
        return m.reshape(-1), go, ge
    raise KeyError(name)


def system(name, W, L, when_to_stop=WHEN_TO_STOP):
    """po.Params of a named system: cap penalty and minimum improvement are 14p43g's."""
    m, go, ge = matrix_of(name)
    p = po.Params.named("14p43g", bandwidth=W, L=L, when_to_stop=when_to_stop)
    p.matrix, p.gapopen, p.gapextn = m, go, ge
    return p


def check_systems():
    """What the systems are said to be (asserted by the CPU tests)."""
    base = _base()[0]
    outside = np.ones((100, 100), bool)
    outside[np.ix_(range(4), CLASS_CODES)] = False
    for name in SYSTEMS:
        m = matrix_of(name)[0].reshape(100, 100)
        assert np.array_equal(m[outside], base[outside]), name              # differs from 14p43g on [0..3] x [0..7, 99] only
    t = sg.class_table(matrix_of("distinct")[0])                            # [class][candidate]
    assert len(set(t.reshape(-1).tolist())) == 36
    assert t.min() >= -128 and t.max() <= 127
    for c in range(8):
        for k in range(4):
            assert (t[c][k] > 0) == ((c & 3) == k), (c, k)
    assert min(t[c][c] for c in range(4)) > max(t[c][c & 3] for c in LOWER)
    assert np.abs(t[8]).max() <= 2 and (t[8] > 0).any() and (t[8] < 0).any()
    t = sg.class_table(matrix_of("nocase")[0])
    assert np.array_equal(t[4:8], t[0:4]) and (t[8] == -1).all() and not np.array_equal(t[0:4], t[0:4].T)
    t = sg.class_table(matrix_of("n_pays")[0])
    assert np.array_equal(t[:8], sg.class_table(base)[:8]) and tuple(t[8]) == N_PAYS
    assert np.array_equal(sg.class_table(matrix_of("distinct_x11")[0]), 11 * sg.class_table(matrix_of("distinct")[0]))
    assert np.array_equal(matrix_of("distinct_go")[0], matrix_of("distinct")[0]) and matrix_of("distinct_go")[1] == 3


def gates(name, W, L):
    """Which gates of tests/score_gates.py admit the system at this shape."""
    m, go, ge = matrix_of(name)
    return dict(pk=sg.pk_plan(W, go, ge, m).admitted, fast=sg.fast_pack_ok(W, L, go, ge, m), cp=sg.cp_value_range_ok(W, L, go, ge, m),
                go_ge=sg.go_ge_ok(go, ge))


def expected_gates(name, W):
    """What the GPU module relies on: the three ordinary systems are admitted to every narrow route that has their band width, a
    positive gap-open penalty closes every one-launch route, and scores eleven times as large close every narrow one but leave
    the int32 rows."""
    wide = W in sg.PK_WIDTHS
    if name in ("distinct", "nocase", "n_pays"):
        return dict(pk=wide, fast=True, cp=wide, go_ge=True)
    if name == "distinct_go":
        return dict(pk=False, fast=True, cp=False, go_ge=False)
    return dict(pk=False, fast=False, cp=False, go_ge=True)


# ---- families ------------------------------------------------------------------------------------------------------------------------

def soft_family(n, L, W, K, seed, frac=0.35):
    """synth_family(n, L, W, K, seed, both strands, N runs) with `frac` of its bases soft-masked -- 4 added to an A C G T code,
    singly for half of the masked bases and in runs of 5 to 40 for the rest; N stays N -- and every window clipped as
    helpers.ragged_family clips it, so that flanks end at different columns and out-of-bounds padding lies beside scored N."""
    fs = synth_family(n, L, W, K=K, seed=seed, both_sides=True, minus_frac=0.4, n_run_frac=0.15)
    rng = np.random.default_rng([seed, 4])
    seq = fs.sequence
    mask = rng.random(len(seq)) < frac / 2
    while mask.mean() < frac:                                   # (runs overlap each other and the single bases: a few passes)
        k = max(1, int((frac - mask.mean()) * len(seq) / 22.5))
        edges = np.zeros(len(seq) + 41, np.int32)
        starts = rng.integers(0, len(seq), k)
        np.add.at(edges, starts, 1)
        np.add.at(edges, starts + rng.integers(5, 41, k), -1)
        mask |= np.cumsum(edges)[:len(seq)] > 0
    fs.sequence = np.where(mask & (seq < 4), seq + 4, seq).astype(np.int8)
    q = np.random.default_rng(seed).integers(40, L + 1, fs.cores.n)
    fs.cores.upper = np.minimum(fs.cores.upper, fs.cores.right_pos + q)
    fs.cores.lower = np.maximum(fs.cores.lower, fs.cores.left_pos - q)
    return fs


def executed_cells(fs, direction, rows, W):
    """-> (library positions, in-bounds flags, minus-strand flags), each [n][rows + W]: the bases the band of the executed rows
    can read in this direction, copy by copy (flank position t lies `t + 1` bases beyond the core's edge)."""
    c = fs.cores
    minus = c.orient.astype(bool)
    up = ~minus if direction else minus
    start = np.where(direction, c.right_pos, c.left_pos)
    t = np.arange(rows + W)[None, :] + 1
    pos = start[:, None] + np.where(up, 1, -1)[:, None] * t
    inb = (pos >= c.lower[:, None]) & (pos <= c.upper[:, None])
    ext = (c.right_ext if direction else c.left_ext).astype(bool)
    return pos, inb & ext[:, None], np.broadcast_to(minus[:, None], pos.shape)


@dataclass
class Run:
    name: str               # the scoring system
    fs: object
    p: object
    cores: object           # after both directions (right, then left)
    master: np.ndarray
    res: tuple              # the oracle's results (right, left)

    def direction(self, d):
        return self.res[0 if d else 1]


def run_oracle(fs, p):
    c, m = fs.cores.copy(), po.new_master(p.L)
    right = po.oracle_extend(1, c, fs.sequence, m, p)
    left = po.oracle_extend(0, c, fs.sequence, m, p)
    return c, m, (right, left)


# Seed 11, except where a 24-copy family under it leaves an entry of N's row or an N confusion without effect
# (three or four of 24 copies carry an N run): the next seed under which tests/test_class_table_ref.py finds nothing blind.
SEEDS = {(24, 9): 13, (24, 20): 13, (24, 40): 12, (24, 80): 12}


def seed_of(n, W):
    return SEEDS.get((n, W), 11)


@lru_cache(maxsize=None)
def family(n, W, L=96, K=70, seed=None):
    """Computed once per process; do not change it."""
    return soft_family(n, L, W, K, seed_of(n, W) if seed is None else seed)


@lru_cache(maxsize=None)
def oracle_run(name, n, W, L=96, K=70, seed=None, when_to_stop=WHEN_TO_STOP):
    """The oracle on family(n, W, ...) under a named system, both directions.  Computed once per process; do not change it."""
    fs = family(n, W, L, K, seed)
    p = system(name, W, L, when_to_stop)
    return Run(name, fs, p, *run_oracle(fs, p))


def warm(keys, threads=8):
    """oracle_run for every (system, copies, band width) of `keys`, side by side: the oracle is plain C without any state of its
    own and ctypes drops the interpreter lock around it, so the large families' expected values cost one run's time."""
    from concurrent.futures import ThreadPoolExecutor
    keys = sorted(set(keys))
    for _, n, W in keys:
        family(n, W)
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(lambda k: oracle_run(*k), keys))


def check_family(run):
    """The premises of a family under a system: a third of the bases soft-masked inside and outside the executed columns, minus-strand
    copies with soft-masked bases in executed columns, N in an executed in-bounds cell, flanks that end inside the executed columns
    (padding beside scored bases) -- and an extension that goes somewhere."""
    fs, W = run.fs, run.p.bandwidth
    seq = fs.sequence
    seen = np.zeros(len(seq), bool)
    n_cells = 0
    for d in (1, 0):
        o = run.direction(d)
        assert o.rows_executed > 40 and o.ret > 20, (run.name, d, o.rows_executed, o.ret)
        pos, inb, minus = executed_cells(fs, d, o.rows_executed, W)
        cells = seq[pos[inb]]
        lower = (cells >= 4) & (cells < 8)
        assert 0.25 < lower.mean() < 0.45, (run.name, d, lower.mean())
        assert lower[minus[inb]].sum() > 20 and lower[~minus[inb]].sum() > 20, (run.name, d)
        n_cells += int((cells == SYM_N).sum())              # (synth_family puts its N runs behind the core only: the right direction)
        for k in LOWER:
            assert (cells == k).any()
        assert (~inb).any(axis=1).sum() >= len(pos) // 4, (run.name, d)          # many flanks end inside the executed columns
        seen[pos[inb]] = True
    assert n_cells > 0, run.name
    rest = seq[~seen]
    assert 0.25 < ((rest >= 4) & (rest < 8)).mean() < 0.45
    return True


# ---- confusions: what a wrongly restated table computes, as the matrix that a correct table would need -----------------------------

def _m(matrix):
    return np.asarray(matrix, np.int32).reshape(100, 100).copy()


def _swap_cols(m, pairs):
    for a, b in pairs:
        m[:4, [a, b]] = m[:4, [b, a]]
    return m.reshape(-1)


def uncomplemented(matrix):
    """Lower case left uncomplemented on the minus strand: 4<->7, 5<->6."""
    return _swap_cols(_m(matrix), [(4, 7), (5, 6)])


def folded(matrix):
    """Lower case folded onto upper case."""
    m = _m(matrix)
    m[:4, 4:8] = m[:4, 0:4]
    return m.reshape(-1)


def a_c(matrix):
    return _swap_cols(_m(matrix), [(4, 5)])


def g_t(matrix):
    return _swap_cols(_m(matrix), [(6, 7)])


def n_as_a(matrix):
    m = _m(matrix)
    m[:4, SYM_N] = m[:4, 4]
    return m.reshape(-1)


def t_as_n(matrix):
    m = _m(matrix)
    m[:4, 7] = m[:4, SYM_N]
    return m.reshape(-1)


def n_rotated(matrix):
    """N's four candidates rotated by one."""
    m = _m(matrix)
    m[:4, SYM_N] = m[[1, 2, 3, 0], SYM_N]
    return m.reshape(-1)


def _swap_cands(matrix, a, b):
    m = _m(matrix)
    block = m[:, 4:8].copy()
    m[a, 4:8], m[b, 4:8] = block[b], block[a]
    return m.reshape(-1)


def lower_cands_03(matrix):
    return _swap_cands(matrix, 0, 3)


def lower_cands_12(matrix):
    return _swap_cands(matrix, 1, 2)


CONFUSIONS = {"lower case uncomplemented": uncomplemented, "lower case folded onto upper case": folded, "a<->c": a_c, "g<->t": g_t,
              "N read as a": n_as_a, "t read as N": t_as_n, "N's candidates rotated": n_rotated,
              "lower-case candidates 0<->3": lower_cands_03, "lower-case candidates 1<->2": lower_cands_12}
N_CONFUSIONS = ("N read as a", "N's candidates rotated")


def control(matrix):
    """4<->7, 5<->6 and N read as a, all at once: invisible where the classes 4..8 hold one constant."""
    return n_as_a(uncomplemented(matrix))


def single_entry_changes(matrix):
    """The 72 matrices that differ from `matrix` in one class-table entry by +1 or -1 -> [((class, candidate, delta), matrix)]."""
    out = []
    for c, code in enumerate(CLASS_CODES):
        for k in range(4):
            for delta in (1, -1):
                m = _m(matrix)
                m[k, code] += delta
                out.append(((c, k, delta), m.reshape(-1)))
    return out


def with_matrix(p, matrix):
    return po.Params(**{**{f: getattr(p, f) for f in p.__dataclass_fields__}, "matrix": np.ascontiguousarray(matrix, np.int32)})


def differs(run, matrix):
    """Does the oracle under `matrix` give another result than `run` -- ret, rows, consensus, lengths or scores -- in at least
    one direction?  (Right first; the left direction is run only if the right one shows nothing.)"""
    p = with_matrix(run.p, matrix)
    c, m = run.fs.cores.copy(), po.new_master(p.L)
    for d in (1, 0):
        o, want = po.oracle_extend(d, c, run.fs.sequence, m, p), run.direction(d)
        if (o.ret, o.rows_executed, o.limit_warning) != (want.ret, want.rows_executed, want.limit_warning):
            return True
        if d == 1 and (not np.array_equal(c.right_len, run.cores.right_len) or not np.array_equal(m[p.L:], run.master[p.L:])):
            return True
    return not (np.array_equal(m, run.master) and np.array_equal(c.left_len, run.cores.left_len)
                and np.array_equal(c.right_len, run.cores.right_len) and np.array_equal(c.score, run.cores.score))


# ---- the (system, family) pairs of tests/test_gpu_class_table.py -----------------------------------------------------------------------

# (copies, band width); L = 96 and K = 70, seed_of(copies, band width)
GPU_FAMILIES = {
    "streaming": [(24, 14), (288, 14), (24, 9), (288, 9)],
    "family kernel": [(24, 14), (192, 14), (24, 40), (192, 40)],
    "cell-parallel, one workgroup": [(24, 14), (24, 20), (24, 40), (24, 80)] + [(24 * 16 // k, w) for k in (2, 4, 8) for w in (14, 40, 80)],
    "int32 rows": [(2016, 14), (2016, 80)],
    "packed rows": [(4032, 14), (4032, 20), (4032, 40), (4032, 80)],
    "cell-parallel, device-wide": [(720, 14), (720, 40)],
    "replays": [(130, 14), (130, 5)],
}
ALL_GPU_FAMILIES = sorted({f for v in GPU_FAMILIES.values() for f in v})
SMALLEST_PER_WIDTH = sorted({w: min(n for n, ww in ALL_GPU_FAMILIES if ww == w) for _, w in ALL_GPU_FAMILIES}.items())


# ---- the two families of the GPU module that are not soft_family: the LEAN band's and the packed library form's ----------------------

LEAN_W, LEAN_GAP = 14, 250
LEAN_L = 300 + LEAN_GAP + 300 + 150


@lru_cache(maxsize=None)
def lean_family():
    """test_gpu_persistent's two-copy family -- 700 one-sided copies on the plus strand: 300 aligned columns, a random gap in
    which every flank sinks to its cap (the LEAN band's territory), a second shared copy -- with the whole gap soft-masked, every
    other base of the second copy soft-masked (all of them, and the lower-case matches of `distinct` do not carry a flank back up
    from its cap), and runs of 1 to 11 N in both copies of a tenth of the flanks.  Computed once per process; do not change it."""
    from test_gpu_persistent import _two_copy_family
    fs = _two_copy_family(700, LEAN_L, LEAN_W, LEAN_GAP, seed=4100 + LEAN_W)
    n = fs.cores.n
    seq = fs.sequence.reshape(n, -1).copy()
    rng = np.random.default_rng(77)
    first, second = 12, 12 + 300 + LEAN_GAP                 # (a core of twelve bases, then the first copy)
    gap = seq[:, first + 300:second]
    gap[gap < 4] += 4
    copy2 = seq[:, second:second + 300]
    copy2[(rng.random(copy2.shape) < 0.5) & (copy2 < 4)] += 4
    for i in np.flatnonzero(rng.random(n) < 0.1):
        for lo, hi in ((first, first + 288), (second, second + 290)):
            a = int(rng.integers(lo, hi))
            seq[i, a:a + int(rng.integers(1, 12))] = SYM_N
    fs.sequence = np.ascontiguousarray(seq.reshape(-1))
    return fs


@lru_cache(maxsize=None)
def lean_run():
    """The oracle on lean_family() under `distinct` with the stop rule out of the way (when_to_stop = L), both directions (the
    left one has no flank).  Computed once per process; do not change it."""
    fs, p = lean_family(), system("distinct", LEAN_W, LEAN_L, when_to_stop=LEAN_L)
    return Run("distinct", fs, p, *run_oracle(fs, p))


def check_lean_family(run):
    """Its premises: plus strand only and one-sided (said here, so that nobody takes it for more), soft-masked bases of all four
    kinds and N in executed in-bounds cells, every row executed, and the soft-masked second copy found again."""
    fs, o = run.fs, run.direction(1)
    assert not fs.cores.orient.any() and not fs.cores.left_ext.any() and fs.cores.right_ext.all()
    assert o.rows_executed == LEAN_L and o.ret > 300 + LEAN_GAP + 200, (o.rows_executed, o.ret)
    pos, inb, _ = executed_cells(fs, 1, o.rows_executed, LEAN_W)
    cells = fs.sequence[pos[inb]]
    assert all((cells == k).sum() > 1000 for k in LOWER) and (cells == SYM_N).sum() > 300
    assert run.direction(0).ret == 0


LOOP_WHEN_TO_STOP = 25


def n_runs_cross_borders(tables):
    """(an N run of the packed tables holds a window's first base behind its own first, one is longer than a word of eight bases
    and so crosses a word border wherever the window begins)."""
    s = np.asarray(tables["n_start"], np.int64)
    e = s + np.asarray(tables["n_len"], np.int64)
    starts = np.asarray(tables["win_start"], np.int64)[1:-1]
    return bool(((starts[None, :] > s[:, None]) & (starts[None, :] < e[:, None])).any()), bool((e - s > 8).any())


def windows_inside_n_runs(c):
    """The packed tables of a case of tests/window_cases.py with its window starts inside flanks and one more window begun in the
    middle of every N run of the library: every such run then crosses a window's first base."""
    import window_cases as wc
    import window_ref as wr
    lib = wr.fold(c.lib)
    isn = np.concatenate(([False], lib == SYM_N, [False]))
    first, behind = np.flatnonzero(isn[1:] & ~isn[:-1]), np.flatnonzero(~isn[1:] & isn[:-1])
    mids = [int((a + b) // 2) for a, b in zip(first, behind) if b - a >= 2]
    assert mids
    return wc.packed_tables(c.lib, [int(x) for x in c.tables["inside"]["win_start"][:-1]] + mids)


def loop_run(name, c):
    """The oracle on a case of window_cases.loop_cases -- an adversarial set, ONE direction -- on the FOLDED library (the packed
    form carries N but no case) under a named system -> (folded library, Params, cores after the direction, master, Result)."""
    import window_ref as wr
    lib = np.ascontiguousarray(wr.fold(c.lib))
    p = system(name, c.W, c.L, when_to_stop=LOOP_WHEN_TO_STOP)
    cores, m = c.extra["fs"].cores.copy(), po.new_master(p.L)
    o = po.oracle_extend(c.extra["direction"], cores, lib, m, p)
    return lib, p, cores, m, o


def loop_differs(name, c, matrix):
    """differs() for one direction of a loop case."""
    lib, p, cores, m, o = loop_run(name, c)
    q = with_matrix(p, matrix)
    c2, m2 = c.extra["fs"].cores.copy(), po.new_master(p.L)
    o2 = po.oracle_extend(c.extra["direction"], c2, lib, m2, q)
    return (o2.ret, o2.rows_executed, o2.limit_warning) != (o.ret, o.rows_executed, o.limit_warning) or not (
        np.array_equal(m, m2) and np.array_equal(cores.left_len, c2.left_len) and np.array_equal(cores.right_len, c2.right_len)
        and np.array_equal(cores.score, c2.score))


# ---- the cases that pin the oracle to the reference on these systems (tests/test_class_table_ref.py, tests/golden) -----------------

REF_L, REF_WIDTHS, REF_SEEDS = 90, (0, 1, 7, 14, 40), tuple(range(6))


@lru_cache(maxsize=None)
def ref_family(kind, seed, W):
    """Computed once per process; do not change it."""
    from repeatafterme_amd.synth import synth_adversarial
    if kind == "soft":
        return soft_family(30, REF_L, W, 60, 200 + seed)
    return synth_adversarial(300 + seed, L=REF_L, W=W, K=60, lowercase=True)


def ref_cases():
    """[(kind, seed, W, system)]: all five systems at five band widths on six soft-masked families and six adversarial sets."""
    return [(kind, seed, W, name) for kind in ("soft", "adversarial") for seed in REF_SEEDS for W in REF_WIDTHS for name in SYSTEMS]


def extreme_systems():
    """[(tag, matrix, gapopen, gapextn)]: `distinct` with exactly one entry set to 127, 128, -128 or -129, in turn at tab[6][2] (a
    lower-case class), tab[8][1] (N) and tab[1][1]: P, mn, mx and the int8 test of every gate must range over all nine classes."""
    out = []
    base, go, ge = matrix_of("distinct")
    for c, k in ((6, 2), (8, 1), (1, 1)):
        for v in (127, 128, -128, -129):
            m = _m(base)
            m[k, CLASS_CODES[c]] = v
            out.append((f"tab[{c}][{k}] = {v}", m.reshape(-1), go, ge))
    return out
