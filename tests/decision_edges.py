"""The two sharp edges of the extension loop's decisions (tests only; no kernel code), and families planted to sit on them.

The vote (ram_extend.c:1081-1085) compares the four candidate sums with a strict `>` from 0 upward: a tie at the top goes to the
lowest base.  The stop rule (:1194-1196) keeps a row when curr >= max_ext + dist * minimprovement: equality is a new maximum.
Random families of 64 copies or more never put a kernel on either edge (tests/test_decision_edges_ref.py counts it), so the
families here are planted: m copies share one left template, one core and one right template and differ only at chosen "tie
columns" of both flanks, where the copies are split evenly over a set of bases.  A split that the scoring matrix treats
symmetrically -- any pair under repeatscout, C/G and A/T under the named matrices, an all-N column under all of them -- ties the
top sums exactly; a minimprovement equal to the step of the top sum puts curr on the bar row after row.

tests/wide_sums.py carries both edges to any family size: every copy repeated r times with r times the minimprovement multiplies
every sum and the bar by r, so ties and equalities stay exact.  `replicate` (np.tile) interleaves the tie groups; `repeat_blocks`
(np.repeat) keeps all copies of one tie group next to each other, the group with the HIGHER base of every two-way tie first -- a
workgroup that holds copies of that group alone sees no tie and guesses the loser, while a workgroup of the other group guesses
the winner: one column, both verdicts.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import FLANK_DTYPE, CoreSet, FlankSet, SYM_N

from wide_sums import INT32_MAX, pk_first_row, replicate, vote       # noqa: F401  (replicate, pk_first_row: re-exported)

BASES = {"A": 0, "C": 1, "G": 2, "T": 3, "N": SYM_N}


def _revcomp(row):
    r = row[::-1].copy()
    acgt = r < 4
    r[acgt] = 3 - r[acgt]
    return r


def planted_family(m, L, W, ties, core_len=10, both_sides=True, minus_stride=0, seed=1, pad=20, cores_only=False):
    """m copies of ONE window -- left template, core, right template, all random from `seed` -- that differ only at the tie columns:
    ties = {column: "CG"} gives copy i the base sorted("CG", descending)[i * 2 // m] at that column of both flanks (columns count
    outward from the core: row r of a direction reads column r where no gap was taken); "N" alone makes the column N in every
    copy.  minus_stride = s: every s-th copy (s - 1, 2 s - 1, ...) lies on the minus strand.  -> FlankSet (cores_only: CoreSet)."""
    rng = np.random.default_rng(seed)
    F = L + W + pad
    FL = F if both_sides else 0
    right = rng.integers(0, 4, size=F, dtype=np.int8)
    left = rng.integers(0, 4, size=F, dtype=np.int8)                 # outward from the core
    core = rng.integers(0, 4, size=core_len, dtype=np.int8)
    win = FL + core_len + F
    seq = np.empty((m, win), np.int8)
    seq[:, FL:FL + core_len] = core
    seq[:, FL + core_len:] = right
    if both_sides:
        seq[:, :FL] = left[::-1]
    for col, bases in ties.items():
        assert 0 <= col < F and m % len(bases) == 0, (col, bases, m)
        codes = sorted((BASES[b] for b in bases), reverse=True)
        per_copy = np.array([codes[i * len(codes) // m] for i in range(m)], np.int8)
        seq[:, FL + core_len + col] = per_copy
        if both_sides:
            seq[:, FL - 1 - col] = per_copy
    minus = np.zeros(m, bool)
    if minus_stride:
        minus[minus_stride - 1::minus_stride] = True
        for i in np.flatnonzero(minus):
            seq[i] = _revcomp(seq[i])
    off = np.arange(m, dtype=np.int64) * win
    lo_core = np.where(minus, off + F, off + FL)                     # (as repeatafterme_amd.synth.synth_family lays a window out)
    hi_core = lo_core + core_len - 1
    cores = CoreSet(left_pos=np.where(minus, hi_core, lo_core), right_pos=np.where(minus, lo_core, hi_core), lower=off, upper=off + win - 1,
                    orient=minus.astype(np.int8), left_ext=np.full(m, 1 if both_sides else 0, np.int8), right_ext=np.ones(m, np.int8))
    if cores_only:
        return cores
    return FlankSet(sequence=seq.reshape(-1), boundaries=np.concatenate((off[1:], [m * win], [0])).astype(np.uint64), cores=cores)


def repeat_blocks(cores, r):
    """The family of `cores` with every core repeated r times IN PLACE: copy i of the result is copy i // r of `cores`, so all the
    copies of one tie group stay next to each other (replicate interleaves them: copy i is copy i % n)."""
    return CoreSet(**{k: np.repeat(getattr(cores, k), r) for k in cores.__dataclass_fields__})


ORDERS = {"tile": (replicate, np.tile), "blocks": (repeat_blocks, np.repeat)}      # order -> (the family, its per-copy results)


def assert_device_order(direction, small, big, r, order, W, L):
    """The flanks the device is handed for `big` are those of `small` in the order that was built: flank i of the big family is
    flank i % n (tile) or i // r (blocks) of the small one, field by field."""
    from repeatafterme_amd.device import resolve_flanks
    (fs_, ns), idx_s = resolve_flanks(direction, small, W, L)
    (fb, nb), idx_b = resolve_flanks(direction, big, W, L)
    assert ns == small.n and nb == r * ns and np.array_equal(idx_b, np.arange(nb)), (ns, nb)
    src = np.arange(nb) % ns if order == "tile" else np.arange(nb) // r
    fb, fs_ = np.frombuffer(fb, FLANK_DTYPE)[:nb], np.frombuffer(fs_, FLANK_DTYPE)[:ns]
    for k in ("start", "t_lo", "t_hi", "step", "compl_"):
        assert np.array_equal(fb[k], fs_[k][src]), (order, k)


def vote_variant(sums, q, stop, ties="lowest", equal="new_max"):
    """wide_sums.vote with either rule flipped: ties="highest" gives a tie at the top to the highest base (a `>=` in the vote),
    equal="not" keeps a row only when curr > bar.  With the defaults it IS vote (asserted by the CPU tests)."""
    assert ties in ("lowest", "highest") and equal in ("new_max", "not")
    L = len(sums)
    max_ext, max_row, cons = 0, -1, []
    for r in range(L):
        curr, besta = 0, 0
        for a in range(4):
            s = int(sums[r][a])
            if s > curr or (ties == "highest" and s == curr and s > 0):
                curr, besta = s, a
        cons.append(besta)
        bar = max_ext + abs(max_row - r) * int(q)
        if curr > bar or (equal == "new_max" and curr == bar):
            max_row, max_ext = r, curr
        if abs(r - max_row) >= stop:
            break
    else:
        r = L
    rows = min(r + 1, L)
    return max_row + 1, rows, int(r == L - 1), np.array(cons[:rows], np.int8)


def top_ties(S, rows):
    """Per executed row with two or more equal sums at a POSITIVE top: (row, the tied bases ascending)."""
    out = []
    for r in range(rows):
        top = int(S[r].max())
        tied = [a for a in range(4) if int(S[r][a]) == top]
        if top > 0 and len(tied) >= 2:
            out.append((r, tied))
    return out


def equal_rows(S, rows, q):
    """The executed rows in which curr == bar, the loop's own state followed with the reference's rule."""
    max_ext, max_row, out = 0, -1, []
    for r in range(rows):
        curr = max(0, int(S[r].max()))
        bar = max_ext + abs(max_row - r) * int(q)
        if curr == bar:
            out.append(r)
        if curr >= bar:
            max_row, max_ext = r, curr
    return out


# ---- the named cases -----------------------------------------------------------------------------------------------------------

ISSUE_TIES = {5: "AC", 17: "CG", 30: "GT", 41: "CT", 55: "ACG", 63: "ACGT", 77: "N", 90: "AT"}
M = 24                      # copies of every small family: divisible by 2, 3 and 4, and by the minus-strand stride


@dataclass(frozen=True)
class Case:
    matrix: str
    W: int
    L: int
    ties: tuple             # ((column, bases), ...)
    stop: int = 30          # when_to_stop
    q: object = None        # minimprovement of the small family (None: the matrix' default)
    core_len: int = 10
    minus_stride: int = 3
    cap: object = None      # cappenalty (None: the matrix' default)
    go: object = None       # gapopen (None: the matrix' own)
    both_sides: bool = True
    tie_case: bool = True   # flipping the vote's tie rule must change the consensus
    equal_case: bool = False        # ... and flipping the stop rule's equality (ret, rows)
    r_max: int = 200        # the largest repetition any test uses with this case


def _t(d):
    return tuple(sorted(d.items()))


PLACED = {0: "CG", 63: "AT", 64: "CG", 100: "CG", 101: "N", 107: "ACGT", 159: "AT"}
HANDOVER_ROW = 4            # pk_first_row of the one-sided families with cores of ten bases at W = 14 (asserted by the CPU tests)

CASES = {
    # every pair ties under repeatscout; the named matrices tie where the split is symmetric under complement
    "rs14": Case("repeatscout", 14, 120, _t(ISSUE_TIES)),
    "m14": Case("14p43g", 14, 120, _t(ISSUE_TIES)),
    "m40": Case("18p43g", 40, 120, _t(ISSUE_TIES)),
    "m80": Case("20p43g", 80, 120, _t(ISSUE_TIES)),
    "rs9": Case("repeatscout", 9, 120, _t(ISSUE_TIES)),                       # no kernel is specialised for this band width
    "rs14_gap": Case("repeatscout", 14, 120, _t(ISSUE_TIES), go=2),          # a positive gap-open penalty: per-column launches
    # placement: row 0; rows 63 and 64 (the piece border of RAMX_PK_SEGMENT=64, and two tie columns in adjacent rows: a rollback
    # lands on another tie); 100 and 101 (adjacent again, the second a four-way tie); a tie inside a block of eight columns
    # behind a checkpoint (row 107 = 104 + 3); the last executed row (L - 1: the limit is reached)
    "place14": Case("14p43g", 14, 160, _t(PLACED)),
    "place40": Case("14p43g", 40, 160, _t(PLACED)),
    # cores of ten bases and no left flank: the int32 kernel runs the rows before pk_first_row, where the low end of the band
    # still lies before the window; ties in the row where the packed rows take over and in the row before it
    "handover14": Case("repeatscout", 14, 120, _t({HANDOVER_ROW - 1: "CG", HANDOVER_ROW: "AC", 40: "ACG", 77: "N"}), both_sides=False),
    # equality: a minimprovement equal to the step of the top sum (24 copies x match 1), so that every row before the first tie
    # column has curr == bar; the tie columns end it, and the stop row (29) is a tie column itself
    "eq_rs": Case("repeatscout", 14, 60, _t({20: "AC", 21: "CG", 22: "ACG", 25: "N", 29: "CG"}), stop=10, q=24, equal_case=True),
    "eq_rs40": Case("repeatscout", 40, 60, _t({20: "AC", 21: "CG", 22: "ACG", 25: "N", 29: "CG"}), stop=10, q=24, equal_case=True),
    # 14p43g: 24 copies x 9 for a matching A or T; the rows whose consensus is A or T behind a kept row sit on the bar, the tie
    # column (28) follows such a row, so a strict rule returns at least one row less
    "eq_m14": Case("14p43g", 14, 60, _t({28: "CG"}), stop=10, q=216, equal_case=True, tie_case=False),
    # a plateau: cappenalty 0 makes every copy contribute its record, so an all-N stretch holds the top sum constant and
    # curr == max_ext row after row (minimprovement 0) -- and every candidate sums to the same: a run of four-way ties at a
    # positive sum, which the lowest base wins to the end (the consensus it writes matches nothing, so no copy's record moves)
    "plateau": Case("14p43g", 14, 100, _t({**{c: "N" for c in range(30, 50)}, 10: "CG"}), stop=12, q=0, cap=0, equal_case=True),
}


def case_params(case, r=1):
    kw = dict(bandwidth=case.W, L=case.L, when_to_stop=case.stop)
    if case.cap is not None:
        kw["cappenalty"] = case.cap
    p = po.Params.named(case.matrix, **kw)
    if case.q is not None:
        p.minimprovement = case.q
    if case.go is not None:
        p.gapopen = case.go
    p.minimprovement *= r
    return p


def case_family(case):
    return planted_family(M, case.L, case.W, dict(case.ties), core_len=case.core_len, both_sides=case.both_sides,
                          minus_stride=case.minus_stride)


@dataclass
class EdgeRun:
    name: str
    case: Case
    fs: object              # the FlankSet of the 24-copy family
    cores: object           # its cores after both directions (right, then left)
    master: np.ndarray
    res: tuple              # the oracle's traced results (right, left)

    @property
    def directions(self):
        return (1, 0) if self.case.both_sides else (1,)

    def direction(self, d):
        return self.res[0 if d else 1]


@lru_cache(maxsize=None)
def small_run(name):
    """The oracle on the 24-copy family of a case, both directions, traced.  Computed once per process; do not change it."""
    case = CASES[name]
    fs = case_family(case)
    p = case_params(case)
    c, m = fs.cores.copy(), po.new_master(case.L)
    right = po.oracle_extend(1, c, fs.sequence, m, p, trace=True)
    left = po.oracle_extend(0, c, fs.sequence, m, p, trace=True) if case.both_sides else None
    return EdgeRun(name, case, fs, c, m, (right, left))


def check_premises(run, d):
    """The conditions under which a case tells the reference's rules from their neighbours; asserted wherever a case is used.
    -> (the tied rows, the rows with curr == bar)."""
    case, o = run.case, run.direction(d)
    S, rows = o.col_sums, o.rows_executed
    q = case_params(case).minimprovement
    got = vote(S, q, case.stop)
    assert got[:3] == (o.ret, rows, o.limit_warning) and np.array_equal(got[3], o.col_base[:rows]), (run.name, d)
    same = vote_variant(S, q, case.stop)
    assert same[:3] == got[:3] and np.array_equal(same[3], got[3])
    tied = top_ties(S, rows)
    eq = equal_rows(S, rows, q)
    if case.tie_case:
        assert len(tied) >= 4, (run.name, d, tied)
        assert any(o.col_base[r] != 0 for r, _ in tied), (run.name, d, "every tie is won by base 0")
        assert any(len(t) >= 3 for _, t in tied), (run.name, d, "no tie of three or more bases")
        assert all(o.col_base[r] == t[0] for r, t in tied)                         # the lowest base did win
        flipped = vote_variant(S, q, case.stop, ties="highest")
        assert not np.array_equal(flipped[3], o.col_base[:rows]), (run.name, d, "the tie rule does not show in the consensus")
    if case.equal_case:
        assert len(eq) >= 10, (run.name, d, eq)
        strict = vote_variant(S, q, case.stop, equal="not")
        assert strict[:2] != (o.ret, rows), (run.name, d, "the equality does not show in (ret, rows)")
    assert 0 <= S.min() and int(S.max()) * case.r_max <= INT32_MAX and case.L * case.r_max * max(q, 1) <= INT32_MAX
    return tied, eq


def copy_contributions(run, d):
    """What every copy adds to the four sums of every executed row along the oracle's own consensus: the loop of
    oracle/ramx_oracle.c restated around its row function (ram_extend.c:1042-1062: max(best, 0), or the copy's record plus the cap
    penalty where that is larger) -> int64 [rows][4][n].  Summed over the copies it must give back the traced sums (asserted)."""
    case, o, cores, seq = run.case, run.direction(d), run.fs.cores, run.fs.sequence
    p = case_params(case)
    n, W, rows = cores.n, case.W, o.rows_executed
    score = np.zeros((2, n, 2 * W + 1, 2), np.int32)
    for off in range(-W, W + 1):
        score[1, :, off + W, :] = 0 if off == 0 else abs(off) * p.gapextn + p.gapopen
    high = np.zeros(n, np.int64)
    out = np.zeros((rows, 4, n), np.int64)

    def row(r, k, a):
        return po.oracle_nw_row(d, r, k, n, a, int(cores.left_pos[k]), int(cores.right_pos[k]), int(cores.orient[k]), score,
                                int(cores.lower[k]), int(cores.upper[k]), seq, p.matrix, p.gapopen, p.gapextn, W)[0]
    for r in range(rows):
        for a in range(4):
            for k in range(n):
                best = max(row(r, k, a), 0)
                out[r, a, k] = best if best >= high[k] + p.cappenalty else high[k] + p.cappenalty
        for k in range(n):
            high[k] = max(high[k], row(r, k, int(o.col_base[r])))
    assert np.array_equal(out.sum(axis=2), o.col_sums[:rows]), (run.name, d)
    return out


TWO_RANK_CASES = ("m14", "eq_rs", "rs14")


def check_rank_halves(name, world=2):
    """The premise of the two-rank cases: with the copies in blocks and the contiguous shards of repeatafterme_amd.sharded.partition,
    every rank's own totals -- its copies' contributions along the whole family's consensus -- have ONE base at the top in every
    row in which the whole family ties between two bases, rank 0's the loser and the last rank's the winner.  -> those rows."""
    from repeatafterme_amd.sharded import partition
    run = small_run(name)
    seen = {}
    for d in run.directions:
        o = run.direction(d)
        per_copy = copy_contributions(run, d)
        two_way = [(r, t) for r, t in top_ties(o.col_sums, o.rows_executed) if len(t) == 2]
        assert two_way, (name, d)
        parts = [per_copy[:, :, partition(M, world, rank)].sum(axis=2) for rank in range(world)]
        assert np.array_equal(sum(parts), o.col_sums[:o.rows_executed])
        for r, (lo, hi) in two_way:
            tops = [[a for a in range(4) if part[r][a] == part[r].max()] for part in parts]
            assert tops[0] == [hi] and tops[-1] == [lo] and all(len(t) == 1 for t in tops), (name, d, r, tops)
            assert o.col_base[r] == lo
        seen[d] = [r for r, _ in two_way]
    return seen
