"""The premises of tests/test_gpu_decision_edges.py, pinned on the oracle (CPU only).  tests/decision_edges.py plants families of
24 copies on the two sharp edges of the loop's decisions -- a tie at the top of the vote goes to the lowest base, curr == bar is a
new maximum -- and carries them to any size by repetition.  Here: every named case does sit on its edge in both directions and
would tell either rule from its neighbour; the repetition identity holds on the oracle in both orders of the copies; the tie
columns lie in the rows they were placed for; every case is on the right side of the route gates; and the random families of the
large-set tests have no tie at the top at all, which is why the planted ones exist."""
import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.synth import synth_family

import decision_edges as de
import score_gates as sg
from decision_edges import CASES, M, ORDERS, check_premises, small_run, vote, vote_variant


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_meet_the_premises(name):
    """Both directions of every case: the restated vote is the oracle's; a tie case has at least four executed rows with an exact
    tie at a positive top, one of them won by a base other than A and one among three or more bases, and giving ties to the
    highest base changes the consensus; an equality case has at least ten rows with curr == bar, and keeping a row only above
    the bar changes (ret, rows); every sum stays within int32 at the largest repetition."""
    run = small_run(name)
    for d in run.directions:
        tied, eq = check_premises(run, d)
        assert run.direction(d).rows_executed > 0 and (tied or eq)


def test_tie_columns_lie_where_they_were_placed():
    for name in ("place14", "place40"):
        run = small_run(name)
        for d in run.directions:
            o = run.direction(d)
            rows = [r for r, _ in de.top_ties(o.col_sums, o.rows_executed)]
            assert rows == sorted(de.PLACED), (name, d, rows)                 # row 0, 63 | 64, 100 and 101 adjacent, 107 = 104 + 3
            assert o.rows_executed == run.case.L and rows[-1] == o.rows_executed - 1         # ... and the last executed row
            assert len(dict(de.top_ties(o.col_sums, o.rows_executed))[101]) == 4           # the rollback of row 100 lands on a four-way tie
    run = small_run("handover14")                                            # the row where the packed rows take over, and the one before
    assert run.directions == (1,) and de.pk_first_row(1, run.fs.cores, run.case.W, run.case.L) == de.HANDOVER_ROW > 0
    o = run.direction(1)
    assert {de.HANDOVER_ROW - 1, de.HANDOVER_ROW} <= {r for r, _ in de.top_ties(o.col_sums, o.rows_executed)}
    run = small_run("eq_rs")                                                 # the stop row is a tie
    for d in run.directions:
        o = run.direction(d)
        assert (o.ret, o.rows_executed, o.limit_warning) == (20, 30, 0)
        assert de.equal_rows(o.col_sums, 30, 24) == list(range(20))
        assert de.top_ties(o.col_sums, 30)[-1] == (29, [1, 2]) and o.col_base[29] == 1
        assert vote_variant(o.col_sums, 24, 10, equal="not")[:2] == (0, 10)
        assert vote(o.col_sums, 25, 10)[:2] == (0, 10)                        # one more and nothing is kept
    run = small_run("plateau")                                               # curr == max_ext > 0 from the stretch to the last row
    for d in run.directions:
        o = run.direction(d)
        assert de.equal_rows(o.col_sums, o.rows_executed, 0)[:20] == list(range(30, 50)) and o.col_sums[30].max() > 0
        assert (o.ret, o.rows_executed) == (100, 100) and vote_variant(o.col_sums, 0, run.case.stop, equal="not")[:2] == (30, 42)


def test_vote_variant_is_vote_with_one_rule_flipped():
    S = np.array([[0, 7, 7, 3], [5, 5, 5, 5], [0, 0, 0, 0], [9, 2, 9, 1], [9, 2, 9, 1], [9, 2, 9, 1]], np.int64)
    assert vote_variant(S, 0, 3)[:3] == vote(S, 0, 3)[:3] and np.array_equal(vote_variant(S, 0, 3)[3], vote(S, 0, 3)[3])
    assert list(vote(S, 0, 10)[3]) == [1, 0, 0, 0, 0, 0]
    assert list(vote_variant(S, 0, 10, ties="highest")[3]) == [2, 3, 0, 2, 2, 2]             # (a row of zeros stays with base 0)
    assert vote(S, 0, 3)[:2] == (6, 6)                                       # 9 >= 9: rows 4 and 5 are kept like row 3
    assert vote_variant(S, 0, 3, equal="not")[:2] == (4, 6)                  # ... and are not above it
    T = np.array([[4, 0, 0, 0], [6, 0, 0, 0], [7, 0, 0, 0]], np.int64)
    assert vote(T, 2, 10)[0] == 2 and vote_variant(T, 2, 10, equal="not")[0] == 1            # 6 == 4 + 1 * 2 in row 1


def test_planted_copies_differ_at_the_tie_columns_only():
    case = CASES["rs14"]
    fs = de.planted_family(M, case.L, case.W, dict(case.ties), minus_stride=0)
    win = len(fs.sequence) // M
    rows = fs.sequence.reshape(M, win)
    F = case.L + case.W + 20
    differ = np.flatnonzero((rows != rows[0]).any(axis=0))
    want = sorted([F + case.core_len + c for c, b in case.ties if len(b) > 1] + [F - 1 - c for c, b in case.ties if len(b) > 1])
    assert list(differ) == want
    assert (rows[:, F + case.core_len + 77] == 99).all() and (rows[:, F - 1 - 77] == 99).all()
    assert list(rows[:, F + case.core_len + 17]) == [2] * 12 + [1] * 12       # the higher base of a two-way tie comes first
    assert list(rows[:, F + case.core_len + 63]) == [3] * 6 + [2] * 6 + [1] * 6 + [0] * 6
    # every third copy on the minus strand: the same family read through the complement -- the oracle's run is identical
    p = de.case_params(case)
    c, m = fs.cores.copy(), po.new_master(case.L)
    run = small_run("rs14")
    for d in (1, 0):
        o = po.oracle_extend(d, c, fs.sequence, m, p, trace=True)
        assert np.array_equal(o.col_sums, run.direction(d).col_sums) and o.ret == run.direction(d).ret
    assert np.array_equal(m, run.master) and fs.cores.orient.sum() == 0 and run.fs.cores.orient.sum() == M // 3


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("r", [2, 3])
def test_replication_identity_on_the_oracle_in_both_orders(r, order):
    """The family repeated r times with r times the minimprovement goes where the small one goes -- copies interleaved (tile) or
    kept in blocks (np.repeat): same ret, rows and consensus, sums r * S, the per-copy results tiled or repeated; and the device
    is handed the flanks in the order that was built."""
    big_of, results_of = ORDERS[order]
    for name in sorted(CASES):
        run = small_run(name)
        case = run.case
        big = big_of(run.fs.cores, r)
        assert big.n == r * M
        c, m = big.copy(), po.new_master(case.L)
        for d in run.directions:
            de.assert_device_order(d, run.fs.cores, big, r, order, case.W, case.L)
            o, b = run.direction(d), po.oracle_extend(d, c, run.fs.sequence, m, de.case_params(case, r), trace=True)
            assert (b.ret, b.rows_executed, b.limit_warning) == (o.ret, o.rows_executed, o.limit_warning), (name, d)
            assert np.array_equal(b.col_sums[:o.rows_executed], r * o.col_sums[:o.rows_executed]), (name, d)
        assert np.array_equal(m, run.master), name
        for k in ("left_len", "right_len", "score"):
            assert np.array_equal(getattr(c, k), results_of(getattr(run.cores, k), r)), (name, k)


def test_block_order_puts_the_higher_base_of_every_two_way_tie_first():
    """The built families themselves, read back through each copy's own strand: in the block order the first half of the copies
    carries the higher base at every two-way tie column of both flanks and the second half the lower one; tiled, every stretch
    of 24 copies holds both."""
    r = 3
    for name, case in CASES.items():
        run = small_run(name)
        seq, small = run.fs.sequence, run.fs.cores

        def base_at(cores, i, col, right):
            minus = bool(cores.orient[i])
            if right:
                b = seq[cores.right_pos[i] - 1 - col] if minus else seq[cores.right_pos[i] + 1 + col]
            else:
                b = seq[cores.left_pos[i] + 1 + col] if minus else seq[cores.left_pos[i] - 1 - col]
            return 3 - int(b) if minus and b < 4 else int(b)
        blocks, tiled = de.repeat_blocks(small, r), de.replicate(small, r)
        two_way = [(col, sorted(de.BASES[b] for b in bases)) for col, bases in case.ties if len(bases) == 2]
        assert two_way, name
        for col, (lo, hi) in two_way:
            for right in (True, False) if case.both_sides else (True,):
                got = [base_at(blocks, i, col, right) for i in range(r * M)]
                assert got == [hi] * (r * M // 2) + [lo] * (r * M // 2), (name, col, right)
                got = [base_at(tiled, i, col, right) for i in range(r * M)]
                assert got == ([hi] * (M // 2) + [lo] * (M // 2)) * r, (name, col, right)


@pytest.mark.parametrize("name", de.TWO_RANK_CASES)
def test_two_rank_halves_do_not_tie_alone(name):
    """The two-rank cases of the GPU file: each contiguous half's own totals along the whole family's consensus have one base at
    the top where the whole family ties between two -- rank 0's the loser, rank 1's the winner -- so the tie exists only in the
    exchanged totals.  (The per-copy contributions come from a restatement of the loop around the oracle's row function; summed
    over all copies they reproduce the oracle's traced sums.)"""
    seen = de.check_rank_halves(name, 2)
    assert all(len(rows) >= 3 for rows in seen.values()), seen


def test_cases_are_on_the_right_side_of_the_route_gates():
    """What each route of the GPU file needs in order to run (tests/score_gates.py)."""
    for name, case in CASES.items():
        p = de.case_params(case)
        if case.go is not None and case.go > 0:
            assert not sg.go_ge_ok(p.gapopen, p.gapextn)                     # per-column launches, whatever the switches say
            continue
        assert sg.go_ge_ok(p.gapopen, p.gapextn)
        if case.W in sg.PK_WIDTHS:
            assert sg.pk_plan(case.W, p.gapopen, p.gapextn, p.matrix).admitted, name
            assert sg.cp_value_range_ok(case.W, case.L, p.gapopen, p.gapextn, p.matrix), name
    assert CASES["rs9"].W not in sg.PK_WIDTHS
    assert max(case.L for case in CASES.values()) <= 200
    assert all(case.r_max >= 168 for case in CASES.values())                 # the largest repetition of the GPU file


@pytest.mark.parametrize("n", [64, 1000, 5000])
def test_random_families_of_the_large_set_tests_never_tie_at_the_top(n):
    """The family of tests/test_gpu_cp.py's device-wide cases, on the oracle: not one row of the 100 aligned columns of either
    direction has two equal sums at the top, and with 1,000 or 5,000 copies no executed row at all, so no large-set route has ever
    been handed a tie by them.  (64 copies do tie once, in row 121 of the left direction: 21 rows behind the last aligned column,
    where most copies contribute their capped record whatever the candidate is.)"""
    fs = synth_family(n, 150, 40, K=100, seed=50, both_sides=True, minus_frac=0.3, n_run_frac=0.1)
    p = po.Params.named("14p43g", bandwidth=40, L=150, when_to_stop=30)
    c, m = fs.cores.copy(), po.new_master(p.L)
    seen = []
    for d in (1, 0):
        o = po.oracle_extend(d, c, fs.sequence, m, p, trace=True)
        assert (o.ret, o.rows_executed) == (100, 130)
        tied = de.top_ties(o.col_sums, o.rows_executed)
        assert all(r >= o.ret + 20 for r, _ in tied), (d, tied)
        seen += [(d, r) for r, _ in tied]
    assert seen == ([(0, 121)] if n == 64 else [])
