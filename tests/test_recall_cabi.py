"""ramx_recall_consensus (host C of libramx.so) against the restatement of tests/pileup_ref.py: random pileups and the edges of
every rule.  No GPU: the function is a pass over the columns."""
import numpy as np

from repeatafterme_amd.datamodel import PILEUP_DTYPE, PILEUP_INS

import pileup_ref as pr


def c_recall(cons, cols, L):
    from repeatafterme_amd.device import recall_consensus
    return recall_consensus(cons, cols, L)


def col(cover=10, match=(0, 0, 0, 0, 0), dele=0, ins=()):
    c = np.zeros(1, PILEUP_DTYPE)
    c["cover"], c["match"], c["del"] = cover, match, dele
    for k, s in enumerate(ins):
        c["ins"][0][k] = s
    c["ins_open"] = sum(ins[0]) if ins else 0
    c["ins_bases"] = sum(sum(s) for s in ins)
    return c


def both(cons, cols, L=100):
    cons = np.asarray(cons, np.int8)
    cols = np.concatenate(cols) if cols else np.zeros(0, PILEUP_DTYPE)
    cols["base"] = cons
    want = pr.recall(cons, cols, L)
    got = c_recall(cons, cols, L)
    assert got.dtype == np.int8 and np.array_equal(got, want), (list(got), list(want))
    return [int(x) for x in got]


def test_the_symbol_is_exported():
    from repeatafterme_amd import _lib
    assert hasattr(_lib.lib(), "ramx_recall_consensus")


def test_random_pileups():
    rng = np.random.default_rng(11)
    changed = grew = shrank = 0
    for trial in range(300):
        rows = int(rng.integers(0, 40))
        L = int(rng.integers(max(rows, 1), rows + 12))
        cons = rng.integers(0, 4, rows).astype(np.int8)
        cols = np.zeros(rows, PILEUP_DTYPE)
        cols["base"] = cons
        cols["cover"] = rng.integers(0, 12, rows)
        for r in range(rows):
            c = int(cols["cover"][r])
            cols["del"][r] = c if rng.random() < 0.25 else rng.integers(0, c + 1)
            cols["match"][r] = rng.multinomial(c - int(cols["del"][r]), [0.3, 0.25, 0.2, 0.15, 0.1])
            n = c if rng.random() < 0.15 else int(rng.integers(0, c // 2 + 2))
            for k in range(PILEUP_INS):
                n = int(rng.integers(0, n + 1)) if k and rng.random() < 0.5 else min(n, c)
                cols["ins"][r][k] = rng.multinomial(n, [0.22, 0.22, 0.22, 0.22, 0.12])
        want = pr.recall(cons, cols, L)
        got = c_recall(cons, cols, L)
        assert np.array_equal(got, want), trial
        assert len(got) <= L
        changed += not np.array_equal(got, cons)
        grew += len(got) > rows
        shrank += len(got) < rows
    assert changed > 100 and grew > 20 and shrank > 20


def test_exact_halves_are_no_majority():
    # deletion: 5 of 10 keeps the column, 6 of 10 drops it; 5 of 9 drops it
    assert both([2], [col(10, (0, 0, 5, 0, 0), 5)]) == [2]
    assert both([2], [col(10, (0, 0, 4, 0, 0), 6)]) == []
    assert both([2], [col(9, (0, 0, 4, 0, 0), 5)]) == []
    # insertion: 5 of 10 inserts nothing, 6 of 10 inserts
    assert both([2], [col(10, (0, 0, 10, 0, 0), 0, [(5, 0, 0, 0, 0)])]) == [2]
    assert both([2], [col(10, (0, 0, 10, 0, 0), 0, [(0, 6, 0, 0, 0)])]) == [1, 2]
    # an inserted column before a dropped one
    assert both([2, 3], [col(10, (0, 0, 2, 0, 0), 8, [(0, 0, 0, 7, 0)]), col(10, (0, 0, 0, 10, 0))]) == [3, 3]


def test_ties_of_the_column_base():
    assert both([3], [col(9, (3, 3, 0, 3, 0))]) == [3]          # three-way tie with the current base: kept
    assert both([2], [col(9, (3, 3, 0, 3, 0))]) == [0]          # without it: the lowest code
    assert both([0], [col(9, (0, 3, 3, 3, 0))]) == [1]
    assert both([1], [col(8, (4, 4, 0, 0, 0))]) == [1]          # two-way tie with the current base
    assert both([3], [col(8, (0, 4, 4, 0, 0))]) == [1]
    assert both([3], [col(8, (0, 0, 0, 0, 8))]) == [3]          # only N matched: all four counts 0, the base stays
    assert both([3], [col(8, (0, 0, 0, 0, 2), 4)]) == [3]
    assert both([3], [col(8, (1, 0, 0, 0, 7))]) == [0]          # N is never a candidate
    assert both([0], [col(8, (2, 0, 5, 1, 0))]) == [2]


def test_ties_and_n_in_the_inserted_columns():
    assert both([0], [col(10, (10, 0, 0, 0, 0), 0, [(0, 3, 0, 3, 1)])]) == [1, 0]     # the lowest code wins
    assert both([0], [col(10, (10, 0, 0, 0, 0), 0, [(0, 0, 0, 0, 9)])]) == [0]        # a slot holding only N ends the run
    assert both([0], [col(10, (10, 0, 0, 0, 0), 0, [(0, 0, 1, 0, 8)])]) == [2, 0]     # ... one base beside the N is enough
    # the first slot that fails ends the run even when a later one would pass
    assert both([0], [col(10, (10, 0, 0, 0, 0), 0, [(7, 0, 0, 0, 0), (0, 0, 0, 0, 7), (0, 7, 0, 0, 0)])]) == [0, 0]
    assert both([0], [col(10, (10, 0, 0, 0, 0), 0, [(7, 0, 0, 0, 0), (0, 5, 0, 0, 0), (0, 7, 0, 0, 0)])]) == [0, 0]


def test_all_four_slots():
    c = col(10, (0, 10, 0, 0, 0), 0, [(0, 0, 0, 9, 0), (0, 0, 8, 0, 0), (7, 0, 0, 0, 0), (0, 6, 0, 0, 0)])
    assert both([1], [c]) == [3, 2, 0, 1, 1]


def test_cover_zero_keeps_the_column():
    c = col(0, (0, 0, 0, 0, 0))
    c["ins"][0][0] = (0, 3, 0, 0, 0)                           # not a pileup the kernel makes: nothing is inserted all the same
    assert both([2, 1], [c, col(4, (0, 0, 0, 4, 0))]) == [2, 3]
    assert both([], []) == []


def test_growth_is_cut_at_L():
    grow = lambda base: col(10, tuple(10 if b == base else 0 for b in range(5)), 0, [(0, 0, 0, 9, 0), (0, 0, 9, 0, 0)])
    assert both([0, 1, 0], [grow(0), grow(1), grow(0)], L=100) == [3, 2, 0, 3, 2, 1, 3, 2, 0]
    assert both([0, 1, 0], [grow(0), grow(1), grow(0)], L=9) == [3, 2, 0, 3, 2, 1, 3, 2, 0]
    assert both([0, 1, 0], [grow(0), grow(1), grow(0)], L=7) == [3, 2, 0, 3, 2, 1, 3]
    assert both([0, 1, 0], [grow(0), grow(1), grow(0)], L=4) == [3, 2, 0, 3]
    assert both([0, 1, 0], [grow(0), grow(1), grow(0)], L=3) == [3, 2, 0]
    assert both([0, 1, 0], [grow(0), grow(1), grow(0)], L=1) == [3]
