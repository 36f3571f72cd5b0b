"""ramx_recall_cpg (host C of libramx.so) against the restatement of tests/dinuc_ref.py: random records and hand-worked ones for
every branch of the second pass.  No GPU: the function is two passes over the columns, exact integers."""
import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import DINUC_DTYPE, PILEUP_DTYPE, PILEUP_INS

import dinuc_ref as dr
import pileup_ref as pr

A, C, G, T = 0, 1, 2, 3
MATRIX = np.asarray(po.Params.named("14p43g", bandwidth=14, L=100).matrix, np.int32)


def test_the_matrix_the_hand_worked_records_assume():
    m = MATRIX.reshape(100, 100)[:4, :4]
    assert m.tolist() == [[9, -18, -10, -21], [-18, 11, -18, -7], [-7, -18, 11, -18], [-21, -10, -18, 9]]


def c_recall(cons, cols, di, rev, cpg_ts, L):
    from repeatafterme_amd.device import recall_cpg
    return recall_cpg(cons, cols, di, MATRIX, rows_reversed=rev, cpg_ts=cpg_ts, L=L)


def both(cons, cols, di, rev=0, cpg_ts=0, L=100):
    cons = np.asarray(cons, np.int8)
    cols["base"] = cons
    want, want_n = dr.recall_cpg(cons, cols, di, rev, MATRIX, cpg_ts, L)
    got, got_n = c_recall(cons, cols, di, rev, cpg_ts, L)
    assert got.dtype == np.int8 and np.array_equal(got, want) and got_n == want_n, (list(got), got_n, list(want), want_n)
    return "".join("ACGT"[x] for x in got), got_n


def columns(*match, cover=10):
    """Columns without gaps whose matched counts are given (A, C, G, T)."""
    cols = np.zeros(len(match), PILEUP_DTYPE)
    cols["cover"] = cover
    for r, m in enumerate(match):
        cols["match"][r][:4] = m
    return cols


def pairs(rows, **at):
    """DINUC_DTYPE [rows] with di of row r from at['r<r>'] = {(x, y): count}."""
    di = np.zeros(rows, DINUC_DTYPE)
    for key, d in at.items():
        for (x, y), n in d.items():
            di[int(key[1:])]["di"][x][y] = n
    di["adjacent"] = di["di"].sum(axis=(1, 2))
    di["both"] = di["adjacent"]
    return di


def test_the_symbol_is_exported():
    from repeatafterme_amd import _lib
    assert hasattr(_lib.lib(), "ramx_recall_cpg")


TA_COLS = ((0, 4, 0, 6), (6, 0, 4, 0))      # plain calls T and A: six of ten copies deaminated on either strand


def test_a_deaminated_pair_is_called_cg():
    # S_plain = 6 * (9 + 9) + 4 * (M[T][C] + M[A][G]) = 108 - 80 = 28; S_CG = 6 * (0 + 0) + 4 * (11 + 11) = 88
    di = pairs(2, r0={(T, A): 6, (C, G): 4})
    assert dr.pair_sums(di[0]["di"], T, A, lambda c, s: int(MATRIX[c * 100 + s]), 0) == (28, 88)
    assert both([T, A], columns(*TA_COLS), di) == ("CG", 1)
    assert pr.recall(np.array([T, A], np.int8), columns(*TA_COLS), 100).tolist() == [T, A]         # the plain rule's answer


def test_a_true_ta_stays():
    # S_plain = 9 * 18 + 1 * (-10 - 10) = 142; S_CG = 22
    assert both([T, A], columns((0, 1, 0, 9), (9, 0, 1, 0)), pairs(2, r0={(T, A): 9, (C, G): 1})) == ("TA", 0)


def test_the_sums_are_additive_over_the_two_columns():
    """The marginals of the deaminated pair (T 6, C 4; A 6, G 4) with another joint table: S_plain = 4 * (9 - 10) + 4 * (-10 + 9)
    + 2 * 18 = 28 and S_CG = 4 * 11 + 4 * 11 + 0 = 88 again.  The rule scores the two columns' counts over the ADJACENT copies."""
    di = pairs(2, r0={(T, G): 4, (C, A): 4, (T, A): 2})
    assert dr.pair_sums(di[0]["di"], T, A, lambda c, s: int(MATRIX[c * 100 + s]), 0) == (28, 88)
    assert both([T, A], columns(*TA_COLS), di) == ("CG", 1)


def test_equal_sums_are_not_a_call():
    di = pairs(2, r0={(T, A): 10})
    cols = columns((0, 0, 0, 10), (10, 0, 0, 0))
    assert both([T, A], cols, di, cpg_ts=9) == ("TA", 0)         # S_CG = 10 * 18 = S_plain: strictly greater is asked
    assert both([T, A], cols, di, cpg_ts=10) == ("CG", 1)
    assert both([T, A], cols, di, cpg_ts=-5) == ("TA", 0)


def test_class_n_is_ignored():
    di = pairs(2, r0={(4, 4): 10, (T, 4): 3, (4, A): 3})
    assert both([T, A], columns((0, 0, 0, 3), (3, 0, 0, 0)), di, cpg_ts=50) == ("TA", 0)          # both sums are 0
    di = pairs(2, r0={(4, 4): 10, (T, A): 1})
    assert both([T, A], columns((0, 0, 0, 3), (3, 0, 0, 0)), di, cpg_ts=10) == ("CG", 1)          # 20 > 18


def test_half_deaminated_pairs():
    # (T, G): S_plain = 6 * (9 + 11) + 4 * (-10 + 11) = 124; S_CG = 6 * (0 + 11) + 4 * 22 = 154
    assert both([T, G], columns((0, 4, 0, 6), (0, 0, 10, 0)), pairs(2, r0={(T, G): 6, (C, G): 4})) == ("CG", 1)
    # (C, A) with a single C G copy: S_plain = 9 * (11 + 9) + (11 - 10) = 181; S_CG = 9 * 11 + 22 = 121
    assert both([C, A], columns((0, 10, 0, 0), (9, 0, 1, 0)), pairs(2, r0={(C, A): 9, (C, G): 1})) == ("CA", 0)
    # an untested pair (A first, or T last) is left alone whatever its counts say
    assert both([A, G], columns((10, 0, 0, 0), (0, 0, 10, 0)), pairs(2, r0={(C, G): 99})) == ("AG", 0)
    assert both([T, T], columns((0, 0, 0, 10), (0, 0, 0, 10)), pairs(2, r0={(C, G): 99})) == ("TT", 0)


def test_a_pair_that_is_cg_already_counts():
    assert both([C, G, A], columns((0, 10, 0, 0), (0, 0, 10, 0), (10, 0, 0, 0)), pairs(3)) == ("CGA", 1)


def test_reversed_rows():
    # rows run against the reading order: row 0 is the 3' column.  di[0].di[x][y] has x in row 0: D is its transpose
    cols = columns(TA_COLS[1], TA_COLS[0])
    di = pairs(2, r0={(A, T): 6, (G, C): 4})
    assert both([A, T], cols, di, rev=1) == ("GC", 1)
    assert both([A, T], cols, di, rev=0) == ("AT", 0)                                             # forward: (A, T) is not tested
    assert both([T, A], columns(*TA_COLS), pairs(2, r0={(T, A): 6, (C, G): 4}), rev=1) == ("TA", 0)


def test_broken_pairs_are_not_tested():
    di = pairs(3, r0={(T, A): 6, (C, G): 4}, r1={(T, A): 6, (C, G): 4})
    # an inserted column is emitted before row 1: the pair (0, 1) is no pair of adjacent output columns
    cols = columns(*TA_COLS)
    cols["ins"][1][0] = (0, 0, 7, 0, 0)
    assert both([T, A], cols, di[:2]) == ("TGA", 0)
    # ... an insertion before row 0 does not break it
    cols = columns(*TA_COLS)
    cols["ins"][0][0] = (0, 0, 7, 0, 0)
    assert both([T, A], cols, di[:2]) == ("GCG", 1)
    # row 1 is dropped: rows 0 and 2 become neighbours in the output but are no row pair, and no record describes them
    cols = columns(TA_COLS[0], (0, 0, 0, 0), TA_COLS[1])
    cols["match"][1][:4] = (2, 0, 0, 0)
    cols["del"][1] = 8
    assert both([T, C, A], cols, di) == ("TA", 0)
    # the cut to L columns reaches row 0 only
    assert both([T, A], columns(*TA_COLS), di[:2], L=1) == ("T", 0)


def test_neighbouring_pairs_cannot_collide():
    # T A T A: pairs (0, 1) and (2, 3) are tested, (1, 2) is (A, T) and is not; both are called, nothing is read after it is written
    di = pairs(4, r0={(T, A): 6, (C, G): 4}, r1={(C, G): 99}, r2={(T, A): 6, (C, G): 4})
    assert both([T, A, T, A], columns(*TA_COLS, *TA_COLS), di) == ("CGCG", 2)
    di = pairs(4, r0={(A, T): 6, (G, C): 4}, r1={(G, C): 99}, r2={(A, T): 6, (G, C): 4})
    assert both([A, T, A, T], columns(TA_COLS[1], TA_COLS[0], TA_COLS[1], TA_COLS[0]), di, rev=1) == ("GCGC", 2)


def test_no_rows():
    assert both([], np.zeros(0, PILEUP_DTYPE), np.zeros(0, DINUC_DTYPE)) == ("", 0)
    assert both([T], columns((0, 0, 0, 10)), pairs(1)) == ("T", 0)


@pytest.mark.parametrize("rev", [0, 1])
def test_random_records(rev):
    rng = np.random.default_rng(23 + rev)
    M = lambda c, s: int(MATRIX[c * 100 + s])
    seen = dict(tested=0, flipped=0, kept=0, already=0, ties=0, all_n=0, broken_ins=0, broken_drop=0, changed_len=0)
    for trial in range(400):
        rows = int(rng.integers(0, 40))
        L = int(rng.integers(max(rows, 1), rows + 12))
        cpg_ts = int(rng.choice([-12, -3, 0, 0, 4, 9, 15]))
        cons = rng.integers(0, 4, rows).astype(np.int8)
        cols = np.zeros(rows, PILEUP_DTYPE)
        cols["base"] = cons
        cols["cover"] = rng.integers(0, 12, rows)
        di = np.zeros(rows, DINUC_DTYPE)
        mode = trial % 4                       # 0, 1: anything; 2: only deaminated pairs (ties with cpg_ts = 9); 3: class N only
        for r in range(rows):
            c = int(cols["cover"][r])
            cols["del"][r] = c if rng.random() < 0.1 else rng.integers(0, c // 3 + 1)
            # pyrimidines and purines alternate often enough for tested pairs to be common
            w = [0.1, 0.35, 0.1, 0.45, 0.0] if (r % 2 == 0) != bool(rev) else [0.45, 0.1, 0.35, 0.1, 0.0]
            cols["match"][r] = rng.multinomial(c - int(cols["del"][r]), w)
            if rng.random() < 0.1:
                cols["ins"][r][0] = rng.multinomial(c, [0.22, 0.22, 0.22, 0.22, 0.12])
            if mode == 2:
                di["di"][r][(A, T) if rev else (T, A)] = rng.integers(1, 12)
            elif mode == 3:
                di["di"][r][4, :] = rng.integers(0, 5, 5)
                di["di"][r][:, 4] = rng.integers(0, 5, 5)
            else:
                di["di"][r] = rng.integers(0, 7, (5, 5)) * (rng.random((5, 5)) < 0.5)
        want, want_n, tested = dr.recall_cpg(cons, cols, di, rev, MATRIX, cpg_ts, L, with_pairs=True)
        got, got_n = c_recall(cons, cols, di, rev, cpg_ts, L)
        assert np.array_equal(got, want) and got_n == want_n, trial
        assert len(got) == len(pr.recall(cons, cols, L))                   # the length is the plain re-call's
        plain, at, before = dr.plain_calls(cons, cols, L)
        for (r, a, b, sp, sc, called) in tested:
            seen["tested"] += 1
            seen["already"] += (a, b) == (C, G)
            seen["flipped"] += called and (a, b) != (C, G)
            seen["kept"] += not called
            seen["ties"] += sp == sc and (a, b) != (C, G) and sp != 0
            seen["all_n"] += mode == 3
            assert called == ((a, b) == (C, G) or sc > sp)
        for r in range(rows - 1):
            seen["broken_ins"] += at[r] is not None and at[r + 1] is not None and before[r + 1] > 0
            seen["broken_drop"] += r + 2 < rows and at[r] is not None and at[r + 1] is None and at[r + 2] is not None
        seen["changed_len"] += len(got) != rows
    assert all(v > 10 for v in seen.values()), seen
