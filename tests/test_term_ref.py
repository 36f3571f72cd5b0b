"""The terminal-repeat contract (include/ramx.h, ramx_term) on the CPU: a literal, hand-worked record for every rule, checked on
the restatement (tests/term_ref.py, both forms) and on the host functions of libramx.so (ramx_term_pair, ramx_term_summary), the
host functions against the restatement on seeded random pairs with planted repeats, the null of the default scores, and two
planted families on the CPU oracle.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from repeatafterme_amd import _lib
from repeatafterme_amd.datamodel import TERM_DTYPE, TermParams
from repeatafterme_amd.extend import term_pair, term_summary

import term_ref as tr

ERR_ARG = -103
ERR_UNSUPPORTED = -106
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 4, "c": 5, "g": 6, "t": 7, "N": 99, "n": -1}


def codes(s):
    return np.array([CODE[ch] for ch in s], np.int8)


def tup(r):
    return tuple(int(r[k]) for k in tr.FIELDS)


def both(a, b, **kw):
    """The record of two strings by the triple loop, the anti-diagonals and ramx_term_pair: all three must agree."""
    p = {**tr.DEFAULT, "min_score": 1, **kw}
    ca, cb = tr.classes(codes(a)), tr.classes(codes(b))
    want = tr.pair_loop(ca, cb, **p)
    assert tr.pair_diag(ca, cb, **p) == want
    if p["min_score"] == 1 and len(a) and len(b):
        assert tr.best_score(ca, cb, **p) == want[0]
    got = tup(term_pair(codes(a), codes(b), TermParams(**p)))
    assert got == want, (got, want)
    return want


def site(lib, lo, hi, seq_lo=None, seq_hi=None, **kw):
    """(direct, inverted) of a site on a library given as a string, by the restatement."""
    p = {**tr.DEFAULT, "min_score": 1, **kw}
    return tr.site_records(codes(lib), (lo, hi, lo if seq_lo is None else seq_lo, hi if seq_hi is None else seq_hi), **p)


# ---- a literal record for every rule (score, a_start, a_end, b_start, b_end, matches, columns, T) ----

def test_a_plain_match_and_its_payload():
    # five agreeing pairs on the main diagonal: 5 * 2
    assert both("ACGTA", "ACGTA") == (10, 0, 4, 0, 4, 5, 5, 5)
    # a mismatch inside: 2 + 2 - 3 + 2 + 2, four matches in five columns
    assert both("ACGTA", "ACTTA") == (5, 0, 4, 0, 4, 4, 5, 5)


def test_d_before_u_before_l_on_equal_values():
    """match 2, mismatch 1, gap 1.  AAAC / ACAC: cell (4, 4) is 5 along the diagonal from (0, 0) (2 - 1 + 2 + 2) and 5 through
    a gap from (1, 0) (2 - 1 + 2 + 2 with L at (2, 2)); at (2, 2) D = 2 - 1 and L = 2 - 1 are equal, and D is taken: the
    alignment begins at (0, 0).  ACAC / AAAC is the same with U in the place of L.  ACAC / CAAC: at (3, 3), U = H[2][3] - 1 and
    L = H[3][2] - 1 are both 1 (D = 0 - 1 + ...): U is taken, and the alignment begins at (0, 1), not at (1, 0)."""
    s = dict(match=2, mismatch=1, gap=1)
    assert both("AAAC", "ACAC", **s) == (5, 0, 3, 0, 3, 3, 4, 4)
    assert both("ACAC", "AAAC", **s) == (5, 0, 3, 0, 3, 3, 4, 4)
    assert both("ACAC", "CAAC", **s) == (5, 0, 3, 1, 3, 3, 4, 4)


def test_best_cell_ties_go_to_the_smallest_i_then_the_smallest_j():
    # AC twice in b: cells (2, 2) and (2, 5) hold 4, the smaller j wins
    assert both("AC", "ACNAC") == (4, 0, 1, 0, 1, 2, 2, 2)
    # AC twice in a: cells (2, 2) and (5, 2), the smaller i wins
    assert both("ACNAC", "AC") == (4, 0, 1, 0, 1, 2, 2, 2)
    # AC at (2, 5) and GT at (5, 2): i before j
    assert both("ACNGT", "GTNAC") == (4, 0, 1, 3, 4, 2, 2, 5)


def test_restart_at_0_resets_the_payload():
    # 2 + 2 - 3 - 3 falls to 0 at (4, 4): the cells behind it begin anew, and GGA scores 6 from (5, 5) with its own counts
    assert both("ACTTTGGA", "ACAAAGGA") == (6, 5, 7, 5, 7, 3, 3, 8)


def test_a_gap_is_linear_and_counts_as_a_column():
    # eight matches, one base of a left out: 16 - 5, nine columns
    assert both("ACGTTACGA", "ACGTACGA") == (11, 0, 8, 0, 7, 8, 9, 8)
    # two bases left out cost 10: 20 - 10 + 20, twenty matches in twenty-two columns
    assert both("ACGGTCATGATTCCTAGTGCAA", "ACGGTCATGACCTAGTGCAA") == (30, 0, 21, 0, 19, 20, 22, 20)
    # ... and the same gap in b
    assert both("ACGGTCATGACCTAGTGCAA", "ACGGTCATGATTCCTAGTGCAA") == (30, 0, 19, 0, 21, 20, 22, 20)


def test_class_4_is_a_mismatch():
    # N against N does not agree: 2 + 2 - 3 + 2 + 2
    assert both("ACNGT", "ACNGT") == (5, 0, 4, 0, 4, 4, 5, 5)
    assert both("ACnGT", "ACNGT") == (5, 0, 4, 0, 4, 4, 5, 5)
    # lower case is its base
    assert both("acgt", "ACGT") == (8, 0, 3, 0, 3, 4, 4, 4)
    # a position outside the library: lo = -2, so a = N N G T T T and b = T T A C G T; GT at (4, 6) and TT at (5, 2) hold 4
    d, v = site("GTTTTTACGT", -2, 9, seq_lo=-2)
    assert d == (4, 2, 3, 4, 5, 2, 2, 6)
    # a position outside seq_lo..seq_hi is never inside lo..hi (the argument checks), so the bounds alone change nothing
    assert site("GTTTTTACGT", 0, 9, seq_lo=-5, seq_hi=30) == site("GTTTTTACGT", 0, 9)


def test_min_score_on_both_sides_of_its_edge():
    assert both("ACGTACGTAC", "ACGTACGTAC", min_score=20) == (20, 0, 9, 0, 9, 10, 10, 10)
    assert both("ACGTACGTAC", "ACGTACGTAC", min_score=21) == (0, 0, 0, 0, 0, 0, 0, 10)


def test_t_0_t_1_and_an_odd_n():
    assert site("A", 0, 0) == ((0,) * 8, (0,) * 8)                       # n = 1: T = 0
    assert site("ACGT", 2, 1, seq_lo=0, seq_hi=3) == ((0,) * 8, (0,) * 8)       # an empty element
    # n = 2: T = 1; A against A, and A against the complement of A
    assert site("AA", 0, 1) == ((2, 0, 0, 0, 0, 1, 1, 1), (0, 0, 0, 0, 0, 0, 0, 1))
    assert site("AT", 0, 1) == ((0, 0, 0, 0, 0, 0, 0, 1), (2, 0, 0, 0, 0, 1, 1, 1))
    # n = 5: T = 2, the base in the middle is in neither window
    assert site("ACGAC", 0, 4) == ((4, 0, 1, 0, 1, 2, 2, 2), (0, 0, 0, 0, 0, 0, 0, 2))
    # tmax below n / 2
    assert site("ACGAC", 0, 4, tmax=1)[0] == (0, 0, 0, 0, 0, 0, 0, 1)
    assert both("", "ACGT") == (0,) * 8 and both("ACGT", "") == (0,) * 8


def test_a_window_and_its_reverse_complement_are_a_full_length_tir():
    w = "ACGGTCATTGCAGTCCATGA"
    rc = "".join("TGCA"["ACGT".index(ch)] for ch in reversed(w))
    d, v = site(w + "GGGGGGGGGG" + rc, 0, 49, tmax=20)
    assert v == (40, 0, 19, 0, 19, 20, 20, 20)
    assert d[0] < 12


def test_a_direct_repeat_ends_at_j_t_minus_1():
    r = "ACGGTCATTGCA"
    d, v = site(r + "TTTTTTTTCCCCCCCC" + r, 0, 39)
    assert d == (24, 0, 11, 8, 19, 12, 12, 20)


# ---- the host functions against the restatement ----

def planted_pair(rng, n, div):
    """Two windows of n bases: b carries a copy of a stretch of a with substitutions and indels at rate div."""
    a = rng.integers(0, 4, n).astype(np.int8)
    b = rng.integers(0, 4, n).astype(np.int8)
    k = int(rng.integers(min(8, n), n + 1))
    at = int(rng.integers(0, n - k + 1))
    rep = []
    for x in a[at:at + k]:
        u = rng.random()
        if u < div / 3:
            continue                                        # a deletion
        if u < 2 * div / 3:
            rep.append(int(rng.integers(0, 4)))             # an insertion in front
        rep.append(int((x + rng.integers(1, 4)) % 4) if rng.random() < div else int(x))
    rep = np.array(rep[:n], np.int8)
    to = int(rng.integers(0, n - len(rep) + 1))
    b[to:to + len(rep)] = rep
    for arr in (a, b):                                      # a few N and lower-case bases
        hit = rng.random(n) < 0.02
        arr[hit] = 99
        low = rng.random(n) < 0.05
        arr[low & (arr < 4)] += 4
    return a, b


def test_term_pair_equals_the_restatement_on_random_pairs():
    rng = np.random.default_rng(20261020)
    shown = 0
    for k in range(300):
        n = int(rng.integers(1, 41)) if k < 200 else int(rng.integers(41, 200))
        a, b = planted_pair(rng, n, float(rng.choice([0.0, 0.05, 0.1, 0.15])))
        if k % 5 == 0:
            b = b[:int(rng.integers(0, n + 1))]             # the lengths may differ
        p = dict(match=int(rng.integers(1, 16)), mismatch=int(rng.integers(1, 16)), gap=int(rng.integers(1, 32)),
                 min_score=int(rng.integers(1, 30))) if k % 2 else dict(match=2, mismatch=3, gap=5, min_score=10)
        ca, cb = tr.classes(a), tr.classes(b)
        want = tr.pair_diag(ca, cb, **p)
        if max(len(a), len(b)) <= 40:
            assert tr.pair_loop(ca, cb, **p) == want
        got = tup(term_pair(a, b, TermParams(tmax=512, slack=3, **p)))
        assert got == want, (k, got, want)
        shown += want[0] > 0
    assert shown > 150


def test_struct_sizes():
    assert C.sizeof(_lib.TermParams) == 32 and C.sizeof(_lib.TermFamily) == 64 and TERM_DTYPE.itemsize == 32


def recs_array(recs):
    out = np.zeros((len(recs), 2), TERM_DTYPE)
    for i, (d, v) in enumerate(recs):
        out[i, 0], out[i, 1] = d, v
    return out


def as_dict(s):
    return {k: getattr(s, k) for k in ("n", "n_direct", "n_inverted", "direct_anchored", "inverted_anchored", "direct_median",
                                       "inverted_median", "verdict", "direct_matches", "direct_columns", "inverted_matches",
                                       "inverted_columns")}


Z = (0, 0, 0, 0, 0, 0, 0, 100)


def D(a_start=0, b_end=99, length=50):
    return (2 * length, a_start, a_start + length - 1, b_end - length + 1, b_end, length, length, 100)


def V(a_start=0, b_start=0, length=30):
    return (2 * length, a_start, a_start + length - 1, b_start, b_start + length - 1, length, length, 100)


def test_summary_anchors_medians_and_sums():
    recs = [(D(0, 99, 50), Z), (D(3, 96, 40), Z), (D(4, 99, 60), Z), (D(0, 95, 70), Z), (Z, V(0, 0, 30)), (Z, V(3, 3, 20)),
            (Z, V(4, 0, 90)), (Z, V(0, 4, 90))]
    want = tr.summary(recs)
    # slack 3: a_start 4 and b_end 95 are not anchored; the lower median of (40, 50) is 40, of (20, 30) is 20
    assert (want["n_direct"], want["direct_anchored"], want["direct_median"], want["direct_matches"], want["direct_columns"]) == (4, 2, 40, 90, 90)
    assert (want["n_inverted"], want["inverted_anchored"], want["inverted_median"], want["inverted_matches"]) == (4, 2, 20, 50)
    assert want["verdict"] == 0
    assert as_dict(term_summary(recs_array(recs))) == want
    # slack 4 takes them all in; three lengths: the middle one
    want4 = tr.summary(recs, slack=4)
    assert (want4["direct_anchored"], want4["inverted_anchored"]) == (4, 4)
    assert as_dict(term_summary(recs_array(recs), TermParams(slack=4))) == want4
    odd = [(D(0, 99, 50), Z), (D(0, 99, 10), Z), (D(0, 99, 30), Z)]
    assert tr.summary(odd)["direct_median"] == 30 and term_summary(recs_array(odd)).direct_median == 30
    assert as_dict(term_summary(recs_array([]))) == tr.summary([])


def test_the_verdict_at_its_edges():
    def verdict(recs):
        want = tr.summary(recs)
        assert as_dict(term_summary(recs_array(recs))) == want
        return want["verdict"]
    # 2 x = n is not a majority
    assert verdict([(D(), Z), (D(), Z), (Z, Z), (Z, Z)]) == 0
    assert verdict([(D(), Z), (D(), Z), (D(), Z), (Z, Z), (Z, Z)]) == 1
    assert verdict([(Z, V()), (Z, V()), (Z, Z), (Z, Z)]) == 0
    assert verdict([(Z, V()), (Z, V()), (Z, V()), (Z, Z), (Z, Z)]) == 2
    # a tie between the orientations goes to LTR; one more inverted record makes it TIR
    assert verdict([(D(), V()), (D(), V()), (Z, Z)]) == 1
    assert verdict([(D(), V()), (D(), V()), (Z, V())]) == 2
    assert verdict([(D(), V()), (D(), V()), (D(), Z)]) == 1
    assert verdict([]) == 0


def test_every_argument_error():
    L = _lib.lib()
    ok = _lib.TermParams(512, 2, 3, 5, 40, 3)
    fam = _lib.TermFamily()
    rec = np.zeros(8, TERM_DTYPE)
    out = np.full(8, 7, np.int32).view(TERM_DTYPE)
    x = codes("ACGTACGTAC")
    good = (512, 2, 3, 5, 40, 3)
    edges = {0: (0, 1025, -1), 1: (0, 16, -2), 2: (0, 16, -3), 3: (0, 32, -5), 4: (0, -40), 5: (-1, 16)}
    for field, values in edges.items():
        for v in values:
            bad = list(good)
            bad[field] = v
            bp = _lib.TermParams(*bad)
            assert L.ramx_term_pair(x.ctypes.data, 10, x.ctypes.data, 10, C.byref(bp), out.ctypes.data) == ERR_ARG, bad
            assert L.ramx_term_summary(rec.ctypes.data, 4, C.byref(bp), C.byref(fam)) == ERR_ARG, bad
    for r in ((1, 0), (0, 1)):
        bp = _lib.TermParams(*good, (C.c_int32 * 2)(*r))
        assert L.ramx_term_pair(x.ctypes.data, 10, x.ctypes.data, 10, C.byref(bp), out.ctypes.data) == ERR_ARG
    assert (out.view(np.int32) == 7).all()                # raised before anything is written
    for fine in [(1, 1, 1, 1, 1, 0), (1024, 15, 15, 31, 1 << 30, 15)]:
        assert L.ramx_term_pair(x.ctypes.data, 10, x.ctypes.data, 10, C.byref(_lib.TermParams(*fine)), out.ctypes.data) == 0, fine
    assert L.ramx_term_pair(x.ctypes.data, 10, x.ctypes.data, 10, None, out.ctypes.data) == ERR_ARG
    assert L.ramx_term_pair(x.ctypes.data, -1, x.ctypes.data, 10, C.byref(ok), out.ctypes.data) == ERR_ARG
    assert L.ramx_term_pair(x.ctypes.data, 10, x.ctypes.data, -1, C.byref(ok), out.ctypes.data) == ERR_ARG
    assert L.ramx_term_pair(None, 10, x.ctypes.data, 10, C.byref(ok), out.ctypes.data) == ERR_ARG
    assert L.ramx_term_pair(x.ctypes.data, 10, None, 10, C.byref(ok), out.ctypes.data) == ERR_ARG
    assert L.ramx_term_pair(x.ctypes.data, 10, x.ctypes.data, 10, C.byref(ok), None) == ERR_ARG
    assert L.ramx_term_pair(x.ctypes.data, 65537, x.ctypes.data, 10, C.byref(ok), out.ctypes.data) == ERR_UNSUPPORTED
    assert L.ramx_term_pair(None, 0, None, 0, C.byref(ok), out.ctypes.data) == 0
    assert L.ramx_term_summary(rec.ctypes.data, 4, None, C.byref(fam)) == ERR_ARG
    assert L.ramx_term_summary(rec.ctypes.data, -1, C.byref(ok), C.byref(fam)) == ERR_ARG
    assert L.ramx_term_summary(None, 4, C.byref(ok), C.byref(fam)) == ERR_ARG
    assert L.ramx_term_summary(rec.ctypes.data, 4, C.byref(ok), None) == ERR_ARG
    assert L.ramx_term_summary(rec.ctypes.data, 4, C.byref(ok), C.byref(fam)) == 0


# ---- the null of the default scores ----

def test_independent_windows_stay_below_the_default_min_score():
    """200 seeded pairs of independent random windows at T = 512 under the default scores: the largest best score of the
    restatement is 30, below the default min_score of 40 (the Karlin-Altschul estimate for the ungapped case is about 20)."""
    rng = np.random.default_rng(512)
    worst = 0
    for _ in range(200):
        a, b = rng.integers(0, 4, 512), rng.integers(0, 4, 512)
        worst = max(worst, tr.best_score(a, b, **tr.DEFAULT))
    print("largest chance score of 200 pairs at T = 512:", worst)
    assert worst < tr.DEFAULT["min_score"] == TermParams().min_score
    assert worst == 30


# ---- two planted families on the CPU oracle ----

def test_planted_tir_family():
    """Copies with a 60-base TIR that carries a deletion and an insertion just inside the 3' end, cores in the middle: after both
    oracle extensions the restatement on the sites says TIR, anchored in most copies, median within slack of 60."""
    e = tr.planted_expectation("TIR")
    s = e["summary"]
    print("planted TIR family:", s)
    assert s["verdict"] == 2 and abs(s["inverted_median"] - 60) <= tr.DEFAULT["slack"]
    assert 2 * s["inverted_anchored"] > s["n"] and s["direct_anchored"] == 0
    assert as_dict(term_summary(recs_array(e["records"]))) == s


def test_planted_ltr_family():
    e = tr.planted_expectation("LTR")
    s = e["summary"]
    print("planted LTR family:", s)
    assert s["verdict"] == 1 and abs(s["direct_median"] - 150) <= tr.DEFAULT["slack"]
    assert 2 * s["direct_anchored"] > s["n"] and s["inverted_anchored"] == 0
    assert as_dict(term_summary(recs_array(e["records"]))) == s
