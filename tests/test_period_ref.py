"""The tandem-periodicity contract (include/ramx.h, ramx_period) on the CPU: the brute-force restatement (tests/period_ref.py)
and the host C function ramx_period_sequence on hand-worked segments with literal records, one per rule and tie; the host
functions ramx_period_sequence, ramx_period_segments and ramx_period_summary against the restatement; every bad parameter; and a
planted family on the CPU oracle whose right extension runs into a (CA)n.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from repeatafterme_amd import _lib
from repeatafterme_amd.datamodel import PERIOD_DTYPE, PERIOD_SEG_DTYPE, CoreSet, PeriodParams
from repeatafterme_amd.extend import period_segments, period_sequence, period_summary

import period_ref as pr

ERR_ARG, ERR_UNSUPPORTED = -103, -106
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 4, "c": 5, "g": 6, "t": 7, "N": 99}


def codes(s):
    return np.array([CODE[ch] for ch in s], np.int8)


def tup(r):
    return tuple(int(r[k]) for k in ("period", "score", "start", "end", "agree", "disagree"))


def both(s, **kw):
    """The record of a string by the restatement and by the host C function, which must agree."""
    params = {**pr.DEFAULT, **kw}
    want = pr.record_of_codes(codes(s), **params)
    got = period_sequence(codes(s), PeriodParams(**params))
    assert tup(got) == want and not got["reserved"].any()
    return want


def test_poly_a_of_24_and_the_short_last_block():
    # 23 pairs at p = 1: two blocks of eight and one of seven; the tract ends at the first member of the last pair
    assert both("A" * 24) == (1, 23, 0, 22, 23, 0)


def test_ca_15():
    # 28 pairs at p = 2, all agreeing (p = 4 has 26): three blocks of eight and one of four
    assert both("CA" * 15) == (2, 28, 0, 27, 28, 0)


def test_a_pair_that_does_not_exist():
    # n = 9: the eight pairs of p = 1 fill block 0; n = 10: pair (8, 9) opens block 1, pair (9, 10) does not exist
    assert both("A" * 9, min_score=1) == (1, 8, 0, 7, 8, 0)
    assert both("A" * 10, min_score=1) == (1, 9, 0, 8, 9, 0)


def test_n_counts_for_nothing_and_lower_case_is_its_base():
    # p = 1: (3, 4) and (4, 5) touch the N and are neither agreement nor disagreement; A against a agrees.  p = 2 has 5, p = 5 has 4
    assert both("AAAANaaaa", min_score=1) == (1, 6, 0, 7, 6, 0)
    assert both("AAAACaaaa", min_score=1)[1] < 6          # a C in its place costs


def test_the_scan_restarts_at_running_sum_0():
    # pmax = 1, mm = 3: block 0 has a = 6, d = 1 (+3); block 1 a = 3, d = 2 (-3); block 2 a = 5 (+5).  Blocks 0..2 and block 2
    # alone both sum to 5 and end at block 2: the larger b0 wins, which is the scan beginning anew where the running sum is 0
    s = "AAAAAAACN" + "GGGGTCN" + "TTTTTT" + "N" + "A" + "N"
    assert len(s) == 25
    a, d, sc = pr.blocks(pr.classes(codes(s)), 1, 3)
    assert list(a) == [6, 3, 5] and list(d) == [1, 2, 0] and list(sc) == [3, -3, 5]
    assert both(s, pmax=1, min_score=1) == (1, 5, 16, 23, 5, 0)


def test_two_equal_tracts_of_one_period_the_earlier_end_wins():
    # pmax = 1: block 0 and block 2 hold five agreeing pairs each, block 1 two disagreeing ones
    s = "TTTTTTNAN" + "ACG" + "NNNN" + "TTTTTTNAN"
    assert len(s) == 25
    a, d, sc = pr.blocks(pr.classes(codes(s)), 1, 3)
    assert list(sc) == [5, -6, 5]
    assert both(s, pmax=1, min_score=1) == (1, 5, 0, 7, 5, 0)


def test_equal_scores_at_two_periods_the_smaller_wins():
    # p = 1: (0, 1) and (3, 4) agree; p = 2: (1, 3); p = 3: (0, 3) and (1, 4): 2, 1, 2
    for p, want in ((1, 2), (2, 1), (3, 2)):
        assert pr.best_tract(pr.blocks(pr.classes(codes("AANAA")), p, 3)[2])[0] == want
    assert both("AANAA", min_score=1) == (1, 2, 0, 3, 2, 0)


def test_score_at_and_below_min_score():
    assert both("A" * 24, min_score=23) == (1, 23, 0, 22, 23, 0)
    assert both("A" * 24, min_score=24) == pr.ZERO
    assert both("A" * 17) == (1, 16, 0, 15, 16, 0)       # the default, 16
    assert both("A" * 16) == pr.ZERO


def test_lengths_0_1_2():
    assert both("", min_score=1) == pr.ZERO
    assert both("A", min_score=1) == pr.ZERO
    assert both("AA", min_score=1) == (1, 1, 0, 0, 1, 0)
    assert both("AC", min_score=1) == pr.ZERO
    assert both("AA") == pr.ZERO


def test_periods_beyond_n_minus_1_do_not_exist():
    # n = 8: the periods are 1..7 whatever pmax says; the unit of four shows at p = 4 only
    assert both("ACGTACGT", min_score=1) == (4, 4, 0, 3, 4, 0)
    assert both("ACGTACGT", pmax=7, min_score=1) == (4, 4, 0, 3, 4, 0)
    assert both("ACGTACGT", pmax=8192, min_score=1) == (4, 4, 0, 3, 4, 0)
    assert both("ACGTACGT", pmax=3, min_score=1) == pr.ZERO              # every tract of p = 1..3 is negative


def test_the_length_limit():
    L = _lib.lib()
    out = np.zeros(1, PERIOD_DTYPE)
    x = np.zeros(65537, np.int8)
    ok = _lib.PeriodParams(1, 3, 16, 0)
    assert L.ramx_period_sequence(x.ctypes.data, 65537, C.byref(ok), out.ctypes.data) == ERR_UNSUPPORTED
    assert L.ramx_period_sequence(x.ctypes.data, 65536, C.byref(ok), out.ctypes.data) == 0
    assert tup(out[0]) == (1, 65535, 0, 65534, 65535, 0)


# ---- the host C functions against the restatement ----

def random_segment(rng, n):
    """Random bases with, sometimes, a planted tandem of a random unit, a few N and lower-case bases."""
    x = rng.integers(0, 4, n).astype(np.int8)
    if n > 40 and rng.random() < 0.6:
        u, ln = int(rng.integers(1, 12)), int(rng.integers(12, 40))
        a = int(rng.integers(0, n - ln))
        x[a:a + ln] = np.resize(rng.integers(0, 4, u), ln)
    x[rng.random(n) < 0.04] = 99
    low = (rng.random(n) < 0.1) & (x < 4)
    x[low] += 4
    return x


def test_period_sequence_equals_the_restatement():
    rng = np.random.default_rng(7)
    found = 0
    for t in range(250):
        n = int(rng.choice([0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 257]))
        x = random_segment(rng, n)
        kw = dict(pmax=int(rng.choice([1, 2, 5, 64, 1024])), mm=int(rng.choice([1, 3, 15])), min_score=int(rng.choice([1, 8, 16])))
        got = period_sequence(x, PeriodParams(**kw))
        assert tup(got) == pr.record_of_codes(x, **kw), (t, n, kw)
        found += int(got["period"] > 0)
    assert 30 < found < 220                               # (the inputs are no empty ground: tracts found and not found)


def test_struct_sizes():
    assert PERIOD_SEG_DTYPE.itemsize == 16 and PERIOD_DTYPE.itemsize == 32
    assert C.sizeof(_lib.PeriodParams) == 16 and C.sizeof(_lib.PeriodHist) == 48


def test_segments_on_both_strands_and_empty_extensions():
    cores = CoreSet(left_pos=[100, 260, 400, 50], right_pos=[150, 200, 420, 60], lower=[10, 120, 0, 0], upper=[300, 390, 999, 99],
                    orient=[0, 1, 0, 1], left_ext=[1, 1, 0, 1], right_ext=[1, 1, 1, 1], left_len=[7, 11, 0, 0], right_len=[13, 5, 9, 0])
    want = {0: [(93, 99), (261, 271), (400, 399), (51, 50)],
            1: [(151, 163), (195, 199), (421, 429), (60, 59)],
            2: [(93, 163), (195, 271), (400, 429), (60, 50)]}
    for which in (0, 1, 2):
        got = [(int(s["lo"]), int(s["hi"])) for s in period_segments(cores, which)]
        assert got == want[which] == pr.segments_of(cores, which), which
    assert len(period_segments(cores.subset(slice(0, 0)), 1)) == 0


def test_summary_against_the_restatement():
    rng = np.random.default_rng(9)
    n = 300
    rec = np.zeros(n, PERIOD_DTYPE)
    rec["period"] = rng.choice([0, 0, 1, 1, 2, 2, 2, 5, 6, 7, 7, 7, 171, 8192], n)
    # 2 and 7 tie for the largest count: the smaller is the mode
    n2, n7 = int((rec["period"] == 2).sum()), int((rec["period"] == 7).sum())
    idx = np.nonzero(rec["period"] == (2 if n2 > n7 else 7))[0][:abs(n2 - n7)]
    rec["period"][idx] = 0
    segs = np.zeros(n, PERIOD_SEG_DTYPE)
    segs["lo"] = rng.integers(-5, 10 ** 6, n)
    ln = rng.integers(8200, 9000, n)
    segs["hi"] = segs["lo"] + ln - 1
    has = rec["period"] > 0
    rec["start"] = np.where(has, rng.choice([0, 0, 8, 16], n), 0)
    rec["end"] = np.where(has, np.where(rng.random(n) < 0.4, ln - rec["period"] - 1, rec["start"] + 3), 0)
    got = period_summary(rec, segs)
    want = pr.summary([tup(r) for r in rec], [(int(s["lo"]), int(s["hi"])) for s in segs])
    assert {k: getattr(got, k) for k in want} == want
    assert want["mode"] == 2 and want["n_mono"] > 0 and want["n_simple"] > 0 and want["n_tandem"] > 0 and 0 < want["at_lo"] < want["n_tract"]
    assert 0 < want["at_hi"] < want["n_tract"] and want["n_tract"] == want["n_mono"] + want["n_simple"] + want["n_tandem"] < n
    empty = period_summary(np.zeros(0, PERIOD_DTYPE), np.zeros(0, PERIOD_SEG_DTYPE))
    assert (empty.n, empty.n_tract, empty.mode, empty.mode_count) == (0, 0, 0, 0)
    # a record without a period counts nowhere, whatever its other fields say
    z = np.zeros(2, PERIOD_DTYPE)
    zs = np.array([(5, 5), (5, 4)], PERIOD_SEG_DTYPE)
    s = period_summary(z, zs)
    assert (s.n, s.n_tract, s.at_lo, s.at_hi) == (2, 0, 0, 0)


def test_every_argument_error():
    L = _lib.lib()
    ok = _lib.PeriodParams(1024, 3, 16, 0)
    h = _lib.PeriodHist()
    rec = np.zeros(4, PERIOD_DTYPE)
    segs = np.zeros(4, PERIOD_SEG_DTYPE)
    out = np.full(8, 7, np.int32).view(PERIOD_DTYPE)
    x = codes("ACGTACGTAC")
    bad_params = [(0, 3, 16), (-1, 3, 16), (8193, 3, 16), (1024, 0, 16), (1024, 16, 16), (1024, -3, 16), (1024, 3, 0), (1024, 3, -5)]
    for bad in bad_params:
        bp = _lib.PeriodParams(*bad, 0)
        assert L.ramx_period_sequence(x.ctypes.data, 10, C.byref(bp), out.ctypes.data) == ERR_ARG, bad
        assert L.ramx_period_summary(rec.ctypes.data, segs.ctypes.data, 4, C.byref(bp), C.byref(h)) == ERR_ARG, bad
    assert (out.view(np.int32) == 7).all()                # raised before anything is written
    for good in [(1, 1, 1), (8192, 15, 1 << 30)]:
        assert L.ramx_period_sequence(x.ctypes.data, 10, C.byref(_lib.PeriodParams(*good, 0)), out.ctypes.data) == 0, good
    assert L.ramx_period_sequence(x.ctypes.data, 10, None, out.ctypes.data) == ERR_ARG
    assert L.ramx_period_sequence(x.ctypes.data, -1, C.byref(ok), out.ctypes.data) == ERR_ARG
    assert L.ramx_period_sequence(None, 10, C.byref(ok), out.ctypes.data) == ERR_ARG
    assert L.ramx_period_sequence(x.ctypes.data, 10, C.byref(ok), None) == ERR_ARG
    assert L.ramx_period_sequence(None, 0, C.byref(ok), out.ctypes.data) == 0
    assert L.ramx_period_summary(rec.ctypes.data, segs.ctypes.data, 4, None, C.byref(h)) == ERR_ARG
    assert L.ramx_period_summary(rec.ctypes.data, segs.ctypes.data, -1, C.byref(ok), C.byref(h)) == ERR_ARG
    assert L.ramx_period_summary(None, segs.ctypes.data, 4, C.byref(ok), C.byref(h)) == ERR_ARG
    assert L.ramx_period_summary(rec.ctypes.data, None, 4, C.byref(ok), C.byref(h)) == ERR_ARG
    assert L.ramx_period_summary(rec.ctypes.data, segs.ctypes.data, 4, C.byref(ok), None) == ERR_ARG
    for p in (-1, 8193):
        rec["period"][2] = p
        assert L.ramx_period_summary(rec.ctypes.data, segs.ctypes.data, 4, C.byref(ok), C.byref(h)) == ERR_ARG
    assert L.ramx_period_summary(rec.ctypes.data, segs.ctypes.data, 2, C.byref(ok), C.byref(h)) == 0
    cores = CoreSet(left_pos=[100], right_pos=[150], lower=[10], upper=[300], orient=[0], left_ext=[1], right_ext=[1])
    from repeatafterme_amd.extend import _flat_cores
    fc = _flat_cores(cores)
    for which in (-1, 3):
        assert L.ramx_period_segments(C.byref(fc), which, segs.ctypes.data) == ERR_ARG
    assert L.ramx_period_segments(None, 0, segs.ctypes.data) == ERR_ARG
    assert L.ramx_period_segments(C.byref(fc), 0, None) == ERR_ARG
    assert L.ramx_period_segments(C.byref(fc), 2, segs.ctypes.data) == 1


# ---- a planted family on the CPU oracle ----

def test_planted_family_shows_its_ca_repeat():
    """Every copy's right extension is a conserved tail followed by a (CA)n of its own length: on the oracle's extents the
    restatement alone finds period 2 in at least half the copies, and nothing of the kind on the left."""
    e = pr.planted_expectation()
    M = pr.PLANTED["M"]
    assert e["rets"][1] > 150 and e["rets"][0] > 100
    right = pr.summary(e["records"][1], e["segs"][1])
    left = pr.summary(e["records"][0], e["segs"][0])
    whole = pr.summary(e["records"][2], e["segs"][2])
    print("planted family: right", right, "left", left, "whole", whole)
    assert right["mode"] == 2 and 2 * right["mode_count"] >= M
    assert whole["mode"] == 2 and 2 * whole["mode_count"] >= M
    assert left["n_tract"] == 0
    # the tracts are the planted repeats: none longer than the copy's own (CA)n and a block of eight at either end, most of
    # them most of it
    spans = [r[3] + r[0] - r[2] + 1 for r in e["records"][1]]
    assert all(s <= run + 16 for s, run in zip(spans, e["runs"]) if s)
    assert sum(2 * s >= run for s, run in zip(spans, e["runs"])) * 2 >= M
    seg = np.array(e["segs"][1], np.int64).view(PERIOD_SEG_DTYPE).reshape(-1)
    rec = np.zeros(M, PERIOD_DTYPE)
    for i, r in enumerate(e["records"][1]):
        rec[i] = r + ([0, 0],)
    got = period_summary(rec, seg)
    assert {k: getattr(got, k) for k in right} == right
    # the host function on the oracle's kept consensus of the right extension sees it too
    p = e["p"]
    cons = e["master"][p.L + 1:p.L + 1 + e["rets"][1]]
    assert tup(period_sequence(cons))[0] == 2 and tup(period_sequence(cons)) == pr.record_of_codes(cons)
