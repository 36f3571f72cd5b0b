"""The target-site duplication contract (include/ramx.h, ramx_tsd) on the CPU: the brute-force restatement (tests/tsd_ref.py) on
hand-made sites with literal records, the host C functions of libramx.so (ramx_tsd_sites, ramx_tsd_summary, ramx_termini)
through ctypes, and a planted family on the CPU oracle.  No GPU."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from repeatafterme_amd import _lib
from repeatafterme_amd.datamodel import TSD_DTYPE, TSD_SITE_DTYPE, CoreSet, TsdParams
from repeatafterme_amd.extend import termini, tsd_sites, tsd_summary

import tsd_ref as tr

ERR_ARG = -103
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 4, "c": 5, "g": 6, "t": 7, "N": 99}


def codes(s):
    return np.array([CODE[ch] for ch in s], np.int8)


def site_of(left, elem, right, lo_off=0, hi_off=0, seq_lo=None, seq_hi=None):
    """left + elem + right as a library with the element where elem is (ends moved by the offsets)."""
    lib = codes(left + elem + right)
    lo, hi = len(left), len(left) + len(elem) - 1
    return lib, (lo + lo_off, hi + hi_off, 0 if seq_lo is None else seq_lo, len(lib) - 1 if seq_hi is None else seq_hi)


A24, C24 = "A" * 24, "C" * 24
ELEM = "GGATGCAAGTCTTGAACGTACAGTGG"       # begins and ends with GG: no word of these tests continues into it


def test_exact_5mer_at_shift_0():
    lib, site = site_of(A24 + "TCAGT", ELEM, "TCAGT" + C24)
    assert tr.tsd(lib, site) == (5, 0, 0, 0)


def test_termini_off_by_plus2_minus1():
    # the reported element begins two bases early and ends one base late: the shifts find the true ends
    lib, site = site_of(A24 + "TCAGT", ELEM, "TCAGT" + C24, lo_off=-2, hi_off=+1)
    assert tr.tsd(lib, site) == (5, 0, 2, -1)


def test_12mer_with_one_mismatch_accepted_at_10_refused_at_0():
    lib, site = site_of(A24 + "TCAGTTGACCAG", ELEM, "TCTGTTGACCAG" + C24)     # base 2 differs
    assert tr.tsd(lib, site, mm_div=10) == (12, 1, 0, 0)
    # without mismatches the nine bases behind it are the word: the right one begins three bases later
    assert tr.tsd(lib, site, mm_div=0) == (9, 0, 0, 3)


def test_mismatch_on_the_last_base_yields_the_shorter_word():
    # one mismatch is allowed in 12, but not on an end (ii): the first eleven bases are the word, the left one ends a base early
    lib, site = site_of(A24 + "TCAGTTGACCAG", ELEM, "TCAGTTGACCAT" + C24)
    assert tr.tsd(lib, site) == (11, 0, -1, 0)


def test_n_inside_a_word_agrees_with_nothing():
    lib, site = site_of(A24 + "TCAGTNGACCAG", ELEM, "TCAGTNGACCAG" + C24)     # N against N
    assert tr.tsd(lib, site) == (12, 1, 0, 0)
    assert tr.tsd(lib, site, mm_div=0)[1] == 0


def test_lower_case_is_its_base():
    lib, site = site_of(A24 + "TCAGT", ELEM, "tcagt" + C24)
    assert tr.tsd(lib, site) == (5, 0, 0, 0)


def test_word_cut_by_seq_lo():
    # eight bases repeat, but the core's bounds begin five bases in front of the element: only those five can be a word
    lib, site = site_of(A24 + "GTCATCAG", ELEM, "GTCATCAG" + C24)
    assert tr.tsd(lib, site) == (8, 0, 0, 0)
    cut = (site[0], site[1], site[0] - 5, site[3])
    assert tr.tsd(lib, cut) == (5, 0, 0, 3)


def test_lo_at_position_0():
    lib, site = site_of("", ELEM, "TCAGT" + C24)
    assert site[0] == 0 and tr.tsd(lib, site) == (0, 0, 0, 0)


def test_empty_element():
    lib, site = site_of(A24 + "TCAGT", "", "TCAGT" + C24)
    assert site[0] == site[1] + 1 and tr.tsd(lib, site) == (5, 0, 0, 0)
    # (i): the left word may not end behind the beginning of the right one
    assert all(-c[3] <= -c[4] for c in tr.candidates(lib, site))


def test_tie_goes_to_the_smaller_shift():
    # TTTTT at (0, 0) and TTTTTT at (+1, -1) through the element's T ends: both q = 10
    lib, site = site_of(A24 + "TTTTT", "TG" + ELEM + "GT", "TTTTT" + C24)
    c = tr.candidates(lib, site)
    assert (10, 0, 5, 0, 0, 0) in c and (10, -2, 6, -1, 1, 0) in c and max(c)[0] == 10
    assert tr.tsd(lib, site) == (5, 0, 0, 0)


def test_tie_goes_to_the_longer_word():
    # twelve bases with one mismatch and the ten exact ones among them: both q = 20 at (0, 0)
    lib, site = site_of(A24 + "GAGTGTGTGTGT", "TT" + ELEM + "TT", "GTGTGTGTGTGT" + C24)
    c = tr.candidates(lib, site)
    assert (20, 0, 12, 0, 0, 1) in c and (20, 0, 10, 0, 0, 0) in c and max(c)[0] == 20
    assert tr.tsd(lib, site) == (12, 1, 0, 0)


def test_tie_goes_to_the_smaller_dl():
    # six bases repeat and five is the longest word looked for: (-1, 0) and (0, +1) both give q = 9
    lib, site = site_of(A24 + "TCAGTG", ELEM, "TCAGTG" + C24)
    c = tr.candidates(lib, site, kmax=5)
    assert (9, -1, 5, 1, 0, 0) in c and (9, -1, 5, 0, -1, 0) in c and max(c)[0] == 9
    assert tr.tsd(lib, site, kmax=5) == (5, 0, -1, 0)


def test_tie_goes_to_the_smaller_dr():
    # GTGTG in front, GTGTGTG from the element's last base on: (0, -1) and (0, +1) both give q = 9
    lib, site = site_of(A24 + "GTGTG", ELEM + "CG", "TGTGTG" + C24)
    c = tr.candidates(lib, site)
    assert (9, -1, 5, 0, 1, 0) in c and (9, -1, 5, 0, -1, 0) in c and max(c)[0] == 9
    assert tr.tsd(lib, site) == (5, 0, 0, -1)


# ---- the host C functions ----

def test_struct_sizes():
    assert TSD_SITE_DTYPE.itemsize == 32 and TSD_DTYPE.itemsize == 16 and C.sizeof(_lib.TsdParams) == 16
    assert C.sizeof(_lib.TsdHist) == 33 * 4 + 12 + 33 * 8 and _lib.TsdHist.null.offset == 144


def test_sites_on_both_strands():
    cores = CoreSet(left_pos=[100, 260, 400], right_pos=[150, 200, 420], lower=[10, 120, 0], upper=[300, 390, 999], orient=[0, 1, 0],
                    left_ext=[1, 1, 0], right_ext=[1, 1, 1], left_len=[7, 11, 0], right_len=[13, 5, 9])
    s = tsd_sites(cores)
    assert [tuple(int(v) for v in r) for r in s] == [(100 - 7, 150 + 13, 10, 300), (200 - 5, 260 + 11, 120, 390), (400, 429, 0, 999)]
    assert [tuple(int(v) for v in r) for r in s] == tr.sites_of(cores)
    assert len(tsd_sites(cores.subset(slice(0, 0)))) == 0


@pytest.mark.parametrize("params", [dict(), dict(slack=0, kmin=1, kmax=32, mm_div=4), dict(slack=7, kmin=32, kmax=32, mm_div=0)])
def test_summary_against_fractions(params):
    rng = np.random.default_rng(5)
    rec = np.zeros(200, TSD_DTYPE)
    rec["k"] = rng.choice([0, 0, 4, 5, 5, 5, 8, 8, 8, 20, 32], 200)
    # make 5 and 8 tie for the largest count: the larger k is the mode
    n5, n8 = int((rec["k"] == 5).sum()), int((rec["k"] == 8).sum())
    idx = np.nonzero(rec["k"] == (5 if n5 > n8 else 8))[0][:abs(n5 - n8)]
    rec["k"][idx] = 0
    tp = TsdParams(**{**tr.DEFAULT, **params})
    got = tsd_summary(rec, tp)
    hist, mode, count, null = tr.summary([(int(k),) for k in rec["k"]], **{**tr.DEFAULT, **params})
    assert list(got.hist) == hist and got.mode == mode == 8 and got.mode_count == count
    for k in range(33):
        want = float(null[k])
        assert abs(got.null[k] - want) <= 1e-12 * abs(want), (k, got.null[k], want)
    assert any(Fraction(0) < null[k] < len(rec) for k in range(1, 33)) or tp.slack == 7
    empty = tsd_summary(np.zeros(0, TSD_DTYPE), tp)
    assert empty.mode == 0 and empty.mode_count == 0 and not empty.hist.any() and not empty.null.any()


def test_termini_on_literal_strings():
    # left rows run outward from the core: the extended consensus begins with the last of them
    left = codes("GATTACA")            # reading order: ACATTAG
    right = codes("CCGTCTAATGT")       # its reverse complement begins ACATTAG: an inverted repeat of 7, stopped by the length of the left
    assert termini(left, right, 4) == ("ACAT", "ATGT", 7)
    assert termini(left, right, 32) == ("ACATTAG", "CCGTCTAATGT", 7)
    assert termini(codes("GATTACA"), codes("CCGTCTAAGGT"), 3) == ("ACA", "GGT", 2)       # stops at the first failure
    assert termini(codes(""), right, 5) == ("", "TAATGT"[1:], 0)
    assert termini(left, right, 0) == ("", "", 7)
    long = codes("ACGT" * 12)
    assert termini(long, (3 - long).astype(np.int8), 2)[2] == 32                         # never more than 32


def test_every_argument_error():
    L = _lib.lib()
    ok = _lib.TsdParams(3, 4, 20, 10)
    h = _lib.TsdHist()
    rec = np.zeros(4, TSD_DTYPE)
    for bad in [(-1, 4, 20, 10), (8, 4, 20, 10), (3, 0, 20, 10), (3, 33, 33, 10), (3, 6, 5, 10), (3, 4, 33, 10), (3, 4, 20, 3), (3, 4, 20, -1)]:
        assert L.ramx_tsd_summary(rec.ctypes.data, 4, C.byref(_lib.TsdParams(*bad)), C.byref(h)) == ERR_ARG, bad
    assert L.ramx_tsd_summary(rec.ctypes.data, 4, None, C.byref(h)) == ERR_ARG
    assert L.ramx_tsd_summary(rec.ctypes.data, -1, C.byref(ok), C.byref(h)) == ERR_ARG
    assert L.ramx_tsd_summary(None, 4, C.byref(ok), C.byref(h)) == ERR_ARG
    assert L.ramx_tsd_summary(rec.ctypes.data, 4, C.byref(ok), None) == ERR_ARG
    rec["k"][2] = 33
    assert L.ramx_tsd_summary(rec.ctypes.data, 4, C.byref(ok), C.byref(h)) == ERR_ARG
    rec["k"][2] = -1
    assert L.ramx_tsd_summary(rec.ctypes.data, 4, C.byref(ok), C.byref(h)) == ERR_ARG
    assert L.ramx_tsd_summary(rec.ctypes.data, 2, C.byref(ok), C.byref(h)) == 0
    assert L.ramx_tsd_sites(None, None) == ERR_ARG
    five, three, tir = C.create_string_buffer(8), C.create_string_buffer(8), C.c_int32()
    a = codes("ACGT")
    assert L.ramx_termini(a.ctypes.data, 4, a.ctypes.data, 4, -1, five, three, C.byref(tir)) == ERR_ARG
    assert L.ramx_termini(a.ctypes.data, -1, a.ctypes.data, 4, 4, five, three, C.byref(tir)) == ERR_ARG
    assert L.ramx_termini(None, 4, a.ctypes.data, 4, 4, five, three, C.byref(tir)) == ERR_ARG
    assert L.ramx_termini(a.ctypes.data, 4, a.ctypes.data, 4, 4, None, three, C.byref(tir)) == ERR_ARG
    assert L.ramx_termini(a.ctypes.data, 4, a.ctypes.data, 4, 4, five, three, None) == ERR_ARG
    assert L.ramx_termini(a.ctypes.data, 4, a.ctypes.data, 4, 4, five, three, C.byref(tir)) == 0


# ---- a planted family on the CPU oracle ----

def test_planted_family_shows_its_duplication():
    e = tr.planted_expectation()
    k, M = tr.PLANTED["k"], tr.PLANTED["M"]
    assert e["rets"][1] > 100 and e["rets"][0] > 100                 # both directions extended to the ends of the element
    hist, mode, count, null = tr.summary(e["records"])
    print("planted family: hist", {i: v for i, v in enumerate(hist) if v}, "mode", mode, count, "null[k]", float(null[k]),
          "exact ends", sum((s[0], s[1]) == w for s, w in zip(e["sites"], e["where"])))
    assert mode == k
    assert 2 * hist[k] >= M
    assert count > null[k]
    got = tsd_summary(np.array(e["records"], np.int32).view(TSD_DTYPE).reshape(-1))
    assert got.mode == k and got.mode_count == count
