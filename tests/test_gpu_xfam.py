"""Pairs of sequences on the device (C-ABI ramx_dev_seq_pairs, include/ramx_xfam.h): every field of every record against the
restatement (tests/term_ref.py through tests/xfam_ref.py) where both lengths are at most 1,500 and against ramx_seq_pair_host,
which tests/test_xfam_ref.py pins, beyond.  RAMX_XFAM_COLS chooses the kernel's specialisation (4, 8 or 16 columns a lane; a
strip is S = 64 C columns), so every one of them meets every edge of its strips."""
import ctypes as C
import os

import numpy as np
import pytest

from repeatafterme_amd import _lib, xfam
from repeatafterme_amd.datamodel import SEQ_PAIR_DTYPE, TERM_DTYPE, PairParams, new_master

import term_ref as tr
import xfam_ref as xr
from helpers import to_extend_params
from test_term_ref import codes

pytestmark = pytest.mark.gpu

ERR_ARG = -103
ERR_STATE = -104
ERR_UNSUPPORTED = -106
COLS = (4, 8, 16)
N = 99                      # a code of class 4
ONE = dict(match=2, mismatch=3, gap=5, min_score=1)


def tup(r):
    return tuple(int(r[k]) for k in tr.FIELDS)


def given(bprime):
    """The B whose inverted reading is bprime: reversed, the classes below 4 complemented."""
    b = np.asarray(bprime, np.int8)[::-1].copy()
    c = tr.classes(b)
    return np.where(c < 4, 3 - c, b).astype(np.int8)


def expected(a, b, inv, params):
    if max(len(a), len(b)) <= 1500:
        return xr.record(a, b, inv, **params)
    return tup(xfam.seq_pair_host(a, b, inv, PairParams(**params))[0])


class cols:
    """RAMX_XFAM_COLS for the calls inside (read per call)."""
    def __init__(self, c):
        self.c = c

    def __enter__(self):
        self.old = os.environ.get("RAMX_XFAM_COLS")
        if self.c is None:
            os.environ.pop("RAMX_XFAM_COLS", None)
        else:
            os.environ["RAMX_XFAM_COLS"] = str(self.c)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("RAMX_XFAM_COLS", None)
        else:
            os.environ["RAMX_XFAM_COLS"] = self.old


@pytest.fixture(scope="module")
def dev():
    from repeatafterme_amd.device import Device
    d = Device(0)
    yield d
    d.close()


def run(dev, cases, params, c=None):
    """cases: (a, b, inverted).  One call of all of them with c columns a lane -> the records as tuples."""
    seqs, pairs = [], []
    for a, b, inv in cases:
        pairs.append((len(seqs), len(seqs) + 1, inv))
        seqs += [a, b]
    with cols(c):
        got = xfam.seq_pairs(seqs, pairs, PairParams(**params), device=dev)
    return [tup(r) for r in got]


def check(dev, cases, params, c=None):
    got = run(dev, cases, params, c)
    for k, (case, g) in enumerate(zip(cases, got)):
        want = expected(*case, params)
        assert g == want, (k, len(case[0]), len(case[1]), case[2], g, want)
    return got


def related(rng, na, nb, letters):
    """Two sequences cut from one source and diverged on their own (substitutions, indels, a class-4 base now and then)."""
    src = rng.integers(0, letters, max(na, nb) + 40).astype(np.int8)

    def cut(n):
        at = int(rng.integers(0, 20))
        s = list(src[at:at + n + 20])
        out = []
        for x in s:
            u = rng.random()
            if u < 0.02:
                continue
            if u < 0.04:
                out.append(int(rng.integers(0, letters)))
            out.append(int((x + 1) % letters) if u > 0.93 else int(x))
        out = np.array((out + [0] * n)[:n], np.int8)
        out[rng.random(n) < 0.01] = N
        return out
    return cut(na), cut(nb)


@pytest.mark.parametrize("inv", (0, 1))
@pytest.mark.parametrize("transposed", (False, True))
@pytest.mark.parametrize("c", COLS)
def test_every_edge_of_a_strip(dev, c, transposed, inv):
    S = 64 * c
    rng = np.random.default_rng(100 * c + 2 * transposed + inv)
    cases = []
    for nb in (1, 2, c - 1, c, c + 1, 63 * c, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1):
        for na in (1, 2, 63, 64, 65, 300):
            a, b = related(rng, na, nb, 2 if (na + nb) % 2 else 4)         # two letters: ties everywhere
            cases.append((b, a, inv) if transposed else (a, b, inv))
    check(dev, cases, ONE, c)


def planted_across(c, at, gap_a=0, gap_b=0, n_run=0, seed=0):
    """a: 160 bases.  B': class 4 everywhere but a copy of a that begins at column `at` (0-based), with gap_b extra bases in B'
    (a gap in a) or gap_a bases of a left out, in its middle, substitutions, and a class-4 run of n_run at its middle + 10."""
    rng = np.random.default_rng(seed + 7 * c)
    a = rng.integers(0, 4, 160).astype(np.int8)
    copy = a.copy()
    hit = rng.random(160) < 0.05
    copy[hit] = (copy[hit] + 1) % 4
    mid = np.concatenate((copy[:80], rng.integers(0, 4, gap_b).astype(np.int8), copy[80 + gap_a:]))
    if n_run:
        mid[90:90 + n_run] = N
    bp = np.concatenate((np.full(at, N, np.int8), mid, np.full(40, N, np.int8)))
    return a, bp


@pytest.mark.parametrize("c", COLS)
def test_alignments_gaps_and_class_4_runs_across_a_border(dev, c):
    S = 64 * c
    cheap = dict(match=15, mismatch=15, gap=1, min_score=1)                 # a long gap is affordable
    for params, kw in ((ONE, dict()), (ONE, dict(gap_a=2)), (ONE, dict(gap_b=1)), (cheap, dict(gap_b=c + 3)), (cheap, dict(gap_a=c + 3)),
                       (ONE, dict(n_run=7)), (cheap, dict(gap_b=c + 3, n_run=5))):
        cases = []
        for k, at in enumerate((S - 80 - (c + 3) // 2, S - 92, 2 * S - 81, S - 160, S)):
            a, bp = planted_across(c, at, seed=at, **kw)
            cases += [(a, bp, 0), (a, given(bp), 1)] + ([(bp, a, 0)] if k < 2 else [])
        got = check(dev, cases, params, c)
        assert all(g[0] > 100 for g in got)
        if kw.get("gap_a") or kw.get("gap_b"):
            assert any(g[6] > g[5] and g[2] - g[1] != g[4] - g[3] for g in got)     # a gapped alignment was found


@pytest.mark.parametrize("c", COLS)
def test_best_cell_ties_across_strips(dev, c):
    S = 64 * c
    P, Q = codes("ACGGTCATGATTCCTAGTGC"), codes("TTGACCAGTCAAGGCATCCA")
    fill = lambda n: np.full(n, N, np.int8)
    a = np.concatenate((P, fill(1), Q))
    cases, want = [], []
    # Q in the first strip, P in the second: the cells (20, S + 30) and (41, 25) hold 40; the smaller i is in the later strip
    bp = np.concatenate((fill(5), Q, fill(S - 15), P, fill(3)))
    cases += [(a, bp, 0), (a, given(bp), 1)]
    want += [(40, 0, 19, S + 10, S + 29, 20, 20, 41)] * 2
    # ... and the other way round: the later strip must not take over with an equal score in a later row
    bp = np.concatenate((fill(5), P, fill(S - 15), Q, fill(3)))
    cases += [(a, bp, 0), (a, given(bp), 1)]
    want += [(40, 0, 19, 5, 24, 20, 20, 41)] * 2
    # a tie in j across a border: P twice in B', one copy ending in each strip, the same row
    bp = np.concatenate((fill(S - 30), P, fill(40), P, fill(2)))
    cases += [(P, bp, 0), (P, given(bp), 1)]
    want += [(40, 0, 19, S - 30, S - 11, 20, 20, 20)] * 2
    # ... and in three strips, the first copy in the second one
    bp = np.concatenate((fill(S + 7), P, fill(S), P, fill(2)))
    cases += [(P, bp, 0), (P, given(bp), 1)]
    want += [(40, 0, 19, S + 7, S + 26, 20, 20, 20)] * 2
    # the last column of a strip and the first of the next hold the best cells of two rows
    bp = np.concatenate((fill(S - 20), Q, P, fill(2)))
    cases += [(a, bp, 0), (np.concatenate((Q, fill(20), P)), bp, 0)]
    want += [(40, 0, 19, S, S + 19, 20, 20, 41), (40, 0, 19, S - 20, S - 1, 20, 20, 60)]
    got = check(dev, cases, ONE, c)
    assert got == want


@pytest.mark.parametrize("c", COLS)
def test_d_before_u_before_l_in_the_first_column_of_a_strip(dev, c):
    """The three cases of tests/test_term_ref.py (match 2, mismatch 1, gap 1), B' shifted so that the cell where two of D, U, L
    are equal -- column 2, 2 and 3 of the word -- is column S + 1, the first of the second strip: its L comes from the border."""
    S = 64 * c
    s = dict(match=2, mismatch=1, gap=1, min_score=1)
    fill = lambda n: np.full(n, N, np.int8)
    cases, want = [], []
    for a, b, col, rec in (("AAAC", "ACAC", 2, (5, 0, 3, 0, 3, 3, 4, 4)), ("ACAC", "AAAC", 2, (5, 0, 3, 0, 3, 3, 4, 4)),
                           ("ACAC", "CAAC", 3, (5, 0, 3, 1, 3, 3, 4, 4))):
        assert xr.record(codes(a), codes(b), 0, **s) == rec
        for shift in (S + 1 - col, 2 * S + 1 - col, S - col, S + 2 - col):
            bp = np.concatenate((fill(shift), codes(b), fill(3)))
            cases += [(codes(a), bp, 0), (codes(a), given(bp), 1)]
            want += [(rec[0], rec[1], rec[2], rec[3] + shift, rec[4] + shift, rec[5], rec[6], 4)] * 2
    assert check(dev, cases, s, c) == want


def test_the_longest_sequences_and_a_square(dev):
    rng = np.random.default_rng(5)
    long_ = rng.integers(0, 4, 32767).astype(np.int8)
    short = long_[20000:20600].copy()
    hit = rng.random(600) < 0.1
    short[hit] = (short[hit] + 1) % 4
    short = np.concatenate((short[:300], short[304:]))
    sq_a = rng.integers(0, 4, 3000).astype(np.int8)
    sq_b = np.concatenate((rng.integers(0, 4, 900).astype(np.int8), sq_a[500:2500], rng.integers(0, 4, 100).astype(np.int8)))
    hit = rng.random(3000) < 0.08
    sq_b[hit] = (sq_b[hit] + 2) % 4
    p = dict(match=2, mismatch=3, gap=5, min_score=80)
    cases = [(long_, short, 0), (short, long_, 0), (long_, given(short), 1), (given(short), long_, 1), (sq_a, sq_b, 0), (sq_a, given(sq_b), 1)]
    got = check(dev, cases, p)
    assert all(g[0] > 500 for g in got) and got[0][2] >= 20590 and got[1][4] >= 20590 and got[4][6] > 1900
    # the end of the longest A and of the longest B': the last rows and columns are cells too
    tail = long_[-50:].copy()
    got = check(dev, [(long_, tail, 0), (tail, long_, 0)], ONE)
    assert got[0][:5] == (100, 32717, 32766, 0, 49) and got[1][:5] == (100, 0, 49, 32717, 32766)


_mixed = {}


def mixed_pairs():
    """130 pairs of mixed sizes on 260 sequences of their own, with what the restatement gives for them (once per process)."""
    if not _mixed:
        rng = np.random.default_rng(77)
        cases = []
        for k in range(130):
            na = int(rng.integers(1, 150)) if k % 13 else int(rng.integers(300, 700))
            nb = int(rng.integers(1, 150)) if k % 11 else int(rng.integers(257, 1100))
            a, b = related(rng, na, nb, 4 if k % 3 else 2)
            cases.append((a, b, k % 2))
        p = dict(match=2, mismatch=3, gap=5, min_score=12)
        _mixed.update(cases=cases, params=p, want=[expected(*c, p) for c in cases])
    return _mixed


@pytest.mark.parametrize("n", (1, 2, 3, 4, 5, 7, 8, 9, 127, 128, 129, 130))
def test_any_number_of_pairs_in_one_call(dev, n):
    m = mixed_pairs()
    assert run(dev, m["cases"][:n], m["params"]) == m["want"][:n]


def test_the_groups_of_a_small_budget_do_not_show(dev):
    m = mixed_pairs()
    # what the header counts for a pair with two sequences of its own
    need = [16 * len(a) + 80 + (len(a) + 15) // 16 * 16 + (len(b) + 15) // 16 * 16 for a, b, _ in m["cases"]]
    budget = max(max(need), sum(need) // 4)                                 # every group holds at most a quarter: four or more groups
    assert sum(need) >= 3 * budget
    old = os.environ.get("RAMX_XFAM_BYTES")
    os.environ["RAMX_XFAM_BYTES"] = str(budget)
    try:
        assert run(dev, m["cases"], m["params"]) == m["want"]
        # one pair alone does not fit
        os.environ["RAMX_XFAM_BYTES"] = str(max(need) - 1)
        with pytest.raises(_lib.RamxError, match="-106"):
            run(dev, m["cases"], m["params"])
    finally:
        if old is None:
            os.environ.pop("RAMX_XFAM_BYTES", None)
        else:
            os.environ["RAMX_XFAM_BYTES"] = old
    assert sum(w[0] > 0 for w in m["want"]) > 60 and sum(w[0] == 0 for w in m["want"]) > 5


def test_empty_sides_timing_and_shared_sequences(dev):
    rng = np.random.default_rng(9)
    s = [rng.integers(0, 4, 200).astype(np.int8), np.zeros(0, np.int8), None, np.zeros(0, np.int8)]
    s[2] = np.concatenate((s[0][50:150], tr.revcomp(s[0][20:90])))
    pairs = [(0, 1, 0), (0, 2, 0), (2, 0, 1), (1, 3, 1), (2, 0, 0), (3, 2, 0), (0, 2, 1)]
    p = dict(match=2, mismatch=3, gap=5, min_score=80)
    got, ms = xfam.seq_pairs(s, pairs, PairParams(**p), device=dev, timing=True)
    assert [tup(r) for r in got] == [xr.record(s[a], s[b], inv, **p) for a, b, inv in pairs]
    assert tup(got[0]) == tup(got[3]) == tup(got[5]) == (0,) * 8 and got[1]["score"] >= 200 and got[6]["score"] >= 140 and ms > 0


def test_no_pair_and_every_refusal(dev):
    L = _lib.lib()
    seqs = [codes("ACGGTCATGATTCCTA"), codes("ACGGTCATGATTCCTA"), np.zeros(40000, np.int8)]
    cds, off = xfam._flatten(seqs)
    good = (2, 3, 5, 8)
    ok = C.byref(_lib.PairParams(*good))
    out = np.full(8 * 4, 7, np.int32).view(TERM_DTYPE)
    pa = np.zeros(4, SEQ_PAIR_DTYPE)
    pa["b"] = 1

    def call(pairs=pa, n=4, pp=ok, o=off, c=cds.ctypes.data, res=out.ctypes.data, ns=3):
        return L.ramx_dev_seq_pairs(dev._h, c, o.ctypes.data if o is not None else None, ns, pairs.ctypes.data if pairs is not None else None,
                                    n, pp, res, None)
    for field, values in {0: (0, 16), 1: (0, 16), 2: (0, 32), 3: (0, -1)}.items():
        for v in values:
            bad = list(good)
            bad[field] = v
            assert call(pp=C.byref(_lib.PairParams(*bad))) == ERR_ARG, bad
    assert call(pp=None) == ERR_ARG and call(n=-1) == ERR_ARG and call(pairs=None) == ERR_ARG and call(res=None) == ERR_ARG
    assert call(o=None) == ERR_ARG and call(c=None) == ERR_ARG and call(ns=-1) == ERR_ARG
    for field, v in (("a", -1), ("a", 3), ("b", -1), ("b", 3), ("a", 1), ("inverted", 2), ("inverted", -1), ("reserved", 1)):
        bad = pa.copy()
        bad[field][2] = v
        assert call(pairs=bad) == ERR_ARG, (field, v)
    assert call(o=np.array([0, 16, 8, 40032], np.int64)) == ERR_ARG
    bad = pa.copy()
    bad["b"][3] = 2
    assert call(pairs=bad) == ERR_UNSUPPORTED
    # raised before anything is written
    assert (out.view(np.int32) == 7).all()
    # no pair: nothing is read, nothing is launched
    assert call(n=0, pairs=None, res=None) == 0 and (out.view(np.int32) == 7).all()
    assert call() == 0 and [tup(r) for r in out] == [(32, 0, 15, 0, 15, 16, 16, 16)] * 4
    # a sequence above the limit that no pair uses is nobody's business
    assert call(n=2) == 0


def test_the_process_wide_session_and_a_real_extension_after_it(dev):
    """d == NULL is seam 1's session: a large call, a small one on the buffers it left, then both directions of a planted family
    through seam 1 on the same session, against the CPU oracle."""
    from repeatafterme_amd.extend import extend_alignment
    m = mixed_pairs()
    rng = np.random.default_rng(2)
    big = rng.integers(0, 4, 9000).astype(np.int8)
    p = PairParams(**m["params"])
    first = xfam.seq_pairs([big, big[100:8000]], [(0, 1, 0)], p)
    assert tup(first[0]) == (15800, 100, 7999, 0, 7899, 7900, 7900, 7900)
    seqs, pairs = [], []
    for a, b, inv in m["cases"][:9]:
        pairs.append((len(seqs), len(seqs) + 1, inv))
        seqs += [a, b]
    assert [tup(r) for r in xfam.seq_pairs(seqs, pairs, p)] == m["want"][:9]
    e = tr.planted_expectation("TIR")
    c, mm = e["cores"].copy(), new_master(e["p"].L)
    rets = {d: extend_alignment(d, c, e["seq"], mm, to_extend_params(e["p"])).ret for d in (1, 0)}
    assert rets == e["rets"] and np.array_equal(c.left_len, e["after"].left_len) and np.array_equal(c.right_len, e["after"].right_len)
    assert np.array_equal(mm, e["master"])
    assert [tup(r) for r in xfam.seq_pairs(seqs, pairs, p)] == m["want"][:9]


def test_a_direction_needs_a_new_begin_after_a_call():
    from repeatafterme_amd.device import Device, resolve_flanks
    e = tr.planted_expectation("TIR")
    p = to_extend_params(e["p"])
    d = Device(0)
    try:
        d.load_library(np.ascontiguousarray(e["seq"]))
        flanks, _ = resolve_flanks(1, e["cores"], p.bandwidth, p.L)
        d.begin_direction(flanks, p)
        w = codes("ACGGTCATGATTCCTA")
        assert tup(xfam.seq_pairs([w, w], [(0, 1, 0)], PairParams(min_score=8), device=d)[0]) == (32, 0, 15, 0, 15, 16, 16, 16)
        ci = _lib.RunInfo()
        assert d._L.ramx_dev_run_direction(d._h, C.byref(ci)) == ERR_STATE
        d.begin_direction(flanks, p)
        assert d.run_direction().rows_executed > 0
    finally:
        d.close()
