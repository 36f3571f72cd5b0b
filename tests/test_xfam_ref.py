"""The contract of include/ramx_xfam.h on the CPU: a literal expected value for every rule of the candidates, the counting rule
and the groups, on the restatement tests/xfam_ref.py and on the library's host functions alike; the three host functions against
the restatement on random small inputs; ramx_seq_pair_host against the restatement of the terminal repeats on rectangles; the
chance score; the refusals; and families planted as fragments of one element, extended by the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

from repeatafterme_amd import _lib, xfam
from repeatafterme_amd.datamodel import SEQ_PAIR_DTYPE, TERM_DTYPE, PairParams, XfamLinkParams

import term_ref as tr
import xfam_ref as xr
from test_term_ref import codes

ERR_ARG = -103
ERR_UNSUPPORTED = -106


def tup(r):
    return tuple(int(r[k]) for k in tr.FIELDS)


def ptup(pairs):
    return [(int(p["a"]), int(p["b"]), int(p["inverted"])) for p in pairs]


def cand_both(strings, owner, K, within=False):
    """The candidates of sequences given as strings by the restatement and by ramx_xfam_candidates: both must agree."""
    seqs = [codes(s) for s in strings]
    want = xr.candidates(seqs, owner, K, within)
    got = xfam.candidates(seqs, owner, K=K, within=within)
    assert ptup(got) == want and (got["reserved"] == 0).all()
    return want


def rc(s):
    return "".join({"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}[ch] for ch in reversed(s))


W8, W16 = "ACGGTCAT", "ACGGTCATGATTCCTA"            # neither is its own reverse complement


# ---- the candidates: a literal list for every rule ----

def test_direct_and_inverted_kmer_sharing():
    for K, w in ((8, W8), (16, W16)):
        a, b, c = "TT" + w + "GG", "C" + w, "AAA" + rc(w) + "C"
        assert cand_both([a, b, c], [0, 1, 2], K) == [(0, 1, 0), (0, 2, 1), (1, 2, 1)]
        # one base short of K in common: nothing
        assert cand_both([a, "C" + w[:-1] + ("A" if w[-1] != "A" else "C")], [0, 1], K) == []
    # the same 16-mer is no 8-mer candidate's loss: a shared 16-mer holds shared 8-mers
    assert cand_both(["TT" + W16, W16 + "A"], [0, 1], 8) == [(0, 1, 0)]


def test_a_kmer_broken_by_a_class_4_base():
    broken = W8[:4] + "N" + W8[4:]
    assert cand_both([W8, broken], [0, 1], 8) == []
    assert cand_both([W8 + "N", "N" + W8], [0, 1], 8) == [(0, 1, 0)]
    # lower case is its base
    assert cand_both([W8, W8.lower()], [0, 1], 8) == [(0, 1, 0)]


def test_a_palindromic_kmer_is_shared_in_both_orientations():
    pal = "ACGTACGT"
    assert rc(pal) == pal
    assert cand_both(["GG" + pal, pal + "TT"], [0, 1], 8) == [(0, 1, 0), (0, 1, 1)]


def test_within_on_and_off_and_empty_sides():
    s = [W8, W8, W8, ""]
    assert cand_both(s, [0, 0, 1, 1], 8) == [(0, 2, 0), (1, 2, 0)]
    assert cand_both(s, [0, 0, 1, 1], 8, within=True) == [(0, 1, 0), (0, 2, 0), (1, 2, 0)]
    # K = 0: every pair without an empty side, both orientations
    assert cand_both(s, [0, 0, 1, 1], 0) == [(0, 2, 0), (0, 2, 1), (1, 2, 0), (1, 2, 1)]
    assert cand_both(["A", "C", ""], [0, 1, 2], 0) == [(0, 1, 0), (0, 1, 1)]


def test_the_order_of_the_pairs_and_a_cap_below_the_count():
    seqs = [codes(W8)] * 4
    want = [(a, b, inv) for a in range(4) for b in range(a + 1, 4) for inv in (0, 1)]
    assert xr.candidates(seqs, [0, 1, 2, 3], 0) == want
    assert ptup(xfam.candidates(seqs, [0, 1, 2, 3], K=0)) == want
    assert ptup(xfam.candidates(seqs, [0, 1, 2, 3], K=0, cap=5)) == want[:5]
    # the count does not depend on the cap, and nothing behind the cap is written
    cds, off = xfam._flatten(seqs)
    own = np.arange(4, dtype=np.int32)
    buf = np.full(7 * 4, 77, np.int32).view(SEQ_PAIR_DTYPE)
    assert _lib.lib().ramx_xfam_candidates(cds.ctypes.data, off.ctypes.data, 4, own.ctypes.data, 0, 0, buf.ctypes.data, 5) == 12
    assert ptup(buf[:5]) == want[:5] and (buf[5:].view(np.int32) == 77).all()


# ---- the counting rule and the groups ----

def rec(score, matches, columns):
    return (score, 0, columns - 1, 0, columns - 1, matches, columns, 100)


def groups_both(pairs, recs, owner, nf, **link):
    want = xr.groups(pairs, recs, owner, nf, **link)
    r = np.array(recs, np.int32).reshape(-1, 8).view(TERM_DTYPE).reshape(-1)
    counts, group = xfam.groups(pairs, r, owner, nf, XfamLinkParams(**{**xr.LINK, **link}))
    assert (counts.tolist(), group.tolist()) == want
    return want


def test_a_record_that_fails_each_counting_condition_alone():
    pairs, owner = [(0, 1, 0)], [0, 1]
    assert groups_both(pairs, [rec(100, 64, 80)], owner, 2) == ([1], [0, 0])             # 80 columns at exactly 800 permille
    assert groups_both(pairs, [rec(0, 64, 80)], owner, 2) == ([0], [0, 1])               # no score
    assert groups_both(pairs, [rec(100, 79, 79)], owner, 2) == ([0], [0, 1])             # a column short
    assert groups_both(pairs, [rec(100, 63, 80)], owner, 2) == ([0], [0, 1])             # 787 permille
    assert groups_both(pairs, [rec(100, 799, 1000)], owner, 2) == ([0], [0, 1])          # 799 permille
    assert groups_both(pairs, [rec(100, 63, 80)], owner, 2, min_permille=787) == ([1], [0, 0])
    assert groups_both(pairs, [rec(100, 79, 79)], owner, 2, min_columns=79) == ([1], [0, 0])


def test_a_chain_becomes_one_group_with_the_smallest_index():
    # sequences 0..4 of families 3, 1, 4, 0, 2: records 1-4 (3 -- 1), then 4-2 (1 -- 4): the group of 1, 3 and 4 is 1
    owner = [3, 1, 4, 0, 2]
    pairs = [(0, 1, 0), (1, 2, 1), (3, 4, 0)]
    good = rec(200, 90, 100)
    assert groups_both(pairs, [good, good, rec(0, 0, 0)], owner, 5) == ([1, 1, 0], [0, 1, 2, 1, 1])
    # joined the other way round, and with the last pair too: everything but family 0 ... and then with it
    assert groups_both(pairs[::-1], [good, good, good], owner, 5) == ([1, 1, 1], [0, 1, 0, 1, 1])
    assert groups_both([], [], owner, 5) == ([], [0, 1, 2, 3, 4])


def test_a_record_within_a_family_counts_but_never_links():
    owner = [0, 0, 1]
    assert groups_both([(0, 1, 0), (0, 2, 1)], [rec(300, 100, 100), rec(0, 0, 0)], owner, 2) == ([1, 0], [0, 1])


# ---- the host functions against the restatement ----

def random_seq(rng, n, pn=0.05):
    s = rng.integers(0, 8, n).astype(np.int8)
    s[rng.random(n) < pn] = rng.choice(np.array([8, 99, -1, 14, -128, 127], np.int8))
    return s


def test_the_three_host_functions_on_random_small_inputs():
    rng = np.random.default_rng(41)
    for trial in range(200):
        n = int(rng.integers(0, 6))
        motif = rng.integers(0, 4, 12).astype(np.int8)
        seqs = []
        for _ in range(n):
            s = random_seq(rng, int(rng.integers(0, 40)))
            if len(s) > 20 and rng.random() < 0.6:                    # plant the motif, or its reverse complement, now and then
                at = int(rng.integers(0, len(s) - 12))
                s[at:at + 12] = motif if rng.random() < 0.5 else tr.revcomp(motif)
            seqs.append(s)
        nf = max(1, int(rng.integers(1, 4)))
        owner = [int(v) for v in rng.integers(0, nf, n)]
        K = int(rng.choice([0, 8, 9, 12]))
        within = bool(rng.integers(0, 2))
        want = xr.candidates(seqs, owner, K, within)
        got = xfam.candidates(seqs, owner, K=K, within=within)
        assert ptup(got) == want, trial
        params = dict(match=int(rng.integers(1, 4)), mismatch=int(rng.integers(1, 4)), gap=int(rng.integers(1, 6)), min_score=int(rng.integers(1, 12)))
        recs = [xr.record(seqs[a], seqs[b], inv, **params) for a, b, inv in want]
        for (a, b, inv), r in zip(want, recs):
            assert tup(xfam.seq_pair_host(seqs[a], seqs[b], inv, PairParams(**params))[0]) == r, (trial, a, b, inv)
        link = dict(min_columns=int(rng.integers(0, 8)), min_permille=int(rng.integers(0, 1001)))
        r = np.array(recs, np.int32).reshape(-1, 8).view(TERM_DTYPE).reshape(-1)
        counts, group = xfam.groups(got, r, owner, nf, XfamLinkParams(**link))
        assert (counts.tolist(), group.tolist()) == xr.groups(want, recs, owner, nf, **link), trial


RECTANGLES = [(0, 7), (7, 0), (0, 0), (1, 1500), (1500, 1), (1100, 1300)]


@pytest.mark.parametrize("na,nb", RECTANGLES)
def test_seq_pair_host_on_rectangles(na, nb):
    rng = np.random.default_rng(na * 7 + nb)
    a = random_seq(rng, na, 0.01)
    b = random_seq(rng, nb, 0.01)
    if na > 1000 and nb > 1000:                                       # something to find: a stretch of a, with a gap, inside b
        b[200:500] = np.concatenate((a[600:750], a[753:903]))
    p = dict(match=2, mismatch=3, gap=5, min_score=1)
    for inv in (0, 1):
        want = (0,) * 8 if na == 0 or nb == 0 else tr.pair_diag(tr.classes(a), xr.oriented(b, inv), **p)
        assert tup(xfam.seq_pair_host(a, b, inv, PairParams(**p))[0]) == want
        if na > 1000 and nb > 1000 and not inv:
            assert want[0] > 500 and want[5] < want[6]


def test_seq_pair_host_on_an_inverted_pair_with_class_4_runs():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 4, 400).astype(np.int8)
    b = tr.revcomp(a[50:350]).astype(np.int8)
    a[100:108] = 99                                                   # a run of N in a, another in b, lower case in between
    b[200:205] = -1
    b[20:60] += 4
    p = dict(match=2, mismatch=3, gap=5, min_score=80)
    want = tr.pair_diag(tr.classes(a), xr.oriented(b, 1), **p)
    assert want[0] >= 80 and want[5] < want[6]
    assert tup(xfam.seq_pair_host(a, b, 1, PairParams(**p))[0]) == want
    assert tup(xfam.seq_pair_host(a, b, 0, PairParams(**p))[0]) == tr.pair_diag(tr.classes(a), tr.classes(b), **p)


def test_independent_sequences_stay_below_half_the_default_min_score():
    rng = np.random.default_rng(11)
    worst = 0
    for _ in range(40):
        a, b = rng.integers(0, 4, 2000), rng.integers(0, 4, 2000)
        worst = max(worst, tr.best_score(a, b, match=2, mismatch=3, gap=5))
    assert 0 < worst < PairParams().min_score // 2 == 40


def test_the_refusals():
    L = _lib.lib()
    a = codes(W8)
    out = np.full(8, 7, np.int32)
    good = (2, 3, 5, 80)
    call = lambda pp, na=8, nb=8, inv=0, pa=a.ctypes.data, po=out.ctypes.data: L.ramx_seq_pair_host(pa, na, a.ctypes.data, nb, inv, pp, po)
    for field, values in {0: (0, 16), 1: (0, 16), 2: (0, 32), 3: (0, -1)}.items():
        for v in values:
            bad = list(good)
            bad[field] = v
            assert call(C.byref(_lib.PairParams(*bad))) == ERR_ARG, bad
    ok = C.byref(_lib.PairParams(*good))
    assert call(None) == ERR_ARG and call(ok, na=-1) == ERR_ARG and call(ok, nb=-1) == ERR_ARG
    assert call(ok, inv=2) == ERR_ARG and call(ok, inv=-1) == ERR_ARG and call(ok, pa=None) == ERR_ARG and call(ok, po=None) == ERR_ARG
    big = np.zeros(32768, np.int8)
    assert L.ramx_seq_pair_host(big.ctypes.data, 32768, a.ctypes.data, 8, 0, ok, out.ctypes.data) == ERR_UNSUPPORTED
    assert L.ramx_seq_pair_host(a.ctypes.data, 8, big.ctypes.data, 32768, 0, ok, out.ctypes.data) == ERR_UNSUPPORTED
    assert (out == 7).all()
    assert L.ramx_seq_pair_host(big.ctypes.data, 32767, a.ctypes.data, 8, 0, ok, out.ctypes.data) == 0 and tuple(out) == (0, 0, 0, 0, 0, 0, 0, 8)
    # candidates: K outside 0, 8..16; a decreasing seq_off; negative counts
    off = np.array([0, 8, 16], np.int64)
    two = np.concatenate((a, a))
    own = np.array([0, 1], np.int32)
    cand = lambda K=8, o=off, n=2, cap=0: L.ramx_xfam_candidates(two.ctypes.data, o.ctypes.data, n, own.ctypes.data, K, 0, None, cap)
    assert cand() == 1 and cand(K=0) == 2 and cand(K=16) == 0
    for K in (-1, 1, 7, 17, 32):
        assert cand(K=K) == ERR_ARG
    assert cand(o=np.array([0, 9, 8], np.int64)) == ERR_ARG and cand(n=-1) == ERR_ARG and cand(cap=-1) == ERR_ARG and cand(cap=1) == ERR_ARG
    # groups: the link parameters, an owner outside the families
    pa = np.zeros(1, SEQ_PAIR_DTYPE)
    pa["b"] = 1
    r = np.zeros(1, TERM_DTYPE)
    cnt, grp = np.full(1, 7, np.int32), np.full(2, 7, np.int32)
    grp_call = lambda lp, nf=2: L.ramx_xfam_groups(pa.ctypes.data, r.ctypes.data, 1, own.ctypes.data, nf, lp, cnt.ctypes.data, grp.ctypes.data)
    for bad in ((-1, 800), (80, -1), (80, 1001)):
        assert grp_call(C.byref(_lib.XfamLinkParams(*bad))) == ERR_ARG
    assert grp_call(None) == ERR_ARG and grp_call(C.byref(_lib.XfamLinkParams(80, 800)), nf=1) == ERR_ARG
    assert cnt[0] == 7 and (grp == 7).all()
    assert grp_call(C.byref(_lib.XfamLinkParams(80, 800))) == 0 and cnt[0] == 0 and grp.tolist() == [0, 1]


# ---- fragments of one element, extended by the CPU oracle ----

def test_planted_fragments_extend_into_each_other():
    P = xr.planted_families()
    seqs, owner = P["seqs"], P["owner"]
    A, B, D, Cf = range(4)
    assert [f["name"] for f in P["families"]] == ["A", "B", "D", "C"]
    assert all(min(f["bp"]) > 0 for f in P["families"]) and P["families"][B]["bp"] == P["families"][D]["bp"][::-1]
    recs, pairs, counts, group = xr.compare(seqs, owner, 4, K=0, within=True)
    links = {(owner[a], owner[b]) for (a, b, _), c in zip(pairs, counts) if c and owner[a] != owner[b]}
    assert links == {(A, B), (A, D), (B, D)}
    assert group == [A, A, A, Cf]
    counting = [(p, r) for p, r, c in zip(pairs, recs, counts) if c]
    assert any(r[5] < r[6] for _, r in counting)
    assert {inv for (a, b, inv), _ in counting if owner[a] != owner[b]} == {0, 1}
    # no record involves C, and none joins a family's own two extensions
    for (a, b, _), r in zip(pairs, recs):
        if Cf in (owner[a], owner[b]) or owner[a] == owner[b]:
            assert r[0] == 0, (a, b, r)
    # the 16-mer filter does not hide the plant: every pair with a record is a candidate, and the exact mode adds none
    c16 = xr.candidates(seqs, owner, 16, True)
    assert {p for p, r in zip(pairs, recs) if r[0] > 0} <= set(c16)
    assert ptup(xfam.candidates(seqs, owner, K=16, within=True)) == c16
    got = [tup(xfam.seq_pair_host(seqs[a], seqs[b], inv)[0]) for a, b, inv in c16]
    assert got == [r for p, r in zip(pairs, recs) if p in set(c16)]
