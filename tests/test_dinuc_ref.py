"""The CPU restatement of the dinucleotide pileup, the CpG-aware re-call and its loop (tests/dinuc_ref.py): the identities that
tie the records to the alignments they are counted from, the planted family of tests/cpg_cases.py -- the plain refinement loses
its deaminated CpGs, the CpG-aware one calls them all and changes nothing else --, and the families of pileup_ref.FAMILIES, which
stay fixed points.  No GPU."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import DINUC_DTYPE, new_master
from repeatafterme_amd.synth import synth_family

import align_ref as ar
import cpg_cases as cc
import dinuc_ref as dr
import pileup_ref as pr

A, C, G, T = 0, 1, 2, 3
RUNS = [(k, d) for k in range(3) for d in (1, 0)]


@functools.lru_cache(maxsize=None)
def family(k):
    (n, L, W, K, seed), matrix = pr.FAMILIES[k]
    fs = synth_family(n, L, W, K=K, seed=seed, both_sides=True, minus_frac=0.4, n_run_frac=0.1)
    return fs, po.Params.named(matrix, bandwidth=W, L=L, when_to_stop=1000), K


@functools.lru_cache(maxsize=None)
def loop_consensus(k, direction):
    fs, p, K = family(k)
    o = po.oracle_extend(direction, fs.cores.copy(), fs.sequence, new_master(p.L), p, trace=True)
    cons = o.col_base[:K].copy()
    cons.setflags(write=False)
    return cons


@functools.lru_cache(maxsize=None)
def planted(direction):
    """-> (FlankSet, params, the loop's consensus over K columns, the plain refinement, the CpG-aware one)"""
    fs, anc_r, anc_l = cc.planted_family()
    p = po.Params.named(cc.MATRIX, bandwidth=cc.W, L=cc.L, when_to_stop=1000)
    o = po.oracle_extend(direction, fs.cores.copy(), fs.sequence, new_master(p.L), p, trace=True)
    cons = o.col_base[:cc.K].copy()
    return fs, p, cons, pr.refine(direction, fs.cores, fs.sequence, p, cons, 10), dr.refine_cpg(direction, fs.cores, fs.sequence, p, cons, 10)


def sites_called(cons, direction):
    want = (C, G) if direction else (G, C)              # the left extension's rows run against the reading order
    return sum((int(cons[r]), int(cons[r + 1])) == want for r in cc.sites_in_rows(direction))


def test_the_struct_is_128_bytes():
    assert DINUC_DTYPE.itemsize == 128
    offs = {k: DINUC_DTYPE.fields[k][1] for k in DINUC_DTYPE.names}
    assert offs == dict(base=0, next=4, both=8, adjacent=12, split=16, gapped=20, di=24, reserved=124)


@pytest.mark.parametrize("k,direction", RUNS)
def test_dinuc_identities(k, direction):
    fs, p, K = family(k)
    cons = loop_consensus(k, direction).copy()
    cons[::7] = (cons[::7] + 1) & 3                    # a foreign consensus: substitutions, insertions and deletions all occur
    cons = np.delete(cons, slice(20, 26))
    cols, di, idx, results = dr.pileups(direction, fs.cores, fs.sequence, p, cons, with_walks=True)
    rows = len(cons)
    assert dr.identities_hold(di)
    assert np.array_equal(di["base"], cons) and np.array_equal(di["next"][:-1], cons[1:])
    assert np.array_equal(di["both"][:-1], cols["cover"][1:])                      # a copy that covers r + 1 covers r
    assert di["split"].sum() > 0 and di["gapped"].sum() > 0
    if direction:                                      # (the N runs of synth_family lie in the right flanks)
        assert di["di"][:, 4, :].sum() > 0 and di["di"][:, :, 4].sum() > 0
    # the same records from col_idx / col_ins, the way the device counts them
    again = np.zeros(rows, DINUC_DTYPE)
    for n, res in zip(idx, results):
        fl = ar.Flank(direction, fs.cores, n, p.bandwidth)
        for r in range(res["end_row"]):
            a, b = int(res["col_idx"][r]), int(res["col_idx"][r + 1])
            again["both"][r] += 1
            if a == ar.DELETED or b == ar.DELETED:
                again["gapped"][r] += 1
            elif res["col_ins"][r + 1] > 0:
                again["split"][r] += 1
            else:
                again["adjacent"][r] += 1
                again["di"][r][pr.base_class(fl, a, fs.sequence)][pr.base_class(fl, b, fs.sequence)] += 1
    for key in ("both", "adjacent", "split", "gapped", "di"):
        assert np.array_equal(again[key], di[key]), key
    # the marginals of the joint counts never exceed the pileup's
    assert np.all(di["di"].sum(axis=2) <= cols["match"]) and np.all(di["di"].sum(axis=1)[:-1] <= cols["match"][1:])


def test_a_copy_that_ends_at_row_r_covers_r_but_not_the_pair():
    fs, p, K = family(0)
    cons = loop_consensus(0, 1)
    cols, di, idx, results = dr.pileups(1, fs.cores, fs.sequence, p, cons, with_walks=True)
    ends = np.array([r["end_row"] for r in results])
    ragged = [r for r in range(K - 1) if (ends == r).any()]
    assert ragged
    for r in ragged:
        assert cols["cover"][r] - di["both"][r] == (ends == r).sum()


@pytest.mark.parametrize("direction", [1, 0])
def test_the_plain_refinement_loses_the_planted_sites_and_the_cpg_aware_one_calls_them(direction):
    fs, p, cons, plain, cpg = planted(direction)
    pcons, _, preplays, pconv = plain
    ccons, ccols, cdi, replays, conv, n_cpg = cpg
    assert (preplays, pconv) == (2, 1) and (replays, conv) == (2, 1)
    assert len(pcons) == len(ccons) == cc.K
    # pinned: of the 8 planted sites the loop's consensus holds 3 (right) / 1 (left), the plain refinement none
    assert sites_called(cons, direction) == (3 if direction else 1)
    assert sites_called(pcons, direction) == 0 < cc.N_SITES // 2
    assert sites_called(ccons, direction) == cc.N_SITES == 8
    site_rows = {x for r in cc.sites_in_rows(direction) for x in (r, r + 1)}
    differ = set(np.flatnonzero(pcons != ccons).tolist())
    assert differ and differ <= site_rows
    assert len(differ) == (16 if direction else 15)
    assert n_cpg == (12 if direction else 19)            # the planted sites and the CG the ancestor holds by chance
    assert dr.identities_hold(cdi) and np.array_equal(cdi["base"], ccons)
    # the result is a fixed point of its own re-call, and the plain rule would take the sites away again
    again, n2 = dr.recall_cpg(ccons, ccols, cdi, not direction, p.matrix, 0, p.L)
    assert np.array_equal(again, ccons) and n2 == n_cpg
    assert sites_called(pr.recall(ccons, ccols, p.L), direction) < cc.N_SITES // 2


def test_the_score_of_a_deaminated_base_decides():
    """cpg_ts = -18 says a deaminated base contradicts CpG as much as a transversion does: no planted site is called then."""
    fs, p, cons, plain, cpg = planted(1)
    out = dr.refine_cpg(1, fs.cores, fs.sequence, p, cons, 10, cpg_ts=-18)
    assert sites_called(out[0], 1) == 0
    assert sites_called(dr.refine_cpg(1, fs.cores, fs.sequence, p, cons, 10, cpg_ts=5)[0], 1) == cc.N_SITES


@pytest.mark.parametrize("k,direction", RUNS)
def test_the_existing_families_stay_fixed_points(k, direction):
    """No family of pileup_ref.FAMILIES holds a tested pair that flips: the CpG-aware loop leaves each where the plain one does.
    Found by the restatement: tested pairs 14, 12, 18, 18, 10, 8 and CG pairs 6, 5, 3, 4, 0, 3 in the order of RUNS."""
    fs, p, K = family(k)
    cons = loop_consensus(k, direction)
    out, cols, di, replays, converged, n_cpg = dr.refine_cpg(direction, fs.cores, fs.sequence, p, cons, 10)
    assert (replays, converged) == (1, 1) and np.array_equal(out, cons)
    _, n, tested = dr.recall_cpg(cons, cols, di, not direction, p.matrix, 0, p.L, with_pairs=True)
    i = RUNS.index((k, direction))
    assert len(tested) == (14, 12, 18, 18, 10, 8)[i] and n == n_cpg == (6, 5, 3, 4, 0, 3)[i]
    assert all((a, b) == (C, G) for (r, a, b, sp, sc, called) in tested if called)


def test_the_cap_on_replays():
    fs, p, cons, plain, cpg = planted(1)
    one = dr.refine_cpg(1, fs.cores, fs.sequence, p, cons, 1)
    assert (one[3], one[4]) == (1, 0) and np.array_equal(one[0], cons)


def test_renderers():
    fs, p, cons, plain, cpg = planted(1)
    text = dr.render_dinuc({1: cpg[2], 0: cpg[2][:3]})
    lines = text.splitlines()
    assert lines[0].split("\t")[:9] == ["dir", "row", "base", "next", "both", "adjacent", "split", "gapped", "AA"] and lines[0].endswith("\tNN")
    assert len(lines) == 1 + cc.K + 3 and all(len(x.split("\t")) == 33 for x in lines)
    assert lines[cc.K].split("\t")[:4] == ["right", str(cc.K - 1), "ACGT"[cpg[0][-1]], "-"]
    fa = dr.render_cpg({1: (np.array([1, 2, 0], np.int8), 2, 1, 1), 0: (np.array([2, 1, 3], np.int8), 3, 0, 1)})
    assert fa == ">right-extension-cpg 3 bp replays=2 converged=1 cpg=1\nCGA\n>left-extension-cpg 3 bp replays=3 converged=0 cpg=1\nTCG\n"
