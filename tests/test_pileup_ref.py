"""The CPU restatement of the pileup, the re-call and the refinement (tests/pileup_ref.py) on three synthetic families, both
directions: the identities that tie the pileup to the alignments it is counted from, and the findings of DESIGN 4.9 -- the
loop's own consensus is a fixed point of majority re-calling, isolated edits are restored in two replays.  No GPU."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import PILEUP_DTYPE, PILEUP_INS, new_master
from repeatafterme_amd.synth import synth_family

import pileup_ref as pr

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


def test_the_struct_is_128_bytes():
    assert PILEUP_DTYPE.itemsize == 128 and PILEUP_INS == 4
    offs = {k: PILEUP_DTYPE.fields[k][1] for k in PILEUP_DTYPE.names}
    assert offs == dict(base=0, cover=4, match=8, ins_open=32, ins_long=36, ins_bases=40, ins=48, **{"del": 28})


@pytest.mark.parametrize("k,direction", RUNS)
def test_pileup_identities(k, direction):
    fs, p, K = family(k)
    cons = loop_consensus(k, direction).copy()
    cons[::7] = (cons[::7] + 1) & 3                    # a foreign consensus: substitutions, insertions and deletions all occur
    cons = np.delete(cons, slice(20, 26))
    cols, idx, results = pr.pileup(direction, fs.cores, fs.sequence, p, cons, with_walks=True)
    rows = len(cons)
    ends = np.array([r["end_row"] for r in results])
    assert (ends >= 0).sum() > len(results) // 2
    for r in range(rows):
        assert cols["cover"][r] == (ends >= r).sum()
    assert np.array_equal(cols["match"].sum(axis=1) + cols["del"], cols["cover"])
    for res in results:                                # per flank: every consumed position is a match, an insertion or the tail
        if res["end_row"] < 0:
            continue
        e = res["end_row"] + 1
        matches = int(((res["col_idx"][:e] != -2 ** 31) & (res["col_idx"][:e] != -2 ** 31 + 1)).sum())
        assert matches + int(res["col_ins"][:e].sum()) + res["tail_ins"] == res["end_idx"] - res["start_idx"] + 1
    slots = cols["ins"].sum(axis=2)                    # [rows][k]
    assert np.all(slots[:, :-1] >= slots[:, 1:])
    assert np.array_equal(slots[:, 0], cols["ins_open"])
    assert np.all(cols["ins_bases"] >= slots.sum(axis=1))
    assert np.array_equal(cols["ins_bases"] == slots.sum(axis=1), cols["ins_long"] == 0)
    assert cols["del"].sum() > 0 and cols["ins_open"].sum() > 0 and cols["ins_long"].sum() > 0
    assert np.array_equal(cols["base"], cons)


@pytest.mark.parametrize("k,direction", RUNS)
def test_the_loops_consensus_is_a_fixed_point(k, direction):
    fs, p, K = family(k)
    cons = loop_consensus(k, direction)
    out, cols, replays, converged = pr.refine(direction, fs.cores, fs.sequence, p, cons, 10)
    assert (replays, converged) == (1, 1) and np.array_equal(out, cons)


@pytest.mark.parametrize("k,direction", RUNS)
def test_isolated_edits_are_restored_in_two_replays(k, direction):
    fs, p, K = family(k)
    cons = loop_consensus(k, direction)
    edited, where = pr.plant_edits(cons)
    assert len(edited) == K and not np.array_equal(edited, cons)
    out, cols, replays, converged = pr.refine(direction, fs.cores, fs.sequence, p, edited, 10)
    assert (replays, converged) == (2, 1), where
    assert np.array_equal(out, cons), where


def test_five_dropped_columns_take_three_replays():
    fs, p, K = family(0)
    cons = loop_consensus(0, 1)
    edited = np.delete(cons, slice(15, 20))
    out, cols, replays, converged = pr.refine(1, fs.cores, fs.sequence, p, edited, 10)
    assert (replays, converged) == (3, 1) and np.array_equal(out, cons)
    first = pr.pileup(1, fs.cores, fs.sequence, p, edited)
    assert first["ins_long"].sum() > 0 and all(first["ins"][:, s].sum() > 0 for s in range(PILEUP_INS))


def test_the_cap_on_replays():
    """Six columns dropped at 20 need four replays: stopped after two, the result is the second consensus with ITS pileup."""
    fs, p, K = family(0)
    cons = loop_consensus(0, 1)
    edited = np.delete(cons, slice(20, 26))
    out, cols, replays, converged = pr.refine(1, fs.cores, fs.sequence, p, edited, 2)
    assert (replays, converged) == (2, 0)
    second = pr.recall(edited, pr.pileup(1, fs.cores, fs.sequence, p, edited), p.L)
    assert np.array_equal(out, second) and not np.array_equal(out, cons)
    assert np.array_equal(cols, pr.pileup(1, fs.cores, fs.sequence, p, second))
    one = pr.refine(1, fs.cores, fs.sequence, p, edited, 1)
    assert (one[2], one[3]) == (1, 0) and np.array_equal(one[0], edited)
    assert pr.refine(1, fs.cores, fs.sequence, p, edited, 10)[2:] == (4, 1)


def test_renderers():
    fs, p, K = family(0)
    cons = loop_consensus(0, 1)
    cols = pr.pileup(1, fs.cores, fs.sequence, p, cons)
    text = pr.render_pileup({1: (cols, None), 0: (cols[:3], cols[:2])})
    lines = text.splitlines()
    assert lines[0].split("\t")[:5] == ["dir", "row", "base", "cover", "A"] and len(lines[0].split("\t")) == 33
    assert len(lines) == 1 + K + 3 + 2 and all(len(x.split("\t")) == 33 for x in lines)
    assert lines[1].split("\t")[0] == "right" and lines[-1].split("\t")[0] == "left-refined"
    fa = pr.render_refined({1: (cons[:4], 1, 1), 0: (np.array([0, 1, 1, 3], np.int8), 3, 0)})
    assert fa == ">right-extension-refined 4 bp replays=1 converged=1\n" + "".join("ACGT"[b] for b in cons[:4]) + \
        "\n>left-extension-refined 4 bp replays=3 converged=0\nTCCA\n"
