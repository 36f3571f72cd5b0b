"""Consensus refinement on the device (C-ABI ramx_dev_refine, the refinement sink of seam 1) against the restatement of
tests/pileup_ref.py: the consensus, its length, the replays, the verdict and the final pileup.  Everything is exact."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import new_master
from repeatafterme_amd.synth import synth_family

import pileup_ref as pr
from helpers import to_extend_params
from test_gpu_pileup import same_pileup

pytestmark = pytest.mark.gpu

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


def gpu_refine(direction, cores, sequence, p, cons, max_replays):
    from repeatafterme_amd.device import Device, resolve_flanks
    d = Device(0)
    try:
        d.load_library(np.ascontiguousarray(sequence, np.int8))
        flanks, _ = resolve_flanks(direction, cores, p.bandwidth, p.L)
        return d.refine(flanks, to_extend_params(p), cons, max_replays=max_replays)
    finally:
        d.close()


def same_refinement(res, f, want, tag):
    cons, cols, replays, converged = want
    assert (int(res.rows[f]), int(res.replays[f]), int(res.converged[f])) == (len(cons), replays, converged), tag
    assert np.array_equal(res.cons[f, :len(cons)], cons), tag
    same_pileup(res.cols[f, :len(cons)], cols, tag)


@pytest.mark.parametrize("k,direction", RUNS)
def test_fixed_points_and_planted_edits(k, direction):
    fs, p, K = family(k)
    cons = loop_consensus(k, direction)
    want = pr.refine(direction, fs.cores, fs.sequence, p, cons, 10)
    assert want[2:] == (1, 1)
    same_refinement(gpu_refine(direction, fs.cores, fs.sequence, p, cons, 10), 0, want, f"fixed point {k} {direction}")
    edited, where = pr.plant_edits(cons)
    want = pr.refine(direction, fs.cores, fs.sequence, p, edited, 10)
    assert want[2:] == (2, 1) and np.array_equal(want[0], cons)
    same_refinement(gpu_refine(direction, fs.cores, fs.sequence, p, edited, 10), 0, want, f"planted {k} {direction} {where}")


def test_three_replays_and_the_cap():
    fs, p, K = family(0)
    cons = loop_consensus(0, 1)
    five, six = np.delete(cons, slice(15, 20)), np.delete(cons, slice(20, 26))
    want = pr.refine(1, fs.cores, fs.sequence, p, five, 10)
    assert want[2:] == (3, 1) and np.array_equal(want[0], cons)
    same_refinement(gpu_refine(1, fs.cores, fs.sequence, p, five, 10), 0, want, "five dropped")
    want = pr.refine(1, fs.cores, fs.sequence, p, six, 2)
    assert want[2:] == (2, 0) and len(want[0]) < K
    same_refinement(gpu_refine(1, fs.cores, fs.sequence, p, six, 2), 0, want, "six dropped, two replays")


def test_one_replay_is_the_pileup():
    from repeatafterme_amd.device import Device, resolve_flanks
    fs, p, K = family(0)
    six = np.delete(loop_consensus(0, 0), slice(20, 26))
    d = Device(0)
    try:
        d.load_library(np.ascontiguousarray(fs.sequence, np.int8))
        flanks, _ = resolve_flanks(0, fs.cores, p.bandwidth, p.L)
        pl = d.pileup(flanks, to_extend_params(p), six)
        rf = d.refine(flanks, to_extend_params(p), six, max_replays=1)
    finally:
        d.close()
    assert (int(rf.rows[0]), int(rf.replays[0]), int(rf.converged[0])) == (len(six), 1, 0)
    assert np.array_equal(rf.cons[0, :len(six)], six) and np.array_equal(rf.cols, pl.cols) and np.array_equal(rf.ends, pl.ends)


def test_growth_is_cut_at_L():
    """Six columns dropped, 44 left, and L = 45: the first re-call would give 48 columns and is cut to 45; the refinement goes
    on from the cut consensus and ends at the loop's first 45 columns."""
    fs, p60, K = family(0)
    cons = loop_consensus(0, 1)
    six = np.delete(cons, slice(20, 26))
    p = po.Params.named(pr.FAMILIES[0][1], bandwidth=p60.bandwidth, L=45, when_to_stop=1000)
    first = pr.pileup(1, fs.cores, fs.sequence, p, six)
    assert len(pr.recall(six, first, 10 ** 6)) == 48 and len(pr.recall(six, first, p.L)) == 45
    want = pr.refine(1, fs.cores, fs.sequence, p, six, 10)
    assert want[2:] == (4, 1) and np.array_equal(want[0], cons[:45])
    same_refinement(gpu_refine(1, fs.cores, fs.sequence, p, six, 10), 0, want, "cut at L")


def test_two_families_converge_at_different_replays():
    """One call, two families: the first is a fixed point (one replay, then left alone), the second takes three."""
    from repeatafterme_amd import _lib
    from repeatafterme_amd.device import Device, resolve_flanks
    fs, p, K = family(0)
    ep = to_extend_params(p)
    cons = loop_consensus(0, 1)
    five = np.delete(cons, slice(15, 20))
    (fl, nx), _ = resolve_flanks(1, fs.cores, p.bandwidth, p.L)
    tile = (nx + 63) // 64 * 64
    arr = (_lib.Flank * (2 * tile))()
    for i in range(2 * tile):
        arr[i].t_lo, arr[i].t_hi, arr[i].step = 1, 0, 1
    for i in range(nx):
        arr[i] = fl[i]
        arr[tile + i] = fl[i]
    both = np.zeros((2, p.L), np.int8)
    both[0, :K], both[1, :K - 5] = cons, five
    d = Device(0)
    try:
        d.load_library(np.ascontiguousarray(fs.sequence, np.int8))
        res = d.refine((arr, 2 * tile), ep, both, rows=[K, K - 5], fam_first=[0, tile], fam_count=[nx, nx], max_replays=10)
        alone = d.refine((fl, nx), ep, cons, max_replays=10)
    finally:
        d.close()
    want0 = pr.refine(1, fs.cores, fs.sequence, p, cons, 10)
    want1 = pr.refine(1, fs.cores, fs.sequence, p, five, 10)
    assert want0[2:] == (1, 1) and want1[2:] == (3, 1)
    same_refinement(res, 0, want0, "family 0")
    same_refinement(res, 1, want1, "family 1")
    assert np.array_equal(res.ends[:tile], alone.ends[:tile])                    # the converged family's records are its own replay's
    assert np.array_equal(res.ends[tile:], alone.ends[:tile])                    # ... and both end at the same consensus


def test_the_sink_of_seam_1():
    """extend_alignment(refine=n): the kept consensus with its pileup, its refinement, and the loop's results beside it
    unchanged; with align=True beside it both sinks are served."""
    from repeatafterme_amd.extend import extend_alignment
    fs, p, K = family(0)
    ep = to_extend_params(p)
    c0, m0 = fs.cores.copy(), new_master(p.L)
    c1, m1 = fs.cores.copy(), new_master(p.L)
    c_o, m_o = fs.cores.copy(), new_master(p.L)
    for direction in (1, 0):
        before = c_o.copy()
        o = po.oracle_extend(direction, c_o, fs.sequence, m_o, p, trace=True)
        plain = extend_alignment(direction, c0, fs.sequence, m0, ep)
        info, rf = extend_alignment(direction, c1, fs.sequence, m1, ep, refine=10)
        for key in ("ret", "rows_executed", "limit_warning", "launches", "persistent", "lanes_per_flank", "packed_rows", "lean_rows"):
            assert getattr(info, key) == getattr(plain, key), key
        assert info.ret == o.ret and rf.direction == direction and rf.family == 0
        kept = o.col_base[:o.ret]
        assert np.array_equal(rf.cons, kept)
        same_pileup(rf.cols, pr.pileup(direction, before, fs.sequence, p, kept), f"kept dir={direction}")
        want = pr.refine(direction, before, fs.sequence, p, kept, 10)
        assert (rf.replays, rf.converged) == want[2:] and np.array_equal(rf.refined_cons, want[0])
        same_pileup(rf.refined_cols, want[1], f"refined dir={direction}")
        info_a, al, rf_a = extend_alignment(direction, fs.cores.copy(), fs.sequence, new_master(p.L), ep, align=True, refine=1) \
            if direction else (None, None, None)
        if direction:
            assert rf_a.replays == 1 and np.array_equal(rf_a.cols, rf.cols) and np.array_equal(al.cons, kept)
    assert np.array_equal(m0, m1) and np.array_equal(m1, m_o)
    for key in ("left_len", "right_len", "score"):
        assert np.array_equal(getattr(c0, key), getattr(c1, key)) and np.array_equal(getattr(c1, key), getattr(c_o, key))
