"""The corners of the replays along a given consensus (C-ABI ramx_dev_profile, ramx_dev_align, ramx_dev_pileup, ramx_dev_refine)
where the four entry points answer differently or share state: nothing to do, a family without flanks, rows = 0 everywhere,
one session's buffers used by all four in turn, and the direction that a replay leaves without its windows.  One small family
(70 flanks, bandwidth 5, L = 30: 128 padded flanks) through the seam-2 forms of repeatafterme_amd.device.Device."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import ALN_END_DTYPE, ALN_NONE, new_master
from repeatafterme_amd.synth import synth_family

import pileup_ref as pr
from helpers import to_extend_params

pytestmark = pytest.mark.gpu

W, L = 5, 30
NONE = (-1, -1, 0, 0, 0)
END_FIELDS = ("end_row", "end_idx", "score", "start_idx", "tail_ins")


@functools.lru_cache(maxsize=None)
def family():
    """-> (FlankSet, oracle parameters, a consensus that is not the family's own: every seventh base of the loop's changed)"""
    fs = synth_family(70, L, W, K=20, seed=62)
    p = po.Params.named("14p43g", bandwidth=W, L=L)
    o = po.oracle_extend(1, fs.cores.copy(), fs.sequence, new_master(L), p, trace=True)
    cons = o.col_base[:o.rows_executed].astype(np.int8)
    assert len(cons) >= 10
    cons[::7] = (cons[::7] + 1) & 3
    cons.setflags(write=False)
    return fs, p, cons


def session():
    """-> (Device with the family's library loaded, (flank array, 128), parameters)"""
    from repeatafterme_amd.device import Device, pad_flanks, resolve_flanks
    fs, p, _ = family()
    d = Device(0)
    try:
        d.load_library(np.ascontiguousarray(fs.sequence, np.int8))
        arr, npad = pad_flanks(resolve_flanks(1, fs.cores, W, L)[0])
        assert npad == 128
    except Exception:
        d.close()
        raise
    return d, (arr, npad), to_extend_params(p)


def sentinel_alignment(rows, npad):
    from repeatafterme_amd.device import AlignResult
    ends = np.zeros(npad, ALN_END_DTYPE)
    ends.view(np.uint8)[:] = 0x5a
    return AlignResult(ends, np.full((max(rows, 1), npad), 12345, np.int32), np.full((max(rows, 1), npad), 54321, np.int32), 0.0, 0.0)


def all_none(ends):
    return all(np.all(ends[k] == v) for k, v in zip(END_FIELDS, NONE))


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_nothing_to_do():
    """n_families == 0 over 128 padded flanks: every call returns OK and writes nothing."""
    d, flanks, ep = session()
    try:
        kw = dict(rows=[], fam_first=[], fam_count=[])
        cons = np.zeros((0, L), np.int8)
        prof = d.profile(flanks, ep, cons, **kw)
        assert len(prof.last_uncapped_row) == 128 and np.all(prof.last_uncapped_row == -1)
        out, keep = sentinel_alignment(3, 128), sentinel_alignment(3, 128)
        res = d.align(flanks, ep, cons, out=out, **kw)
        assert res.ends is out.ends and res.col_idx is out.col_idx
        for k in ("ends", "col_idx", "col_ins"):
            assert same_bytes(getattr(out, k), getattr(keep, k)), k
        pile = d.pileup(flanks, ep, cons, **kw)
        assert pile.cols.shape[0] == 0 and all_none(pile.ends)              # Device.pileup's own prefill, left alone
        ref = d.refine(flanks, ep, cons, **kw)
        assert len(ref.rows) == 0 and len(ref.replays) == 0 and all_none(ref.ends)
    finally:
        d.close()


def test_a_family_without_flanks():
    """fam_count = [0] over no flanks at all: the profile gets its bases from the sum kernel, pileup and refine answer on the
    host; the re-call of columns without cover is the restatement's (tests/pileup_ref.py)."""
    d, (arr, _), ep = session()
    try:
        cons = np.zeros((1, L), np.int8)
        cons[0] = np.random.default_rng(7).integers(0, 4, L)
        kw = dict(rows=[10], fam_first=[0], fam_count=[0])
        prof = d.profile((arr, 0), ep, cons, **kw)
        assert np.array_equal(prof.cols["base"][0, :10], cons[0, :10])
        for k in prof.cols.dtype.names:
            if k != "base":
                assert not prof.cols[k][0, :10].any(), k
        assert not prof.cols[0, 10:].view(np.uint8).any()
        pile = d.pileup((arr, 0), ep, cons, **kw)
        assert np.array_equal(pile.cols["base"][0, :10], cons[0, :10])
        for k in pile.cols.dtype.names:
            if k != "base":
                assert not pile.cols[k][0, :10].any(), k
        assert not pile.cols[0, 10:].view(np.uint8).any()
        ref = d.refine((arr, 0), ep, cons, max_replays=1, **kw)
        assert same_bytes(ref.cols, pile.cols) and int(ref.replays[0]) == 1
        want = pr.recall(cons[0, :10], pile.cols[0, :10], L)
        assert int(ref.rows[0]) == len(want) == 10 and np.array_equal(ref.cons[0, :10], want)
        assert int(ref.converged[0]) == 1                                    # nothing covers a column: the consensus stays
    finally:
        d.close()


def test_a_family_without_flanks_after_another():
    """The same empty family as the second of two, at fam_first == n_padded: its answers are those above, and the first family's
    are those of a call with it alone."""
    _, _, c0 = family()
    d, flanks, ep = session()
    try:
        r0 = min(len(c0), 12)
        cons = np.zeros((2, L), np.int8)
        cons[0, :r0] = c0[:r0]
        cons[1] = np.random.default_rng(7).integers(0, 4, L)
        one = dict(rows=[r0], fam_first=[0], fam_count=[70])
        two = dict(rows=[r0, 10], fam_first=[0, 128], fam_count=[70, 0])
        for name, extra in (("profile", {}), ("align", {}), ("pileup", {}), ("refine", dict(max_replays=1))):
            call = getattr(d, name)
            a = call(flanks, ep, cons[:1], **one, **extra)
            b = call(flanks, ep, cons, **two, **extra)
            if name == "profile":
                assert same_bytes(b.cols[0], a.cols[0]) and np.array_equal(b.last_uncapped_row, a.last_uncapped_row)
                assert a.cols["total"][0, :r0].any()
            elif name == "align":
                for k in ("ends", "col_idx", "col_ins"):
                    assert same_bytes(getattr(b, k), getattr(a, k)), k
                assert (a.ends["end_row"] >= 0).any()
            else:
                assert same_bytes(b.cols[0], a.cols[0]) and same_bytes(b.ends, a.ends), name
                assert a.cols["cover"][0, :r0].sum() > 0
            if name == "refine":
                assert int(b.rows[0]) == int(a.rows[0]) and np.array_equal(b.cons[0], a.cons[0])
                assert (int(b.replays[0]), int(b.converged[0])) == (int(a.replays[0]), int(a.converged[0]))
                want = pr.recall(cons[1, :10], b.cols[1, :10], L)
                assert int(b.rows[1]) == len(want) and np.array_equal(b.cons[1, :len(want)], want) and int(b.replays[1]) == 1
            if name != "align":
                assert np.array_equal(b.cols["base"][1, :10], cons[1, :10])
                for k in b.cols.dtype.names:
                    if k != "base":
                        assert not b.cols[k][1, :10].any(), (name, k)
                assert not b.cols[1, 10:].view(np.uint8).any(), name
    finally:
        d.close()


def test_all_rows_zero():
    """rows = [0] over 70 flanks: no kernel runs; align and pileup answer "no alignment" for the 128 entries of the family's
    tiles, and align writes no column (there is none)."""
    d, flanks, ep = session()
    try:
        cons = np.zeros((1, L), np.int8)
        kw = dict(rows=[0], fam_first=[0], fam_count=[70])
        prof = d.profile(flanks, ep, cons, **kw)
        assert len(prof.last_uncapped_row) == 128 and np.all(prof.last_uncapped_row == -1)
        assert not prof.cols.view(np.uint8).any()
        res = d.align(flanks, ep, cons, **kw)
        assert len(res.ends) == 128 and all_none(res.ends)
        assert np.all(res.col_idx == ALN_NONE) and np.all(res.col_ins == 0)
        # ... into a caller's arrays: the records are written, the columns (rows beyond the largest rows[f] = 0) are not
        out, keep = sentinel_alignment(3, 128), sentinel_alignment(3, 128)
        d.align(flanks, ep, cons, out=out, **kw)
        assert all_none(out.ends)
        assert same_bytes(out.col_idx, keep.col_idx) and same_bytes(out.col_ins, keep.col_ins)
        pile = d.pileup(flanks, ep, cons, **kw)
        assert len(pile.ends) == 128 and all_none(pile.ends) and not pile.cols.view(np.uint8).any()
    finally:
        d.close()


def test_one_session_serves_all_four_in_turn():
    """profile, align, pileup, refine, profile on one Device: the calls share their device buffers and none leaves anything behind
    for the next.  The second profile is the first, bit for bit; each of the others is the same call on a fresh Device."""
    _, _, cons = family()

    def calls(d, flanks, ep):
        return dict(profile=lambda: d.profile(flanks, ep, cons, row_best=True), align=lambda: d.align(flanks, ep, cons),
                    pileup=lambda: d.pileup(flanks, ep, cons), refine=lambda: d.refine(flanks, ep, cons, max_replays=3))

    fresh = {}
    for name in ("align", "pileup", "refine"):
        d, (arr, _), ep = session()
        try:
            fresh[name] = calls(d, (arr, 70), ep)[name]()
        finally:
            d.close()
    d, (arr, _), ep = session()
    try:
        c = calls(d, (arr, 70), ep)
        first, al, pl, rf, second = c["profile"](), c["align"](), c["pileup"](), c["refine"](), c["profile"]()
    finally:
        d.close()
    assert first.cols["total"][0, :len(cons)].any()
    for k in ("cols", "last_uncapped_row", "row_best", "row_best_idx"):
        assert same_bytes(getattr(second, k), getattr(first, k)), k
    assert (al.ends["end_row"] >= 0).any() and pl.cols["cover"].sum() > 0
    for k in ("ends", "col_idx", "col_ins"):
        assert same_bytes(getattr(al, k), getattr(fresh["align"], k)), k
    for k in ("cols", "ends"):
        assert same_bytes(getattr(pl, k), getattr(fresh["pileup"], k)), k
    for k in ("cons", "rows", "replays", "converged", "cols", "ends"):
        assert same_bytes(getattr(rf, k), getattr(fresh["refine"], k)), k
    assert int(rf.replays[0]) > 1                                            # the refinement did replay more than once


@pytest.mark.parametrize("name", ["profile", "align", "pileup"])
def test_a_replay_ends_the_direction(name):
    """A replay packs its own windows into the direction's buffers: run_direction after it, without a new begin_direction, is
    RAMX_ERR_STATE (-104) and runs nothing; after begin_direction the direction is what it was."""
    from repeatafterme_amd import _lib
    from repeatafterme_amd.device import resolve_flanks
    fs, _, cons = family()
    d, (arr, _), ep = session()
    try:
        direction = resolve_flanks(1, fs.cores, W, L)[0]
        d.begin_direction(direction, ep)
        before = d.run_direction()
        cons_before = d.download()[0].copy()
        d.begin_direction(direction, ep)
        getattr(d, name)((arr, 70), ep, cons)
        with pytest.raises(_lib.RamxError, match=r"\(-104\)"):
            d.run_direction()
        d.begin_direction(direction, ep)
        after = d.run_direction()
        assert (after.ret, after.rows_executed) == (before.ret, before.rows_executed) and before.rows_executed > 0
        assert np.array_equal(d.download()[0], cons_before)
    finally:
        d.close()
