"""The dinucleotide pileup and the CpG-aware refinement on the device (C-ABI ramx_dev_dinuc, ramx_dev_refine_cpg, the CpG sink of
seam 1) against the restatement of tests/dinuc_ref.py: records, consensus, replays, converged and n_cpg.  Counts are integers,
everything is exact."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import DINUC_DTYPE, new_master
from repeatafterme_amd.synth import synth_family

import cpg_cases as cc
import dinuc_ref as dr
import pileup_ref as pr
from helpers import ragged_family, to_extend_params
from test_gpu_pileup import foreign, same_ends, same_pileup

pytestmark = pytest.mark.gpu

FIELDS = ("base", "next", "both", "adjacent", "split", "gapped", "di", "reserved")


def params(matrix, W, L, **kw):
    return po.Params.named(matrix, bandwidth=W, L=L, **kw)


def same_dinuc(got, want, tag):
    assert got.dtype == DINUC_DTYPE and len(got) == len(want), tag
    for k in FIELDS:
        assert np.array_equal(got[k], want[k]), f"{tag}: {k}: rows {np.flatnonzero((got[k] != want[k]).reshape(len(want), -1).any(axis=1))[:8]}"
    assert dr.identities_hold(got), tag


def gpu_dinuc(direction, cores, sequence, p, cons, pileup=True):
    from repeatafterme_amd.device import Device, resolve_flanks
    d = Device(0)
    try:
        d.load_library(np.ascontiguousarray(sequence, np.int8))
        flanks, idx = resolve_flanks(direction, cores, p.bandwidth, p.L)
        res = d.dinuc(flanks, to_extend_params(p), cons, pileup=pileup)
    finally:
        d.close()
    return res, idx


def check_one_family(direction, cores, seq, p, cons, tag, pileup=True):
    """One family along cons on the device against the restatement; -> the restatement's (pileup, records, walks)."""
    cols, di, widx, results = dr.pileups(direction, cores, seq, p, cons, with_walks=True)
    res, idx = gpu_dinuc(direction, cores, seq, p, cons, pileup)
    rows = len(cons)
    assert list(idx) == widx, tag
    same_dinuc(res.di[0, :rows], di, tag)
    assert not res.di[0, rows:].view(np.uint8).any(), tag                              # entries beyond rows: untouched
    if pileup:
        same_pileup(res.cols[0, :rows], cols, tag)
    else:
        assert res.cols is None and res.kernel_ms[2] == 0
    same_ends(res.ends, results, tag)
    assert np.all(res.ends["end_row"][len(idx):] == -1), tag                           # padding flanks
    return cols, di, results


# (flanks, W, L, matrix): one flank; one short of a tile; the tile edge (64, 65); three tiles; the widest band
SHAPES = [(1, 5, 60, "14p43g"), (63, 14, 60, "25p43g"), (64, 20, 60, "14p43g"), (65, 40, 60, "18p43g"), (130, 40, 60, "18p43g"),
          (37, 80, 150, "25p43g")]


@pytest.mark.parametrize("n,W,L,matrix", SHAPES)
def test_dinuc_matches_the_restatement(n, W, L, matrix):
    fs = synth_family(n, L, W, K=L // 2, seed=700 + n + W, both_sides=True, minus_frac=0.4, n_run_frac=0.1)
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    p = params(matrix, W, L, when_to_stop=30)
    seen = dict(adjacent=0, split=0, gapped=0, n=0)
    for direction in (1, 0):
        o = po.oracle_extend(direction, fs.cores.copy(), seq, new_master(L), p, trace=True)
        for what, cons in (("kept", o.col_base[:o.ret]), ("foreign", foreign(o.col_base[:o.rows_executed], at=10, k=3))):
            _, di, _ = check_one_family(direction, fs.cores, seq, p, cons, f"n={n} W={W} L={L} dir={direction} {what}")
            for k in ("adjacent", "split", "gapped"):
                seen[k] += int(di[k].sum())
            seen["n"] += int(di["di"][:, 4, :].sum() + di["di"][:, :, 4].sum())
    assert seen["adjacent"] > 0
    if n >= 37:
        assert seen["split"] > 0 and seen["gapped"] > 0 and seen["n"] > 0, seen           # on the restatement's side
        assert fs.cores.orient.any() and not fs.cores.orient.all()                       # both strands


@functools.lru_cache(maxsize=None)
def ragged():
    """70 copies that end at different columns of a 300-column extension, W = 14 -> (sequence, cores, parameters, the loop's
    consensus per direction)"""
    fs, cores = ragged_family(70, 300, 14, 280, 11, True)
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    seq.setflags(write=False)
    p = params("25p43g", 14, 300, when_to_stop=1000)
    cons = {d: po.oracle_extend(d, cores.copy(), seq, new_master(300), p, trace=True).col_base[:300].copy() for d in (1, 0)}
    return seq, cores, p, cons


@pytest.mark.parametrize("direction", [1, 0])
@pytest.mark.parametrize("rows", [1, 2, 255, 256, 257])
def test_rows_round_the_block_row_of_the_sum(rows, direction):
    """One row has no pair; 255 / 256 / 257 rows end before, at and behind the 256 columns one block row of the sum kernel serves.
    The copies are ragged: one that ends at row r exactly covers r but not the pair (r, r + 1)."""
    seq, cores, p, cons = ragged()
    c = cons[direction][:rows]
    cols, di, results = check_one_family(direction, cores, seq, p, c, f"rows={rows} dir={direction}")
    ends = np.array([r["end_row"] for r in results])
    assert di["next"][-1] == -1 and not di["both"][-1]
    if rows >= 255:
        inner = [r for r in range(rows - 1) if (ends == r).any()]
        assert len(inner) > 10 and all(cols["cover"][r] - di["both"][r] == (ends == r).sum() for r in inner)
        assert (ends >= rows - 2).any() and di["both"][rows - 2] > 0                  # copies reach the last pair


def test_a_positive_gap_term_and_no_pileup():
    fs = synth_family(70, 40, 14, K=25, seed=43, both_sides=True, minus_frac=0.3, n_run_frac=0.1)
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    p = params("14p43g", 14, 40, cappenalty=-10, when_to_stop=1000)
    p.gapopen, p.gapextn = 3, -7
    o = po.oracle_extend(1, fs.cores.copy(), seq, new_master(40), p, trace=True)
    _, di, _ = check_one_family(1, fs.cores, seq, p, o.col_base[:o.ret], "positive gap term", pileup=False)
    assert di["split"].sum() + di["gapped"].sum() > 0


FIVE = ((5, 20, 51, 0), (70, 45, 52, 1), (100, 70, 53, 41), (37, 50, 54, 2), (64, 60, 55, 57))      # (flanks, K, seed, rows)


@functools.lru_cache(maxsize=None)
def five_families():
    """Five families of 0, 1, 41, 2 and 57 columns laid out in 1 + 2 + 2 + 1 + 1 tiles with a tile of no family before the second.
    -> (library, (flank array, n_padded), first, count, rows, cons [5][120], parameters, the restatement per family)"""
    from repeatafterme_amd import _lib
    from repeatafterme_amd.device import resolve_flanks
    p = params("20p43g", 14, 120, cappenalty=-10, when_to_stop=25)
    fams = [synth_family(n, 120, 14, K=K, seed=seed, both_sides=True, minus_frac=0.3, n_run_frac=0.1) for n, K, seed, _ in FIVE]
    lib = np.concatenate([fs.sequence for fs in fams])
    offs = np.cumsum([0] + [len(fs.sequence) for fs in fams])
    cons = np.zeros((5, 120), np.int8)
    tiles = sum((fs.cores.n + 63) // 64 for fs in fams) + 1
    arr = (_lib.Flank * (64 * tiles))()
    for i in range(64 * tiles):
        arr[i].t_lo, arr[i].t_hi, arr[i].step = 1, 0, 1
    rows, first, count, want, at = [], [], [], [], 0
    for f, fs in enumerate(fams):
        o = po.oracle_extend(1, fs.cores.copy(), fs.sequence, new_master(120), p, trace=True)
        c = foreign(o.col_base[:o.rows_executed], at=8, k=5)[:FIVE[f][3]]
        assert len(c) == FIVE[f][3]
        rows.append(len(c))
        cons[f, :len(c)] = c
        want.append(dr.pileups(1, fs.cores, fs.sequence, p, c, with_walks=True))
        (fl, nx), _ = resolve_flanks(1, fs.cores, 14, 120)
        if f == 1:
            at += 64                                                                     # the tile of no family
        first.append(at)
        count.append(nx)
        for i in range(nx):
            arr[at + i] = fl[i]
            arr[at + i].start += int(offs[f])
        at += (nx + 63) // 64 * 64
    assert at == 64 * tiles == 512
    return lib, (arr, 64 * tiles), first, count, rows, cons, p, want


def check_five(res, tag, pileup=True):
    lib, flanks, first, count, rows, cons, p, want = five_families()
    for f in range(5):
        cols, di, _, results = want[f]
        same_dinuc(res.di[f, :rows[f]], di, f"{tag} family {f}")
        assert not res.di[f, rows[f]:].view(np.uint8).any(), f"{tag} family {f}"
        if pileup:
            same_pileup(res.cols[f, :rows[f]], cols, f"{tag} family {f}")
        if rows[f]:
            same_ends(res.ends[first[f]:], results, f"{tag} family {f}")
        else:
            assert np.all(res.ends["end_row"][first[f]:first[f] + 64] == -1)


def test_five_families_in_one_call_and_in_tile_groups(monkeypatch):
    """Five families, rows 0 and 1 among them, in one call; then RAMX_ALIGN_BYTES of three tiles: the eight tiles go through
    groups of 3 + 3 + 2 with both group edges inside a family of two tiles (tiles 2, 3 and 4, 5), and the records are the same."""
    from repeatafterme_amd import _lib
    from repeatafterme_amd.device import Device
    lib, flanks, first, count, rows, cons, p, want = five_families()
    ep = to_extend_params(p)
    kw = dict(rows=rows, fam_first=first, fam_count=count)
    tile_bytes = max(rows) * 64 * (4 * (14 // 4 + 1) + 8)
    d = Device(0)
    try:
        d.load_library(lib)
        monkeypatch.delenv("RAMX_ALIGN_BYTES", raising=False)
        whole = d.dinuc(flanks, ep, cons, **kw)
        check_five(whole, "one group")
        assert whole.kernel_ms[3] > 0
        monkeypatch.setenv("RAMX_ALIGN_BYTES", str(3 * tile_bytes + 1))
        parts = d.dinuc(flanks, ep, cons, **kw)
        assert np.array_equal(parts.di, whole.di) and np.array_equal(parts.cols, whole.cols) and np.array_equal(parts.ends, whole.ends)
        alone = d.dinuc(flanks, ep, cons, pileup=False, **kw)
        assert np.array_equal(alone.di, whole.di) and np.array_equal(alone.ends, whole.ends)
        assert first[1:3] == [128, 256] and count[1] > 64 and count[2] > 64
        monkeypatch.setenv("RAMX_ALIGN_BYTES", str(tile_bytes - 1))
        with pytest.raises(_lib.RamxError, match=r"\(-106\).*RAMX_ALIGN_BYTES"):
            d.dinuc(flanks, ep, cons, **kw)
    finally:
        d.close()


def test_groups_of_two_two_and_one_tile(monkeypatch):
    """One family of 300 flanks (five tiles, the last with 44) under a budget of two tiles: groups of 2 + 2 + 1 tiles, every
    group edge inside the family, and the result of the one-group call."""
    from repeatafterme_amd.device import Device, resolve_flanks
    fs = synth_family(300, 60, 5, K=40, seed=21, both_sides=True, minus_frac=0.4, n_run_frac=0.1)
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    p = params("14p43g", 5, 60, when_to_stop=1000)
    o = po.oracle_extend(1, fs.cores.copy(), seq, new_master(60), p, trace=True)
    cons = foreign(o.col_base[:40], at=8, k=3)
    cols, di, widx, results = dr.pileups(1, fs.cores, seq, p, cons, with_walks=True)
    ends = np.array([r["end_row"] for r in results])
    assert all((ends[a:b] >= 1).any() for a, b in ((0, 128), (128, 256), (256, 300)))          # every group contributes pairs
    tile_bytes = len(cons) * 64 * (4 * (5 // 4 + 1) + 8)
    d = Device(0)
    try:
        d.load_library(seq)
        flanks, idx = resolve_flanks(1, fs.cores, 5, 60)
        assert len(idx) == 300
        monkeypatch.delenv("RAMX_ALIGN_BYTES", raising=False)
        whole = d.dinuc(flanks, to_extend_params(p), cons)
        monkeypatch.setenv("RAMX_ALIGN_BYTES", str(2 * tile_bytes + tile_bytes // 2))
        parts = d.dinuc(flanks, to_extend_params(p), cons)
    finally:
        d.close()
    same_dinuc(whole.di[0, :len(cons)], di, "one group")
    same_pileup(whole.cols[0, :len(cons)], cols, "one group")
    assert np.array_equal(parts.di, whole.di) and np.array_equal(parts.cols, whole.cols) and np.array_equal(parts.ends, whole.ends)


def test_the_pileup_call_is_unchanged_by_a_dinuc_call():
    from repeatafterme_amd.device import Device, resolve_flanks
    fs = synth_family(130, 60, 14, K=30, seed=71, both_sides=True, minus_frac=0.4, n_run_frac=0.1)
    p = params("25p43g", 14, 60, cappenalty=-10, when_to_stop=30)
    ep = to_extend_params(p)
    d = Device(0)
    try:
        d.load_library(np.ascontiguousarray(fs.sequence, np.int8))
        for direction in (1, 0):
            o = po.oracle_extend(direction, fs.cores.copy(), fs.sequence, new_master(60), p, trace=True)
            cons = foreign(o.col_base[:o.ret], at=8, k=5)
            flanks, _ = resolve_flanks(direction, fs.cores, 14, 60)
            before = d.pileup(flanks, ep, cons)
            dn = d.dinuc(flanks, ep, cons)
            after = d.pileup(flanks, ep, cons)
            only = d.dinuc(flanks, ep, cons, pileup=False)
            last = d.pileup(flanks, ep, cons)
            for other in (dn, after, last):
                assert np.array_equal(other.cols, before.cols) and np.array_equal(other.ends, before.ends)
            assert np.array_equal(only.di, dn.di) and (before.cols["cover"] > 0).any()
            # the marginal every record can be checked against: a copy covers r + 1 iff it covers both
            rows = len(cons)
            assert np.array_equal(dn.di["both"][0, :rows - 1], before.cols["cover"][0, 1:rows])
    finally:
        d.close()


def test_no_flank_has_an_alignment_and_no_rows():
    from repeatafterme_amd.datamodel import CoreSet
    p = params("14p43g", 5, 30, when_to_stop=10)
    c = CoreSet(left_pos=[10], right_pos=[12], lower=[0], upper=[79], orient=[0], left_ext=[1], right_ext=[1])
    cons = np.array([1, 2, 3, 0, 1, 1, 2], np.int8)
    res, _ = gpu_dinuc(1, c, np.zeros(80, np.int8), p, cons)
    want = dr.pileups(1, c, np.zeros(80, np.int8), p, cons)[1]
    assert not want["both"].any()
    same_dinuc(res.di[0, :7], want, "no alignment")
    res, _ = gpu_dinuc(1, c, np.zeros(80, np.int8), p, cons[:0])
    assert not res.di.view(np.uint8).any() and res.ends["end_row"][0] == -1


def test_a_family_without_flanks_is_answered_on_the_host():
    from repeatafterme_amd.device import Device, pad_flanks, resolve_flanks
    fs = synth_family(70, 30, 5, K=20, seed=62)
    ep = to_extend_params(params("14p43g", 5, 30))
    d = Device(0)
    try:
        d.load_library(fs.sequence)
        arr, npad = pad_flanks(resolve_flanks(1, fs.cores, 5, 30)[0])
        cons = np.zeros((1, 30), np.int8)
        cons[0] = np.random.default_rng(7).integers(0, 4, 30)
        kw = dict(rows=[10], fam_first=[0], fam_count=[0])
        res = d.dinuc((arr, 0), ep, cons, **kw)
        assert np.array_equal(res.di["base"][0, :10], cons[0, :10]) and np.array_equal(res.di["next"][0, :9], cons[0, 1:10])
        assert res.di["next"][0, 9] == -1 and not res.di[0, 10:].view(np.uint8).any()
        for k in ("both", "adjacent", "split", "gapped", "di", "reserved"):
            assert not res.di[k][0, :10].any(), k
        rf = d.refine_cpg((arr, 0), ep, cons, max_replays=3, **kw)
        assert (int(rf.rows[0]), int(rf.replays[0]), int(rf.converged[0])) == (10, 1, 1) and np.array_equal(rf.cons[0, :10], cons[0, :10])
        assert np.array_equal(rf.di, res.di)
        assert int(rf.n_cpg[0]) == dr.recall_cpg(cons[0, :10], rf.cols[0, :10], rf.di[0, :10], False, ep.matrix, 0, 30)[1]
    finally:
        d.close()


def test_argument_errors_come_before_any_launch():
    from repeatafterme_amd import _lib
    from repeatafterme_amd.device import Device, pad_flanks, resolve_flanks
    fs = synth_family(70, 30, 5, K=20, seed=62)
    ep = to_extend_params(params("14p43g", 5, 30))
    d = Device(0)
    try:
        d.load_library(fs.sequence)
        arr, npad = pad_flanks(resolve_flanks(1, fs.cores, 5, 30)[0])
        good = d.dinuc((arr, npad), ep, np.zeros((1, 30), np.int8), fam_first=[0], fam_count=[70], rows=[10])
        for kw in (dict(fam_first=[32], fam_count=[70], rows=[10]), dict(fam_first=[64], fam_count=[70], rows=[10]),
                   dict(fam_first=[0, 64], fam_count=[70, 10], rows=[10, 10]), dict(fam_first=[0], fam_count=[70], rows=[31])):
            c2 = np.zeros((len(kw["rows"]), 30), np.int8)
            for call in (d.dinuc, d.refine_cpg):
                with pytest.raises(_lib.RamxError, match=r"\(-103\)"):
                    call((arr, npad), ep, c2, **kw)
        cons = np.zeros((1, 30), np.int8)
        cons[0, 3] = 4                                                     # not a base
        with pytest.raises(_lib.RamxError, match=r"\(-103\)"):
            d.dinuc((arr, npad), ep, cons, fam_first=[0], fam_count=[70], rows=[10])
        with pytest.raises(_lib.RamxError, match=r"\(-103\)"):
            d.refine_cpg((arr, npad), ep, np.zeros((1, 30), np.int8), fam_first=[0], fam_count=[70], rows=[10], max_replays=0)
        # di missing, straight through the C-ABI
        import ctypes as C
        from repeatafterme_amd.extend import _params
        cp, keep = _params(ep)
        first, count, rows = (np.array(v, np.int32) for v in ([0], [70], [10]))
        rc = _lib.lib().ramx_dev_dinuc(d._h, arr, npad, first.ctypes.data, count.ctypes.data, 1, C.byref(cp),
                                       np.zeros((1, 30), np.int8).ctypes.data, rows.ctypes.data, None, None, None, None)
        assert rc == -103
        # nothing was launched by any of them: the session's buffers still hold the good call, and it repeats to the byte
        again = d.dinuc((arr, npad), ep, np.zeros((1, 30), np.int8), fam_first=[0], fam_count=[70], rows=[10])
        assert np.array_equal(again.di, good.di) and np.array_equal(again.cols, good.cols) and np.array_equal(again.ends, good.ends)
    finally:
        d.close()


# ---------------------------------------------------------------------------------------------------- the loop

def gpu_refine_cpg(direction, cores, sequence, p, cons, max_replays, cpg_ts=0):
    from repeatafterme_amd.device import Device, resolve_flanks
    d = Device(0)
    try:
        d.load_library(np.ascontiguousarray(sequence, np.int8))
        flanks, _ = resolve_flanks(direction, cores, p.bandwidth, p.L)
        return d.refine_cpg(flanks, to_extend_params(p), cons, max_replays=max_replays, rows_reversed=not direction, cpg_ts=cpg_ts)
    finally:
        d.close()


def same_cpg_refinement(res, f, want, tag):
    cons, cols, di, replays, converged, n_cpg = want
    got = (int(res.rows[f]), int(res.replays[f]), int(res.converged[f]), int(res.n_cpg[f]))
    assert got == (len(cons), replays, converged, n_cpg), (tag, got)
    assert np.array_equal(res.cons[f, :len(cons)], cons), tag
    same_pileup(res.cols[f, :len(cons)], cols, tag)
    same_dinuc(res.di[f, :len(cons)], di, tag)


@functools.lru_cache(maxsize=None)
def planted(direction):
    fs, anc_r, anc_l = cc.planted_family()
    p = params(cc.MATRIX, cc.W, cc.L, when_to_stop=1000)
    o = po.oracle_extend(direction, fs.cores.copy(), fs.sequence, new_master(p.L), p, trace=True)
    return fs, p, o.col_base[:cc.K].copy()


@pytest.mark.parametrize("direction", [1, 0])
def test_the_planted_family_through_the_loop(direction):
    """The plain refinement on the device loses the planted sites, the CpG-aware one calls all eight and differs nowhere else."""
    from test_gpu_refine import gpu_refine
    fs, p, cons = planted(direction)
    want = dr.refine_cpg(direction, fs.cores, fs.sequence, p, cons, 10)
    assert want[3:5] == (2, 1)
    res = gpu_refine_cpg(direction, fs.cores, fs.sequence, p, cons, 10)
    same_cpg_refinement(res, 0, want, f"planted dir={direction}")
    plain = gpu_refine(direction, fs.cores, fs.sequence, p, cons, 10)
    pc, gc = plain.cons[0, :int(plain.rows[0])], res.cons[0, :int(res.rows[0])]
    pair = (cc.C, cc.G) if direction else (cc.G, cc.C)
    called = lambda c: sum((int(c[r]), int(c[r + 1])) == pair for r in cc.sites_in_rows(direction))
    assert called(pc) == 0 and called(gc) == 8 and len(pc) == len(gc)
    assert set(np.flatnonzero(pc != gc).tolist()) <= {x for r in cc.sites_in_rows(direction) for x in (r, r + 1)}
    # the cap, the other direction's reading order, and a score that takes the call away
    capped = dr.refine_cpg(direction, fs.cores, fs.sequence, p, cons, 1)
    assert capped[3:5] == (1, 0)
    same_cpg_refinement(gpu_refine_cpg(direction, fs.cores, fs.sequence, p, cons, 1), 0, capped, "one replay")
    harsh = dr.refine_cpg(direction, fs.cores, fs.sequence, p, cons, 10, cpg_ts=-18)
    assert called(harsh[0]) == 0
    same_cpg_refinement(gpu_refine_cpg(direction, fs.cores, fs.sequence, p, cons, 10, cpg_ts=-18), 0, harsh, "cpg_ts = -18")


@pytest.mark.parametrize("k,direction", [(0, 1), (1, 0), (2, 1)])
def test_the_existing_families_stay_fixed_points(k, direction):
    from test_gpu_refine import family, loop_consensus
    fs, p, K = family(k)
    cons = loop_consensus(k, direction)
    want = dr.refine_cpg(direction, fs.cores, fs.sequence, p, cons, 10)
    assert want[3:5] == (1, 1) and np.array_equal(want[0], cons)
    same_cpg_refinement(gpu_refine_cpg(direction, fs.cores, fs.sequence, p, cons, 10), 0, want, f"fixed point {k} {direction}")
    edited, where = pr.plant_edits(cons)
    want = dr.refine_cpg(direction, fs.cores, fs.sequence, p, edited, 10)
    assert want[3:5] == (2, 1) and np.array_equal(want[0], cons)
    same_cpg_refinement(gpu_refine_cpg(direction, fs.cores, fs.sequence, p, edited, 10), 0, want, f"planted edits {k} {direction}")


def test_the_refinement_does_not_touch_the_plain_one():
    """ramx_dev_refine before and after a ramx_dev_refine_cpg call on one session: the same bytes."""
    from repeatafterme_amd.device import Device, resolve_flanks
    fs, p, cons = planted(1)
    d = Device(0)
    try:
        d.load_library(np.ascontiguousarray(fs.sequence, np.int8))
        flanks, _ = resolve_flanks(1, fs.cores, p.bandwidth, p.L)
        before = d.refine(flanks, to_extend_params(p), cons, max_replays=10)
        d.refine_cpg(flanks, to_extend_params(p), cons, max_replays=10)
        after = d.refine(flanks, to_extend_params(p), cons, max_replays=10)
    finally:
        d.close()
    for k in ("cons", "rows", "replays", "converged", "cols", "ends"):
        assert np.array_equal(getattr(before, k), getattr(after, k)), k


def test_the_sink_of_seam_1():
    """extend_alignment(cpg=n): both directions with their rows_reversed, the loop's results beside it unchanged, and the plain
    refinement sink served beside it."""
    from repeatafterme_amd.extend import extend_alignment
    fs, anc_r, anc_l = cc.planted_family()
    p = params(cc.MATRIX, cc.W, cc.L, when_to_stop=100)
    ep = to_extend_params(p)
    c0, m0 = fs.cores.copy(), new_master(p.L)
    c1, m1 = fs.cores.copy(), new_master(p.L)
    c_o, m_o = fs.cores.copy(), new_master(p.L)
    for direction in (1, 0):
        before = c_o.copy()
        o = po.oracle_extend(direction, c_o, fs.sequence, m_o, p, trace=True)
        plain = extend_alignment(direction, c0, fs.sequence, m0, ep)
        info, rf, cr = extend_alignment(direction, c1, fs.sequence, m1, ep, refine=10, cpg=10)
        for key in ("ret", "rows_executed", "limit_warning", "launches", "persistent", "lanes_per_flank", "packed_rows", "lean_rows"):
            assert getattr(info, key) == getattr(plain, key), key
        kept = o.col_base[:o.ret]
        assert info.ret == o.ret and (cr.direction, cr.family) == (direction, 0) and np.array_equal(cr.cons, kept)
        want = dr.refine_cpg(direction, before, fs.sequence, p, kept, 10)
        assert (cr.replays, cr.converged, cr.n_cpg) == want[3:] and np.array_equal(cr.refined_cons, want[0])
        same_pileup(cr.refined_cols, want[1], f"sink dir={direction}")
        same_dinuc(cr.refined_di, want[2], f"sink dir={direction}")
        wp = pr.refine(direction, before, fs.sequence, p, kept, 10)
        assert (rf.replays, rf.converged) == wp[2:] and np.array_equal(rf.refined_cons, wp[0])
        assert not np.array_equal(rf.refined_cons, cr.refined_cons)                   # the sites the plain rule loses
    assert np.array_equal(m0, m1) and np.array_equal(m1, m_o)
    for key in ("left_len", "right_len", "score"):
        assert np.array_equal(getattr(c0, key), getattr(c1, key)) and np.array_equal(getattr(c1, key), getattr(c_o, key))
    # a direction without an extendable core, and one with ret = 0, are answered on the host
    none = fs.cores.copy()
    none.right_ext[:] = 0
    info, cr = extend_alignment(1, none, fs.sequence, new_master(p.L), ep, cpg=3)
    assert info.ret == 0 and (len(cr.cons), len(cr.refined_cons), len(cr.refined_di)) == (0, 0, 0)
    assert (cr.replays, cr.converged, cr.n_cpg) == (1, 1, 0)
