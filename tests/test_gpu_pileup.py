"""The pileup of an extension on the device (C-ABI ramx_dev_pileup) against the restatement of tests/pileup_ref.py, field by
field: counts are integers, everything is exact."""
import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import PILEUP_DTYPE, PILEUP_INS, CoreSet, new_master
from repeatafterme_amd.synth import synth_family

import pileup_ref as pr
from helpers import to_extend_params

pytestmark = pytest.mark.gpu

FIELDS = ("base", "cover", "match", "del", "ins_open", "ins_long", "ins_bases", "ins")


def params(matrix, W, L, **kw):
    return po.Params.named(matrix, bandwidth=W, L=L, **kw)


def same_pileup(got, want, tag):
    assert got.dtype == PILEUP_DTYPE and len(got) == len(want), tag
    for k in FIELDS:
        assert np.array_equal(got[k], want[k]), f"{tag}: {k}: rows {np.flatnonzero((got[k] != want[k]).reshape(len(want), -1).any(axis=1))[:8]}"


def same_ends(ends, results, tag):
    for i, res in enumerate(results):
        got = tuple(int(ends[i][k]) for k in ("end_row", "end_idx", "score", "start_idx", "tail_ins"))
        assert got == tuple(int(res[k]) for k in ("end_row", "end_idx", "score", "start_idx", "tail_ins")), f"{tag}: flank {i}"


def gpu_pileup(direction, cores, sequence, p, cons):
    from repeatafterme_amd.device import Device, resolve_flanks
    d = Device(0)
    try:
        d.load_library(np.ascontiguousarray(sequence, np.int8))
        flanks, idx = resolve_flanks(direction, cores, p.bandwidth, p.L)
        res = d.pileup(flanks, to_extend_params(p), cons)
    finally:
        d.close()
    return res, idx


def foreign(cons, at=20, k=6):
    """Every seventh base changed and k columns dropped: substitutions, deletions, and insertions longer than the slots."""
    c = np.array(cons, np.int8)
    c[::7] = (c[::7] + 1) & 3
    return np.delete(c, slice(at, at + k))


# (flanks, W, L, matrix): one flank; a partial tile with padding lanes; the tile edge (64, 65); three tiles; the widest band
SHAPES = [(1, 5, 60, "14p43g"), (37, 14, 60, "25p43g"), (64, 20, 60, "14p43g"), (65, 40, 60, "18p43g"), (130, 40, 60, "18p43g"),
          (37, 80, 150, "25p43g")]


@pytest.mark.parametrize("n,W,L,matrix", SHAPES)
def test_pileup_matches_the_restatement(n, W, L, matrix):
    fs = synth_family(n, L, W, K=L // 2, seed=500 + n + W, both_sides=True, minus_frac=0.4, n_run_frac=0.1)
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    p = params(matrix, W, L, when_to_stop=30)
    seen = dict(cover=0, dele=0, ins=0)
    for direction in (1, 0):
        o = po.oracle_extend(direction, fs.cores.copy(), seq, new_master(L), p, trace=True)
        for what, cons in (("kept", o.col_base[:o.ret]), ("foreign", foreign(o.col_base[:o.rows_executed], at=10, k=3))):
            tag = f"n={n} W={W} L={L} dir={direction} {what}"
            want, widx, results = pr.pileup(direction, fs.cores, seq, p, cons, with_walks=True)
            res, idx = gpu_pileup(direction, fs.cores, seq, p, cons)
            assert list(idx) == widx, tag
            same_pileup(res.cols[0, :len(cons)], want, tag)
            same_ends(res.ends, results, tag)
            assert np.all(res.ends["end_row"][len(idx):] == -1), tag                       # padding flanks
            assert not res.cols[0, len(cons):].view(np.uint8).any(), tag                   # entries beyond rows: untouched
            seen["cover"] += int(want["cover"].sum()); seen["dele"] += int(want["del"].sum()); seen["ins"] += int(want["ins_open"].sum())
    assert seen["cover"] > 0
    if n >= 37:
        assert seen["dele"] > 0 and seen["ins"] > 0, seen                                  # on the restatement's side


@pytest.mark.parametrize("direction", [1, 0])
def test_long_insertions_fill_every_slot(direction):
    """Six columns dropped from a foreign consensus: most copies insert six bases there, more than the slots hold."""
    (n, L, W, K, seed), matrix = pr.FAMILIES[0]
    fs = synth_family(n, L, W, K=K, seed=seed, both_sides=True, minus_frac=0.4, n_run_frac=0.1)
    p = params(matrix, W, L, when_to_stop=1000)
    o = po.oracle_extend(direction, fs.cores.copy(), fs.sequence, new_master(L), p, trace=True)
    cons = foreign(o.col_base[:K])
    want = pr.pileup(direction, fs.cores, fs.sequence, p, cons)
    assert want["ins_long"].sum() > 0 and all(want["ins"][:, k].sum() > 0 for k in range(PILEUP_INS))      # on the CPU side
    assert (want["ins_bases"] > want["ins"].sum(axis=(1, 2))).any()
    if direction:
        assert want["match"][:, 4].sum() > 0 and want["ins"][:, :, 4].sum() > 0         # class N, matched and inserted
    res, _ = gpu_pileup(direction, fs.cores, fs.sequence, p, cons)
    same_pileup(res.cols[0, :len(cons)], want, f"long insertions dir={direction}")


def _three_families():
    return [synth_family(n, 120, 14, K=K, seed=seed, both_sides=True, minus_frac=0.3, n_run_frac=0.1)
            for n, K, seed in ((5, 20, 51), (70, 45, 52), (100, 70, 53))]


def test_families_of_different_rows_in_one_call():
    """Three families along their own consensus over their own number of columns, one of them with rows = 0, and a tile that
    belongs to no family between them."""
    from repeatafterme_amd import _lib
    from repeatafterme_amd.device import Device, resolve_flanks
    p = params("20p43g", 14, 120, cappenalty=-10, when_to_stop=25)
    ep = to_extend_params(p)
    fams = _three_families()
    lib = np.concatenate([fs.sequence for fs in fams])
    offs = np.cumsum([0] + [len(fs.sequence) for fs in fams])
    cons = np.zeros((3, 120), np.int8)
    rows, first, count, want = [], [], [], []
    tiles = sum((fs.cores.n + 63) // 64 for fs in fams) + 1
    arr = (_lib.Flank * (64 * tiles))()
    for i in range(64 * tiles):
        arr[i].t_lo, arr[i].t_hi, arr[i].step = 1, 0, 1
    at = 0
    for f, fs in enumerate(fams):
        o = po.oracle_extend(1, fs.cores.copy(), fs.sequence, new_master(120), p, trace=True)
        c = foreign(o.col_base[:o.ret], at=8, k=5) if f else o.col_base[:0]              # family 0: rows = 0
        rows.append(len(c))
        cons[f, :len(c)] = c
        want.append(pr.pileup(1, fs.cores, fs.sequence, p, c, with_walks=True))
        (fl, nx), _ = resolve_flanks(1, fs.cores, 14, 120)
        if f == 1:
            at += 64                                                                     # the tile of no family
        first.append(at)
        count.append(nx)
        for i in range(nx):
            arr[at + i] = fl[i]
            arr[at + i].start += int(offs[f])
        at += (nx + 63) // 64 * 64
    assert rows[0] == 0 and rows[1] != rows[2] and min(rows[1:]) > 10
    d = Device(0)
    try:
        d.load_library(lib)
        res = d.pileup((arr, 64 * tiles), ep, cons, rows=rows, fam_first=first, fam_count=count)
    finally:
        d.close()
    for f in range(3):
        same_pileup(res.cols[f, :rows[f]], want[f][0], f"family {f}")
        assert not res.cols[f, rows[f]:].view(np.uint8).any()
        if rows[f]:
            same_ends(res.ends[first[f]:], want[f][2], f"family {f}")
        else:
            assert np.all(res.ends["end_row"][first[f]:first[f] + 64] == -1)


def test_pileup_in_tile_groups_is_the_same(monkeypatch):
    """RAMX_ALIGN_BYTES of exactly one tile's codes and columns: 130 flanks go through three groups of one tile, and the records
    are the one-group call's; one byte less and the call says that it cannot serve the tile."""
    from repeatafterme_amd import _lib
    fs = synth_family(130, 60, 14, K=30, seed=71, both_sides=True, minus_frac=0.4, n_run_frac=0.1)
    p = params("25p43g", 14, 60, cappenalty=-10, when_to_stop=30)
    o = po.oracle_extend(1, fs.cores.copy(), fs.sequence, new_master(60), p, trace=True)
    cons = foreign(o.col_base[:o.ret], at=8, k=5)
    monkeypatch.delenv("RAMX_ALIGN_BYTES", raising=False)
    whole, idx = gpu_pileup(1, fs.cores, fs.sequence, p, cons)
    assert len(idx) > 128
    same_pileup(whole.cols[0, :len(cons)], pr.pileup(1, fs.cores, fs.sequence, p, cons), "one group")
    tile_bytes = len(cons) * 64 * (4 * (14 // 4 + 1) + 8)
    monkeypatch.setenv("RAMX_ALIGN_BYTES", str(tile_bytes))
    parts, _ = gpu_pileup(1, fs.cores, fs.sequence, p, cons)
    assert np.array_equal(parts.cols, whole.cols) and np.array_equal(parts.ends, whole.ends)
    assert (whole.ends["end_row"][128:len(idx)] >= 0).any()          # the third group did contribute
    monkeypatch.setenv("RAMX_ALIGN_BYTES", str(tile_bytes - 1))
    with pytest.raises(_lib.RamxError, match=r"\(-106\).*RAMX_ALIGN_BYTES"):
        gpu_pileup(1, fs.cores, fs.sequence, p, cons)


def test_a_flank_without_an_alignment_contributes_nothing():
    rng = np.random.default_rng(5)
    seq = rng.integers(0, 4, 80).astype(np.int8)
    p = params("14p43g", 5, 30, when_to_stop=10)
    # a flank without sequence (the core ends where its window ends) beside an ordinary one
    c = CoreSet(left_pos=[70, 10], right_pos=[79, 12], lower=[60, 0], upper=[79, 59], orient=[0, 0], left_ext=[1, 1], right_ext=[1, 1])
    cons = seq[13:33].copy()
    want, _, results = pr.pileup(1, c, seq, p, cons, with_walks=True)
    assert results[0]["end_row"] == -1 and results[1]["end_row"] == 19 and np.all(want["cover"] == 1)
    res, _ = gpu_pileup(1, c, seq, p, cons)
    same_pileup(res.cols[0, :20], want, "empty flank")
    # no flank has an alignment: every count is 0, the bases are the consensus
    c = CoreSet(left_pos=[10], right_pos=[12], lower=[0], upper=[79], orient=[0], left_ext=[1], right_ext=[1])
    cons = np.ones(15, np.int8)
    want = pr.pileup(1, c, np.zeros(80, np.int8), p, cons)
    assert not want["cover"].any()
    res, _ = gpu_pileup(1, c, np.zeros(80, np.int8), p, cons)
    same_pileup(res.cols[0, :15], want, "no alignment")
    # a path that leaves the flank through an edge-fill cell: columns 0..3 are deletions (test_gpu_align.py)
    c = CoreSet(left_pos=[10], right_pos=[12], lower=[16], upper=[79], orient=[0], left_ext=[1], right_ext=[1])
    cons = np.array([seq[13 + r - 1] if r >= 4 else (seq[13 + r + 3] + 2) & 3 for r in range(20)], np.int8)
    want = pr.pileup(1, c, seq, p, cons)
    assert list(want["del"][:5]) == [1, 1, 1, 1, 0]
    res, _ = gpu_pileup(1, c, seq, p, cons)
    same_pileup(res.cols[0, :20], want, "edge fill")
    # rows = 0
    res, _ = gpu_pileup(1, c, seq, p, cons[:0])
    assert not res.cols.view(np.uint8).any() and res.ends["end_row"][0] == -1


def test_ends_are_those_of_the_alignment_call():
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
            al = d.align(flanks, ep, cons)
            pl = d.pileup(flanks, ep, cons)
            again = d.align(flanks, ep, cons)
            assert np.array_equal(pl.ends, al.ends) and (al.ends["end_row"] >= 0).any()
            for k in ("ends", "col_idx", "col_ins"):                       # and the alignment call is what it was
                assert np.array_equal(getattr(again, k), getattr(al, k))
            # the pileup recounted from the alignment call's columns
            rows, nx = len(cons), flanks[1]
            on = np.arange(rows)[:, None] <= al.ends["end_row"][None, :nx]
            assert np.array_equal(pl.cols["cover"][0, :rows], on.sum(axis=1))
            assert np.array_equal(pl.cols["del"][0, :rows], (on & (al.col_idx[:rows, :nx] == -2 ** 31)).sum(axis=1))
            assert np.array_equal(pl.cols["ins_bases"][0, :rows], np.where(on, al.col_ins[:rows, :nx], 0).sum(axis=1))
    finally:
        d.close()


def test_pileup_argument_errors():
    from repeatafterme_amd import _lib
    from repeatafterme_amd.device import Device, pad_flanks, resolve_flanks
    fs = synth_family(70, 30, 5, K=20, seed=62)
    ep = to_extend_params(params("14p43g", 5, 30))
    d = Device(0)
    try:
        d.load_library(fs.sequence)
        arr, npad = pad_flanks(resolve_flanks(1, fs.cores, 5, 30)[0])
        for kw in (dict(fam_first=[32], fam_count=[70], rows=[10]), dict(fam_first=[64], fam_count=[70], rows=[10]),
                   dict(fam_first=[0, 64], fam_count=[70, 10], rows=[10, 10]), dict(fam_first=[0], fam_count=[70], rows=[31])):
            c2 = np.zeros((len(kw["rows"]), 30), np.int8)
            for call in (d.pileup, d.refine):
                with pytest.raises(_lib.RamxError, match=r"\(-103\)"):
                    call((arr, npad), ep, c2, **kw)
        cons = np.zeros((1, 30), np.int8)
        cons[0, 3] = 4                                                     # not a base
        with pytest.raises(_lib.RamxError, match=r"\(-103\)"):
            d.pileup((arr, npad), ep, cons, fam_first=[0], fam_count=[70], rows=[10])
        with pytest.raises(_lib.RamxError, match=r"\(-103\)"):
            d.refine((arr, npad), ep, np.zeros((1, 30), np.int8), fam_first=[0], fam_count=[70], rows=[10], max_replays=0)
    finally:
        d.close()
