"""The replays along a given consensus (C-ABI ramx_dev_profile, ramx_dev_align, ramx_dev_pileup, ramx_dev_refine and their sinks
of seam 1) on extensions of several hundred columns: past the 256 columns one block row of the sum kernels serves, with copies
that end before column 256, between 256 and 512 and behind 512, and in tile groups of several tiles with a shorter last group.
The references are those of the short tests -- the oracle's loop and its row traces, tests/align_ref.py, tests/pileup_ref.py --;
every comparison is exact, and every case first asserts on the reference's side what it is there for."""
import functools
import types

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import ALN_END_DTYPE, ALN_NONE, COL_PROFILE_DTYPE, Profile, new_master

import align_ref as ar
import pileup_ref as pr
from helpers import ragged_family, to_extend_params
from test_gpu_align import check_against_walker
from test_gpu_pileup import foreign, same_ends, same_pileup
from test_gpu_profile import check_against_oracle, derived_from_row_best, replay_reference
from test_gpu_refine import same_refinement

pytestmark = pytest.mark.gpu

# name: (flanks, L, W, K, seed, matrix, windows clipped); all with both sides, 40 % minus strands, runs of N in 10 % of the copies,
# and no early stop (when_to_stop = 1000).  A, W40, W80: the long ragged families; G: five tiles, the last with 44 flanks, for the
# tile groups; R: the refinement's family; F0 .. F4: the families of one call
LONG = {"A": (130, 600, 14, 560, 11, "25p43g", True), "W40": (70, 600, 40, 560, 7, "14p43g", True),
        "W80": (37, 600, 80, 560, 3, "18p43g", True), "G": (300, 320, 5, 300, 21, "14p43g", True),
        "R": (70, 600, 20, 560, 7, "14p43g", False),
        "F0": (5, 600, 14, 560, 31, "25p43g", True), "F1": (70, 600, 14, 560, 32, "25p43g", True),
        "F2": (37, 600, 14, 560, 33, "25p43g", True), "F3": (70, 600, 14, 560, 34, "25p43g", True),
        "F4": (37, 600, 14, 560, 35, "25p43g", True)}


@functools.lru_cache(maxsize=None)
def family(name, W=None):
    """-> (sequence, cores, oracle parameters); shared between the tests and never written to.  W: another band width on the
    same recipe."""
    n, L, W0, K, seed, matrix, clip = LONG[name]
    fs, cores = ragged_family(n, L, W or W0, K, seed, clip)
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    seq.setflags(write=False)
    return seq, cores, po.Params.named(matrix, bandwidth=W or W0, L=L, when_to_stop=1000)


@functools.lru_cache(maxsize=None)
def loop(name, direction, W=None):
    """The oracle's loop over one direction of a family, from its untouched cores, with both traces."""
    seq, cores, p = family(name, W)
    return po.oracle_extend(direction, cores.copy(), seq, new_master(p.L), p, trace=True, row_trace=True)


@functools.lru_cache(maxsize=None)
def foreign_consensus(name, direction):
    """Every seventh base of the loop's consensus changed and the six columns before column 256 dropped."""
    o = loop(name, direction)
    cons = foreign(o.col_base[:o.rows_executed], at=250, k=6)
    cons.setflags(write=False)
    return cons


def end_rows(results):
    return np.array([int(r["end_row"]) for r in results])


def spans_the_edges(results, rows):
    """On the reference's side: copies end in every block row of 256 columns that `rows` columns reach."""
    er = end_rows(results)
    ok = ((er >= 0) & (er < 256)).any()
    if rows > 256:
        ok = ok and ((er >= 256) & (er < 512)).any()
    if rows > 512:
        ok = ok and (er >= 512).any()
    return bool(ok)


def paths_hold_together(direction, cores, widx, results, seq, p, cons):
    """The walker's paths rescored without any DP, and their consumed positions without a hole (tests/test_align_ref.py)."""
    for n, res in zip(widx, results):
        if res["end_row"] >= 0:
            assert ar.rescore(res, ar.Flank(direction, cores, n, p.bandwidth), seq, p, cons) == res["score"], n
            assert ar.consumed_is_contiguous(res), n


def lay_out(parts, hole_before):
    """parts: per family (flank array, number of flanks, offset of its sequence in the library).  Every family begins at a tile
    of its own, and a tile that belongs to no family lies before family `hole_before`.  -> ((array, n_padded), first, count)"""
    from repeatafterme_amd import _lib
    tiles = sum((nx + 63) // 64 for _, nx, _ in parts) + 1
    arr = (_lib.Flank * (64 * tiles))()
    for i in range(64 * tiles):
        arr[i].t_lo, arr[i].t_hi, arr[i].step = 1, 0, 1
    at, first, count = 0, [], []
    for f, (fl, nx, off) in enumerate(parts):
        if f == hole_before:
            at += 64
        first.append(at)
        count.append(nx)
        for i in range(nx):
            arr[at + i] = fl[i]
            arr[at + i].start += int(off)
        at += (nx + 63) // 64 * 64
    assert at == 64 * tiles
    return (arr, 64 * tiles), first, count


# ------------------------------------------------------------------------------ 1. pileup and alignments at the block-row edges

# (family, flanks, columns): the loop's own consensus cut to 255 / 256 / 257 and 512 / 513 columns, the edges of the sum kernel's
# block rows of 256 columns -- a prefix of a consensus is a consensus --, and None: the whole foreign consensus, 594 columns.  The
# boundary lengths of the W = 14 family take its first 70 flanks (two tiles, the second partial), its full length all 130 (three
# tiles).  The foreign consensus is not cut: behind its six dropped columns no copy is back above its earlier best by column 256.
CUTS = [("A", 70, 255), ("A", 70, 256), ("A", 70, 257), ("A", 70, 512), ("A", 70, 513), ("A", 130, None),
        ("W40", 70, 255), ("W40", 70, 256), ("W40", 70, 257), ("W40", 70, 512), ("W40", 70, 513), ("W40", 70, None),
        ("W80", 37, 257), ("W80", 37, None)]


def edge_case(name, n, cut, direction):
    """The reference side of one case of CUTS, with what the case is there for asserted."""
    seq, cores, p = family(name)
    sub = cores.subset(slice(0, n))
    cons = loop(name, direction).col_base[:cut] if cut else foreign_consensus(name, direction)
    rows = len(cons)
    assert rows == (cut or 594)
    want, widx, results = pr.pileup(direction, sub, seq, p, cons, with_walks=True)
    er = end_rows(results)
    assert len(widx) == n and (er >= 0).all()
    assert spans_the_edges(results, rows), np.bincount(er // 256)
    if rows in (257, 513):
        assert (er == rows - 1).any()                                    # copies whose end cell is in the last block row's only column
    if rows >= 512:                                                      # gaps behind column 256, counted by the walker
        assert want["del"][256:].sum() > 0 and want["ins_open"][256:].sum() > 0
    if cut is None:
        assert want["del"][512:].sum() + want["ins_open"][512:].sum() > 0
        assert want["ins_long"][240:256].sum() > 0                       # the six dropped columns: insertions longer than the slots
        if name == "A" and direction == 1:
            assert want["ins_long"][256:].sum() > 0 and want["match"][256:, 4].sum() > 0
    paths_hold_together(direction, sub, widx, results, seq, p, cons)
    return seq, sub, p, cons, want, widx, results


@pytest.mark.parametrize("direction", [1, 0])
@pytest.mark.parametrize("name,n,cut", CUTS)
def test_pileup_and_alignments_at_the_block_row_edges(name, n, cut, direction):
    from repeatafterme_amd.device import Device, resolve_flanks
    seq, sub, p, cons, want, widx, results = edge_case(name, n, cut, direction)
    rows, tag = len(cons), f"{name} n={n} rows={len(cons)} dir={direction}"
    d = Device(0)
    try:
        d.load_library(seq)
        flanks, idx = resolve_flanks(direction, sub, p.bandwidth, p.L)
        pl = d.pileup(flanks, to_extend_params(p), cons)
        al = d.align(flanks, to_extend_params(p), cons)
    finally:
        d.close()
    nx = len(idx)
    assert list(idx) == widx, tag
    same_pileup(pl.cols[0, :rows], want, tag)
    same_ends(pl.ends, results, tag)
    assert not pl.cols[0, rows:].view(np.uint8).any(), tag                               # entries beyond rows: untouched
    assert len(pl.ends) > nx and np.all(pl.ends["end_row"][nx:] == -1), tag              # padding flanks
    assert al.col_idx.shape == (rows, len(pl.ends)), tag
    check_against_walker(al.ends, al.col_idx, al.col_ins, results, rows, tag)
    assert np.all(al.ends["end_row"][nx:] == -1) and np.all(al.col_idx[:, nx:] == ALN_NONE) and not al.col_ins[:, nx:].any(), tag


# --------------------------------------------------------------------- 2. families of different lengths in one call, across the edges

ONE_CALL = ("F0", "F1", "F2", "F3", "F4")
ONE_CALL_ROWS = (0, 256, 257, 600, 40)


@functools.lru_cache(maxsize=None)
def one_call_family(name, rows):
    """One family of the call along the first `rows` columns of its own loop's consensus (direction 1): the consensus, the
    restatement's pileup and walks, with what the family is there for asserted."""
    seq, cores, p = family(name)
    o = loop(name, 1)
    assert o.rows_executed == 600
    cons = o.col_base[:rows].copy()
    cons.setflags(write=False)
    want, widx, results = pr.pileup(1, cores, seq, p, cons, with_walks=True)
    if rows >= 256:
        assert spans_the_edges(results, rows), np.bincount(end_rows(results) // 256)
    if rows == 257:
        assert (end_rows(results) == 256).any()
    if rows == 600:
        assert want["del"][256:].sum() > 0 and want["ins_open"][256:].sum() > 0
    return cons, want, widx, results


def one_call_layout(names, rows, hole_before):
    """-> (library, (flank array, n_padded), first, count, cons [n][600])"""
    from repeatafterme_amd.device import resolve_flanks
    seqs = [family(name)[0] for name in names]
    offs = np.cumsum([0] + [len(s) for s in seqs])
    parts, cons = [], np.zeros((len(names), 600), np.int8)
    for f, name in enumerate(names):
        _, cores, p = family(name)
        (fl, nx), idx = resolve_flanks(1, cores, p.bandwidth, p.L)
        assert list(idx) == one_call_family(name, rows[f])[2]
        parts.append((fl, nx, offs[f]))
        cons[f, :rows[f]] = one_call_family(name, rows[f])[0]
    flanks, first, count = lay_out(parts, hole_before)
    return np.concatenate(seqs), flanks, first, count, cons


def check_one_call_pileup(res, names, rows, first, tag):
    for f, name in enumerate(names):
        _, want, _, results = one_call_family(name, rows[f])
        same_pileup(res.cols[f, :rows[f]], want, f"{tag} family {f}")
        assert not res.cols[f, rows[f]:].view(np.uint8).any(), f"{tag} family {f}"      # entries beyond rows[f]: zero
        if rows[f]:
            same_ends(res.ends[first[f]:], results, f"{tag} family {f}")
        else:
            assert np.all(res.ends["end_row"][first[f]:first[f] + 64] == -1)


def check_one_call_alignments(res, names, rows, first, count, tag):
    for f, name in enumerate(names):
        _, _, _, results = one_call_family(name, rows[f])
        a, w = first[f], (count[f] + 63) // 64 * 64
        if rows[f]:
            check_against_walker(res.ends[a:], res.col_idx[:, a:], res.col_ins[:, a:], results, rows[f], f"{tag} family {f}")
        assert np.all(res.ends["end_row"][a + count[f]:a + w] == -1) and (rows[f] or np.all(res.ends["end_row"][a:a + w] == -1))
        assert np.all(res.col_idx[rows[f]:, a:a + w] == ALN_NONE) and not res.col_ins[rows[f]:, a:a + w].any(), f"{tag} family {f}"
        assert np.all(res.col_idx[:, a + count[f]:a + w] == ALN_NONE) and not res.col_ins[:, a + count[f]:a + w].any()


def marked_alignment(npad, maxrows):
    """An alignment result to write into, every entry marked: what a call leaves alone still reads -7."""
    from repeatafterme_amd.device import AlignResult
    ends = np.zeros(npad, ALN_END_DTYPE)
    ends["end_row"] = ends["score"] = -7
    return AlignResult(ends, np.full((maxrows, npad), -7, np.int32), np.full((maxrows, npad), -7, np.int32), 0.0, 0.0)


def test_families_across_the_edges_in_one_pileup_and_one_alignment_call():
    """Five families of 0, 256, 257, 600 and 40 columns and a tile of no family between them: the longest family makes the sums
    run three block rows, and the shorter ones come back exactly, with nothing written behind their own columns."""
    from repeatafterme_amd.device import Device
    lib, flanks, first, count, cons = one_call_layout(ONE_CALL, ONE_CALL_ROWS, 1)
    ep = to_extend_params(family("F0")[2])
    out = marked_alignment(flanks[1], 600)
    d = Device(0)
    try:
        d.load_library(lib)
        pl = d.pileup(flanks, ep, cons, rows=list(ONE_CALL_ROWS), fam_first=first, fam_count=count)
        al = d.align(flanks, ep, cons, rows=list(ONE_CALL_ROWS), fam_first=first, fam_count=count, out=out)
    finally:
        d.close()
    check_one_call_pileup(pl, ONE_CALL, ONE_CALL_ROWS, first, "pileup")
    check_one_call_alignments(al, ONE_CALL, ONE_CALL_ROWS, first, count, "align")
    hole = slice(first[1] - 64, first[1])
    assert np.all(pl.ends["end_row"][hole] == -1)
    assert np.all(al.ends["end_row"][hole] == -7) and np.all(al.col_idx[:, hole] == -7) and np.all(al.col_ins[:, hole] == -7)


def test_families_across_the_edges_in_one_profile_call():
    """The same layout through ramx_dev_profile with the row buffers, every family against its own loop's first rows[f] rows."""
    from repeatafterme_amd.device import Device
    lib, flanks, first, count, cons = one_call_layout(ONE_CALL, ONE_CALL_ROWS, 1)
    p = family("F0")[2]
    out = np.zeros((5, 600), COL_PROFILE_DTYPE)
    out["total"], out["base"], out["n_capped"] = -7, -7, -7
    d = Device(0)
    try:
        d.load_library(lib)
        res = d.profile(flanks, to_extend_params(p), cons, rows=list(ONE_CALL_ROWS), fam_first=first, fam_count=count, row_best=True,
                        out=out)
    finally:
        d.close()
    assert res.row_best.shape == (600, flanks[1])
    for f, name in enumerate(ONE_CALL):
        o, rows, idx = loop(name, 1), ONE_CALL_ROWS[f], np.array(one_call_family(name, ONE_CALL_ROWS[f])[2])
        a, nx = first[f], count[f]
        # the loop's rows do not depend on the rows behind them: its first rows[f] rows are the replay of that prefix
        prefix = types.SimpleNamespace(rows_executed=rows, col_sums=o.col_sums, col_base=o.col_base, col_score=o.col_score, row_best=o.row_best)
        prof = Profile(1, f, min(o.ret, rows), res.cols[f, :rows], idx, res.last_uncapped_row[a:a + nx])
        check_against_oracle(1, prefix, prof, rows, p.cappenalty, f"family {f}")
        assert np.array_equal(res.row_best[:rows, a:a + nx], o.row_best[:rows, idx]), f
        assert np.array_equal(res.row_best_idx[:rows, a:a + nx], o.row_best_idx[:rows, idx]), f
        assert np.all(res.cols[f, rows:]["total"] == -7) and np.all(res.cols[f, rows:]["base"] == -7), f
        assert np.all(res.last_uncapped_row[a + nx:a + (nx + 63) // 64 * 64] == -1), f
        if rows == 600:
            assert derived_from_row_best(o.row_best[:, idx], rows, p.cappenalty)[1][300:].max() > 0      # capped flanks behind column 256


# ------------------------------------------------------------------------------------------ 3. the profile past 256 columns

@pytest.mark.parametrize("W", [5, 14, 20, 40, 80])
def test_profile_past_256_columns_on_chip_and_through_the_global_buffer(W, monkeypatch):
    """test_gpu_profile.py's comparison of the two row routes at L = 600 on family A's recipe: W = 14/20/40/80 keep the rows on
    chip unless RAMX_PROFILE_NO_RESIDENT is set, W = 5 has the global row buffer only; with and without the row buffers (asking
    for them switches the LEAN band off); both directions; all against the oracle, the out-of-sequence count for W = 14 against
    the oracle's single-row function as well."""
    from repeatafterme_amd.device import Device, resolve_flanks
    seq, cores, p = family("A", W)
    got = {}
    d = Device(0)
    try:
        d.load_library(seq)
        for direction in (1, 0):
            o = loop("A", direction, W)
            assert o.rows_executed == 600
            flanks, idx = resolve_flanks(direction, cores, W, p.L)
            for rb in (False, True):
                for off in (False, True):
                    if off:
                        monkeypatch.setenv("RAMX_PROFILE_NO_RESIDENT", "1")
                    else:
                        monkeypatch.delenv("RAMX_PROFILE_NO_RESIDENT", raising=False)
                    got[direction, rb, off] = d.profile(flanks, to_extend_params(p), o.col_base[:600], rows=600, row_best=rb), idx
    finally:
        d.close()
    for (direction, rb, off), (res, idx) in got.items():
        o, nx, key = loop("A", direction, W), len(idx), (W, direction, rb, off)
        n_new, n_cap, last = derived_from_row_best(o.row_best[:, idx], 600, p.cappenalty)
        assert n_cap[300:].max() > 0 and 0 < (last < 256).sum() < nx, key   # on the oracle's side: capped flanks behind column 256
        c = res.cols[0, :600]
        assert np.array_equal(c["total"], o.col_sums[:600]), key
        assert np.array_equal(c["base"], o.col_base[:600]) and np.array_equal(c["n_new_high"], n_new) and np.array_equal(c["n_capped"], n_cap), key
        assert np.array_equal(res.last_uncapped_row[:nx], last) and np.all(res.last_uncapped_row[nx:] == -1), key
        assert np.array_equal(c, got[direction, False, True][0].cols[0, :600]), key       # n_out_of_seq included
        if rb:
            assert np.array_equal(res.row_best[:600, :nx], o.row_best[:600, idx]), key
            assert np.array_equal(res.row_best_idx[:600, :nx], o.row_best_idx[:600, idx]), key
    if W == 14:
        ref = replay_reference(1, cores, seq, p, loop("A", 1, W).col_base[:600])
        assert ref[1][256:, 2].max() > 0                                    # flanks do run out of sequence behind column 256
        assert np.array_equal(got[1, False, False][0].cols[0, :600]["n_out_of_seq"], ref[1][:, 2])


# ------------------------------------------------------------------ 4. tile groups of several tiles with a shorter last group

def group_sizes(tiles, tile_bytes, budget):
    """Tiles per group under RAMX_ALIGN_BYTES = budget (include/ramx.h): as many whole tiles as fit, the last group the rest."""
    group = min(budget // tile_bytes, tiles)
    return [min(group, tiles - t) for t in range(0, tiles, group)]


@functools.lru_cache(maxsize=None)
def grouped_case(direction):
    seq, cores, p = family("G")
    cons = foreign_consensus("G", direction)
    assert len(cons) == 314
    want, widx, results = pr.pileup(direction, cores, seq, p, cons, with_walks=True)
    er = end_rows(results)
    assert len(widx) == 300 and ((er >= 0) & (er < 256)).sum() > 250 and (er >= 256).sum() > 10
    assert (er[256:] >= 256).any()                                       # ... one of them in the last, shorter group
    assert ((er < 0).sum() == 1) == (direction == 0)                     # one flank on the left has no alignment at all
    return seq, cores, p, cons, want, widx, results


@pytest.mark.parametrize("direction", [1, 0])
def test_groups_of_several_tiles_with_a_shorter_last_group(direction, monkeypatch):
    """300 flanks are five tiles, the last with 44 flanks; RAMX_ALIGN_BYTES makes them groups of 2 + 2 + 1, 3 + 2 and 4 + 1 tiles:
    the walk's rebased column arrays and the codes' group-wide row stride with a last group narrower than the stride.  Every
    run equals the restatement and, byte for byte, the run in one group."""
    from repeatafterme_amd.device import Device, resolve_flanks
    seq, cores, p, cons, want, widx, results = grouped_case(direction)
    rows, W, ep = len(cons), p.bandwidth, to_extend_params(p)
    pile_bytes, align_bytes = rows * 64 * (4 * (W // 4 + 1) + 8), rows * 64 * 4 * (W // 4 + 1)
    budgets = [(None, [5]), (lambda t: 2 * t, [2, 2, 1]), (lambda t: 4 * t - 1, [3, 2]), (lambda t: 4 * t, [4, 1])]
    got = []
    d = Device(0)
    try:
        d.load_library(seq)
        flanks, idx = resolve_flanks(direction, cores, W, p.L)
        assert list(idx) == widx
        for budget, groups in budgets:
            for tile_bytes, call in ((pile_bytes, d.pileup), (align_bytes, d.align)):
                if budget is None:
                    monkeypatch.delenv("RAMX_ALIGN_BYTES", raising=False)
                else:
                    assert group_sizes(5, tile_bytes, budget(tile_bytes)) == groups
                    monkeypatch.setenv("RAMX_ALIGN_BYTES", str(budget(tile_bytes)))
                got.append(call(flanks, ep, cons))
    finally:
        d.close()
    for k, (_, groups) in enumerate(budgets):
        pl, al, tag = got[2 * k], got[2 * k + 1], f"dir={direction} groups {groups}"
        same_pileup(pl.cols[0, :rows], want, tag)
        same_ends(pl.ends, results, tag)
        check_against_walker(al.ends, al.col_idx, al.col_ins, results, rows, tag)
        assert np.array_equal(pl.cols, got[0].cols) and np.array_equal(pl.ends, got[0].ends), tag
        assert np.array_equal(al.ends, got[1].ends) and np.array_equal(al.col_idx, got[1].col_idx) and np.array_equal(al.col_ins, got[1].col_ins), tag


def test_refinement_in_groups_of_several_tiles(monkeypatch):
    """Three replays of the 300 flanks (left direction, with its flank without an alignment) in groups of 2 + 2 + 1 tiles."""
    from repeatafterme_amd.device import Device, resolve_flanks
    seq, cores, p, cons, _, _, _ = grouped_case(0)
    want = pr.refine(0, cores, seq, p, cons, 3)
    assert want[2:] == (3, 1) and len(want[0]) == 314 and not np.array_equal(want[0], cons)
    tile_bytes = len(cons) * 64 * (4 * (p.bandwidth // 4 + 1) + 8)
    assert group_sizes(5, tile_bytes, 2 * tile_bytes) == [2, 2, 1]
    d = Device(0)
    try:
        d.load_library(seq)
        flanks, _ = resolve_flanks(0, cores, p.bandwidth, p.L)
        monkeypatch.delenv("RAMX_ALIGN_BYTES", raising=False)
        whole = d.refine(flanks, to_extend_params(p), cons, max_replays=3)
        monkeypatch.setenv("RAMX_ALIGN_BYTES", str(2 * tile_bytes))
        parts = d.refine(flanks, to_extend_params(p), cons, max_replays=3)
    finally:
        d.close()
    same_refinement(whole, 0, want, "one group")
    same_refinement(parts, 0, want, "groups of two tiles")
    for k in ("cons", "rows", "replays", "converged", "cols", "ends"):
        assert np.array_equal(getattr(parts, k), getattr(whole, k)), k


def test_families_in_groups_whose_edges_fall_inside_a_family(monkeypatch):
    """Three families of section 2 -- one tile, two tiles, the tile of no family, two tiles -- in groups of two tiles: the first
    group ends inside the second family, and the second group holds the tile of no family."""
    from repeatafterme_amd.device import Device
    names, rows = ("F2", "F1", "F3"), (257, 256, 600)
    lib, flanks, first, count, cons = one_call_layout(names, rows, 2)
    assert first == [0, 64, 256] and count == [37, 70, 70] and flanks[1] == 6 * 64
    ep = to_extend_params(family("F1")[2])
    pile_bytes, align_bytes = 600 * 64 * (4 * (14 // 4 + 1) + 8), 600 * 64 * 4 * (14 // 4 + 1)
    assert group_sizes(6, pile_bytes, 2 * pile_bytes) == [2, 2, 2] == group_sizes(6, align_bytes, 2 * align_bytes)
    kw = dict(rows=list(rows), fam_first=first, fam_count=count)
    d = Device(0)
    try:
        d.load_library(lib)
        monkeypatch.delenv("RAMX_ALIGN_BYTES", raising=False)
        pl_whole = d.pileup(flanks, ep, cons, **kw)
        al_whole = d.align(flanks, ep, cons, out=marked_alignment(flanks[1], 600), **kw)
        monkeypatch.setenv("RAMX_ALIGN_BYTES", str(2 * pile_bytes))
        pl = d.pileup(flanks, ep, cons, **kw)
        monkeypatch.setenv("RAMX_ALIGN_BYTES", str(2 * align_bytes))
        al = d.align(flanks, ep, cons, out=marked_alignment(flanks[1], 600), **kw)
    finally:
        d.close()
    check_one_call_pileup(pl, names, rows, first, "groups")
    check_one_call_alignments(al, names, rows, first, count, "groups")
    assert np.array_equal(pl.cols, pl_whole.cols) and np.array_equal(pl.ends, pl_whole.ends)
    assert np.array_equal(al.ends, al_whole.ends) and np.array_equal(al.col_idx, al_whole.col_idx) and np.array_equal(al.col_ins, al_whole.col_ins)
    assert np.all(al.ends["end_row"][192:256] == -7) and np.all(al.col_idx[:, 192:256] == -7)      # the tile of no family


# --------------------------------------------------------------------------- 5. refinement whose length changes across the edges

# case: (direction, the columns dropped from the loop's consensus or "planted" / None, replays and verdict of the restatement)
REFINE_CASES = {"fixed right": (1, None, (1, 1)), "fixed left": (0, None, (1, 1)),
                "planted right": (1, "planted", (2, 1)), "planted left": (0, "planted", (2, 1)),
                "254..258 dropped": (0, (254, 259), (3, 1)), "253..258 dropped": (0, (253, 259), (3, 1)),
                "510..514 dropped": (0, (510, 515), (3, 1))}


def refine_start(case):
    direction, edit, _ = REFINE_CASES[case]
    cons = loop("R", direction).col_base[:560]
    if edit == "planted":
        edited, where = pr.plant_edits(cons)
        assert where[0] < 256 < where[1] < 512 and where[1] < where[2]      # one edit in each of the first two block rows at least
        return edited
    return cons.copy() if edit is None else np.delete(cons, slice(*edit))


@functools.lru_cache(maxsize=None)
def refine_case(case):
    """-> (direction, the consensus the refinement starts from, pr.refine's answer), the answer's verdict asserted."""
    direction, edit, verdict = REFINE_CASES[case]
    seq, cores, p = family("R")
    start = refine_start(case)
    want = pr.refine(direction, cores, seq, p, start, 10)
    assert want[2:] == verdict, (case, want[2:])
    assert np.array_equal(want[0], loop("R", direction).col_base[:560]), case        # a fixed point, or restored to it
    if isinstance(edit, tuple):
        assert len(start) == 560 - (edit[1] - edit[0]) and len(want[0]) == 560      # the length grows again, behind column 256 or 512
    return direction, start, want


def gpu_refine(direction, cores, seq, p, cons, max_replays):
    from repeatafterme_amd.device import Device, resolve_flanks
    d = Device(0)
    try:
        d.load_library(seq)
        flanks, _ = resolve_flanks(direction, cores, p.bandwidth, p.L)
        return d.refine(flanks, to_extend_params(p), cons, max_replays=max_replays)
    finally:
        d.close()


@pytest.mark.parametrize("case", list(REFINE_CASES))
def test_refinement_across_the_block_row_edges(case):
    """560 columns: fixed points, planted edits in three block rows, and five or six columns dropped at 256 and at 512, so that
    the consensus grows through the edge from one replay to the next."""
    seq, cores, p = family("R")
    direction, start, want = refine_case(case)
    same_refinement(gpu_refine(direction, cores, seq, p, start, 10), 0, want, case)


def test_growth_across_the_edge_is_cut_at_L():
    """Six columns dropped before column 256 and L one less than the length the first re-call would give."""
    seq, cores, p600 = family("R")
    cons = loop("R", 0).col_base[:560]
    six = np.delete(cons, slice(253, 259))
    first = pr.pileup(0, cores, seq, p600, six)
    full = len(pr.recall(six, first, 10 ** 6))
    assert full > len(six) + 1 and full > 256
    p = po.Params.named(LONG["R"][5], bandwidth=p600.bandwidth, L=full - 1, when_to_stop=1000)
    assert len(pr.recall(six, first, p.L)) == full - 1
    want = pr.refine(0, cores, seq, p, six, 10)
    assert want[2:] == (3, 1) and len(want[0]) == p.L and np.array_equal(want[0], cons[:p.L]), want[2:]
    same_refinement(gpu_refine(0, cores, seq, p, six, 10), 0, want, "cut at L")


def test_two_long_families_converge_at_different_replays():
    """One call, two families of 560 and 555 columns: the first is a fixed point and drops out, the second takes three replays."""
    from repeatafterme_amd.device import Device, resolve_flanks
    seq, cores, p = family("R")
    _, cons, want0 = refine_case("fixed left")
    _, five, want1 = refine_case("254..258 dropped")
    assert want0[2:] == (1, 1) and want1[2:] == (3, 1)
    (fl, nx), _ = resolve_flanks(0, cores, p.bandwidth, p.L)
    flanks, first, count = lay_out([(fl, nx, 0), (fl, nx, 0)], 1)
    both = np.zeros((2, p.L), np.int8)
    both[0, :560], both[1, :555] = cons, five
    d = Device(0)
    try:
        d.load_library(seq)
        res = d.refine(flanks, to_extend_params(p), both, rows=[560, 555], fam_first=first, fam_count=count, max_replays=10)
    finally:
        d.close()
    same_refinement(res, 0, want0, "family 0")
    same_refinement(res, 1, want1, "family 1")
    w = (nx + 63) // 64 * 64
    assert np.array_equal(res.ends[first[0]:first[0] + w], res.ends[first[1]:first[1] + w])      # both end at the same consensus


# ----------------------------------------------------------------------------------- 6. the sinks of seam 1 on a long extension

@pytest.mark.parametrize("direction", [1, 0])
def test_the_sinks_of_seam_1_on_a_long_extension(direction):
    """extend_alignment(profile=True) and extend_alignment(align=True, refine=10) on family A: more than 512 kept columns, the
    loop's results beside the sinks unchanged, every sink against its reference."""
    from repeatafterme_amd.extend import extend_alignment
    seq, cores, p = family("A")
    ep, o = to_extend_params(p), loop("A", direction)
    assert o.ret > 512
    kept = o.col_base[:o.ret]
    runs = []
    for kw in ({}, dict(profile=True), dict(align=True, refine=10)):
        c, m = cores.copy(), new_master(p.L)
        r = extend_alignment(direction, c, seq, m, ep, **kw)
        runs.append((c, m) + (r if kw else (r,)))
    for c, m, info, *_ in runs:
        for key in ("ret", "rows_executed", "limit_warning", "launches", "persistent", "lanes_per_flank", "packed_rows", "lean_rows"):
            assert getattr(info, key) == getattr(runs[0][2], key), key
        assert (info.ret, info.rows_executed) == (o.ret, o.rows_executed)
        assert np.array_equal(m, o.master)
        for key in ("left_len", "right_len", "score"):
            assert np.array_equal(getattr(c, key), getattr(o, key)), key
    prof, al, rf = runs[1][3], runs[2][3], runs[2][4]
    tag = f"dir={direction}"
    assert prof.ret == o.ret and prof.direction == direction
    check_against_oracle(direction, o, prof, o.rows_executed, p.cappenalty, tag)
    want_cols, widx, results = pr.pileup(direction, cores, seq, p, kept, with_walks=True)
    assert spans_the_edges(results, o.ret) and want_cols["del"][256:].sum() > 0 and want_cols["ins_open"][256:].sum() > 0
    assert np.array_equal(al.cons, kept) and list(al.core_index) == widx and al.direction == direction
    check_against_walker(al.ends, al.col_idx, al.col_ins, results, o.ret, tag)
    assert np.array_equal(rf.cons, kept) and rf.direction == direction
    same_pileup(rf.cols, want_cols, tag + " kept")
    want = pr.refine(direction, cores, seq, p, kept, 10)
    assert (rf.replays, rf.converged) == want[2:] and np.array_equal(rf.refined_cons, want[0]), tag
    same_pileup(rf.refined_cols, want[1], tag + " refined")
