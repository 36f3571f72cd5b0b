"""The bit planes of a replay and the Gram matrix of chosen planes on the device (C-ABI ramx_dev_planes, ramx_dev_plane_gram)
against the restatement of tests/linkage_ref.py: the planes' words and every count are integers, everything is exact.  The
shapes, families and layouts are those of tests/test_gpu_pileup.py, tests/test_gpu_replay_long.py and tests/copystats_ref.py.
The kernel's edges: 64 planes a block side (1, 63, 64, 65 and 130 planes), 32 tiles a chunk (32 and 33 tiles)."""
import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import PLANE_COVER, new_master

import copystats_ref as cr
import linkage_ref as lr
import pileup_ref as pr
import test_gpu_pileup as tp
import test_gpu_replay_long as rl
from helpers import to_extend_params

pytestmark = pytest.mark.gpu


def check_gram(d, pl, planes, n_flanks, tag):
    """One plane list of one family on the resident replay: the words, then the counts."""
    co, bits = d.plane_gram(planes, bits=True)
    want_bits = lr.words(pl, planes, n_flanks)
    assert bits.shape == want_bits.shape and np.array_equal(bits, want_bits), f"{tag}: planes {np.flatnonzero((bits != want_bits).any(axis=1))[:8]}"
    want = lr.gram(pl, planes)
    assert co.shape == want.shape and np.array_equal(co, want), f"{tag}: {np.argwhere(co != want)[:8]}"
    assert np.array_equal(d.plane_gram(planes), co), tag                     # without the words: the same counts


def run_case(c, direction, tag, lists=None):
    from repeatafterme_amd.device import Device, resolve_flanks, select_planes
    ep, cons, rows = to_extend_params(c["p"]), c["cons"], len(c["cons"])
    pl = c["planes"] if "planes" in c else lr.planes_of(direction, c["fs"].cores, c["idx"], c["results"], c["seq"], c["p"].bandwidth, cons)
    d = Device(0)
    try:
        d.load_library(c["seq"])
        flanks, idx = resolve_flanks(direction, c["fs"].cores, c["p"].bandwidth, c["p"].L)
        assert list(idx) == c["idx"], tag
        pile = d.pileup(flanks, ep, cons)
        res = d.planes(flanks, ep, cons)
        tp.same_pileup(res.cols[0, :rows], c["cols"], tag)
        assert np.array_equal(res.cols, pile.cols) and np.array_equal(res.ends, pile.ends), tag
        assert len(res.kernel_ms) == 4 and all(t >= 0 for t in res.kernel_ms)
        sel = select_planes(cons, res.cols[0, :rows], 2, 50, 1024)
        assert np.array_equal(sel, lr.select(cons, c["cols"], 2, 50, 1024)), tag
        for k, planes in enumerate([sel] + ([lr.all_planes(rows)] if 8 * rows <= 2048 else []) + list(lists or [])):
            check_gram(d, pl, planes, len(idx), f"{tag} list {k} ({len(planes)} planes)")
    finally:
        d.close()
    return sel


@pytest.mark.parametrize("n,W,L,matrix", tp.SHAPES)
def test_words_and_counts_match_the_restatement(n, W, L, matrix):
    for direction in (1, 0):
        for what in ("kept", "foreign"):
            sel = run_case(lr.shape_case(n, W, L, matrix, direction, what), direction, f"n={n} W={W} L={L} dir={direction} {what}")
            assert n < 37 or len(sel) > 0


def test_plane_counts_at_the_block_edge_on_one_resident_replay():
    """1, 63, 64, 65 and 130 planes cut from one family's full list: one block, a block one short, a full one, one with a single
    plane in the second block row and column, and three block rows with a partial last -- all on one replay, the call repeated."""
    n, W, L, matrix = tp.SHAPES[4]
    c = lr.shape_case(n, W, L, matrix, 1, "foreign")
    full = lr.all_planes(len(c["cons"]))
    lists = [full[80:80 + k] for k in (1, 63, 64, 65, 130)] + [full[3::7][:65]]
    assert all(lr.gram(c["planes"], x).any() for x in lists)
    run_case(c, 1, "block edge", lists)


def test_tile_counts_at_the_chunk_edge():
    """One family of 2,112 flanks (33 tiles), 40 columns, W = 5, and its first 2,048 flanks (32 tiles) as a family of their own,
    both in one call along the same consensus: one full chunk, and a second chunk of a single tile."""
    from repeatafterme_amd.device import Device, resolve_flanks
    from repeatafterme_amd.synth import synth_family
    n, L, W = 2112, 40, 5
    fs = synth_family(n, L, W, K=30, seed=77, both_sides=True, minus_frac=0.4, n_run_frac=0.1)
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    p = tp.params("14p43g", W, L, when_to_stop=30)
    o = po.oracle_extend(1, fs.cores.copy(), seq, new_master(L), p, trace=True)
    cons = tp.foreign(o.col_base[:o.rows_executed], at=10, k=2)
    rows = len(cons)
    cols, idx, results = pr.pileup(1, fs.cores, seq, p, cons, with_walks=True)
    assert len(idx) == n and rows >= 30
    whole = lr.planes_of(1, fs.cores, idx, results, seq, W, cons)
    low = {k: v & ((1 << 2048) - 1) for k, v in whole.items()}
    assert any(v >> 2048 for v in whole.values())                              # the 33rd tile has bits of its own
    (fl, nx), _ = resolve_flanks(1, fs.cores, W, L)
    flanks, first, count = rl.lay_out([(fl, 2048, 0), (fl, nx, 0)], hole_before=1)
    assert first == [0, 2048 + 64] and count == [2048, 2112]
    planes = lr.all_planes(rows)[:400]
    assert len(planes) > 256
    d = Device(0)
    try:
        d.load_library(seq)
        res = d.planes(flanks, to_extend_params(p), np.stack([np.resize(cons, L)] * 2), rows=[rows, rows], fam_first=first, fam_count=count)
        tp.same_pileup(res.cols[1, :rows], cols, "33 tiles")
        cos, bits = d.plane_gram([planes, planes], bits=True)
    finally:
        d.close()
    for f, (pl, nf) in enumerate(((low, 2048), (whole, 2112))):
        assert bits[f].shape == (len(planes), 32 + f) and np.array_equal(bits[f], lr.words(pl, planes, nf)), f
        assert np.array_equal(cos[f], lr.gram(pl, planes)), f
    assert not np.array_equal(cos[0], cos[1])


def test_families_of_different_rows_in_one_call():
    """Three families along their own consensus over their own number of columns, one of them with rows = 0, and a tile that
    belongs to no family between them (the layout of tests/test_gpu_pileup.py)."""
    from repeatafterme_amd.device import Device, resolve_flanks
    p = tp.params("20p43g", 14, 120, cappenalty=-10, when_to_stop=25)
    fams = tp._three_families()
    lib = np.concatenate([fs.sequence for fs in fams])
    offs = np.cumsum([0] + [len(fs.sequence) for fs in fams])
    cons = np.zeros((3, 120), np.int8)
    rows, parts, want = [], [], []
    for f, fs in enumerate(fams):
        o = po.oracle_extend(1, fs.cores.copy(), fs.sequence, new_master(120), p, trace=True)
        c = tp.foreign(o.col_base[:o.ret], at=8, k=5) if f else o.col_base[:0]               # family 0: rows = 0
        rows.append(len(c))
        cons[f, :len(c)] = c
        cols, idx, results = pr.pileup(1, fs.cores, fs.sequence, p, c, with_walks=True)
        want.append((lr.planes_of(1, fs.cores, idx, results, fs.sequence, 14, c), len(idx), cols))
        (fl, nx), _ = resolve_flanks(1, fs.cores, 14, 120)
        parts.append((fl, nx, offs[f]))
    flanks, first, count = rl.lay_out(parts, hole_before=1)
    assert rows[0] == 0 and rows[1] != rows[2] and min(rows[1:]) > 10
    lists = [lr.as_planes([]), lr.all_planes(rows[1])[5:200], lr.all_planes(rows[2])[::3]]
    d = Device(0)
    try:
        d.load_library(lib)
        res = d.planes(flanks, to_extend_params(p), cons, rows=rows, fam_first=first, fam_count=count)
        cos, bits = d.plane_gram(lists, bits=True)
        with pytest.raises(Exception, match=r"\(-103\)"):                                    # no row of a family with rows = 0
            d.plane_gram([lr.as_planes([(0, 6)]), lists[1], lists[2]])
    finally:
        d.close()
    assert cos[0].shape == (0, 0)
    for f in (1, 2):
        pl, nf, cols = want[f]
        tp.same_pileup(res.cols[f, :rows[f]], cols, f"family {f}")
        assert np.array_equal(bits[f], lr.words(pl, lists[f], nf)) and np.array_equal(cos[f], lr.gram(pl, lists[f])), f
        assert cos[f].any()


@pytest.mark.parametrize("direction", [1, 0])
def test_groups_of_several_tiles_with_a_shorter_last_group(direction, monkeypatch):
    """300 flanks in groups of 2 + 2 + 1 tiles under RAMX_ALIGN_BYTES: the planes' buffer lives across the groups, and the result
    is the restatement's and the run's in one group."""
    from repeatafterme_amd.device import Device, resolve_flanks
    seq, cores, p, cons, want_cols, widx, results = rl.grouped_case(direction)
    pl = lr.planes_of(direction, cores, widx, results, seq, p.bandwidth, cons)
    rows, W, ep = len(cons), p.bandwidth, to_extend_params(p)
    tile_bytes = rows * 64 * (4 * (W // 4 + 1) + 8)
    assert rl.group_sizes(5, tile_bytes, 2 * tile_bytes) == [2, 2, 1]
    planes = lr.select(cons, want_cols, 4, 100, 200)
    assert rows > 257
    edge = lr.as_planes([(r, c) for r in (0, 255, 256, rows - 1) for c in (int(cons[r]), PLANE_COVER)])
    assert len(planes) > 20 and any(v >> 256 for v in pl.values())                  # the last, shorter group has bits of its own
    d = Device(0)
    try:
        d.load_library(seq)
        flanks, idx = resolve_flanks(direction, cores, W, p.L)
        got = {}
        for name, budget in (("one group", None), ("2 + 2 + 1", 2 * tile_bytes)):
            if budget is None:
                monkeypatch.delenv("RAMX_ALIGN_BYTES", raising=False)
            else:
                monkeypatch.setenv("RAMX_ALIGN_BYTES", str(budget))
            res = d.planes(flanks, ep, cons)
            tp.same_pileup(res.cols[0, :rows], want_cols, name)
            got[name] = [d.plane_gram(x, bits=True) for x in (planes, edge)]
            for (co, bits), x in zip(got[name], (planes, edge)):
                assert np.array_equal(bits, lr.words(pl, x, 300)) and np.array_equal(co, lr.gram(pl, x)), name
    finally:
        d.close()
    assert list(idx) == widx


def test_a_long_extension_past_512_columns():
    """Family A of tests/test_gpu_replay_long.py along its foreign consensus of 594 columns, three tiles: 4,752 planes in all,
    of which the selected ones and a cut across columns 255 / 256 and 511 / 512 and the last are asked for."""
    seq, sub, p, cons, want_cols, widx, results = rl.edge_case("A", 130, None, 1)
    c = dict(fs=type("F", (), dict(cores=sub))(), seq=seq, p=p, cons=cons, idx=widx, results=results, cols=want_cols)
    cut = lr.as_planes([(r, k) for r in (254, 255, 256, 257, 510, 511, 512, 513, 592, 593) for k in range(8)])
    assert len(cons) == 594 and lr.gram(lr.planes_of(1, sub, widx, results, seq, p.bandwidth, cons), cut[48:64]).any()    # rows 512, 513
    run_case(c, 1, "long", [cut])


def test_the_limit_of_2048_planes():
    """On the 594-column replay, where 4,752 planes exist: 2,049 valid, strictly increasing planes are refused for their number
    alone, 2,048 are served -- a 32 x 32 grid of blocks, every one full -- and 2,047 too (a partial last block)."""
    from repeatafterme_amd import _lib
    from repeatafterme_amd.device import Device, resolve_flanks
    seq, sub, p, cons, want_cols, widx, results = rl.edge_case("A", 130, None, 1)
    pl = lr.planes_of(1, sub, widx, results, seq, p.bandwidth, cons)
    full = lr.all_planes(len(cons))
    assert len(full) == 4752
    d = Device(0)
    try:
        d.load_library(seq)
        flanks, idx = resolve_flanks(1, sub, p.bandwidth, p.L)
        d.planes(flanks, to_extend_params(p), cons)
        with pytest.raises(_lib.RamxError, match=r"\(-103\).*2049 planes outside \[0, 2048\]"):
            d.plane_gram(full[100:100 + 2049])
        co = d.plane_gram(full[100:100 + 2048])
        co47 = d.plane_gram(full[101:101 + 2047])
    finally:
        d.close()
    assert co.shape == (2048, 2048) and np.array_equal(co, co.T) and np.array_equal(co[1:, 1:], co47)
    # the diagonal is the pileup's; rows and columns of the first, a middle and the last block against the restatement
    names = {0: None, 1: None, 2: None, 3: None, 4: None}
    for k in range(2048):
        r, c = int(full[100 + k]["row"]), int(full[100 + k]["cls"])
        want = want_cols["match"][r][c] if c in names else want_cols["del"][r] if c == 5 else want_cols["cover"][r] if c == 6 else want_cols["ins_open"][r]
        assert co[k, k] == want, (r, c)
    pick = np.r_[0:40, 1000:1040, 2008:2048]
    assert np.array_equal(co[np.ix_(pick, pick)], lr.gram(pl, full[100:100 + 2048][pick])) and co[np.ix_(pick, pick)].any()


@pytest.mark.parametrize("direction", [1, 0])
def test_tail_insertions_set_nothing(direction):
    """copystats_ref.tail_case: W = 7, a gap that pays, paths that end in inserted bases."""
    c = cr.tail_case(direction)
    assert c["p"].gapopen > 0 and sum(r["tail_ins"] > 0 for r in c["results"]) >= 6
    run_case(c, direction, f"tail dir={direction}")


def test_state_and_argument_errors(monkeypatch):
    """All refused on the host, before a launch."""
    from repeatafterme_amd import _lib
    from repeatafterme_amd.device import Device, resolve_flanks
    c = lr.shape_case(*tp.SHAPES[1], 1, "kept")
    ep, cons, rows = to_extend_params(c["p"]), c["cons"], len(c["cons"])
    ok = lr.as_planes([(0, 6), (1, 0), (1, 6)])
    d = Device(0)
    try:
        d.load_library(c["seq"])
        flanks, idx = resolve_flanks(1, c["fs"].cores, 14, 60)
        with pytest.raises(_lib.RamxError, match=r"\(-104\)"):                               # before any planes
            d.plane_gram(ok)
        d.planes(flanks, ep, cons)
        want = lr.gram(c["planes"], ok)
        assert np.array_equal(d.plane_gram(ok), want)
        for bad, why in (([(1, 6), (1, 0)], "not strictly increasing"), ([(1, 0), (0, 6)], "not strictly increasing"),
                         ([(1, 0), (1, 0)], "not strictly increasing"), ([(rows, 0)], "outside the resident replay"),
                         ([(0, 8)], "outside the resident replay"), ([(0, -1)], "outside the resident replay"),
                         ([(-1, 0)], "outside the resident replay")):
            with pytest.raises(_lib.RamxError, match=r"\(-103\).*" + why):
                d.plane_gram(lr.as_planes(bad))
        assert np.array_equal(d.plane_gram(ok), want)                                        # a refused list leaves the planes resident
        d.copy_stats(flanks, ep, cons)
        with pytest.raises(_lib.RamxError, match=r"\(-104\)"):                               # a later replay dropped them
            d.plane_gram(ok)
        need = rows * 8 * 1 * 8
        monkeypatch.setenv("RAMX_LINKAGE_BYTES", str(need - 1))
        with pytest.raises(_lib.RamxError, match=r"\(-106\).*RAMX_LINKAGE_BYTES"):
            d.planes(flanks, ep, cons)
        monkeypatch.setenv("RAMX_LINKAGE_BYTES", str(need))
        d.planes(flanks, ep, cons)
        assert np.array_equal(d.plane_gram(ok), want)
    finally:
        d.close()
