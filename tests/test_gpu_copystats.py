"""The per-copy statistics of an extension on the device (C-ABI ramx_dev_copy_stats) against the restatement of
tests/copystats_ref.py, field by field: counts are integers, everything is exact.  The shapes, families and layouts are those of
tests/test_gpu_pileup.py and tests/test_gpu_replay_long.py; what each case is there for is asserted on the reference's side in
tests/test_copystats_ref.py or here, before the device is asked."""
import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import COPY_STATS_DTYPE, COPY_STATS_FIELDS, new_master

import copystats_ref as cr
import pileup_ref as pr
import test_gpu_pileup as tp
import test_gpu_replay_long as rl
from helpers import to_extend_params

pytestmark = pytest.mark.gpu


def same_stats(got, want, tag):
    assert got.dtype == COPY_STATS_DTYPE and len(got) == len(want), tag
    for k in COPY_STATS_FIELDS:
        assert np.array_equal(got[k], want[k]), f"{tag}: {k}: flanks {np.flatnonzero(got[k] != want[k])[:8]}"


def all_zero(stats):
    return not np.ascontiguousarray(stats).view(np.uint8).any()


def marked(npad):
    """Records to write into, every field marked: what a call leaves alone still reads -7."""
    out = np.zeros(npad, COPY_STATS_DTYPE)
    for k in COPY_STATS_FIELDS:
        out[k] = -7
    return out


def gpu_copy_stats(direction, cores, sequence, p, cons, rows_reversed=None):
    from repeatafterme_amd.device import Device, resolve_flanks
    d = Device(0)
    try:
        d.load_library(np.ascontiguousarray(sequence, np.int8))
        flanks, idx = resolve_flanks(direction, cores, p.bandwidth, p.L)
        res = d.copy_stats(flanks, to_extend_params(p), cons, rows_reversed=(not direction) if rows_reversed is None else rows_reversed)
    finally:
        d.close()
    return res, idx


def check_case(c, direction, tag):
    res, idx = gpu_copy_stats(direction, c["fs"].cores, c["seq"], c["p"], c["cons"])
    nx = len(idx)
    assert list(idx) == c["idx"], tag
    same_stats(res.stats[:nx], c["stats"], tag)
    tp.same_ends(res.ends, c["results"], tag)
    assert len(res.stats) % 64 == 0 and len(res.stats) > nx - 64 and all_zero(res.stats[nx:]), tag    # padding flanks: all zero
    assert np.all(res.ends["end_row"][nx:] == -1), tag
    for s, res_w in zip(res.stats[:nx], c["results"]):                                                # flanks without an alignment
        assert res_w["end_row"] >= 0 or all_zero(s), tag
    return res


@pytest.mark.parametrize("n,W,L,matrix", tp.SHAPES)
def test_copy_stats_match_the_restatement(n, W, L, matrix):
    for direction in (1, 0):
        for what in ("kept", "foreign"):
            check_case(cr.shape_case(n, W, L, matrix, direction, what), direction, f"n={n} W={W} L={L} dir={direction} {what}")


def test_the_row_order_is_the_callers():
    """The same flanks and consensus with the flag the other way round: only the CpG counters differ, as on the restatement."""
    sh = tp.SHAPES[1]
    c = cr.shape_case(*sh, 1, "foreign")
    other = cr.stats_of(1, c["fs"].cores, c["idx"], c["results"], c["seq"], sh[1], c["cons"], True)
    assert not np.array_equal(other["cpg_cols"], c["stats"]["cpg_cols"])
    res, idx = gpu_copy_stats(1, c["fs"].cores, c["seq"], c["p"], c["cons"], rows_reversed=True)
    same_stats(res.stats[:len(idx)], other, "reversed")


@pytest.mark.parametrize("direction", [1, 0])
def test_tail_insertions_a_positive_gap_term_and_a_width_of_its_own(direction):
    """TAIL_FAMILY: paths that end in inserted bases (counted nowhere), under a gap that pays (the forward kernel's row-buffer
    route) and band width 7, which no kernel is instantiated for."""
    c = cr.tail_case(direction)
    assert c["p"].gapopen > 0 and sum(r["tail_ins"] > 0 for r in c["results"]) >= 6
    res = check_case(c, direction, f"tail dir={direction}")
    assert (res.ends["tail_ins"] > 0).sum() >= 6


def test_families_of_different_rows_in_one_call():
    """Three families along their own consensus over their own number of columns, one of them with rows = 0, and a tile that
    belongs to no family between them (the layout of tests/test_gpu_pileup.py): the records of that tile and of the tiles behind
    the last family stay as the caller left them."""
    from repeatafterme_amd import _lib
    from repeatafterme_amd.device import Device, resolve_flanks
    p = tp.params("20p43g", 14, 120, cappenalty=-10, when_to_stop=25)
    ep = to_extend_params(p)
    fams = tp._three_families()
    lib = np.concatenate([fs.sequence for fs in fams])
    offs = np.cumsum([0] + [len(fs.sequence) for fs in fams])
    cons = np.zeros((3, 120), np.int8)
    rows, first, count, want = [], [], [], []
    tiles = sum((fs.cores.n + 63) // 64 for fs in fams) + 2                                  # ... and one more tile behind them
    arr = (_lib.Flank * (64 * tiles))()
    for i in range(64 * tiles):
        arr[i].t_lo, arr[i].t_hi, arr[i].step = 1, 0, 1
    at = 0
    for f, fs in enumerate(fams):
        o = po.oracle_extend(1, fs.cores.copy(), fs.sequence, new_master(120), p, trace=True)
        c = tp.foreign(o.col_base[:o.ret], at=8, k=5) if f else o.col_base[:0]               # family 0: rows = 0
        rows.append(len(c))
        cons[f, :len(c)] = c
        want.append(cr.copy_stats(1, fs.cores, fs.sequence, p, c, rows_reversed=False, with_walks=True))
        (fl, nx), _ = resolve_flanks(1, fs.cores, 14, 120)
        if f == 1:
            at += 64                                                                         # the tile of no family
        first.append(at)
        count.append(nx)
        for i in range(nx):
            arr[at + i] = fl[i]
            arr[at + i].start += int(offs[f])
        at += (nx + 63) // 64 * 64
    assert rows[0] == 0 and rows[1] != rows[2] and min(rows[1:]) > 10 and at == 64 * (tiles - 1)
    assert all(w[0]["del"].sum() > 0 and w[0]["ins"].sum() > 0 for w in want[1:])
    d = Device(0)
    try:
        d.load_library(lib)
        res = d.copy_stats((arr, 64 * tiles), ep, cons, rows=rows, fam_first=first, fam_count=count, rows_reversed=False,
                           out=marked(64 * tiles))
    finally:
        d.close()
    for f in range(3):
        a, w = first[f], (count[f] + 63) // 64 * 64
        same_stats(res.stats[a:a + count[f]], want[f][0], f"family {f}")
        assert all_zero(res.stats[a + count[f]:a + w]), f
        if rows[f]:
            tp.same_ends(res.ends[a:], want[f][2], f"family {f}")
        else:
            assert all_zero(res.stats[a:a + w]) and np.all(res.ends["end_row"][a:a + w] == -1)
    for hole in (slice(first[1] - 64, first[1]), slice(at, at + 64)):
        assert all(np.all(res.stats[k][hole] == -7) for k in COPY_STATS_FIELDS)


@pytest.mark.parametrize("direction", [1, 0])
def test_groups_of_several_tiles_with_a_shorter_last_group(direction, monkeypatch):
    """300 flanks in groups of 2 + 2 + 1 tiles under RAMX_ALIGN_BYTES (the budget is the pileup's): the result is the restatement's
    and, byte for byte, the run in one group; one tile that does not fit is refused in the pileup's words."""
    from repeatafterme_amd import _lib
    from repeatafterme_amd.device import Device, resolve_flanks
    seq, cores, p, cons, _, widx, results = rl.grouped_case(direction)
    want = cr.stats_of(direction, cores, widx, results, seq, p.bandwidth, cons, not direction)
    assert (want["cols"][256:] > 256).any() and want["del"][256:].sum() > 0            # the last, shorter group has work of its own
    rows, W, ep = len(cons), p.bandwidth, to_extend_params(p)
    tile_bytes = rows * 64 * (4 * (W // 4 + 1) + 8)
    assert rl.group_sizes(5, tile_bytes, 2 * tile_bytes) == [2, 2, 1]
    d = Device(0)
    try:
        d.load_library(seq)
        flanks, idx = resolve_flanks(direction, cores, W, p.L)
        monkeypatch.delenv("RAMX_ALIGN_BYTES", raising=False)
        whole = d.copy_stats(flanks, ep, cons, rows_reversed=not direction)
        monkeypatch.setenv("RAMX_ALIGN_BYTES", str(2 * tile_bytes))
        parts = d.copy_stats(flanks, ep, cons, rows_reversed=not direction)
        monkeypatch.setenv("RAMX_ALIGN_BYTES", str(tile_bytes - 1))
        with pytest.raises(_lib.RamxError, match=r"\(-106\).*decision codes and columns.*RAMX_ALIGN_BYTES"):
            d.copy_stats(flanks, ep, cons, rows_reversed=not direction)
    finally:
        d.close()
    assert list(idx) == widx
    same_stats(whole.stats[:300], want, f"dir={direction} one group")
    tp.same_ends(whole.ends, results, f"dir={direction} one group")
    assert np.array_equal(parts.stats, whole.stats) and np.array_equal(parts.ends, whole.ends)
    assert all_zero(whole.stats[300:])


def test_a_long_extension_past_512_columns():
    """Family A of tests/test_gpu_replay_long.py along its foreign consensus of 594 columns: copies end before column 256 and
    behind 512 (asserted by edge_case), three tiles."""
    seq, sub, p, cons, _, widx, results = rl.edge_case("A", 130, None, 1)
    want = cr.stats_of(1, sub, widx, results, seq, p.bandwidth, cons, False)
    assert (want["cols"] <= 256).any() and (want["cols"] > 512).any() and len(cons) == 594
    res, idx = gpu_copy_stats(1, sub, seq, p, cons)
    assert list(idx) == widx
    same_stats(res.stats[:len(idx)], want, "long")
    tp.same_ends(res.ends, results, "long")


def test_the_sums_over_the_copies_are_the_pileups():
    """Device against device, without the CPU walker: the per-copy records summed over the copies against Device.pileup of the
    same call, at (130, 40, 60)."""
    from repeatafterme_amd.device import Device, resolve_flanks
    n, W, L, matrix = tp.SHAPES[4]
    for direction in (1, 0):
        c = cr.shape_case(n, W, L, matrix, direction, "foreign")
        cons, ep = c["cons"], to_extend_params(c["p"])
        d = Device(0)
        try:
            d.load_library(c["seq"])
            flanks, _ = resolve_flanks(direction, c["fs"].cores, W, L)
            st = d.copy_stats(flanks, ep, cons, rows_reversed=not direction)
            pl = d.pileup(flanks, ep, cons)
        finally:
            d.close()
        s, cols = st.stats, pl.cols[0, :len(cons)]
        assert np.array_equal(st.ends, pl.ends)
        assert np.array_equal(s["match"] + s["ts"] + s["tv"] + s["n_match"] + s["del"], s["cols"])
        assert s["cols"].sum() == cols["cover"].sum() > 0 and s["del"].sum() == cols["del"].sum() > 0
        assert s["ins"].sum() == cols["ins_bases"].sum() > 0 and s["ins_open"].sum() == cols["ins_open"].sum() > 0
        assert (s["match"] + s["ts"] + s["tv"] + s["n_match"]).sum() == cols["match"].sum()
        assert s["match"].sum() == sum(int(cols["match"][r, int(cons[r])]) for r in range(len(cons))) > 0
        assert np.array_equal(s["score"], np.where(st.ends["end_row"] >= 0, st.ends["score"], 0))


def test_nothing_to_run_and_argument_errors():
    from repeatafterme_amd import _lib
    from repeatafterme_amd.device import Device, pad_flanks, resolve_flanks
    c = cr.shape_case(*tp.SHAPES[1], 1, "kept")
    ep = to_extend_params(c["p"])
    d = Device(0)
    try:
        d.load_library(c["seq"])
        flanks, _ = resolve_flanks(1, c["fs"].cores, 14, 60)
        res = d.copy_stats(flanks, ep, c["cons"][:0], out=marked(64))                  # rows = 0: answered on the host
        assert all_zero(res.stats) and np.all(res.ends["end_row"] == -1)
        arr, npad = pad_flanks(flanks)
        for kw in (dict(fam_first=[32], fam_count=[37], rows=[10]), dict(fam_first=[0], fam_count=[65], rows=[10]),
                   dict(fam_first=[0], fam_count=[37], rows=[61])):
            with pytest.raises(_lib.RamxError, match=r"\(-103\)"):
                d.copy_stats((arr, npad), ep, np.zeros((1, 60), np.int8), **kw)
    finally:
        d.close()
