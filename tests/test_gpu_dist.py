"""Pairwise divergence between the copies of a replay on the device (C-ABI ramx_dev_copy_dist, include/ramx_dist.h) against the
restatement of tests/dist_ref.py: every field of every record is an integer, everything is exact.  The shapes, families and
layouts are those of tests/test_gpu_pileup.py, tests/test_gpu_replay_long.py and tests/test_gpu_linkage.py.  The kernels' edges:
64 copies a block side, 64 rows a row word, 8 row words a staging chunk, 64 copies a tile."""
import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import COPY_DIST_DTYPE, COPY_DIST_FIELDS, new_master

import copystats_ref as cr
import dist_ref as dr
import linkage_ref as lr
import pileup_ref as pr
import test_gpu_pileup as tp
import test_gpu_replay_long as rl
from helpers import to_extend_params

pytestmark = pytest.mark.gpu

CHUNK_ROWS = 8 * 64                  # RAMX_DIST_CHUNK row words of 64 rows


def comb2(x):
    x = np.asarray(x, np.int64)
    return x * (x - 1) // 2


def check_identities(m, cols, rows, tag):
    """The whole family's matrix against the pileup's columns: pairs counted by copies equal pairs counted by columns."""
    iu = np.triu_indices(len(m), 1)
    up = {f: int(m[f][iu].astype(np.int64).sum()) for f in COPY_DIST_FIELDS}
    mt = cols["match"][:rows].astype(np.int64)
    assert up["sites"] == int(comb2(mt[:, :4].sum(axis=1)).sum()), tag
    assert up["sites"] - up["ts"] - up["tv"] == int(comb2(mt[:, :4]).sum()), tag
    assert up["ts"] == int((mt[:, 0] * mt[:, 2] + mt[:, 1] * mt[:, 3]).sum()), tag
    assert up["del_both"] == int(comb2(cols["del"][:rows]).sum()), tag
    assert up["cover"] == int(comb2(cols["cover"][:rows]).sum()), tag


def check_list(d, maps, copies, tag, want=None):
    got = d.copy_dist(np.asarray(copies, np.int32))
    want = dr.matrix(maps, copies) if want is None else want
    assert got.shape == want.shape and np.array_equal(got, want), f"{tag}: {np.argwhere(got != want)[:8]}"
    for f in COPY_DIST_FIELDS:
        assert np.array_equal(got[f], got[f].T), (tag, f)
    return got


def check_diagonal(m, stats, copies, tag):
    s = stats[np.asarray(copies, np.int64)]
    dg = m[np.arange(len(m)), np.arange(len(m))]
    assert np.array_equal(dg["cover"], s["cols"]) and np.array_equal(dg["sites"], s["match"] + s["ts"] + s["tv"]), tag
    assert np.array_equal(dg["del_both"], s["del"]) and not dg["ts"].any() and not dg["tv"].any() and not dg["del_one"].any(), tag


def run_case(c, direction, tag, lists=(), whole=True):
    """One family on one resident replay: the list of all copies with the identities and the diagonal, then further lists."""
    from repeatafterme_amd.device import Device, resolve_flanks
    ep, cons, rows = to_extend_params(c["p"]), c["cons"], len(c["cons"])
    maps = c["maps"] if "maps" in c else dr.maps_of(direction, c["fs"].cores, c["idx"], c["results"], c["seq"], c["p"].bandwidth, cons)
    n = len(c["idx"])
    d = Device(0)
    try:
        d.load_library(c["seq"])
        flanks, idx = resolve_flanks(direction, c["fs"].cores, c["p"].bandwidth, c["p"].L)
        assert list(idx) == c["idx"], tag
        stats = d.copy_stats(flanks, ep, cons, rows_reversed=not direction).stats
        res = d.planes(flanks, ep, cons)
        if whole:
            m = check_list(d, maps, range(n), tag + " all", c.get("dist"))
            check_diagonal(m, stats, range(n), tag)
            check_identities(m, res.cols[0], rows, tag)
        for k, copies in enumerate(lists):
            m = check_list(d, maps, copies, f"{tag} list {k} ({len(copies)} copies)")
            check_diagonal(m, stats, copies, f"{tag} list {k}")
        ms = d.copy_dist_ms()
        assert len(ms) == 2 and all(t >= 0 for t in ms)
    finally:
        d.close()


@pytest.mark.parametrize("n,W,L,matrix", tp.SHAPES)
def test_every_field_matches_the_restatement(n, W, L, matrix):
    for direction in (1, 0):
        for what in ("kept", "foreign"):
            c = dr.shape_case(n, W, L, matrix, direction, what)
            run_case(c, direction, f"n={n} W={W} L={L} dir={direction} {what}")
            assert n < 37 or (c["dist"]["tv"].any() and c["dist"]["del_one"].any())


def test_copy_counts_at_the_block_edge_on_one_resident_replay():
    """1, 2, 63, 64, 65 and 130 copies of the 130-flank family, a strided list and one that holds only copies 63, 64 and 129
    (three tiles, one copy each; the last lane of a tile and the first of the next): all on one replay, the call repeated."""
    n, W, L, matrix = tp.SHAPES[4]
    c = dr.shape_case(n, W, L, matrix, 1, "foreign")
    lists = [list(range(k)) for k in (1, 2, 63, 64, 65, 130)] + [list(range(130))[3::7], [63, 64, 129]]
    run_case(c, 1, "block edge", lists, whole=False)


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 128, 129])
def test_row_counts_at_the_word_edge(rows):
    """Family A of tests/test_gpu_replay_long.py, its first 70 flanks, along the loop's consensus cut to a row word's edges."""
    seq, cores, p = rl.family("A")
    sub = cores.subset(slice(0, 70))
    cons = rl.loop("A", 1).col_base[:rows].copy()
    cols, idx, results = pr.pileup(1, sub, seq, p, cons, with_walks=True)
    c = dict(fs=type("F", (), dict(cores=sub))(), seq=seq, p=p, cons=cons, idx=idx, results=results, cols=cols)
    run_case(c, 1, f"rows={rows}", [[0, 5, 69]])


@pytest.mark.parametrize("name,n,cut", [("A", 130, None), ("W40", 70, 513), ("W80", 37, None)])
def test_long_extensions_past_one_staging_chunk(name, n, cut):
    """The 600-column families: copies end before column 256, between 256 and 512 and behind 512 (edge_case asserts it), and
    more than 8 x 64 + 65 rows where uncut: the pair kernel's chunk loop runs twice, the second chunk partial."""
    seq, sub, p, cons, want_cols, widx, results = rl.edge_case(name, n, cut, 1)
    assert len(cons) == 513 or len(cons) >= CHUNK_ROWS + 65
    c = dict(fs=type("F", (), dict(cores=sub))(), seq=seq, p=p, cons=cons, idx=widx, results=results, cols=want_cols)
    run_case(c, 1, f"long {name}", [list(range(0, n, 3)), list(range(n - 5, n))], whole=n < 100)


@pytest.fixture(scope="module")
def wide():
    """The 2,112-flank family of tests/test_gpu_linkage.py (33 tiles, 40 columns, W = 5) and its maps."""
    from repeatafterme_amd.synth import synth_family
    n, L, W = 2112, 40, 5
    fs = synth_family(n, L, W, K=30, seed=77, both_sides=True, minus_frac=0.4, n_run_frac=0.1)
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    p = tp.params("14p43g", W, L, when_to_stop=30)
    o = po.oracle_extend(1, fs.cores.copy(), seq, new_master(L), p, trace=True)
    cons = tp.foreign(o.col_base[:o.rows_executed], at=10, k=2)
    cols, idx, results = pr.pileup(1, fs.cores, seq, p, cons, with_walks=True)
    assert len(idx) == n and 30 <= len(cons) <= 64
    return dict(fs=fs, seq=seq, p=p, cons=cons, cols=cols, idx=idx, results=results,
                maps=dr.maps_of(1, fs.cores, idx, results, seq, W, cons))


def test_tile_edges_and_the_limit_of_2048_copies(wide):
    from repeatafterme_amd import _lib
    from repeatafterme_amd.device import Device, resolve_flanks
    c, rows = wide, len(wide["cons"])
    seventy = sorted({0, 63, 64, 2047, 2048, 2111} | set(range(5, 2112, 33)))
    assert len(seventy) == 70 and {0, 63, 64, 2047, 2048, 2111} <= set(seventy)
    small = dr.matrix_of_one_word(c["maps"], seventy, rows)
    assert np.array_equal(small, dr.matrix(c["maps"], seventy))                  # the two restatements agree
    d = Device(0)
    try:
        d.load_library(c["seq"])
        flanks, idx = resolve_flanks(1, c["fs"].cores, 5, 40)
        d.planes(flanks, to_extend_params(c["p"]), c["cons"])
        check_list(d, c["maps"], seventy, "70 of 33 tiles", small)
        m = check_list(d, c["maps"], range(2048), "the limit", dr.matrix_of_one_word(c["maps"], range(2048), rows))
        assert m["tv"].any() and m["del_one"].any() and m["del_both"].any()
        with pytest.raises(_lib.RamxError, match=r"\(-103\).*2049 copies outside \[0, 2048\]"):
            d.copy_dist(np.arange(2049, dtype=np.int32))
        # session reuse: a small family after the large one, sentinels intact beyond [C][C]
        s = dr.shape_case(*tp.SHAPES[1], 1, "kept")
        d.load_library(s["seq"])
        fl2, _ = resolve_flanks(1, s["fs"].cores, 14, 60)
        d.planes(fl2, to_extend_params(s["p"]), s["cons"])
        out = sentinel_call(d, [np.array([1, 4, 30], np.int32)], extra=64)
        assert np.array_equal(out[:9].reshape(3, 3), dr.matrix(s["maps"], [1, 4, 30]))
        assert (out[9:].view(np.uint8) == 0x5A).all()
    finally:
        d.close()


def sentinel_call(d, lists, extra=0, expect=None, nf=None, why=None):
    """ramx_dev_copy_dist on a buffer of 0x5A bytes with `extra` records of room behind the result -> the buffer, or the error
    code with `expect` (and the buffer untouched; `why`: what the refusal's message holds)."""
    from repeatafterme_amd import _lib
    nf = len(lists) if nf is None else nf
    cnt = np.array([len(x) for x in lists], np.int32)
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int32)
    allc = np.concatenate(list(lists) + [np.zeros(1, np.int32)]).astype(np.int32)
    cells = cnt.astype(np.int64) ** 2
    o_first = np.concatenate([[0], np.cumsum(cells)[:-1]]).astype(np.int64)
    out = np.zeros(int(cells.sum()) + extra + 1, COPY_DIST_DTYPE)
    out.view(np.uint8)[:] = 0x5A
    rc = d._L.ramx_dev_copy_dist(d._h, nf, allc.ctypes.data, first.ctypes.data, cnt.ctypes.data, out.ctypes.data, o_first.ctypes.data)
    if expect is not None:
        assert rc == expect, (rc, _lib.lib().ramx_last_error())
        assert why is None or why in _lib.lib().ramx_last_error().decode(), (why, _lib.lib().ramx_last_error())
        assert (out.view(np.uint8) == 0x5A).all()
        return rc
    assert rc == 0, _lib.lib().ramx_last_error()
    return out


def test_families_of_different_rows_in_one_call():
    """Three families along their own consensus over their own number of columns, one of them with rows = 0 (all-zero
    records), a fourth without flanks, a tile that belongs to no family between them, and an empty list for one family."""
    from repeatafterme_amd.device import Device, resolve_flanks
    p = tp.params("20p43g", 14, 120, cappenalty=-10, when_to_stop=25)
    fams = tp._three_families()
    lib = np.concatenate([fs.sequence for fs in fams])
    offs = np.cumsum([0] + [len(fs.sequence) for fs in fams])
    cons = np.zeros((4, 120), np.int8)
    rows, parts, maps = [], [], []
    for f, fs in enumerate(fams):
        o = po.oracle_extend(1, fs.cores.copy(), fs.sequence, new_master(120), p, trace=True)
        c = tp.foreign(o.col_base[:o.ret], at=8, k=5) if f else o.col_base[:0]               # family 0: rows = 0
        rows.append(len(c))
        cons[f, :len(c)] = c
        cols, idx, results = pr.pileup(1, fs.cores, fs.sequence, p, c, with_walks=True)
        maps.append(dr.maps_of(1, fs.cores, idx, results, fs.sequence, 14, c))
        (fl, nx), _ = resolve_flanks(1, fs.cores, 14, 120)
        parts.append((fl, nx, offs[f]))
    flanks, first, count = rl.lay_out(parts, hole_before=1)
    first.append(first[-1]); count.append(0); rows.append(rows[2])                            # a family without flanks
    cons[3] = cons[2]
    assert rows[0] == 0 and rows[1] != rows[2] and min(rows[1:]) > 10
    d = Device(0)
    try:
        d.load_library(lib)
        d.planes(flanks, to_extend_params(p), cons, rows=rows, fam_first=first, fam_count=count)
        for lists in ([[0, 2, 4], list(range(count[1])), list(range(0, count[2], 3)), []],
                      [[1], [], [5, 64, 65, 99], []]):
            got = d.copy_dist([np.asarray(x, np.int32) for x in lists], fill=0x5A)
            assert not got[0].view(np.uint8).any() and got[0].shape == (len(lists[0]),) * 2   # rows = 0: zero records
            for f in (1, 2):
                assert np.array_equal(got[f], dr.matrix(maps[f], lists[f])), f
            assert got[3].shape == (0, 0)
        assert sentinel_call(d, [np.zeros(0, np.int32)] * 3 + [np.array([0], np.int32)], expect=-103) == -103
    finally:
        d.close()


@pytest.mark.parametrize("direction", [1, 0])
def test_groups_of_several_tiles_with_a_shorter_last_group(direction, monkeypatch):
    """300 flanks in groups of 2 + 2 + 1 tiles under RAMX_ALIGN_BYTES, as tests/test_gpu_linkage.py: the result is the
    restatement's whatever the grouping of the replay."""
    from repeatafterme_amd.device import Device, resolve_flanks
    seq, cores, p, cons, want_cols, widx, results = rl.grouped_case(direction)
    maps = dr.maps_of(direction, cores, widx, results, seq, p.bandwidth, cons)
    rows, W, ep = len(cons), p.bandwidth, to_extend_params(p)
    tile_bytes = rows * 64 * (4 * (W // 4 + 1) + 8)
    assert rl.group_sizes(5, tile_bytes, 2 * tile_bytes) == [2, 2, 1]
    copies = list(range(0, 300, 4)) + [297, 299]
    want = dr.matrix(maps, copies)
    d = Device(0)
    try:
        d.load_library(seq)
        flanks, idx = resolve_flanks(direction, cores, W, p.L)
        for name, budget in (("one group", None), ("2 + 2 + 1", 2 * tile_bytes)):
            if budget is None:
                monkeypatch.delenv("RAMX_ALIGN_BYTES", raising=False)
            else:
                monkeypatch.setenv("RAMX_ALIGN_BYTES", str(budget))
            d.planes(flanks, ep, cons)
            check_list(d, maps, copies, name, want)
    finally:
        d.close()
    assert list(idx) == widx


def test_state_and_argument_errors():
    """All refused on the host, before a launch; `out` keeps its sentinel bytes."""
    from repeatafterme_amd.device import Device, resolve_flanks
    c = dr.shape_case(*tp.SHAPES[1], 1, "kept")
    ep, cons = to_extend_params(c["p"]), c["cons"]
    ok = np.array([0, 3, 36], np.int32)
    d = Device(0)
    try:
        d.load_library(c["seq"])
        flanks, idx = resolve_flanks(1, c["fs"].cores, 14, 60)
        sentinel_call(d, [ok], expect=-104, why="ramx_dev_copy_dist: no resident bit planes")  # before any planes
        d.planes(flanks, ep, cons)
        want = dr.matrix(c["maps"], ok)
        assert np.array_equal(d.copy_dist(ok), want)
        for bad, why in (([3, 0], "family 0, entry 1: the copies are not strictly increasing"),
                         ([3, 3], "family 0, entry 1: the copies are not strictly increasing"),
                         ([-1, 2], "family 0, entry 0: copy -1 outside the family's 37 flanks"),
                         ([0, 37], "family 0, entry 1: copy 37 outside the family's 37 flanks"),
                         (list(range(37)) + list(range(2049 - 37)), "family 0: 2049 copies outside [0, 2048]")):
            sentinel_call(d, [np.asarray(bad, np.int32)], expect=-103, why=why)
        sentinel_call(d, [ok, ok], expect=-103, why="2 families, the resident replay has 1")   # another n_families
        sentinel_call(d, [], expect=-103, nf=0, why="0 families, the resident replay has 1")
        assert np.array_equal(d.copy_dist(ok), want)                                         # a refused list leaves the planes resident
        d.align(flanks, ep, cons)
        sentinel_call(d, [ok], expect=-104)                                                  # a later replay dropped them
    finally:
        d.close()


@pytest.mark.parametrize("direction", [1, 0])
def test_tail_insertions_count_nowhere(direction):
    c = cr.tail_case(direction)
    run_case(c, direction, f"tail dir={direction}")


def test_the_planted_family_has_structure():
    """linkage_ref.planted_family: every third copy carries another base at three columns.  Records exact; the mean Kimura
    distance within a lineage is below the mean between the lineages; the medoid is the restatement's."""
    from repeatafterme_amd.device import Device, dist_kimura, dist_summary, resolve_flanks, select_copies
    c = lr.planted_case(1)
    maps = dr.maps_of(1, c["fs"].cores, c["idx"], c["results"], c["seq"], c["p"].bandwidth, c["cons"])
    d = Device(0)
    try:
        d.load_library(c["seq"])
        flanks, idx = resolve_flanks(1, c["fs"].cores, c["p"].bandwidth, c["p"].L)
        res = d.planes(flanks, to_extend_params(c["p"]), c["cons"])
        sel = select_copies(res.ends[:len(idx)], len(c["cons"]), 20, 256)
        assert list(sel) == dr.select([r["end_row"] for r in c["results"]], len(c["cons"]), 20, 256) and len(sel) > 40
        m = check_list(d, maps, sel, "planted")
    finally:
        d.close()
    lineage = np.array([int(i) % lr.PLANTED_EVERY == 0 for i in sel])
    within, between = [], []
    for a in range(len(sel)):
        for b in range(a + 1, len(sel)):
            k = dist_kimura(m[a, b])
            want = dr.kimura(m[a, b])
            assert (k < 0) == (want is None) and (want is None or abs(k - want) < 1e-9)
            if k >= 0:
                (within if lineage[a] == lineage[b] else between).append(k)
    assert len(within) > 100 and len(between) > 100 and np.mean(within) < np.mean(between)
    s, w = dist_summary(m, 20), dr.summary(m, 20)
    assert (s.n, s.pairs, s.used, s.medoid) == (w["n"], w["pairs"], w["used"], w["medoid"]) and s.medoid >= 0
    assert abs(s.mean - w["mean"]) < 1e-9 and abs(s.medoid_mean - w["medoid_mean"]) < 1e-9
