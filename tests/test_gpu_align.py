"""Per-copy alignments (C-ABI ramx_dev_align, the alignment sink of seam 1) against the CPU walker of tests/align_ref.py
and against the loop's own trimmed end points: per flank end_row / end_idx / score / start_idx / tail_ins, per (column,
flank) the matched position and the insertions before it.  Everything is integer-exact."""
import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import ALN_DELETED, ALN_END_DTYPE, ALN_NONE, CoreSet, new_master
from repeatafterme_amd.synth import synth_family

import align_ref as ar
from helpers import to_extend_params

pytestmark = pytest.mark.gpu


def params(matrix, W, L, cap=None, **kw):
    if matrix == "repeatscout":
        kw.update(match=2, mismatch=-2, gap=-6)
    if cap is not None:
        kw["cappenalty"] = cap
    return po.Params.named(matrix, bandwidth=W, L=L, **kw)


def check_against_walker(ends, col_idx, col_ins, results, rows, tag):
    """ends / col_idx / col_ins of the flanks in flank order (columns of the arrays) against walk() results."""
    seen = dict(aligned=0, n_ins=0, n_del=0)
    for i, res in enumerate(results):
        e = ends[i]
        got = tuple(int(e[k]) for k in ("end_row", "end_idx", "score", "start_idx", "tail_ins"))
        want = tuple(int(res[k]) for k in ("end_row", "end_idx", "score", "start_idx", "tail_ins"))
        assert got == want, f"{tag}: flank {i}: {got} != {want}"
        assert np.array_equal(col_idx[:rows, i], res["col_idx"]), f"{tag}: flank {i}: col_idx"
        assert np.array_equal(col_ins[:rows, i], res["col_ins"]), f"{tag}: flank {i}: col_ins"
        seen["aligned"] += res["end_row"] >= 0
        seen["n_ins"] += res["n_ins"]
        seen["n_del"] += res["n_del"]
    return seen


# (flanks, W, L, matrix, cappenalty or None = the matrix's default): the shapes of test_gpu_profile.py's PARITY -- 64 / 65 the
# tile edge, 130 three tiles with a partial one, W = 5 a partly filled code dword, W = 80 the widest
PARITY = [
    (1, 5, 60, "14p43g", None), (1, 40, 150, "repeatscout", -10), (37, 14, 60, "25p43g", -10),
    (37, 20, 60, "14p43g", None), (37, 80, 150, "repeatscout", -10), (64, 20, 150, "repeatscout", None),
    (64, 5, 150, "25p43g", -10), (65, 40, 60, "14p43g", None), (130, 40, 60, "18p43g", -10),
    (130, 80, 150, "25p43g", None), (130, 14, 150, "repeatscout", -10), (65, 5, 60, "20p43g", None),
]


@pytest.mark.parametrize("n,W,L,matrix,cap", PARITY)
def test_alignments_match_the_walker_and_the_loops_end_points(n, W, L, matrix, cap):
    from repeatafterme_amd.device import Device, resolve_flanks
    from repeatafterme_amd.extend import extend_alignment
    fs = synth_family(n, L, W, K=L // 2, seed=300 + n + W, both_sides=True, minus_frac=0.4, n_run_frac=0.1)
    p = params(matrix, W, L, cap, when_to_stop=30)
    ep = to_extend_params(p)
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    c_g, c_o = fs.cores.copy(), fs.cores.copy()
    m_g, m_o = new_master(L), new_master(L)
    seen = dict(aligned=0, n_ins=0, n_del=0)
    d = Device(0)
    try:
        d.load_library(seq)
        for direction in (1, 0):
            tag = f"n={n} W={W} L={L} {matrix} dir={direction}"
            before = c_o.copy()
            o = po.oracle_extend(direction, c_o, seq, m_o, p, trace=True, row_trace=True)
            cons = o.col_base[:o.ret]
            idx, results = ar.walk_family(direction, before, seq, p, cons)
            # through the sink of seam 1
            info, al = extend_alignment(direction, c_g, seq, m_g, ep, align=True)
            assert info.ret == o.ret and al.direction == direction and al.family == 0, tag
            assert np.array_equal(al.cons, cons) and list(al.core_index) == idx, tag
            got = check_against_walker(al.ends, al.col_idx, al.col_ins, results, o.ret, tag + " sink")
            for k in seen:
                seen[k] += got[k]
            # through seam 2, beside the loop's own run of the direction: its trimmed high score and position are the end cell
            flanks, fidx = resolve_flanks(direction, before, W, L)
            d.begin_direction(flanks, ep)
            run = d.run_direction()
            g_cons, th, tp = d.download()
            assert run.ret == o.ret and np.array_equal(g_cons[:o.ret], cons), tag
            res = d.align(flanks, ep, cons, rows=o.ret)
            nx = len(fidx)
            check_against_walker(res.ends[:nx], res.col_idx[:, :nx], res.col_ins[:, :nx], results, o.ret, tag + " seam 2")
            has = res.ends["end_row"][:nx] >= 0
            assert np.array_equal(has, th > 0), tag
            assert np.array_equal(res.ends["score"][:nx][has], th[has]) and np.array_equal(res.ends["end_idx"][:nx][has], tp[has]), tag
            # padding flanks: no alignment
            assert np.all(res.ends["end_row"][nx:] == -1) and np.all(res.col_idx[:, nx:] == ALN_NONE) and not res.col_ins[:, nx:].any()
        assert np.array_equal(m_g, m_o)
    finally:
        d.close()
    if n >= 37:
        assert seen["aligned"] > 0 and seen["n_ins"] > 0 and seen["n_del"] > 0, seen      # on the walker's side


def gpu_align(direction, cores, sequence, p, cons, rows=None, **kw):
    from repeatafterme_amd.device import Device, resolve_flanks
    d = Device(0)
    try:
        d.load_library(np.ascontiguousarray(sequence, np.int8))
        flanks, idx = resolve_flanks(direction, cores, p.bandwidth, p.L)
        res = d.align(flanks, to_extend_params(p), cons, rows=len(cons) if rows is None else rows, **kw)
    finally:
        d.close()
    return res, idx


@pytest.mark.parametrize("direction", [1, 0])
def test_alignment_to_a_foreign_consensus(direction):
    """The oracle's consensus with every seventh base changed: the replay is a primitive in its own right."""
    fs = synth_family(37, 60, 14, K=30, seed=41, both_sides=True, minus_frac=0.4, n_run_frac=0.1)
    p = params("25p43g", 14, 60, -10, when_to_stop=1000)
    o = po.oracle_extend(direction, fs.cores.copy(), fs.sequence, new_master(60), p, trace=True)
    cons = o.col_base[:60].copy()
    cons[::7] = (cons[::7] + 1) & 3
    res, idx = gpu_align(direction, fs.cores, fs.sequence, p, cons)
    widx, results = ar.walk_family(direction, fs.cores, np.ascontiguousarray(fs.sequence, np.int8), p, cons)
    assert list(idx) == widx
    seen = check_against_walker(res.ends, res.col_idx, res.col_ins, results, 60, f"foreign dir={direction}")
    assert seen["aligned"] > 0 and seen["n_ins"] + seen["n_del"] > 0


def test_alignment_positive_gap_term_and_odd_widths():
    """Band widths without a specialised kernel anywhere (3, 500) and a scoring system with a positive gap term."""
    fs = synth_family(70, 40, 3, K=25, seed=43, both_sides=True, minus_frac=0.3, n_run_frac=0.1)
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    for W, go, ge in ((3, -28, -5), (500, -28, -5), (14, 3, -7)):
        p = params("14p43g", W, 40, -10, when_to_stop=1000)
        p.gapopen, p.gapextn = go, ge
        o = po.oracle_extend(1, fs.cores.copy(), seq, new_master(40), p, trace=True)
        cons = o.col_base[:o.ret]
        res, idx = gpu_align(1, fs.cores, seq, p, cons)
        widx, results = ar.walk_family(1, fs.cores, seq, p, cons)
        check_against_walker(res.ends, res.col_idx, res.col_ins, results, o.ret, f"W={W} go={go} ge={ge}")


def test_alignment_constructed_edges():
    rng = np.random.default_rng(5)
    seq = rng.integers(0, 4, 80).astype(np.int8)
    p = params("14p43g", 5, 30, when_to_stop=10)
    # a flank without sequence (the core ends where its window ends) beside an ordinary one
    c = CoreSet(left_pos=[70, 10], right_pos=[79, 12], lower=[60, 0], upper=[79, 59], orient=[0, 0], left_ext=[1, 1], right_ext=[1, 1])
    cons = seq[13:33].copy()
    res, idx = gpu_align(1, c, seq, p, cons)
    _, results = ar.walk_family(1, c, seq, p, cons)
    assert results[0]["end_row"] == -1 and results[1]["end_row"] == 19 and results[1]["score"] > 0
    check_against_walker(res.ends, res.col_idx, res.col_ins, results, 20, "empty flank")
    assert np.all(res.col_idx[:, 0] == ALN_NONE)
    # a flank whose row bests never exceed 0 (asserted on the oracle): no alignment, every column RAMX_ALN_NONE
    seq_a = np.zeros(80, np.int8)
    c = CoreSet(left_pos=[10], right_pos=[12], lower=[0], upper=[79], orient=[0], left_ext=[1], right_ext=[1])
    cons = np.ones(15, np.int8)
    _, results = ar.walk_family(1, c, seq_a, p, cons)
    assert max(results[0]["row_best"]) <= 0 and results[0]["end_row"] == -1
    res, _ = gpu_align(1, c, seq_a, p, cons)
    assert tuple(res.ends[0]) == (-1, -1, 0, 0, 0)
    assert np.all(res.col_idx == ALN_NONE) and not res.col_ins.any()
    # a flank cut by t_hi inside the band: seven bases of sequence, twenty columns
    c = CoreSet(left_pos=[10], right_pos=[12], lower=[0], upper=[19], orient=[0], left_ext=[1], right_ext=[1])
    cons = seq[13:33].copy()
    _, results = ar.walk_family(1, c, seq, p, cons)
    assert results[0]["end_idx"] == 6 and 0 <= results[0]["end_row"] < 19
    res, _ = gpu_align(1, c, seq, p, cons)
    check_against_walker(res.ends, res.col_idx, res.col_ins, results, 20, "cut by t_hi")
    # rows = 0
    res, _ = gpu_align(1, c, seq, p, cons, rows=0)
    assert tuple(res.ends[0]) == (-1, -1, 0, 0, 0) and np.all(res.col_idx == ALN_NONE)


def test_walk_stops_at_an_edge_fill_cell():
    """t_lo = 3 > 0: the flank's first three positions lie outside it.  A consensus whose columns 4.. spell the flank from
    position 3 on, one diagonal below the main one, makes the best path run down that diagonal from the cell (3, W - 1), which
    is outside the flank and holds the matrix-edge fill go + 4 ge (bnw_extend.c:990-994): columns 0..3 are deletions.  The
    oracle does produce this path (asserted: edge_end), and the rescoring identity holds on it."""
    rng = np.random.default_rng(5)
    seq = rng.integers(0, 4, 80).astype(np.int8)
    p = params("14p43g", 5, 30, when_to_stop=10)
    c = CoreSet(left_pos=[10], right_pos=[12], lower=[16], upper=[79], orient=[0], left_ext=[1], right_ext=[1])
    cons = np.array([seq[13 + r - 1] if r >= 4 else (seq[13 + r + 3] + 2) & 3 for r in range(20)], np.int8)
    _, results = ar.walk_family(1, c, seq, p, cons)
    w = results[0]
    assert w["edge_end"] == 1 and w["bound_end"] == 0 and w["start_idx"] == 3 and w["end_row"] == 19
    assert list(w["col_idx"][:5]) == [ALN_DELETED] * 4 + [3]
    assert ar.rescore(w, ar.Flank(1, c, 0, 5), seq, p, cons) == w["score"]
    res, _ = gpu_align(1, c, seq, p, cons)
    check_against_walker(res.ends, res.col_idx, res.col_ins, results, 20, "edge fill")


def _three_families():
    return [synth_family(n, 120, 14, K=K, seed=seed, both_sides=True, minus_frac=0.3, n_run_frac=0.1)
            for n, K, seed in ((5, 20, 51), (70, 45, 52), (100, 70, 53))]


def test_alignment_batch_equals_single_runs():
    from repeatafterme_amd.extend import extend_alignment, extend_batch
    p = params("20p43g", 14, 120, -10, when_to_stop=25)
    ep = to_extend_params(p)
    fams = _three_families()
    single = []
    for fs in fams:
        c, m = fs.cores.copy(), new_master(120)
        single.append([extend_alignment(d, c, fs.sequence, m, ep, align=True) for d in (1, 0)])
    batch = [(fs.cores.copy(), fs.sequence, new_master(120)) for fs in fams]
    for k, direction in enumerate((1, 0)):
        infos, profs, als = extend_batch(direction, batch, ep, profile=True, align=True)
        assert len({i.ret for i in infos}) > 1                       # the families keep different numbers of columns
        for f in range(3):
            s_info, s_al = single[f][k]
            assert infos[f].ret == s_info.ret and profs[f].ret == s_info.ret
            assert als[f].family == f and als[f].direction == direction
            for key in ("cons", "flanks", "core_index", "ends", "col_idx", "col_ins"):
                assert np.array_equal(getattr(als[f], key), getattr(s_al, key)), (f, direction, key)
            assert (als[f].ends["end_row"] >= 0).any()


def test_alignment_families_in_one_call_leave_the_rest_untouched():
    """Seam 2 with several families, each along its own consensus over its own number of columns, and a tile that belongs to
    no family between them: entries of that tile keep what the caller put there."""
    from repeatafterme_amd import _lib
    from repeatafterme_amd.device import AlignResult, Device, resolve_flanks
    p = params("20p43g", 14, 120, -10, when_to_stop=25)
    ep = to_extend_params(p)
    fams = _three_families()
    lib = np.concatenate([fs.sequence for fs in fams])
    offs = np.cumsum([0] + [len(fs.sequence) for fs in fams])
    cons = np.zeros((3, 120), np.int8)
    rows, first, count, alone = [], [], [], []
    tiles = sum((fs.cores.n + 63) // 64 for fs in fams) + 1
    arr = (_lib.Flank * (64 * tiles))()
    for i in range(64 * tiles):
        arr[i].t_lo, arr[i].t_hi, arr[i].step = 1, 0, 1
    at = 0
    d = Device(0)
    try:
        for f, fs in enumerate(fams):
            o = po.oracle_extend(1, fs.cores.copy(), fs.sequence, new_master(120), p, trace=True)
            rows.append(o.ret)
            cons[f, :o.ret] = o.col_base[:o.ret]
            (fl, nx), _ = resolve_flanks(1, fs.cores, 14, 120)
            d.load_library(fs.sequence)
            alone.append(d.align((fl, nx), ep, cons[f, :rows[f]]))
            if f == 1:
                at += 64                                             # the tile of no family
            first.append(at)
            count.append(nx)
            for i in range(nx):
                arr[at + i] = fl[i]
                arr[at + i].start += int(offs[f])
            at += (nx + 63) // 64 * 64
        assert len(set(rows)) == 3 and min(rows) > 0
        npad, mr = 64 * tiles, max(rows)
        ends = np.zeros(npad, ALN_END_DTYPE)
        ends["end_row"] = ends["score"] = -7
        out = AlignResult(ends, np.full((mr, npad), -7, np.int32), np.full((mr, npad), -7, np.int32), 0.0, 0.0)
        d.load_library(lib)
        res = d.align((arr, npad), ep, cons, rows=rows, fam_first=first, fam_count=count, out=out)
        for f in range(3):
            a, w = first[f], (count[f] + 63) // 64 * 64
            assert np.array_equal(res.ends[a:a + w], alone[f].ends[:w]), f
            assert np.array_equal(res.col_idx[:rows[f], a:a + w], alone[f].col_idx[:rows[f], :w]), f
            assert np.array_equal(res.col_ins[:rows[f], a:a + w], alone[f].col_ins[:rows[f], :w]), f
            assert np.all(res.col_idx[rows[f]:, a:a + w] == ALN_NONE) and not res.col_ins[rows[f]:, a:a + w].any()
        hole = slice(first[1] - 64, first[1])
        assert np.all(res.ends["end_row"][hole] == -7) and np.all(res.col_idx[:, hole] == -7) and np.all(res.col_ins[:, hole] == -7)
    finally:
        d.close()


def test_alignment_in_tile_groups_is_the_same(monkeypatch):
    """RAMX_ALIGN_BYTES of exactly one tile's codes: 130 flanks go through three groups of one tile; one byte less and the
    call says that it cannot serve the tile."""
    from repeatafterme_amd import _lib
    fs = synth_family(130, 60, 14, K=30, seed=71, both_sides=True, minus_frac=0.4, n_run_frac=0.1)
    p = params("25p43g", 14, 60, -10, when_to_stop=30)
    o = po.oracle_extend(1, fs.cores.copy(), fs.sequence, new_master(60), p, trace=True)
    cons = o.col_base[:o.ret]
    assert o.ret > 10
    monkeypatch.delenv("RAMX_ALIGN_BYTES", raising=False)
    whole, idx = gpu_align(1, fs.cores, fs.sequence, p, cons)
    assert len(idx) > 128
    tile_bytes = o.ret * (14 // 4 + 1) * 64 * 4
    monkeypatch.setenv("RAMX_ALIGN_BYTES", str(tile_bytes))
    parts, _ = gpu_align(1, fs.cores, fs.sequence, p, cons)
    assert np.array_equal(parts.ends, whole.ends) and np.array_equal(parts.col_idx, whole.col_idx) and np.array_equal(parts.col_ins, whole.col_ins)
    assert (whole.ends["end_row"][128:len(idx)] >= 0).any()          # the third group did align something
    monkeypatch.setenv("RAMX_ALIGN_BYTES", str(tile_bytes - 1))
    with pytest.raises(_lib.RamxError, match=r"\(-106\).*RAMX_ALIGN_BYTES"):
        gpu_align(1, fs.cores, fs.sequence, p, cons)


def test_alignment_argument_errors():
    import ctypes as C
    from repeatafterme_amd import _lib
    from repeatafterme_amd.device import Device, pad_flanks, resolve_flanks
    from repeatafterme_amd.extend import _params
    fs = synth_family(70, 30, 5, K=20, seed=62)
    p = params("14p43g", 5, 30)
    ep = to_extend_params(p)
    d = Device(0)
    try:
        d.load_library(fs.sequence)
        arr, npad = pad_flanks(resolve_flanks(1, fs.cores, 5, 30)[0])
        for kw in (dict(fam_first=[32], fam_count=[70], rows=[10]),        # a family that does not start at a multiple of 64
                   dict(fam_first=[64], fam_count=[70], rows=[10]),        # ... that leaves the flank array
                   dict(fam_first=[0, 64], fam_count=[70, 10], rows=[10, 10]),   # two families in one tile
                   dict(fam_first=[0], fam_count=[70], rows=[31])):        # rows[f] > L
            c2 = np.zeros((len(kw["rows"]), 30), np.int8)
            with pytest.raises(_lib.RamxError, match=r"\(-103\)"):
                d.align((arr, npad), ep, c2, **kw)
        cons = np.zeros((1, 30), np.int8)
        cons[0, 3] = 4                                                     # not a base
        with pytest.raises(_lib.RamxError, match=r"\(-103\)"):
            d.align((arr, npad), ep, cons, fam_first=[0], fam_count=[70], rows=[10])
        # one of the two column buffers without the other
        cp, _keep = _params(ep)
        cons[:] = 0
        zero, ten, seventy = np.zeros(1, np.int32), np.array([10], np.int32), np.array([70], np.int32)
        ends = np.zeros(npad, ALN_END_DTYPE)
        buf = np.zeros((10, npad), np.int32)
        for a, b in ((buf.ctypes.data, None), (None, buf.ctypes.data)):
            rc = _lib.lib().ramx_dev_align(d._h, arr, npad, zero.ctypes.data, seventy.ctypes.data, 1, C.byref(cp), cons.ctypes.data,
                                           ten.ctypes.data, ends.ctypes.data, a, b, None)
            assert rc == -103
        # and the call itself is fine, with and without the column buffers
        full = d.align((arr, npad), ep, cons, fam_first=[0], fam_count=[70], rows=[10])
        lean = d.align((arr, npad), ep, cons, fam_first=[0], fam_count=[70], rows=[10], columns=False)
        assert lean.col_idx is None and np.array_equal(full.ends, lean.ends)
    finally:
        d.close()


def test_no_sink_no_change():
    """Without a sink an extension is what it was: same outputs and run info before, between and after aligned runs."""
    from repeatafterme_amd.extend import extend_alignment
    fs = synth_family(130, 80, 14, K=40, seed=63, both_sides=True, minus_frac=0.3)
    p = params("20p43g", 14, 80, when_to_stop=20)
    ep = to_extend_params(p)

    def run(align):
        c, m = fs.cores.copy(), new_master(80)
        infos = []
        for d in (1, 0):
            r = extend_alignment(d, c, fs.sequence, m, ep, align=align)
            infos.append(r[0] if align else r)
        keys = ("ret", "rows_executed", "limit_warning", "overflow32", "n_extendable", "launches", "persistent", "lanes_per_flank",
                "respeculated_rows", "packed_rows", "lean_rows")
        return m, c.left_len, c.right_len, c.score, [[getattr(i, k) for k in keys] for i in infos]

    a, b, c = run(False), run(True), run(False)
    for x, y in ((a, b), (a, c)):
        for u, v in zip(x[:4], y[:4]):
            assert np.array_equal(u, v)
        assert x[4] == y[4]
