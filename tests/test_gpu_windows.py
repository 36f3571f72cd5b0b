"""The transposed 4-bit flank windows in d_bases, read back with Device.peek_windows() and compared word for word with the
restatement of tests/window_ref.py, on both library forms: ramx_pack_kernel on the one-byte-per-base library, ramx_pack2_kernel
on the .2bit payload (its per-word fast path, its per-base path, the cached window index, the N mask, block rows of 32 words,
pieces that begin at any word).  Every comparison is exact.  The inputs are built in tests/window_cases.py;
tests/test_window_ref.py asserts on the CPU that they hold what they are here for."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd import _lib
from repeatafterme_amd.datamodel import new_master

import window_cases as wc
import window_ref as wr
from helpers import to_extend_params

pytestmark = pytest.mark.gpu
ERR_ARG = -103
ROUTE_VARS = ("RAMX_NO_FAMILY_ROUTE", "RAMX_NO_CP_DEVICE", "RAMX_NO_CP", "RAMX_NO_PK", "RAMX_NO_PERSISTENT", "RAMX_PK_SEGMENT")


@pytest.fixture(autouse=True)
def _plain_routes(monkeypatch):
    for k in ROUTE_VARS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def dev():
    from repeatafterme_amd.device import Device
    d = Device(0)
    yield d
    d.close()


def whole(W, L, matrix="14p43g", **kw):
    """Parameters under which begin_direction packs every word at once: the stop rule cannot fire before the last column."""
    kw.setdefault("when_to_stop", L)
    return po.Params.named(matrix, bandwidth=W, L=L, **kw)


def reference(c, form):
    """(words, bounds) of a case on the byte form of its library, or on the packed form (lower case folded away)."""
    key = "_ref_" + form
    if key not in c.extra:
        lib = c.lib if form == "byte" else wr.fold(c.lib)
        c.extra[key] = wr.windows(lib, c.descs, wr.padded_lanes(len(c.descs)), c.W, c.KW, packed=form != "byte")
    return c.extra[key]


def same(got, want, c, tag):
    words, bounds = got
    diff = wr.first_difference(words, want[0], c.descs)
    assert not diff, f"{c.name}, {tag}: {diff}"
    bad = np.flatnonzero((bounds != want[1]).any(axis=1))
    assert bounds.shape == want[1].shape and not len(bad), f"{c.name}, {tag}: bounds of lane {bad[:1]}: {bounds[bad[:1]]}, want {want[1][bad[:1]]}"


def packed_once(d, c, p=None):
    d.begin_direction(c.flanks, to_extend_params(p or whole(c.W, c.L)))
    return d.peek_windows()


def both_forms(d, c, table_names):
    """begin_direction on the byte library, on the folded byte library and on every set of packed tables: each equals the
    restatement in full (bounds and pad lanes included), and the packed form's words equal the byte form's on the folded library."""
    d.load_library(np.ascontiguousarray(c.lib))
    same(packed_once(d, c), reference(c, "byte"), c, "byte library")
    d.load_library(np.ascontiguousarray(wr.fold(c.lib)))
    folded = packed_once(d, c)
    same(folded, reference(c, "packed"), c, "folded byte library")
    for name in table_names:
        d.load_library_packed(c.tables[name])
        got = packed_once(d, c)
        same(got, reference(c, "packed"), c, f"packed library, windows '{name}'")
        assert np.array_equal(got[0], folded[0]) and np.array_equal(got[1], folded[1]), (c.name, name)


@pytest.mark.parametrize("L", wc.SWEEP_L)
@pytest.mark.parametrize("W", wc.SWEEP_W)
def test_both_forms_equal_the_restatement(dev, W, L):
    """Hostile sets, both directions: windows that begin at the sets' own boundaries with phases cycling 0..3, and again with
    extra window starts inside flanks (words straddle, the cached window index must be searched again)."""
    for c in wc.sweep_cases(W, L):
        assert reference(c, "byte")[0].shape == (wr.window_words(L, W), wr.padded_lanes(len(c.descs)))
        both_forms(dev, c, ("bounds", "inside"))
    assert not np.array_equal(reference(c, "byte")[0], reference(c, "packed")[0])        # lower case is kept by the byte form


@pytest.mark.parametrize("n", wc.FLANK_COUNTS)
def test_flank_counts_round_the_edges(dev, n):
    """1 .. 321 flanks: round the wave, the 256-thread block of the pack grid, a padded count that is no multiple of 256."""
    for c in wc.count_cases(n):
        both_forms(dev, c, ("bounds",))


def test_library_written_for_the_n_mask(dev):
    """Runs of N of length 1 .. 300 at every alignment, at both ends of the library, in pairs and triples within a word,
    touching at a window's first base; whole-library flanks on both strands from all eight alignments; one window, several
    windows, and a copy of the library without any N (n_blocks = 0: the branch that skips the search)."""
    c = wc.nmask_case()
    both_forms(dev, c, ("one", "windows"))
    clean = wc.Case("N mask, clean copy", c.extra["clean_lib"], c.descs, c.W, c.L, flanks=c.flanks,
                    tables={"clean": c.extra["clean_tables"]})
    both_forms(dev, clean, ("clean",))
    assert not np.array_equal(reference(c, "packed")[0], reference(clean, "packed")[0])


def test_the_loaders_own_tables(dev, tmp_path):
    """A .2bit file through ramx_load_sequence_subset_packed, the tables uploaded as they come (records whose lengths are no
    multiples of 4, ranges at a record's first and last base): the payload's real padding under the three-byte fetch."""
    for c in wc.loader_case(tmp_path):
        dev.load_library_packed(c.tables["loader"])
        same(packed_once(dev, c), reference(c, "packed"), c, "the loader's tables")


def _trim_lengths(th, tp):
    ext = (th > 0) & (tp >= 0)                                    # ram_extend.c:1234-1247
    return np.where(ext, tp + 1, 0), np.where(ext, th, 0)


def _run(d, c, p, peek):
    d.begin_direction(c.flanks, to_extend_params(p))
    info = d.run_direction()
    cons, th, tp = d.download()
    state = [d.peek_state(i) for i in peek]
    return info, cons, th, tp, state, d.peek_windows()


def _same_run(a, b, tag):
    assert (a[0].ret, a[0].rows_executed, a[0].limit_warning) == (b[0].ret, b[0].rows_executed, b[0].limit_warning), tag
    assert np.array_equal(a[1], b[1]), f"{tag}: consensus"
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), f"{tag}: trim records"
    for i, ((ca, ha, pa), (cb, hb, pb)) in enumerate(zip(a[4], b[4])):
        assert np.array_equal(ca, cb) and (ha, pa) == (hb, pb), f"{tag}: final DP row of peeked flank {i}"


def _equals_oracle(got, direction, cores, idx, lib, p, tag):
    oc, m = cores.copy(), new_master(p.L)
    o = po.oracle_extend(direction, oc, lib, m, p, trace=True)
    info, cons, th, tp = got[:4]
    assert (info.ret, info.rows_executed, info.limit_warning) == (o.ret, o.rows_executed, o.limit_warning), tag
    assert np.array_equal(cons, o.col_base[:o.rows_executed]), f"{tag}: consensus"
    lengths, scores = _trim_lengths(th, tp)
    assert np.array_equal(lengths, (oc.right_len if direction else oc.left_len)[idx]), f"{tag}: lengths"
    assert np.array_equal(scores, oc.score[idx] - cores.score[idx]), f"{tag}: scores"
    return o


@pytest.mark.parametrize("seg", ["16", "50"])
def test_packed_form_in_pieces(seg, monkeypatch):
    """The packed-row route packs a direction's windows in pieces, the later ones on the second stream from a start word that is
    no multiple of 32.  After run_direction every packed word equals the restatement; at least the words the executed rows read
    are packed, and fewer than the whole window when the stop rule fired early; the results equal the byte library's and the
    oracle's."""
    from repeatafterme_amd.device import Device
    c = wc.pieces_case()
    W, L, n = c.W, c.L, len(c.descs)
    fs = c.extra["fs"]
    monkeypatch.setenv("RAMX_NO_CP_DEVICE", "1")
    monkeypatch.setenv("RAMX_PK_SEGMENT", seg)
    first = ((int(seg) + 8) >> 3) + 28                   # begin_direction's piece: the words its columns read
    assert first % 32 != 0 and first < c.KW
    want = reference(c, "packed")
    early = 0
    for wts in (L, 40):
        p = whole(W, L, when_to_stop=wts)
        runs = {}
        for form in ("packed", "byte"):
            d = Device(0)
            try:
                if form == "packed":
                    d.load_library_packed(c.tables["bounds"])
                else:
                    d.load_library(c.lib)
                d.begin_direction(c.flanks, to_extend_params(p))
                at_begin = d.peek_windows()[0].shape[0]
                runs[form] = _run(d, c, p, (0, n - 1))
            finally:
                d.close()
            info, (words, bounds) = runs[form][0], runs[form][5]
            tag = f"seg {seg} when_to_stop {wts} {form}"
            assert at_begin == first and info.packed_rows > 0, (tag, at_begin, info.packed_rows)
            kw = words.shape[0]
            assert words.shape == (kw, wr.padded_lanes(n)) and kw <= c.KW
            diff = wr.first_difference(words, want[0][:kw], c.descs)
            assert not diff, f"{tag}: {diff}"
            assert np.array_equal(bounds, want[1]), tag
            # what the executed rows read: words_for() of prk_run -- the rows' own words, the band's, the look-ahead
            assert kw >= min(c.KW, ((info.rows_executed + 7) >> 3) + (2 * W + 1 + 8) // 8 + 2 + 2), (tag, kw, info.rows_executed)
            if info.rows_executed < L:
                assert first < kw < c.KW, (tag, kw)
                early += 1
        _same_run(runs["packed"], runs["byte"], f"seg {seg} when_to_stop {wts}")
        _equals_oracle(runs["packed"], 1, fs.cores, np.arange(n), c.lib, p, f"seg {seg} when_to_stop {wts}")
    assert early == 2                                    # when_to_stop = 40 stops behind the first copy, on both forms


@pytest.mark.parametrize("W", wc.LOOP_W)
def test_the_loop_on_the_packed_form(dev, W):
    """run_direction on the packed library (windows that begin inside flanks) equals the run on the folded byte library and the
    oracle: consensus, trim records, rows_executed, limit_warning; the final DP rows of every flank for one seed."""
    for c in wc.loop_cases(W):
        seed, direction, idx, fs = (c.extra[k] for k in ("seed", "direction", "idx", "fs"))
        p = po.Params.named("14p43g" if seed % 2 else "repeatscout", bandwidth=W, L=c.L, when_to_stop=25)
        lib = np.ascontiguousarray(wr.fold(c.lib))
        peek = range(len(c.descs)) if seed == wc.SWEEP_SEEDS[0] else ()
        dev.load_library_packed(c.tables["inside"])
        a = _run(dev, c, p, peek)
        dev.load_library(lib)
        b = _run(dev, c, p, peek)
        _same_run(a, b, c.name)
        o = _equals_oracle(a, direction, fs.cores, idx, lib, p, c.name)
        kw = a[5][0].shape[0]
        assert np.array_equal(a[5][0], reference(c, "packed")[0][:kw]) and np.array_equal(a[5][0], b[5][0]), c.name
        assert o.rows_executed > 0


def test_a_replays_pack(dev):
    """Device.profile on the packed form, two families with a tile that belongs to neither between them: the windows it left
    equal the restatement over the padded flank array, the hole's and the tiles' empty lanes included."""
    c = wc.replay_case()
    first, count = c.extra["first"], c.extra["count"]
    npad = c.flanks[1]
    rng = np.random.default_rng(8)
    cons = rng.integers(0, 4, (2, c.L)).astype(np.int8)
    dev.load_library_packed(c.tables["bounds"])
    dev.profile(c.flanks, to_extend_params(whole(c.W, c.L)), cons, rows=[100, 90], fam_first=first, fam_count=count)
    words, bounds = dev.peek_windows()
    want = wr.windows(wr.fold(c.lib), c.descs, npad, c.W, c.KW, packed=True)
    assert words.shape == (c.KW, npad) and npad == 320
    diff = wr.first_difference(words, want[0], c.descs)
    assert not diff, diff
    assert np.array_equal(bounds, want[1])
    assert (words[:, 70:192] == wr.PAD_WORD).all() and (bounds[70:192] == (1 + c.W, c.W)).all()


def test_the_hook_itself():
    from repeatafterme_amd.device import Device
    L = _lib.lib()
    c = wc.count_cases(65)[0]
    kw, lanes = C.c_int32(-7), C.c_int32(-7)
    d = Device(0)
    try:
        words = np.zeros((c.KW, 128), np.uint32)
        bounds = np.zeros((128, 2), np.int32)
        args = (words.ctypes.data, words.size, bounds.ctypes.data, 128, C.byref(kw), C.byref(lanes))
        assert L.ramx_dev_peek_windows(d._h, *args) == ERR_ARG                 # nothing has been packed on this device
        assert (kw.value, lanes.value) == (-7, -7) and not words.any()
        with pytest.raises(_lib.RamxError, match=r"\(-103\)"):
            d.peek_windows()
        d.load_library(np.ascontiguousarray(c.lib))
        assert L.ramx_dev_peek_windows(d._h, *args) == ERR_ARG                 # a library alone is no pack
        d.begin_direction(c.flanks, to_extend_params(whole(c.W, c.L)))
        assert L.ramx_dev_peek_windows(None, *args) == ERR_ARG
        assert L.ramx_dev_peek_windows(d._h, None, words.size, bounds.ctypes.data, 128, C.byref(kw), C.byref(lanes)) == ERR_ARG
        assert L.ramx_dev_peek_windows(d._h, words.ctypes.data, words.size, None, 128, C.byref(kw), C.byref(lanes)) == ERR_ARG
        assert L.ramx_dev_peek_windows(d._h, words.ctypes.data, words.size, bounds.ctypes.data, 128, None, C.byref(lanes)) == ERR_ARG
        assert L.ramx_dev_peek_windows(d._h, words.ctypes.data, words.size, bounds.ctypes.data, 128, C.byref(kw), None) == ERR_ARG
        assert L.ramx_dev_peek_windows(d._h, words.ctypes.data, words.size - 1, bounds.ctypes.data, 128, C.byref(kw), C.byref(lanes)) == ERR_ARG
        assert L.ramx_dev_peek_windows(d._h, words.ctypes.data, words.size, bounds.ctypes.data, 127, C.byref(kw), C.byref(lanes)) == ERR_ARG
        assert L.ramx_dev_peek_windows(d._h, words.ctypes.data, -1, bounds.ctypes.data, 128, C.byref(kw), C.byref(lanes)) == ERR_ARG
        assert (kw.value, lanes.value) == (c.KW, 128) and not words.any() and not bounds.any()       # refused before anything is copied
        assert L.ramx_dev_peek_windows(d._h, *args) == 0
        same((words, bounds), reference(c, "byte"), c, "raw call")
        one, two = d.peek_windows(), d.peek_windows()
        assert one[0].tobytes() == two[0].tobytes() == words.tobytes() and one[1].tobytes() == two[1].tobytes() == bounds.tobytes()
    finally:
        d.close()
