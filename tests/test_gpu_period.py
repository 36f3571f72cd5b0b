"""ramx_dev_period and the three seam-1 calls against the brute-force restatement (tests/period_ref.py), record for record:
segment counts round the tile of 64, lengths round the block of 8, the stream word of 32 and the workgroup of 256 threads mixed
in one call, every parameter at its edges, planted poly-A, (CA)n and a satellite of unit 171, the tie cases, N runs across block
and word edges, both library forms, segments at and past the ends of the library, tile groups; then the seam-1 calls after real
extension calls."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd import _lib
from repeatafterme_amd.datamodel import PERIOD_DTYPE, PERIOD_SEG_DTYPE, CoreSet, PeriodParams, new_master
from repeatafterme_amd.loader import pack_library

import period_ref as pr
from helpers import to_extend_params
from test_period_ref import codes

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -103, -104, -106
N_SEGS = 130
SHORT = [0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257]
# the tie cases of tests/test_period_ref.py, as segments 3, 4 and 5
TIE_RESTART = "AAAAAAACN" + "GGGGTCN" + "TTTTTT" + "N" + "A" + "N"
TIE_EARLIER = "TTTTTTNAN" + "ACG" + "NNNN" + "TTTTTTNAN"
TIE_PERIOD = "AANAA"
LONG_AT, LONG_LEN = 70, 2100           # the one long segment: in the calls of more than 70 segments only


def tup(r):
    return tuple(int(r[k]) for k in ("period", "score", "start", "end", "agree", "disagree"))


def make_library(seed=5):
    """N_SEGS segments back to back, two bases between them: random background with planted repeats -- poly-A, (CA)n, a unit of
    171 four times at 10 % divergence, short units --, N runs across the edges of blocks (8) and stream words (32), lower case.
    Segment 0 begins at position 0, segment 1 four bases in front of the library; the last one ends at the last position and
    the one before it reaches past it."""
    rng = np.random.default_rng(seed)
    parts, segs, at = [], [], 0
    for i in range(N_SEGS):
        n = SHORT[i % len(SHORT)]
        if i == LONG_AT:
            n = LONG_LEN
        elif i in (20, 60, 90):
            n = {20: 597, 60: 600, 90: 613}[i]
        x = rng.integers(0, 4, n).astype(np.int8)
        if i == 3:
            x = codes(TIE_RESTART)
        elif i == 4:
            x = codes(TIE_EARLIER)
        elif i == 5:
            x = codes(TIE_PERIOD)
        elif i == LONG_AT:
            unit = rng.integers(0, 4, 171).astype(np.int8)
            sat = np.tile(unit, 4)
            hit = rng.random(len(sat)) < 0.10
            sat[hit] = (sat[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
            x[700:700 + len(sat)] = sat
            x[100:124] = 0                                  # poly-A of 24
            x[1500:1530] = np.tile([1, 0], 15)              # (CA)15
        elif n >= 31:
            kind = int(rng.integers(0, 4))
            ln = int(rng.integers(12, min(n, 60)))
            a = int(rng.integers(0, n - ln + 1))
            if kind == 0:
                x[a:a + ln] = 0
            elif kind == 1:
                x[a:a + ln] = np.resize([1, 0], ln)
            elif kind == 2:
                x[a:a + ln] = np.resize(rng.integers(0, 4, int(rng.integers(3, 12))), ln)
            if n >= 63:
                for edge in (8, 32, 56):                    # N runs across a block edge, a word edge, and both
                    if rng.random() < 0.5:
                        x[edge - int(rng.integers(1, 4)):edge + int(rng.integers(1, 4))] = 99
        segs.append((at, at + len(x) - 1))
        gap = rng.integers(0, 4, 2).astype(np.int8) if i + 1 < N_SEGS else np.zeros(0, np.int8)
        parts += [x, gap]
        at += len(x) + len(gap)
    lib = np.concatenate(parts).astype(np.int8)
    low = (rng.random(len(lib)) < 0.1) & (lib < 4)
    low[segs[3][0]:segs[5][1] + 1] = False
    lib[low] += 4
    segs[1] = (-4, segs[1][1])
    segs[N_SEGS - 2] = (segs[N_SEGS - 2][0], len(lib) + 5)
    s = np.array(segs, np.int64).view(PERIOD_SEG_DTYPE).reshape(-1)
    assert s["lo"][0] == 0 and s["hi"][-1] == len(lib) - 1 and (s["lo"] == s["hi"] + 1).any()
    return lib, s


_cache = {}


def library(form):
    """The library of the seam-2 tests and its segments; for the packed form the tables, with windows that begin inside
    segments, at odd phases."""
    if not _cache:
        lib, segs = make_library()
        # the packed form knows A C G T and N only: lower case is not part of it
        plain = np.where((lib >= 4) & (lib <= 7), lib - 4, lib).astype(np.int8)
        starts = [0, int(segs["lo"][20]) + 301, int(segs["lo"][40]) + 3, int(segs["lo"][LONG_AT]) + 777, int(segs["lo"][100]) + 1]
        _cache.update(byte=(lib, segs, None), packed=(plain, segs, pack_library(plain, starts, [0, 3, 1, 2, 3])))
        _cache["expected"] = {}
    return _cache[form]


def expected(form, n, pp):
    key = (form, n, pp.pmax, pp.mm, pp.min_score)
    lib, segs, _ = library(form)
    if key not in _cache["expected"]:
        _cache["expected"][key] = pr.records(lib, [(int(s["lo"]), int(s["hi"])) for s in segs[:n]], pmax=pp.pmax, mm=pp.mm,
                                             min_score=pp.min_score)
    return _cache["expected"][key]


@pytest.fixture(scope="module")
def devices():
    from repeatafterme_amd.device import Device
    out = {}
    for form in ("byte", "packed"):
        lib, _, tables = library(form)
        d = Device(0)
        if tables is None:
            d.load_library(np.ascontiguousarray(lib))
        else:
            d.load_library_packed(tables)
        out[form] = d
    yield out
    for d in out.values():
        d.close()


# every count round the tile, every pmax round the workgroup's 256 threads and above every length, every mm, a min_score no
# tract reaches, on both forms; the long segment is in the calls of 130 only
SHAPES = [
    ("byte", 130, PeriodParams(1024, 3, 16)),
    ("packed", 130, PeriodParams(1024, 3, 16)),
    ("byte", 1, PeriodParams(1024, 3, 1)),
    ("packed", 63, PeriodParams(1, 3, 1)),
    ("byte", 64, PeriodParams(2, 1, 1)),
    ("packed", 65, PeriodParams(255, 15, 16)),
    ("byte", 65, PeriodParams(256, 3, 1)),
    ("packed", 64, PeriodParams(257, 1, 8)),
    ("byte", 63, PeriodParams(8192, 3, 1)),
    ("packed", 130, PeriodParams(8192, 15, 1)),
    ("byte", 65, PeriodParams(1024, 3, 1 << 20)),
]


@pytest.mark.parametrize("form,n,pp", SHAPES, ids=lambda v: v if isinstance(v, str) else (str(v) if isinstance(v, int) else
                                                                                         f"p{v.pmax}m{v.mm}s{v.min_score}"))
def test_records_equal_the_restatement(devices, form, n, pp):
    _, segs, _ = library(form)
    got = devices[form].period(segs[:n], pp)
    want = expected(form, n, pp)
    bad = [(i, tup(got[i]), want[i]) for i in range(n) if tup(got[i]) != want[i]]
    assert not bad, bad[:5]
    assert not got["reserved"].any()
    # a second call with the same arguments gives the same bytes
    assert devices[form].period(segs[:n], pp).tobytes() == got.tobytes()


def test_the_shapes_are_not_empty_ground():
    """The restatement's own records on these segments: the planted repeats show, the satellite as period 171, the ties as the
    CPU tests have them, and the N runs and the library's ends change what is found."""
    lib, segs, _ = library("byte")
    want = expected("byte", 130, PeriodParams(1024, 3, 16))
    periods = [w[0] for w in want]
    assert periods.count(1) >= 5 and periods.count(2) >= 5 and periods.count(0) >= 30 and sum(3 <= p <= 11 for p in periods) >= 3
    sat = want[LONG_AT]
    assert sat[0] == 171 and sat[1] > 100 and 690 <= sat[2] <= 712 and sat[5] > 20, sat
    one = expected("byte", 63, PeriodParams(1, 3, 1))
    assert one[3] == (1, 5, 16, 23, 5, 0) and one[4] == (1, 5, 0, 7, 5, 0)
    assert expected("byte", 1, PeriodParams(1024, 3, 1)) == [pr.ZERO]
    assert expected("byte", 63, PeriodParams(8192, 3, 1))[5] == (1, 2, 0, 3, 2, 0)
    assert all(w == pr.ZERO for w in expected("byte", 65, PeriodParams(1024, 3, 1 << 20)))
    nofold = np.where(lib == 99, 0, lib)
    s = [(int(a), int(b)) for a, b in zip(segs["lo"], segs["hi"])]
    assert sum(a != b for a, b in zip(pr.records(nofold, s[:70]), want[:70])) > 2
    # what lies outside the library is no base: the segment that reaches past the end is not its clipped self shifted
    assert segs["lo"][1] == -4 and segs["hi"][128] == len(lib) + 5


def test_the_poly_a_and_ca_of_the_issue(devices):
    """A poly-A of 24 and a (CA)15 alone in random-free ground (N around them) score 23 and 28."""
    from repeatafterme_amd.device import Device
    lib = np.concatenate((codes("N" * 9), codes("A" * 24), codes("N" * 11), codes("CA" * 15), codes("N" * 7))).astype(np.int8)
    d = Device(0)
    try:
        d.load_library(lib)
        segs = np.array([(9, 32), (44, 73), (0, len(lib) - 1), (5, 40)], np.int64).view(PERIOD_SEG_DTYPE).reshape(-1)
        got = [tup(r) for r in d.period(segs, PeriodParams(1024, 3, 16))]
    finally:
        d.close()
    assert got[0] == (1, 23, 0, 22, 23, 0) and got[1] == (2, 28, 0, 27, 28, 0)
    assert got == pr.records(lib, [(int(a), int(b)) for a, b in zip(segs["lo"], segs["hi"])])
    # the whole library at p = 2: the 22 pairs of the poly-A and the 28 of the (CA)15 are one tract, for the blocks of N between
    # them score 0 and end nothing; it begins with the block that holds offset 9
    assert got[2] == (2, 50, 8, 71, 50, 0) and got[3][0] == 1


def test_the_length_limit():
    """65,536 bases of poly-A with one C: the longest segment, the largest score the key holds, every period of the largest
    pmax; one base more is refused."""
    from repeatafterme_amd.device import Device
    lib = np.zeros(65540, np.int8)
    lib[65536] = 1
    d = Device(0)
    try:
        d.load_library(lib)
        seg = lambda lo, hi: np.array([(lo, hi)], np.int64).view(PERIOD_SEG_DTYPE).reshape(-1)      # noqa: E731
        assert tup(d.period(seg(0, 65535), PeriodParams(8192, 3, 16))[0]) == (1, 65535, 0, 65534, 65535, 0)
        # with the C as the last base the last pair of every period disagrees: at mm = 15 the last block (six agreeing pairs and
        # that one at p = 1, five and that one at p = 2) is not worth having, and p = 1 and p = 2 tie at 65,528: the smaller wins
        assert tup(d.period(seg(1, 65536), PeriodParams(8192, 15, 16))[0]) == (1, 65528, 0, 65527, 65528, 0)
        out = np.zeros(1, PERIOD_DTYPE)
        pp = _lib.PeriodParams(1024, 3, 16, 0)
        assert _lib.lib().ramx_dev_period(d._h, seg(0, 65536).ctypes.data, 1, C.byref(pp), out.ctypes.data, None) == ERR_UNSUPPORTED
    finally:
        d.close()


def tile_bytes(nmax):
    """The windows and streams of one tile of 64 segments: 4 bytes a window word (one of 8 bases and the pad word), 12 bytes a
    stream word of 32 bases."""
    return 64 * (4 * ((nmax + 7) // 8 + 1) + 12 * max((nmax + 31) // 32, 1))


def test_tile_groups_do_not_show(devices):
    lib, segs, _ = library("byte")
    pp = PeriodParams(1024, 3, 16)
    want = expected("byte", 130, pp)
    nmax = int((segs["hi"] + 1 - segs["lo"]).max())
    assert nmax == LONG_LEN
    old = os.environ.get("RAMX_PERIOD_BYTES")
    try:
        for budget in (tile_bytes(nmax), 2 * tile_bytes(nmax) + 5):              # three groups of one tile; two groups of 2 + 1
            os.environ["RAMX_PERIOD_BYTES"] = str(budget)
            got, ms = devices["byte"].period(segs, pp, timing=True)
            assert [tup(r) for r in got] == want
            assert len(ms) == 3 and all(m > 0 for m in ms)
        os.environ["RAMX_PERIOD_BYTES"] = str(tile_bytes(nmax) - 1)
        out = np.full(130 * 8, 7, np.int32).view(PERIOD_DTYPE)
        cp = _lib.PeriodParams(1024, 3, 16, 0)
        assert _lib.lib().ramx_dev_period(devices["byte"]._h, segs.ctypes.data, 130, C.byref(cp), out.ctypes.data, None) == ERR_UNSUPPORTED
        assert (out.view(np.int32) == 7).all()
        # the budget is per call and counts the call's own longest segment
        assert [tup(r) for r in devices["byte"].period(segs[:64], pp)] == want[:64]
    finally:
        if old is None:
            os.environ.pop("RAMX_PERIOD_BYTES", None)
        else:
            os.environ["RAMX_PERIOD_BYTES"] = old


def test_no_segment_and_bad_arguments(devices):
    d = devices["byte"]
    _, segs, _ = library("byte")
    assert len(d.period(segs[:0])) == 0
    L, ok = _lib.lib(), _lib.PeriodParams(1024, 3, 16, 0)
    out = np.full(4 * 8, 7, np.int32).view(PERIOD_DTYPE)
    for bad in [(0, 3, 16), (8193, 3, 16), (1024, 0, 16), (1024, 16, 16), (1024, 3, 0), (-1, 3, 16), (1024, -1, 16)]:
        assert L.ramx_dev_period(d._h, segs.ctypes.data, 4, C.byref(_lib.PeriodParams(*bad, 0)), out.ctypes.data, None) == ERR_ARG, bad
    assert L.ramx_dev_period(d._h, segs.ctypes.data, 4, None, out.ctypes.data, None) == ERR_ARG
    assert L.ramx_dev_period(d._h, segs.ctypes.data, -1, C.byref(ok), out.ctypes.data, None) == ERR_ARG
    assert L.ramx_dev_period(d._h, None, 4, C.byref(ok), out.ctypes.data, None) == ERR_ARG
    assert L.ramx_dev_period(d._h, segs.ctypes.data, 4, C.byref(ok), None, None) == ERR_ARG
    assert L.ramx_dev_period(None, segs.ctypes.data, 4, C.byref(ok), out.ctypes.data, None) == ERR_ARG
    s = segs[:4].copy()
    s["lo"][2] = s["hi"][2] + 2
    assert L.ramx_dev_period(d._h, s.ctypes.data, 4, C.byref(ok), out.ctypes.data, None) == ERR_ARG
    # raised before anything is written
    assert (out.view(np.int32) == 7).all()
    assert L.ramx_dev_period(d._h, segs.ctypes.data, 0, C.byref(ok), None, None) == 0


def test_a_direction_needs_a_new_begin_after_a_period_call():
    from repeatafterme_amd.device import Device, resolve_flanks
    e = pr.planted_expectation()
    p = to_extend_params(e["p"])
    d = Device(0)
    try:
        d.load_library(np.ascontiguousarray(e["seq"]))
        flanks, _ = resolve_flanks(1, e["cores"], p.bandwidth, p.L)
        d.begin_direction(flanks, p)
        got = d.period(np.array(e["segs"][1], np.int64).view(PERIOD_SEG_DTYPE).reshape(-1))
        assert [tup(r) for r in got] == e["records"][1]
        ci = _lib.RunInfo()
        assert d._L.ramx_dev_run_direction(d._h, C.byref(ci)) == ERR_STATE
        d.begin_direction(flanks, p)
        assert d.run_direction().rows_executed > 0
    finally:
        d.close()


# ---- seam 1 ----

def gpu_both_directions(cores, seq, p):
    from repeatafterme_amd.extend import extend_alignment
    c, m = cores.copy(), new_master(p.L)
    rets = {d: extend_alignment(d, c, seq, m, to_extend_params(p)).ret for d in (1, 0)}
    return c, m, rets


def test_period_flat_on_the_planted_family():
    """Two extend_alignment calls, then ramx_period_flat on the library they left on the device: the CPU expectation (the loop
    is bit-exact against the oracle, so the segments are the same)."""
    from repeatafterme_amd.extend import extend_alignment, period_flat, period_segments, period_summary
    e = pr.planted_expectation()
    c, m, rets = gpu_both_directions(e["cores"], e["seq"], e["p"])
    assert rets == e["rets"] and np.array_equal(c.left_len, e["after"].left_len) and np.array_equal(c.right_len, e["after"].right_len)
    for which in (0, 1, 2):
        got = period_flat(c, e["seq"], which)
        assert [tup(r) for r in got] == e["records"][which], which
    s = period_summary(period_flat(c, e["seq"], 1), period_segments(c, 1))
    assert s.mode == 2 and 2 * s.mode_count >= pr.PLANTED["M"]
    # on a library the device does not hold (a copy at another address): uploaded, the same records
    assert [tup(r) for r in period_flat(c, e["seq"].copy(), 1)] == e["records"][1]
    assert period_flat(c.subset(slice(0, 0)), e["seq"], 1).shape == (0,)
    # other parameters through the same call
    pp = PeriodParams(1, 3, 16)
    assert [tup(r) for r in period_flat(c, e["seq"], 1, pp)] == pr.records(e["seq"], e["segs"][1], pmax=1)
    # ... and as the extension call's own last result
    c2, m2 = e["cores"].copy(), new_master(e["p"].L)
    info, rec = extend_alignment(1, c2, e["seq"], m2, to_extend_params(e["p"]), period=True)
    assert info.ret == e["rets"][1] and [tup(r) for r in rec] == e["records"][1]


def test_period_alignment_on_the_list():
    """The same through the reference's data model: a linked list of cores and a sequence library."""
    from repeatafterme_amd.extend import period_alignment
    from repeatafterme_amd.loader import _Core, _SeqLib
    e = pr.planted_expectation()
    c, n = e["after"], e["after"].n
    arr = (_Core * n)()
    for i in range(n):
        a = arr[i]
        a.next = C.pointer(arr[i + 1]) if i + 1 < n else None
        a.leftSeqPos, a.rightSeqPos, a.lowerSeqBound, a.upperSeqBound = int(c.left_pos[i]), int(c.right_pos[i]), int(c.lower[i]), int(c.upper[i])
        a.orient = bytes([int(c.orient[i])])
        a.leftExtensionLen, a.rightExtensionLen = int(c.left_len[i]), int(c.right_len[i])
    seq = np.ascontiguousarray(e["seq"])
    sl = _SeqLib(seq.ctypes.data_as(C.POINTER(C.c_int8)), None, None, None, len(seq), 0, 0, None)
    for which in (0, 1, 2):
        got = period_alignment(arr, C.pointer(sl), n, which)
        assert [tup(r) for r in got] == e["records"][which], which


def test_period_batch_with_an_empty_family_between():
    from repeatafterme_amd.extend import extend_batch, period_batch
    p = pr.planted_expectation()["p"]
    fams = []
    for kw in (dict(M=14, seed=21), None, dict(M=9, seed=22)):
        if kw is None:
            seq = np.random.default_rng(5).integers(0, 4, 333).astype(np.int8)
            cores = CoreSet(left_pos=[], right_pos=[], lower=[], upper=[], orient=[], left_ext=[], right_ext=[])
        else:
            seq, cores, _ = pr.planted_family(**kw)
        fams.append((cores, seq))
    batch = [(c.copy(), s, new_master(p.L)) for c, s in fams]
    for d in (1, 0):
        extend_batch(d, batch, to_extend_params(p))
    for which in (1, 2):
        got = period_batch(batch, which)
        assert [len(g) for g in got] == [14, 0, 9]
        for (c0, s), (c, _, m), g in zip(fams, batch, got):
            if c0.n == 0:
                continue
            oc, om = c0.copy(), new_master(p.L)
            for d in (1, 0):
                po.oracle_extend(d, oc, s, om, p)
            assert np.array_equal(c.left_len, oc.left_len) and np.array_equal(c.right_len, oc.right_len)
            want = pr.records(s, pr.segments_of(oc, which))
            assert [tup(r) for r in g] == want
            assert pr.summary(want, pr.segments_of(oc, which))["mode"] == 2
    # once more on copies of the libraries: the concatenation is built and sent again, the records are the same
    again = period_batch([(c, s.copy(), m) for c, s, m in batch], 2)
    assert all(a.tobytes() == g.tobytes() for a, g in zip(again, got))


def border_families():
    """Three families of five copies each, the extension lengths set by hand.  Every library begins with 20 A and ends with 24 A:
    across a border they are one tract of 44.  Copy 0 begins at base 0 of its library and copy 4 ends at its last base; copy 1's
    left extension begins 10 bases in front of the library and copy 3's right extension ends 10 bases behind it: read across the
    border, both would hold more of the tract.  Copy 2 lies in the middle, on the reverse strand, with a (CA)20 in its left
    extension.  -> [(cores, sequence)]"""
    rng = np.random.default_rng(43)
    fams = []
    for f in range(3):
        seq = rng.integers(0, 4, 300).astype(np.int8)
        seq[:20] = 0
        seq[-24:] = 0
        seq[20], seq[-25] = 1, 2                    # (the tracts end where they are said to)
        seq[160:200] = np.tile([1, 0], 20)
        n = len(seq)
        # (lo, hi, core's first base, core's last base, reverse strand)
        ext = [(0, 69, 30, 40, 0), (-10, 59, 25, 35, 0), (100, 219, 140, 150, 1), (240, n + 9, 255, 265, 0), (230, n - 1, 250, 260, 0)]
        lp = [c1 if m else c0 for lo, hi, c0, c1, m in ext]
        rp = [c0 if m else c1 for lo, hi, c0, c1, m in ext]
        ll = [hi - c1 if m else c0 - lo for lo, hi, c0, c1, m in ext]
        rl = [c0 - lo if m else hi - c1 for lo, hi, c0, c1, m in ext]
        cores = CoreSet(left_pos=lp, right_pos=rp, lower=[0] * 5, upper=[n - 1] * 5, orient=[e[4] for e in ext], left_ext=[1] * 5,
                        right_ext=[1] * 5, left_len=ll, right_len=rl)
        assert pr.segments_of(cores, 2) == [e[:2] for e in ext]
        fams.append((cores, seq))
    return fams


def test_a_batch_never_reads_across_a_familys_border():
    """ramx_period_batch on the concatenated library: every family's records are those of the family alone, although the
    neighbouring library continues the tract at either end."""
    from repeatafterme_amd.extend import period_batch
    fams = border_families()
    cat = np.concatenate([s for _, s in fams])
    at = np.cumsum([0] + [len(s) for _, s in fams])
    for which in (0, 1, 2):
        got = period_batch([(c, s, None) for c, s in fams], which)
        alone = [pr.records(s, pr.segments_of(c, which)) for c, s in fams]
        assert [[tup(r) for r in g] for g in got] == alone, which
        # not empty ground: tracts are found, and the same segments read on the concatenation hold longer ones
        assert all(sum(a != pr.ZERO for a in al) >= 2 for al in alone), which
        wide = [pr.records(cat, [(lo + int(at[f]), hi + int(at[f])) for lo, hi in pr.segments_of(c, which)]) for f, (c, _) in enumerate(fams)]
        differ = [[w != a for w, a in zip(wide[f], alone[f])] for f in range(3)]
        # (copy 1's left extension, copy 3's right one; the first library has nothing in front of it, the last nothing behind)
        assert differ == [[False, f > 0 and which != 1, False, f < 2 and which != 0, False] for f in range(3)], (which, differ)
