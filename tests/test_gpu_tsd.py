"""ramx_dev_tsd and the three seam-1 calls against the brute-force restatement (tests/tsd_ref.py), record for record: site
counts round the wave of 64, every slack / length range / mismatch rule, both library forms, sites at both ends of the library,
bounds that cut a word, N runs and window boundaries of the packed form; then the seam-1 calls after real extension calls, and a
batch whose families' libraries would complete each other's duplications."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd import _lib
from repeatafterme_amd.datamodel import TSD_DTYPE, TSD_SITE_DTYPE, CoreSet, TsdParams, new_master
from repeatafterme_amd.loader import pack_library

import tsd_ref as tr
from helpers import to_extend_params

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -103, -104
N_SITES = 130


def make_sites(seed=3):
    """A library with N_SITES planted sites: element i sits between two copies of a word of 1..32 bases, sometimes with a
    mismatch, an N run across the word's beginning, lower-case bases; the reported ends are off by up to three bases and the
    bounds sometimes cut a word.  Site 0 begins at position 0, the last site ends at the last position, some elements are empty."""
    rng = np.random.default_rng(seed)
    parts, sites, at = [], [], 0
    for i in range(N_SITES):
        k = int(rng.choice([1, 2, 4, 5, 6, 8, 9, 12, 15, 20, 26, 32, 32, 32]))
        word = rng.integers(0, 4, k).astype(np.int8)
        right = word.copy()
        if k >= 4 and rng.random() < 0.3:
            j = int(rng.integers(1, k - 1))
            right[j] = (right[j] + 1) % 4
        left = word.copy()
        if k >= 8 and rng.random() < 0.15:
            left[:2] = 99                                   # an N run that begins in the filler and crosses into the word
        elem = rng.integers(0, 4, int(rng.choice([0, 3, 17, 25, 33, 40, 61]))).astype(np.int8)
        filler = rng.integers(0, 4, 70).astype(np.int8)
        if k >= 8 and (left[:2] == 99).all():
            filler[-3:] = 99
        first, last = i == 0, i == N_SITES - 1
        pre = [] if first else [filler, left]
        post = [] if last else [right]
        if first or last:
            elem = rng.integers(0, 4, 40).astype(np.int8)
        lo = at + sum(len(x) for x in pre)
        hi = lo + len(elem) - 1
        for x in pre + [elem] + post:
            parts.append(x)
            at += len(x)
        # what the caller reports: ends off by up to three bases (never crossing), bounds wide or cutting into a word
        sl, sr = (0, 0) if len(elem) < 7 or first or last else (int(rng.integers(-3, 4)), int(rng.integers(-3, 4)))
        rlo, rhi = lo - sl, hi + sr
        seq_lo = rlo - int(rng.choice([200, 200, 200, 35, max(k - 2, 0), 0]))
        seq_hi = rhi + int(rng.choice([200, 200, 200, 35, max(k - 2, 0), 0]))
        sites.append((rlo, rhi, seq_lo, seq_hi))
    lib = np.concatenate(parts).astype(np.int8)
    lower = (rng.random(len(lib)) < 0.1) & (lib < 4)
    lib[lower] += 4
    s = np.array(sites, np.int64).view(TSD_SITE_DTYPE).reshape(-1)
    assert s["lo"][0] == 0 and s["hi"][-1] == len(lib) - 1 and (s["lo"] == s["hi"] + 1).any()
    return lib, s


_cache = {}


def library(form):
    """The library of the seam-2 tests, its sites, and for the packed form the tables: windows that begin at a site's first base
    (the left word ends in the window before), in the middle of a word, at odd phases."""
    if not _cache:
        lib, sites = make_sites()
        # the packed form knows A C G T and N only: lower case is not part of it
        plain = np.where((lib >= 4) & (lib <= 7), lib - 4, lib).astype(np.int8)
        starts = [0, int(sites["lo"][40]), int(sites["hi"][77]) + 3, int(sites["lo"][100]) - 2]
        _cache.update(byte=(lib, sites, None), packed=(plain, sites, pack_library(plain, starts, [0, 3, 1, 2])))
        _cache["expected"] = {}
    return _cache[form]


def expected(form, n, tp):
    key = (form, n, tp.slack, tp.kmin, tp.kmax, tp.mm_div)
    lib, sites, _ = library(form)
    if key not in _cache["expected"]:
        _cache["expected"][key] = tr.tsd_all(lib, [tuple(int(v) for v in s) for s in sites[:n]], slack=tp.slack, kmin=tp.kmin,
                                             kmax=tp.kmax, mm_div=tp.mm_div)
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


# every n round the wave, every slack, every length range and every mismatch rule at least once on each form; the widest search
# (slack 7, lengths 1..32) on the sites of one wave and a bit
SHAPES = [
    ("byte", 130, TsdParams(3, 4, 20, 10)),
    ("packed", 130, TsdParams(3, 4, 20, 10)),
    ("byte", 65, TsdParams(0, 1, 32, 4)),
    ("packed", 64, TsdParams(7, 4, 20, 0)),
    ("byte", 130, TsdParams(3, 32, 32, 10)),
    ("packed", 130, TsdParams(0, 32, 32, 4)),
    ("packed", 1, TsdParams(7, 1, 32, 4)),
    ("byte", 1, TsdParams(3, 1, 32, 0)),
    ("byte", 63, TsdParams(3, 1, 32, 0)),
    ("byte", 65, TsdParams(7, 1, 32, 10)),
    ("packed", 63, TsdParams(7, 1, 32, 10)),
]


@pytest.mark.parametrize("form,n,tp", SHAPES, ids=lambda v: v if isinstance(v, str) else (str(v) if isinstance(v, int) else
                                                                                         f"S{v.slack}k{v.kmin}-{v.kmax}m{v.mm_div}"))
def test_records_equal_the_restatement(devices, form, n, tp):
    _, sites, _ = library(form)
    got = devices[form].tsd(sites[:n], tp)
    want = expected(form, n, tp)
    bad = [(i, tuple(int(v) for v in got[i]), want[i]) for i in range(n) if tuple(int(v) for v in got[i]) != want[i]]
    assert not bad, bad[:5]
    # a second call with the same arguments gives the same bytes
    assert devices[form].tsd(sites[:n], tp).tobytes() == got.tobytes()


def test_the_shapes_are_not_empty_ground():
    """The restatement's own records on these sites: duplications found, with and without mismatches, at every shift, none at
    the two ends of the library, and the bounds and the N runs change what is found."""
    for form in ("byte", "packed"):
        lib, sites, _ = library(form)
        want = np.array(expected(form, 130, TsdParams(3, 4, 20, 10)))
        assert (want[:, 0] > 0).sum() > 40 and (want[:, 1] > 0).sum() > 5 and (want[:, 0] == 0).sum() > 5
        assert set(want[:, 2]) >= set(range(-3, 4)) and set(want[:, 3]) >= set(range(-3, 4))
        assert tuple(want[0]) == (0, 0, 0, 0) and tuple(want[-1]) == (0, 0, 0, 0)
        wide = [(int(s["lo"]), int(s["hi"]), -10 ** 6, 10 ** 6) for s in sites]
        assert sum(a != tuple(b) for a, b in zip(tr.tsd_all(lib, wide), want)) > 3
        nofold = np.where(lib == 99, 0, lib)
        assert sum(a != tuple(b) for a, b in zip(tr.tsd_all(nofold, [tuple(int(v) for v in s) for s in sites]), want)) > 0
    assert (np.array(expected("byte", 130, TsdParams(3, 32, 32, 10)))[:, 0] == 32).sum() >= 5
    # the calls of 65 sites have two tiles, the second with one site; windows wholly outside their bounds (seq_lo == lo: no left
    # word; seq_hi == hi: no right one) share the first tile with ordinary sites
    _, sites, _ = library("byte")
    assert (sites["seq_lo"][:64] == sites["lo"][:64]).any() and (sites["seq_hi"][:64] == sites["hi"][:64]).any()
    assert ((sites["seq_lo"][:64] < sites["lo"][:64] - 40) & (sites["seq_hi"][:64] > sites["hi"][:64] + 40)).any()
    assert (np.array(expected("packed", 130, TsdParams(0, 32, 32, 4)))[:, 0] == 32).sum() >= 2


def test_no_site_and_bad_arguments(devices):
    d = devices["byte"]
    _, sites, _ = library("byte")
    assert len(d.tsd(sites[:0])) == 0
    L, ok = _lib.lib(), _lib.TsdParams(3, 4, 20, 10)
    out = np.full(4, 7, np.int32).repeat(4).view(TSD_DTYPE)
    keep = out.copy()
    for bad in [(-1, 4, 20, 10), (8, 4, 20, 10), (3, 0, 20, 10), (3, 6, 5, 10), (3, 4, 33, 10), (3, 4, 20, 3)]:
        assert L.ramx_dev_tsd(d._h, sites.ctypes.data, 4, C.byref(_lib.TsdParams(*bad)), out.ctypes.data, None) == ERR_ARG, bad
    assert L.ramx_dev_tsd(d._h, sites.ctypes.data, 4, None, out.ctypes.data, None) == ERR_ARG
    assert L.ramx_dev_tsd(d._h, sites.ctypes.data, -1, C.byref(ok), out.ctypes.data, None) == ERR_ARG
    assert L.ramx_dev_tsd(d._h, None, 4, C.byref(ok), out.ctypes.data, None) == ERR_ARG
    assert L.ramx_dev_tsd(d._h, sites.ctypes.data, 4, C.byref(ok), None, None) == ERR_ARG
    assert L.ramx_dev_tsd(None, sites.ctypes.data, 4, C.byref(ok), out.ctypes.data, None) == ERR_ARG
    for field, delta in (("seq_lo", +1), ("seq_hi", -1), ("lo", None)):
        s = sites[:4].copy()
        if delta is None:
            s["lo"][2] = s["hi"][2] + 2
        else:
            s[field][2] = (s["lo"][2] if field == "seq_lo" else s["hi"][2]) + delta
        assert L.ramx_dev_tsd(d._h, s.ctypes.data, 4, C.byref(ok), out.ctypes.data, None) == ERR_ARG, field
    # raised before anything is written
    assert out.tobytes() == keep.tobytes()
    assert L.ramx_dev_tsd(d._h, sites.ctypes.data, 0, C.byref(ok), None, None) == 0


def test_timing_and_a_direction_needs_a_new_begin_after_a_tsd_call():
    from repeatafterme_amd.device import Device, resolve_flanks
    e = tr.planted_expectation()
    p = to_extend_params(e["p"])
    d = Device(0)
    try:
        d.load_library(np.ascontiguousarray(e["seq"]))
        flanks, _ = resolve_flanks(1, e["cores"], p.bandwidth, p.L)
        d.begin_direction(flanks, p)
        sites = np.array(e["sites"], np.int64).view(TSD_SITE_DTYPE).reshape(-1)
        got, ms = d.tsd(sites, timing=True)
        assert [tuple(int(v) for v in r) for r in got] == e["records"]
        assert len(ms) == 2 and all(m > 0 for m in ms)
        ci = _lib.RunInfo()
        assert d._L.ramx_dev_run_direction(d._h, C.byref(ci)) == ERR_STATE
        d.begin_direction(flanks, p)
        assert d.run_direction().rows_executed > 0
        # without the times: the same bytes
        assert d.tsd(sites).tobytes() == got.tobytes()
    finally:
        d.close()


# ---- seam 1 ----

def gpu_both_directions(cores, seq, p):
    from repeatafterme_amd.extend import extend_alignment
    c, m = cores.copy(), new_master(p.L)
    rets = {d: extend_alignment(d, c, seq, m, to_extend_params(p)).ret for d in (1, 0)}
    return c, m, rets


def test_tsd_flat_on_the_planted_family():
    """Two extend_alignment calls, then ramx_tsd_flat on the library they left on the device: the CPU expectation (the loop is
    bit-exact against the oracle, so the sites are the same)."""
    from repeatafterme_amd.extend import tsd_flat, tsd_summary
    e = tr.planted_expectation()
    c, m, rets = gpu_both_directions(e["cores"], e["seq"], e["p"])
    assert rets == e["rets"] and np.array_equal(c.left_len, e["after"].left_len) and np.array_equal(c.right_len, e["after"].right_len)
    got = tsd_flat(c, e["seq"])
    assert [tuple(int(v) for v in r) for r in got] == e["records"]
    s = tsd_summary(got)
    assert s.mode == tr.PLANTED["k"] and 2 * s.mode_count >= tr.PLANTED["M"]
    # on a library the device does not hold (a copy at another address): uploaded, the same records
    assert tsd_flat(c, e["seq"].copy()).tobytes() == got.tobytes()
    assert tsd_flat(c.subset(slice(0, 0)), e["seq"]).shape == (0,)


def test_tsd_alignment_on_the_list():
    """The same through the reference's data model: a linked list of cores and a sequence library."""
    from repeatafterme_amd.extend import tsd_alignment
    from repeatafterme_amd.loader import _Core, _SeqLib
    e = tr.planted_expectation()
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
    got = tsd_alignment(arr, C.pointer(sl), n)
    assert [tuple(int(v) for v in r) for r in got] == e["records"]


def test_tsd_batch_with_an_empty_family_between():
    from repeatafterme_amd.extend import extend_batch, tsd_batch
    p = tr.planted_expectation()["p"]
    fams = []
    for kw in (dict(M=14, k=5, seed=21, div=0.05), None, dict(M=9, k=8, seed=22, div=0.05)):
        if kw is None:
            seq = np.random.default_rng(5).integers(0, 4, 333).astype(np.int8)
            cores = CoreSet(left_pos=[], right_pos=[], lower=[], upper=[], orient=[], left_ext=[], right_ext=[])
        else:
            seq, cores, _ = tr.planted_family(**kw)
        fams.append((cores, seq))
    batch = [(c.copy(), s, new_master(p.L)) for c, s in fams]
    for d in (1, 0):
        extend_batch(d, batch, to_extend_params(p))
    got = tsd_batch(batch)
    assert [len(g) for g in got] == [14, 0, 9]
    modes = []
    for (c0, s), (c, _, m), g in zip(fams, batch, got):
        if c0.n == 0:
            continue
        oc, om = c0.copy(), new_master(p.L)
        for d in (1, 0):
            po.oracle_extend(d, oc, s, om, p)
        assert np.array_equal(c.left_len, oc.left_len) and np.array_equal(c.right_len, oc.right_len)
        want = tr.tsd_all(s, tr.sites_of(oc))
        assert [tuple(int(v) for v in r) for r in g] == want
        modes.append(tr.summary(want)[1])
    assert modes == [5, 8]
    # once more on copies of the libraries: the concatenation is built and sent again, the records are the same
    again = tsd_batch([(c, s.copy(), m) for c, s, m in batch])
    assert all(a.tobytes() == g.tobytes() for a, g in zip(again, got))


def test_an_extension_after_a_tsd_call_is_unchanged():
    """The TSD call reuses the device's flank and window buffers and may replace the library: an extension between and after TSD
    calls still gives the oracle's result."""
    from repeatafterme_amd.extend import extend_alignment, tsd_flat
    from repeatafterme_amd.synth import synth_family
    e = tr.planted_expectation()
    p = e["p"]
    ep = to_extend_params(p)
    fs = synth_family(200, 300, 14, K=200, seed=3, both_sides=True, minus_frac=0.3, n_run_frac=0.1)
    oc, om = fs.cores.copy(), new_master(p.L)
    orets = [po.oracle_extend(d, oc, fs.sequence, om, p).ret for d in (1, 0)]
    c, m = fs.cores.copy(), new_master(p.L)
    r1 = extend_alignment(1, c, fs.sequence, m, ep).ret
    mid = tsd_flat(c, fs.sequence)                        # on the resident library, between the two directions
    tsd_flat(e["after"], e["seq"])                        # ... and on another one, which replaces it
    r0 = extend_alignment(0, c, fs.sequence, m, ep).ret
    assert [r1, r0] == orets and np.array_equal(m, om)
    for key in ("left_len", "right_len", "score"):
        assert np.array_equal(getattr(c, key), getattr(oc, key)), key
    assert len(mid) == 200


def border_families(k=6):
    """Three families of four copies each, the extension lengths set by hand.  In every family copy 0 begins at base 0 of its
    library and copy 3 ends at its last base; copies 1 and 2 (one on the reverse strand) lie between planted words.  The
    libraries complete each other: the word in front of a family's last copy is the first word of the next family's library,
    and the word behind a family's first copy is the last word of the family before -- read across the border, both would be
    duplications of k bases.  Half the copies have bounds wider than their library.  -> [(cores, sequence)], [(lo, hi)] per family"""
    rng = np.random.default_rng(41)
    r = lambda n: rng.integers(0, 4, n).astype(np.int8)                         # noqa: E731
    seqs = []
    for f in range(3):
        a, b, w1, w2 = r(40), r(40), r(k), r(k)
        seqs.append([a, r(k), r(50), w1, r(30), w1, r(45), w2, r(33), w2, r(50), r(k), b])
    for f in range(2):
        seqs[f + 1][0][:k] = seqs[f][11]            # the next library begins with the word in front of this one's last copy
        seqs[f][12][-k:] = seqs[f + 1][1]           # this library ends with the word behind the next one's first copy
    fams, where = [], []
    for f in range(3):
        at = np.cumsum([0] + [len(x) for x in seqs[f]])
        seq = np.concatenate(seqs[f]).astype(np.int8)
        ext = [(int(at[i]), int(at[i + 1]) - 1) for i in (0, 4, 8, 12)]
        lp, rp, ll, rl = [], [], [], []
        for i, (lo, hi) in enumerate(ext):
            c0, c1 = lo + 10, lo + 14                                           # the core; copy 2 is on the reverse strand
            lp.append(c1 if i == 2 else c0); rp.append(c0 if i == 2 else c1)
            ll.append(hi - c1 if i == 2 else c0 - lo); rl.append(c0 - lo if i == 2 else hi - c1)
        n = len(seq)
        cores = CoreSet(left_pos=lp, right_pos=rp, lower=[-50, 0, -50, 0], upper=[n - 1, n + 50, n - 1, n + 50],
                        orient=[0, 0, 1, 0], left_ext=[1] * 4, right_ext=[1] * 4, left_len=ll, right_len=rl)
        assert tr.sites_of(cores)[0][0] == 0 and tr.sites_of(cores)[3][1] == n - 1
        assert [s[:2] for s in tr.sites_of(cores)] == ext
        fams.append((cores, seq))
        where.append(ext)
    return fams, where


def test_a_batch_never_reads_across_a_familys_border():
    """ramx_tsd_batch on the concatenated library: every family's records are those of the family alone, although the
    neighbouring library holds the word that would complete a duplication at either end."""
    from repeatafterme_amd.extend import tsd_batch
    fams, where = border_families()
    got = tsd_batch([(c, s, None) for c, s in fams])
    alone = [tr.tsd_all(s, tr.sites_of(c)) for c, s in fams]
    assert [[tuple(int(v) for v in r) for r in g] for g in got] == alone
    # not empty ground: the planted words are found, the copies at the libraries' ends have none ...
    assert all(a[0] == (0, 0, 0, 0) == a[3] and a[1] == (6, 0, 0, 0) == a[2] for a in alone)
    # ... and the same sites on the concatenation with its whole length for bounds find the neighbours' words
    cat = np.concatenate([s for _, s in fams])
    at = np.cumsum([0] + [len(s) for _, s in fams])
    wide = [tr.tsd_all(cat, [(lo + int(at[f]), hi + int(at[f]), 0, len(cat) - 1) for lo, hi in where[f]]) for f in range(3)]
    assert [[w != a for w, a in zip(wide[f], alone[f])] for f in range(3)] == [[False, False, False, True], [True, False, False, True],
                                                                             [True, False, False, False]]
