"""ramx_dev_term and the seam-1 calls on the GPU, record for record against the restatement of the contract (tests/term_ref.py):
every window length round the lanes' columns, planted direct and inverted repeats with indels, N runs, windows outside the
library, the ties, the parameters' ends, both library forms, tile groups, the refusals, and the three seam-1 calls after real
extension calls on the two planted families."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd import _lib
from repeatafterme_amd.datamodel import TERM_DTYPE, TSD_SITE_DTYPE, CoreSet, TermParams, new_master
from repeatafterme_amd.loader import pack_library

import term_ref as tr
from helpers import to_extend_params
from test_term_ref import codes

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -103, -104, -106
N_SITES = 130
# window lengths of the sites 0..64 (cycled) -- every C up to 4 and its partly filled last lane --; the long ones sit behind
SHORT_T = [0, 1, 2, 63, 64, 65, 127, 128, 129, 20, 33]
LONG_T = {70: 255, 71: 256, 72: 257, 100: 511, 101: 512, 102: 513, 103: 1023, 104: 1024}
# the tie cases of tests/test_term_ref.py as elements (the 5' half against the 3' half): best-cell ties in i, in j, i before j,
# and the three D / U / L cases (they show with match 2, mismatch 1, gap 1)
TIES = {2: "ACNACACNTT", 13: "ACNTTACNAC", 24: "ACNGTGTNAC", 35: "AAACACAC", 46: "ACACAAAC", 57: "ACACCAAC"}


def tup(r):
    return tuple(int(r[k]) for k in tr.FIELDS)


def mutate(rng, x, div, indel):
    """x with substitutions at rate div and single-base indels at rate indel."""
    out = []
    for b in x:
        u = rng.random()
        if u < indel / 2:
            continue
        if u < indel:
            out.append(int(rng.integers(0, 4)))
        out.append(int((b + rng.integers(1, 4)) % 4) if rng.random() < div else int(b))
    return np.array(out, np.int8)


def make_element(rng, i, T):
    n = 2 * T + i % 2
    x = rng.integers(0, 4, n).astype(np.int8)
    if i in TIES:
        return codes(TIES[i])
    if T < 20:
        return x
    kind = i % 5
    k = int(rng.integers(max(T // 3, 12), T + 1))
    if kind == 0:                                           # a direct repeat that ends at the 3' terminus, with indels
        rep = mutate(rng, x[:k], float(rng.choice([0, 0.05, 0.15])), 0.03)[:T]
        x[n - len(rep):] = rep
    elif kind == 1:                                         # an inverted repeat from both termini, with indels
        rep = mutate(rng, x[:k], float(rng.choice([0, 0.05, 0.15])), 0.03)[:T]
        x[n - len(rep):] = tr.revcomp(rep)
    elif kind == 2:                                         # an inner repeat: begins behind row 40 and, from T = 65 on, crosses row 64
        a0 = min(40, T // 2)
        rep = mutate(rng, x[a0:a0 + max(k // 2, 12)], 0.05, 0.0)[:T - a0]
        to = n - T + int(rng.integers(0, T - len(rep) + 1))
        x[to:to + len(rep)] = rep if i % 2 else tr.revcomp(rep)
    elif kind == 3:                                         # one long gap: more bases than a lane has columns
        g = int(rng.integers(3, 21))
        if k > g + 24:
            cut = int(rng.integers(12, k - g - 12 + 1))
            rep = np.concatenate((x[:cut], x[cut + g:k]))
            x[n - len(rep):] = rep
    if T >= 63:
        for base in (0, n - T):                             # N runs across the edges of a window word (8) and a stream word (32)
            for edge in (8, 32, 56):
                if rng.random() < 0.4:
                    x[base + edge - int(rng.integers(1, 4)):base + edge + int(rng.integers(1, 4))] = 99
    return x


def make_library(seed=7):
    """N_SITES elements back to back, two bases between them.  Site 0 begins at position 0, site 1 four bases in front of the
    library; the last site ends at the last position and the one before it reaches past it; the bounds of a site lie a few
    bases outside its element."""
    rng = np.random.default_rng(seed)
    parts, sites, at = [], [], 0
    for i in range(N_SITES):
        T = LONG_T.get(i, SHORT_T[i % len(SHORT_T)])
        x = make_element(rng, i, T)
        sites.append([at, at + len(x) - 1, at - int(rng.integers(0, 9)), at + len(x) - 1 + int(rng.integers(0, 9))])
        gap = rng.integers(0, 4, 2).astype(np.int8) if i + 1 < N_SITES else np.zeros(0, np.int8)
        parts += [x, gap]
        at += len(x) + len(gap)
    lib = np.concatenate(parts).astype(np.int8)
    low = (rng.random(len(lib)) < 0.1) & (lib < 4)
    lib[low] += 4
    sites[0][2] = 0
    sites[1][0] = sites[1][2] = -4
    sites[N_SITES - 2][1] = sites[N_SITES - 2][3] = len(lib) + 5
    sites[N_SITES - 1][3] = len(lib) - 1
    s = np.array(sites, np.int64).view(TSD_SITE_DTYPE).reshape(-1)
    assert s["lo"][0] == 0 and s["hi"][-1] == len(lib) - 1 and (s["lo"] == s["hi"] + 1).any()
    return lib, s


_cache = {}


def library(form):
    if not _cache:
        lib, sites = make_library()
        # the packed form knows A C G T and N only: lower case is not part of it (its classes are the same)
        plain = np.where((lib >= 4) & (lib <= 7), lib - 4, lib).astype(np.int8)
        starts = [0, int(sites["lo"][20]) + 31, int(sites["lo"][40]) + 3, int(sites["lo"][103]) + 777, int(sites["lo"][110]) + 1]
        _cache.update(byte=(lib, sites, None), packed=(plain, sites, pack_library(plain, starts, [0, 3, 1, 2, 3])))
    return _cache[form]


def expected(form, sel, tp):
    lib, sites, _ = library(form)
    p = dict(tmax=tp.tmax, match=tp.match, mismatch=tp.mismatch, gap=tp.gap, min_score=tp.min_score)
    return [tr.site_records(lib, tuple(int(v) for v in sites[i]), **p) for i in sel]


def as_pairs(got):
    return [(tup(r[0]), tup(r[1])) for r in got]


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


# every count round the tile; the specialisation by the call's longest window: 16 columns a lane (130 sites), 4 (the first 65:
# T up to 129), 8 (the first 100: T up to 257), 2 and 1 through tmax; every parameter at both ends of its range
SHAPES = [
    ("byte", 130, TermParams()),
    ("packed", 130, TermParams(tmax=1024, min_score=20)),
    ("byte", 1, TermParams(min_score=1)),
    ("packed", 63, TermParams(min_score=1)),
    ("byte", 64, TermParams(tmax=64, min_score=1)),
    ("packed", 65, TermParams(tmax=128, min_score=10)),
    ("byte", 100, TermParams(tmax=1024, min_score=30)),
    ("packed", 100, TermParams(tmax=256, min_score=30)),
    ("byte", 65, TermParams(tmax=1, min_score=1)),
    ("byte", 65, TermParams(match=2, mismatch=1, gap=1, min_score=1)),
    ("packed", 65, TermParams(match=1, mismatch=15, gap=1, min_score=1)),
    ("byte", 65, TermParams(match=15, mismatch=1, gap=31, min_score=1)),
    ("packed", 64, TermParams(match=15, mismatch=15, gap=1, min_score=100)),
    ("byte", 65, TermParams(match=1, mismatch=1, gap=31, min_score=1 << 30, slack=15)),
    ("byte", 63, TermParams(slack=0, min_score=1)),
]


@pytest.mark.parametrize("form,n,tp", SHAPES, ids=lambda v: v if isinstance(v, str) else (str(v) if isinstance(v, int) else
                         "-".join(str(x) for x in (v.tmax, v.match, v.mismatch, v.gap, v.min_score, v.slack))))
def test_records_equal_the_restatement(devices, form, n, tp):
    _, sites, _ = library(form)
    want = expected(form, range(n), tp)
    got = as_pairs(devices[form].term(sites[:n], tp))
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:4]


def test_the_shapes_are_not_empty_ground():
    """The library holds what the cases are about: every window length, records in both orientations, anchored and inner ones,
    alignments with gaps, a gap run of more bases than a lane has columns, and repeats across row 64."""
    _, sites, _ = library("byte")
    n = sites["hi"] + 1 - sites["lo"]
    assert set(np.minimum(n // 2, 1024).tolist()) >= {0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024}
    want = expected("byte", range(100), TermParams(tmax=1024, min_score=30))
    d = [w[0] for w in want if w[0][0] > 0]
    v = [w[1] for w in want if w[1][0] > 0]
    assert len(d) >= 20 and len(v) >= 15
    assert sum(r[1] <= 3 and r[4] >= r[7] - 4 for r in d) >= 5 and sum(r[1] <= 3 and r[3] <= 3 for r in v) >= 5
    assert sum(r[1] > 20 for r in d + v) >= 5                                   # inner repeats
    assert sum(r[1] < 64 <= r[2] for r in d + v) >= 10                          # across row 64
    assert sum(r[6] > r[5] + 2 for r in d + v) >= 10                            # columns that are no matches
    assert any(abs((r[2] - r[1]) - (r[4] - r[3])) > 4 for r in d if r[7] <= 256)    # a gap run longer than C = 4
    ties = expected("byte", sorted(TIES)[:3], TermParams(min_score=1)) + \
        expected("byte", sorted(TIES)[3:], TermParams(match=2, mismatch=1, gap=1, min_score=1))
    assert [t[0] for t in ties] == [(4, 0, 1, 0, 1, 2, 2, 5), (4, 0, 1, 0, 1, 2, 2, 5), (4, 0, 1, 3, 4, 2, 2, 5),
                                    (5, 0, 3, 0, 3, 3, 4, 4), (5, 0, 3, 0, 3, 3, 4, 4), (5, 0, 3, 1, 3, 3, 4, 4)]


def tile_bytes(tmax):
    """The three windows and streams of one tile of 64 sites."""
    return 3 * 64 * (4 * ((tmax + 7) // 8 + 1) + 12 * max((tmax + 31) // 32, 1))


def test_tile_groups_do_not_show(devices):
    _, sites, _ = library("byte")
    tp = TermParams()
    want = expected("byte", range(130), tp)
    old = os.environ.get("RAMX_TERM_BYTES")
    try:
        for budget in (tile_bytes(512), 2 * tile_bytes(512) + 5):                 # three groups of one tile; two groups of 2 + 1
            os.environ["RAMX_TERM_BYTES"] = str(budget)
            got, ms = devices["byte"].term(sites, tp, timing=True)
            assert as_pairs(got) == want
            assert len(ms) == 3 and all(m > 0 for m in ms)
        os.environ["RAMX_TERM_BYTES"] = str(tile_bytes(512) - 1)
        out = np.full(260 * 8, 7, np.int32).view(TERM_DTYPE)
        cp = _lib.TermParams(512, 2, 3, 5, 40, 3)
        assert _lib.lib().ramx_dev_term(devices["byte"]._h, sites.ctypes.data, 130, C.byref(cp), out.ctypes.data, None) == ERR_UNSUPPORTED
        assert (out.view(np.int32) == 7).all()
        # the budget is per call and counts the call's own longest window
        assert as_pairs(devices["byte"].term(sites[:64], tp)) == want[:64]
    finally:
        if old is None:
            os.environ.pop("RAMX_TERM_BYTES", None)
        else:
            os.environ["RAMX_TERM_BYTES"] = old


def test_no_site_and_bad_arguments(devices):
    d = devices["byte"]
    _, sites, _ = library("byte")
    assert len(d.term(sites[:0])) == 0
    L, good = _lib.lib(), (512, 2, 3, 5, 40, 3)
    ok = _lib.TermParams(*good)
    out = np.full(8 * 8, 7, np.int32).view(TERM_DTYPE)
    for field, values in {0: (0, 1025, -1), 1: (0, 16), 2: (0, 16), 3: (0, 32), 4: (0, -1), 5: (-1, 16)}.items():
        for v in values:
            bad = list(good)
            bad[field] = v
            assert L.ramx_dev_term(d._h, sites.ctypes.data, 4, C.byref(_lib.TermParams(*bad)), out.ctypes.data, None) == ERR_ARG, bad
    assert L.ramx_dev_term(d._h, sites.ctypes.data, 4, C.byref(_lib.TermParams(*good, (C.c_int32 * 2)(0, 1))), out.ctypes.data, None) == ERR_ARG
    assert L.ramx_dev_term(d._h, sites.ctypes.data, 4, None, out.ctypes.data, None) == ERR_ARG
    assert L.ramx_dev_term(d._h, sites.ctypes.data, -1, C.byref(ok), out.ctypes.data, None) == ERR_ARG
    assert L.ramx_dev_term(d._h, None, 4, C.byref(ok), out.ctypes.data, None) == ERR_ARG
    assert L.ramx_dev_term(d._h, sites.ctypes.data, 4, C.byref(ok), None, None) == ERR_ARG
    assert L.ramx_dev_term(None, sites.ctypes.data, 4, C.byref(ok), out.ctypes.data, None) == ERR_ARG
    for field, value in (("lo", lambda s: s["hi"] + 2), ("seq_lo", lambda s: s["lo"] + 1), ("seq_hi", lambda s: s["hi"] - 1)):
        s = sites[:4].copy()
        s[field][2] = value(s[2])
        assert L.ramx_dev_term(d._h, s.ctypes.data, 4, C.byref(ok), out.ctypes.data, None) == ERR_ARG, field
    # raised before anything is written
    assert (out.view(np.int32) == 7).all()
    assert L.ramx_dev_term(d._h, sites.ctypes.data, 0, C.byref(ok), None, None) == 0


def test_a_direction_needs_a_new_begin_after_a_term_call():
    from repeatafterme_amd.device import Device, resolve_flanks
    e = tr.planted_expectation("TIR")
    p = to_extend_params(e["p"])
    d = Device(0)
    try:
        d.load_library(np.ascontiguousarray(e["seq"]))
        flanks, _ = resolve_flanks(1, e["cores"], p.bandwidth, p.L)
        d.begin_direction(flanks, p)
        got = d.term(np.array(e["sites"], np.int64).view(TSD_SITE_DTYPE).reshape(-1))
        assert as_pairs(got) == e["records"]
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


@pytest.mark.parametrize("kind,verdict", [("TIR", 2), ("LTR", 1)])
def test_term_flat_on_the_planted_families(kind, verdict):
    """Two extend_alignment calls, then ramx_term_flat on the library they left on the device: the CPU expectation (the loop is
    bit-exact against the oracle, so the sites are the same)."""
    from repeatafterme_amd.extend import term_flat, term_summary
    e = tr.planted_expectation(kind)
    c, m, rets = gpu_both_directions(e["cores"], e["seq"], e["p"])
    assert rets == e["rets"] and np.array_equal(c.left_len, e["after"].left_len) and np.array_equal(c.right_len, e["after"].right_len)
    got = term_flat(c, e["seq"])
    assert as_pairs(got) == e["records"]
    s = term_summary(got)
    assert s.verdict == verdict == e["summary"]["verdict"]
    assert (s.direct_median, s.inverted_median) == (e["summary"]["direct_median"], e["summary"]["inverted_median"])
    # on a library the device does not hold (a copy at another address): uploaded, the same records
    assert as_pairs(term_flat(c, e["seq"].copy())) == e["records"]
    assert term_flat(c.subset(slice(0, 0)), e["seq"]).shape == (0, 2)
    # other parameters through the same call
    tp = TermParams(tmax=100, match=1, mismatch=2, gap=3, min_score=15)
    assert as_pairs(term_flat(c, e["seq"], tp)) == [tr.site_records(e["seq"], s_, tmax=100, match=1, mismatch=2, gap=3, min_score=15)
                                                    for s_ in e["sites"]]


def test_term_alignment_on_the_list():
    """The same through the reference's data model: a linked list of cores and a sequence library."""
    from repeatafterme_amd.extend import term_alignment
    from repeatafterme_amd.loader import _Core, _SeqLib
    e = tr.planted_expectation("LTR")
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
    assert as_pairs(term_alignment(arr, C.pointer(sl), n)) == e["records"]


def test_term_batch_with_an_empty_family_between():
    from repeatafterme_amd.extend import extend_batch, term_batch, term_summary
    tir, ltr = tr.planted_expectation("TIR"), tr.planted_expectation("LTR")
    p = tir["p"]
    empty = (CoreSet(left_pos=[], right_pos=[], lower=[], upper=[], orient=[], left_ext=[], right_ext=[]),
             np.random.default_rng(5).integers(0, 4, 333).astype(np.int8))
    fams = [(tir["cores"], tir["seq"]), empty, (ltr["cores"], ltr["seq"])]
    batch = [(c.copy(), s, new_master(p.L)) for c, s in fams]
    for d in (1, 0):
        extend_batch(d, batch, to_extend_params(p))
    got = term_batch(batch)
    assert [g.shape for g in got] == [(tir["cores"].n, 2), (0, 2), (ltr["cores"].n, 2)]
    for e, (c, _, m), g, verdict in ((tir, batch[0], got[0], 2), (ltr, batch[2], got[2], 1)):
        assert np.array_equal(c.left_len, e["after"].left_len) and np.array_equal(c.right_len, e["after"].right_len)
        assert as_pairs(g) == e["records"]
        assert term_summary(g).verdict == verdict
    # once more on copies of the libraries: the concatenation is built and sent again, the records are the same
    again = term_batch([(c, s.copy(), m) for c, s, m in batch])
    assert all(a.tobytes() == g.tobytes() for a, g in zip(again, got))


def border_families(reach=False):
    """Three families of four copies each, the extension lengths set by hand.  Copy 0 begins at base 0 of its library with 30
    bases that it ends with again (a direct repeat); copy 3 ends at the library's last base with the reverse complement of its
    first 30; copies 1 and 2 (one on the reverse strand) lie in the middle, with a direct and an inverted repeat; half the
    copies have bounds wider than their library.  Every library but the last holds, 50 bases in front of its end, the first 30
    bases of the next one.  With reach, the first two families have a fifth copy that begins there and ends 30 bases behind the
    library: read across the border it would end with the 30 bases it begins with.  -> [(cores, sequence)]"""
    rng = np.random.default_rng(47)
    seqs = [rng.integers(0, 4, 400).astype(np.int8) for _ in range(3)]
    fams = []
    for f, seq in enumerate(seqs):
        n = len(seq)
        ext = [(0, 79, 0), (100, 189, 0), (200, 299, 1), (n - 90, n - 1, 0)]
        for i, (lo, hi, _) in enumerate(ext):
            seq[hi - 29:hi + 1] = seq[lo:lo + 30] if i < 2 else tr.revcomp(seq[lo:lo + 30])
        if f < 2:
            seq[n - 50:n - 20] = seqs[f + 1][:30]             # (written after copy 3's repeat, of which it keeps the last 20 bases)
            if reach:
                ext.append((n - 50, n + 29, 0))
        m = len(ext)
        lp = [lo + (44 if minus else 40) for lo, hi, minus in ext]
        rp = [lo + (40 if minus else 44) for lo, hi, minus in ext]
        ll = [hi - lo - 44 if minus else 40 for lo, hi, minus in ext]
        rl = [40 if minus else hi - lo - 44 for lo, hi, minus in ext]
        cores = CoreSet(left_pos=lp, right_pos=rp, lower=([-50, 0, -50, 0, 0])[:m], upper=([n - 1, n + 50, n - 1, n + 50, n + 50])[:m],
                        orient=[e[2] for e in ext], left_ext=[1] * m, right_ext=[1] * m, left_len=ll, right_len=rl)
        assert [s[:2] for s in tr.sites_of(cores)] == [e[:2] for e in ext]
        fams.append((cores, seq))
    return fams


def test_a_batch_never_reads_across_a_familys_border():
    """ramx_term_batch on the concatenated library: every family's records are those of the family alone.  The windows of a site
    lie inside it and a site lies inside its bounds, which the batch cuts to the family's own library: so a copy that reaches
    behind its library -- where the neighbour's bases would complete a repeat -- is refused, not read."""
    from repeatafterme_amd.extend import term_batch
    fams = border_families()
    got = term_batch([(c, s, None) for c, s in fams])
    alone = [[tr.site_records(s, site) for site in tr.sites_of(c)] for c, s in fams]
    assert [as_pairs(g) for g in got] == alone
    # not empty ground: the planted repeats are found in their orientation ...
    for f, al in enumerate(alone):
        assert al[0][0][0] >= 40 and al[1][0][0] >= 40 and al[2][1][0] >= 40, (f, al)
        assert al[3][1][0] >= (40 if f == 2 else 0)
    # ... and the reaching copy, read on the concatenation with its whole length for bounds, has the repeat the neighbour completes
    reach = border_families(reach=True)
    cat = np.concatenate([s for _, s in reach])
    at = np.cumsum([0] + [len(s) for _, s in reach])
    for f in range(2):
        c, s = reach[f]
        lo, hi = tr.sites_of(c)[4][:2]
        assert tr.site_records(s, (lo, hi, 0, hi)) == ((0, 0, 0, 0, 0, 0, 0, 40),) * 2
        assert tr.site_records(cat, (lo + int(at[f]), hi + int(at[f]), 0, len(cat) - 1))[0] == (60, 0, 29, 10, 39, 30, 30, 40)
    with pytest.raises(_lib.RamxError, match=r"\(-103\)"):
        term_batch([(c, s, None) for c, s in reach])
