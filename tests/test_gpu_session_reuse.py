"""Every device call on a session whose buffers hold an earlier, larger call.  A Device keeps its buffers between calls and
reallocates only to grow (ensure() in csrc/ramx_device.hip), and most of them are deliberately not cleared: a kernel that reads
one tile, row, window word or stream word too far, a sum kernel that strides by the earlier call's rows, a host copy that fetches
the earlier call's extent would return the earlier family's numbers -- plausible, in range, and invisible on a buffer that was
just allocated.  Here every entry point runs on BIG first and then on SMALL (tests/session_cases.py; tests/test_session_cases.py
vouches for the two on the CPU), and SMALL's answer is compared with the CPU restatements: the oracle, align_ref, pileup_ref,
dinuc_ref, copystats_ref, linkage_ref, subfam_ref, tsd_ref, period_ref, term_ref, window_ref.  Everything is exact.  Where the
contract says "not written" the caller's sentinel must be intact, where it says "reads as 0" it must be 0; the same call on a
fresh Device is a second, byte-for-byte comparison (it covers the padding lanes, whose content no contract words).

That these tests can fail was shown once on two scratch builds of the library (tools/build_variant.sh; nothing of them is kept).
Without the two clears of d_pf_best / d_pf_bidx in ramx_dev_profile, test_profile_small_after_big failed on both paths at "rows
beyond a family's count read as 0": rows 17..27 of the 3-flank family's tile held BIG's row_best (-19, -47, ... 75, 52).  Without
the clear of d_lk_planes in ramx_dev_planes, test_small_after_big[planes] failed at "words of every plane": the planes of the
70-flank family's last rows, which no copy reaches and the planes' kernel therefore never writes, held BIG's words
(17590021652223, 144115188080058368, ...) where the restatement has 0.  Both buffers hold results that are only downloaded or
popcounted; nothing on the device reads them as an index, an address or a control word."""
import functools
import subprocess

import numpy as np
import pytest

from repeatafterme_amd import _lib
from repeatafterme_amd.datamodel import (ALN_NONE, COL_PROFILE_DTYPE, COPY_STATS_DTYPE, PeriodParams, TermParams, TsdParams,
                                         new_master)

import linkage_ref as lr
import session_cases as sc
import subfam_ref as sr
import window_ref as wr
from helpers import to_extend_params
from test_gpu_align import check_against_walker
from test_gpu_pileup import same_ends, same_pileup
from test_gpu_replay_corners import all_none, same_bytes, sentinel_alignment
from test_gpu_subfam import same as same_subfam

pytestmark = pytest.mark.gpu

SENTINEL = 0x5a
ROUTE_VARS = ("RAMX_NO_FAMILY_ROUTE", "RAMX_NO_CP_DEVICE", "RAMX_NO_CP", "RAMX_NO_PK", "RAMX_NO_PERSISTENT", "RAMX_FORCE_CHAIN", "RAMX_CP_K",
              "RAMX_CP_DEVICE_MAXN", "RAMX_PK_SEGMENT", "RAMX_PROFILE_NO_RESIDENT", "RAMX_ALIGN_BYTES", "RAMX_TERM_BYTES", "RAMX_PERIOD_BYTES",
              "RAMX_LINKAGE_BYTES")
REPLAYS = ("profile", "align", "pileup", "refine", "dinuc", "refine_cpg", "copy_stats", "copy_stats_reversed", "planes")
SITES = ("tsd", "period", "term")
ENTRIES = REPLAYS + SITES


@pytest.fixture(autouse=True)
def _plain_environment(monkeypatch):
    for k in ROUTE_VARS:
        monkeypatch.delenv(k, raising=False)


def device(world):
    from repeatafterme_amd.device import Device
    d = Device(0)
    d.load_library(world.lib if hasattr(world, "lib") else world.seq)
    return d


def filled(shape, dtype):
    a = np.zeros(shape, dtype)
    a.view(np.uint8)[:] = SENTINEL
    return a


def untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------- the calls

def call_big(d, name):
    """One entry point on BIG; no more is asserted than that it answered (its correctness is other tests' business)."""
    b = sc.big()
    flanks, first, count = sc.big_layout()
    ep = to_extend_params(b.p)
    kw = dict(rows=b.rows, fam_first=first, fam_count=count)
    if name == "profile":
        res = d.profile(flanks, ep, b.cons, row_best=True, **kw)
        assert res.cols["total"][0, :b.rows[0]].any() and res.row_best[b.rows[0] - 1, :sc.BIG_N].any() and res.row_best_idx.any()
        assert (res.last_uncapped_row[:sc.BIG_N] >= 0).any()
    elif name == "align":
        res = d.align(flanks, ep, b.cons, **kw)
        assert (res.ends["end_row"][:sc.BIG_N] > 256).any() and (res.col_idx[257, :sc.BIG_N] != ALN_NONE).any() and res.col_ins.any()
    elif name == "pileup":
        res = d.pileup(flanks, ep, b.cons, **kw)
        assert res.cols["cover"][0, 257:b.rows[0]].any() and res.cols["cover"][3, :40].any()
    elif name == "refine":
        res = d.refine(flanks, ep, b.cons, max_replays=2, **kw)
        assert res.rows[0] > 256 and res.cols["cover"][0].any()
    elif name == "dinuc":
        res = d.dinuc(flanks, ep, b.cons, **kw)
        assert res.di["adjacent"][0, 257:b.rows[0] - 1].any() and res.cols["cover"][0].any()
    elif name == "refine_cpg":
        res = d.refine_cpg(flanks, ep, b.cons, max_replays=2, **kw)
        assert res.rows[0] > 256 and res.di["adjacent"][0].any()
    elif name in ("copy_stats", "copy_stats_reversed"):
        res = d.copy_stats(flanks, ep, b.cons, rows_reversed=name.endswith("reversed"), **kw)
        assert (res.stats["cols"][:sc.BIG_N] > 256).any() and res.stats["match"][first[3]:first[3] + 5].any()
    elif name == "planes":
        res = d.planes(flanks, ep, b.cons, **kw)
        cos, bits = d.plane_gram(b.planes, bits=True)
        assert cos[0].shape == (len(b.planes[0]),) * 2 and cos[0].any() and bits[0].shape[1] == 5 and bits[0][:, 4].any()
        # patterns of one variant each, the three most frequent ones by the Gram's diagonal: every group finds copies
        inits = []
        for f, x in enumerate(b.planes):
            var = sr.variants_of(x)[0]
            init = np.zeros((len(var), 4), np.uint8)
            for k, v in enumerate(np.argsort(-np.diag(cos[f])[var], kind="stable")[:3]):
                init[v, k + 1] = 1
            inits.append(init)
        sub = d.subfamilies(b.planes, inits, masks=True)
        assert sub[0].size.sum() == sc.BIG_N and (sub[0].size > 0).sum() >= 2 and sub[0].masks[:, 4].any()
    elif name == "tsd":
        res = d.tsd(b.sites)
        assert len(res) == 130 and (res["k"] > 0).any()
    elif name == "period":
        res = d.period(b.segs)
        assert len(res) == 130 and (res["period"] > 0).sum() >= 5
    elif name == "term":
        res = d.term(b.sites, TermParams(tmax=1024, min_score=30))
        assert res.shape == (130, 2) and (res["T"] == 1024).any() and (res["score"] > 0).sum() >= 20
    else:
        raise KeyError(name)


def call_small(d, name):
    """One entry point on SMALL, into sentinel-filled arrays where the Device takes them -> whatever it returns."""
    s = sc.small()
    flanks, first, count = sc.small_layout()
    ep = to_extend_params(s.p)
    kw = dict(rows=s.rows, fam_first=first, fam_count=count)
    if name == "profile":
        return d.profile(flanks, ep, s.cons, row_best=True, out=filled((3, sc.SMALL_L), COL_PROFILE_DTYPE), **kw)
    if name == "align":
        return d.align(flanks, ep, s.cons, out=sentinel_alignment(max(s.rows), s.n_padded), **kw)
    if name == "pileup":
        return d.pileup(flanks, ep, s.cons, **kw)
    if name == "refine":
        return d.refine(flanks, ep, s.cons, max_replays=3, **kw)
    if name == "dinuc":
        return d.dinuc(flanks, ep, s.cons, **kw)
    if name == "refine_cpg":
        return d.refine_cpg(flanks, ep, s.cons, max_replays=3, **kw)
    if name in ("copy_stats", "copy_stats_reversed"):
        return d.copy_stats(flanks, ep, s.cons, rows_reversed=name.endswith("reversed"), out=filled(s.n_padded, COPY_STATS_DTYPE), **kw)
    if name == "planes":
        return small_planes(d)
    if name == "tsd":
        return d.tsd(s.sites, TsdParams(**sc.TSD))
    if name == "period":
        return d.period(s.segs, PeriodParams(**sc.PERIOD))
    if name == "term":
        return d.term(s.sites, TermParams(**sc.TERM))
    raise KeyError(name)


def small_lists():
    t = sc.small_truth()
    inits = [np.zeros((0, sc.SUBFAM_K), np.uint8) if x is None else x for x in t["init"]]
    return t["planes"], inits


def every_plane():
    """All eight planes of every row of every family that has flanks and rows"""
    s = sc.small()
    return [lr.all_planes(s.rows[f]) if s.fams[f] is not None else lr.as_planes([]) for f in range(3)]


def small_planes(d, replay=True):
    """planes, then plane_gram, then subfamilies with the masks, then plane_gram over every plane there is
    -> (planes' result, Gram matrices, words, splits, all labels, (Gram matrices, words) of every plane)"""
    s = sc.small()
    flanks, first, count = sc.small_layout()
    lists, inits = small_lists()
    res = d.planes(flanks, to_extend_params(s.p), s.cons, rows=s.rows, fam_first=first, fam_count=count) if replay else None
    cos, bits = d.plane_gram(lists, bits=True)
    sub = d.subfamilies(lists, inits, masks=True, K=sc.SUBFAM_K)
    labels = d._subfam_labels.copy()
    every = d.plane_gram(every_plane(), bits=True)          # rows no copy reaches included: the planes' kernel never writes them
    return res, cos, bits, sub, labels, every


@functools.lru_cache(maxsize=None)
def fresh(name):
    """The SMALL call on a Device that has run nothing else."""
    d = device(sc.small())
    try:
        return call_small(d, name)
    finally:
        d.close()


# ---------------------------------------------------------------------------------------------------- the comparisons

def families_with_rows():
    s = sc.small()
    _, first, count = sc.small_layout()
    return [(f, first[f], count[f], s.rows[f]) for f in range(3) if count[f] and s.rows[f]]


def inside_a_family():
    """bool [n_padded]: the lanes of the tiles that belong to a family"""
    s = sc.small()
    _, first, count = sc.small_layout()
    m = np.zeros(s.n_padded, bool)
    for f in range(3):
        m[first[f]:first[f] + (count[f] + 63) // 64 * 64] = True
    assert (~m).sum() == 64 and not m[64 * s.hole_tile]
    return m


def check_ends(ends, tag, hole):
    """The flanks' records against the walker's, -1 on the padding lanes of a family's tiles; the tile of no family holds what
    the caller put there (`hole`: a predicate on those 64 records)."""
    t = sc.small_truth()
    for f, at, n, rows in families_with_rows():
        same_ends(ends[at:at + n], t["walks"][f][1], f"{tag}: family {f}")
        assert (ends["end_row"][at + n:at + (n + 63) // 64 * 64] == -1).all(), f"{tag}: padding lanes of family {f}"
    assert hole(ends[~inside_a_family()]), f"{tag}: the tile of no family"


def check_pileup_cols(cols, tag, truth="cols"):
    s, t = sc.small(), sc.small_truth()
    for f in range(3):
        rows = s.rows[f]
        if t[truth][f] is not None:
            same_pileup(cols[f, :rows], t[truth][f], f"{tag}: family {f}")
        assert not cols[f, rows:].view(np.uint8).any(), f"{tag}: family {f}: entries beyond its rows"


def check(name, got, also_fresh=True):
    s, t = sc.small(), sc.small_truth()
    hole = ~inside_a_family()
    maxrows = max(s.rows)
    if name == "profile":
        for f, at, n, rows in families_with_rows():
            total, counts, best, bidx, last = t["profile"][f]
            c = got.cols[f, :rows]
            assert np.array_equal(c["total"], total) and np.array_equal(c["base"], s.cons[f, :rows]), (name, f)
            for k, j in (("n_capped", 0), ("n_new_high", 1), ("n_out_of_seq", 2)):
                assert np.array_equal(c[k], counts[:, j]), (name, f, k)
            assert np.array_equal(got.row_best[:rows, at:at + n], best) and np.array_equal(got.row_best_idx[:rows, at:at + n], bidx), (name, f)
            assert np.array_equal(got.last_uncapped_row[at:at + n], last), (name, f)
            assert (got.last_uncapped_row[at + n:at + (n + 63) // 64 * 64] == -1).all(), (name, f)
            # rows beyond a family's count are never written: they read as 0
            tile = slice(at, at + (n + 63) // 64 * 64)
            assert not got.row_best[rows:, tile].any() and not got.row_best_idx[rows:, tile].any(), (name, f)
        for f in range(3):
            assert untouched(got.cols[f, s.rows[f]:]), (name, f)                       # entries beyond rows[f] are left alone
        assert got.row_best.shape == (maxrows, s.n_padded)
        assert not got.row_best[:, hole].any() and not got.row_best_idx[:, hole].any()      # a tile outside every family reads as 0
        assert (got.last_uncapped_row[hole] == -1).all()
    elif name == "align":
        for f, at, n, rows in families_with_rows():
            check_against_walker(got.ends[at:at + n], got.col_idx[:, at:at + n], got.col_ins[:, at:at + n], t["walks"][f][1], rows, f"family {f}")
            tile = slice(at, at + (n + 63) // 64 * 64)
            assert (got.col_idx[rows:, tile] == ALN_NONE).all() and not got.col_ins[rows:, tile].any(), (name, f)
            pad = slice(at + n, tile.stop)
            assert (got.col_idx[:, pad] == ALN_NONE).all() and not got.col_ins[:, pad].any(), (name, f)
        check_ends(got.ends, name, untouched)
        keep = sentinel_alignment(maxrows, s.n_padded)
        assert np.array_equal(got.col_idx[:, hole], keep.col_idx[:, hole]) and np.array_equal(got.col_ins[:, hole], keep.col_ins[:, hole])
    elif name == "pileup":
        check_pileup_cols(got.cols, name)
        check_ends(got.ends, name, all_none)
    elif name in ("refine", "refine_cpg"):
        for f, at, n, rows in families_with_rows():
            want = t[name][f]
            cons, cols, replays, conv = want[0], want[1], want[-3 if name == "refine_cpg" else -2], want[-2 if name == "refine_cpg" else -1]
            assert int(got.rows[f]) == len(cons) and np.array_equal(got.cons[f, :len(cons)], cons), (name, f)
            assert (int(got.replays[f]), int(got.converged[f])) == (replays, conv), (name, f)
            same_pileup(got.cols[f, :len(cons)], cols, f"{name}: family {f}")
            # (entries beyond the result's rows hold what an earlier, longer replay of the same call wrote there: no contract
            # words them, the comparison with the fresh Device covers them)
            assert not got.cons[f, len(cons):].any(), (name, f)
            if name == "refine_cpg":
                assert int(got.n_cpg[f]) == want[5] and np.array_equal(got.di[f, :len(cons)], want[2]), (name, f)
        assert int(got.rows[1]) == 0 and not got.cols[1].view(np.uint8).any()
        assert all_none(got.ends[hole])
    elif name == "dinuc":
        check_pileup_cols(got.cols, name)
        for f in range(3):
            rows = s.rows[f]
            if t["di"][f] is not None:
                assert np.array_equal(got.di[f, :rows], t["di"][f]), (name, f, np.flatnonzero(got.di[f, :rows] != t["di"][f])[:8])
            assert not got.di[f, rows:].view(np.uint8).any(), (name, f)
        check_ends(got.ends, name, all_none)
    elif name in ("copy_stats", "copy_stats_reversed"):
        key = "stats_reversed" if name.endswith("reversed") else "stats"
        for f, at, n, rows in families_with_rows():
            assert np.array_equal(got.stats[at:at + n], t[key][f]), (name, f, np.flatnonzero(got.stats[at:at + n] != t[key][f])[:8])
            assert not got.stats[at + n:at + (n + 63) // 64 * 64].view(np.uint8).any(), (name, f)     # padding lanes: no alignment, no count
        assert untouched(got.stats[hole])                                              # records of tiles outside every family are left alone
        check_ends(got.ends, name, all_none)
    elif name == "planes":
        res, cos, bits, sub, labels, (all_cos, all_bits) = got
        for f, planes in enumerate(every_plane()):
            if len(planes):
                assert np.array_equal(all_bits[f], lr.words(t["pl"][f], planes, sc.small_layout()[2][f])), (name, f, "words of every plane")
                assert np.array_equal(all_cos[f], lr.gram(t["pl"][f], planes)), (name, f, "Gram of every plane")
        lists, inits = small_lists()
        if res is not None:
            check_pileup_cols(res.cols, name)
            check_ends(res.ends, name, all_none)
        _, first, count = sc.small_layout()
        for f in range(3):
            if t["pl"][f] is None:
                e = sub[f]
                assert cos[f].shape == (0, 0) and len(e.labels) == 0 and e.masks.shape == (sc.SUBFAM_K, 0) and not e.size.any()
                assert (e.iterations, e.converged) == (1, 1)
                continue
            n = count[f]
            assert np.array_equal(cos[f], t["gram"][f]), (name, f, np.argwhere(cos[f] != t["gram"][f])[:8])
            assert np.array_equal(bits[f], lr.words(t["pl"][f], lists[f], n)), (name, f)
            same_subfam(sub[f], t["subfam"][f], f"{name}: family {f}")
        inside = np.zeros(s.n_padded, bool)
        for f in range(3):
            inside[first[f]:first[f] + count[f]] = True
        assert (labels[~inside] == -1).all() and (labels[inside] >= 0).all()
    elif name == "tsd":
        assert [tuple(int(r[k]) for k in ("k", "mm", "dl", "dr")) for r in got] == t["tsd"]
    elif name == "period":
        assert [tuple(int(r[k]) for k in ("period", "score", "start", "end", "agree", "disagree")) for r in got] == t["period"]
        assert not got["reserved"].any()
    elif name == "term":
        assert [tuple(tuple(int(r[j][k]) for k in ("score", "a_start", "a_end", "b_start", "b_end", "matches", "columns", "T")) for j in (0, 1))
                for r in got] == t["term"]
    else:
        raise KeyError(name)
    if also_fresh:
        assert_same_result(got, fresh(name), name)


def assert_same_result(a, b, where):
    """Two results of one call, every array byte for byte (times apart)."""
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            assert_same_result(x, y, f"{where}[{i}]")
    elif isinstance(a, np.ndarray):
        assert same_bytes(np.ascontiguousarray(a), np.ascontiguousarray(b)), where
    elif hasattr(a, "__dataclass_fields__"):
        for k in a.__dataclass_fields__:
            if not k.endswith("_ms"):
                assert_same_result(getattr(a, k), getattr(b, k), f"{where}.{k}")
    elif a is None or isinstance(a, (int, np.integer)):
        assert a == b, (where, a, b)


# ---------------------------------------------------------------------------------------------------- a. small after big

@pytest.mark.parametrize("name", [e for e in ENTRIES if e != "profile"])
def test_small_after_big(name):
    d = device(sc.big())
    try:
        call_big(d, name)
        d.load_library(sc.small().lib)
        got = call_small(d, name)
    finally:
        d.close()
    check(name, got)


@pytest.mark.parametrize("path", ["resident", "row_buffer"])
def test_profile_small_after_big(path, monkeypatch):
    """BIG's replay (W = 40) with the rows on chip and through the global row buffer, the way tests/test_gpu_profile.py chooses
    between them; SMALL's band width (5) has no on-chip instantiation, so its rows go through the row buffer that BIG's second
    path has filled."""
    if path == "row_buffer":
        monkeypatch.setenv("RAMX_PROFILE_NO_RESIDENT", "1")
    d = device(sc.big())
    try:
        call_big(d, "profile")
        d.load_library(sc.small().lib)
        got = call_small(d, "profile")
    finally:
        d.close()
    check("profile", got)


def test_packed_windows_small_after_big():
    """The flank windows in d_bases: BIG's pack leaves words behind what SMALL's pack writes (59 words of 576 lanes against 17 of
    256 in one buffer); SMALL's own words and bounds are the restatement's, pad lanes and the tile of no family included."""
    b, s = sc.big(), sc.small()
    flanks, first, count = sc.big_layout()
    d = device(b)
    try:
        d.align(flanks, to_extend_params(b.p), b.cons, rows=b.rows, fam_first=first, fam_count=count, columns=False)
        big_words, _ = d.peek_windows()
        d.load_library(s.lib)
        call_small(d, "align")
        words, bounds = d.peek_windows()
    finally:
        d.close()
    want_words, want_bounds = sc.small_windows()
    assert big_words.shape == (wr.window_words(sc.BIG_L, sc.BIG_W), b.n_padded) and words.shape == want_words.shape
    assert big_words.size > words.size and (big_words.reshape(-1)[words.size:] != 0).all()       # the dirt behind SMALL's extent
    assert not np.array_equal(big_words.reshape(-1)[:words.size], want_words.reshape(-1))
    descs = wr.descriptors(sc.small_layout()[0])
    assert not wr.first_difference(words, want_words, descs), wr.first_difference(words, want_words, descs)
    assert np.array_equal(bounds, want_bounds)


# ---------------------------------------------------------------------------------------------------- b. cross-dirtying

BIG_ORDER = ("profile", "align", "pileup", "refine", "dinuc", "refine_cpg", "copy_stats", "planes", "tsd", "period", "term")
# each SMALL call behind another kind of call: term after period after tsd, copy_stats after dinuc, profile after align, ...
SMALL_ORDER = ("tsd", "period", "term", "align", "profile", "dinuc", "copy_stats", "refine", "planes", "pileup", "refine_cpg",
               "copy_stats_reversed", "term", "pileup", "tsd")


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_calls_dirty_each_others_buffers(order):
    """The replays share d_flanks, d_bases, d_rp_*, d_al_codes, d_pl_idx and d_pl_ins, the site-window calls the direction's flank
    and window buffers and the period's streams: all BIG calls in a fixed order, then all SMALL calls, each behind a call of
    another kind."""
    d = device(sc.big())
    got = []
    try:
        for name in BIG_ORDER:
            call_big(d, name)
        d.load_library(sc.small().lib)
        for name in (SMALL_ORDER if order == "forward" else SMALL_ORDER[::-1]):
            got.append((name, call_small(d, name)))
    finally:
        d.close()
    for name, res in got:
        check(name, res)


# ---------------------------------------------------------------------------------------------------- c. resident state

def test_resident_planes_and_foreign_calls():
    """The planes stay resident until the next replay or site-window call on the device (include/ramx.h): they serve any number
    of plane_gram and subfamilies calls, in any order, and after a foreign call -- a BIG pileup, a BIG term -- the device
    refuses with RAMX_ERR_STATE where it could only answer from buffers that call has reused.  planes(SMALL) again: the
    restatement's answer, whatever ran in between."""
    b, s = sc.big(), sc.small()
    big_flanks, big_first, big_count = sc.big_layout()
    lists, inits = small_lists()
    d = device(s)
    try:
        first_answer = small_planes(d)
        again = small_planes(d, replay=False)                      # Gram and split once more on the same resident planes
        sub_first = d.subfamilies(lists, inits, masks=True, K=sc.SUBFAM_K)
        cos_after = d.plane_gram(lists)
        for foreign in ("pileup", "term"):
            d.load_library(b.lib)
            if foreign == "pileup":
                d.pileup(big_flanks, to_extend_params(b.p), b.cons, rows=b.rows, fam_first=big_first, fam_count=big_count)
            else:
                d.term(b.sites, TermParams(tmax=1024))
            for refused in (lambda: d.plane_gram(lists), lambda: d.subfamilies(lists, inits, K=sc.SUBFAM_K)):
                with pytest.raises(_lib.RamxError, match=r"\(-104\)"):
                    refused()
            d.load_library(s.lib)
            after = small_planes(d)
            check("planes", after, also_fresh=False)
            assert_same_result(after, first_answer, f"planes after a BIG {foreign}")
    finally:
        d.close()
    check("planes", first_answer)
    assert_same_result(again[1:], first_answer[1:], "the second Gram and split")
    assert_same_result(sub_first, first_answer[3], "subfamilies before plane_gram")
    assert_same_result(list(cos_after), list(first_answer[1]), "plane_gram after subfamilies")


def test_planes_of_small_replace_the_planes_of_big():
    """planes(BIG), then planes(SMALL): plane_gram answers for SMALL alone, and a plane of BIG's extent -- a row SMALL does not
    have, BIG's number of families -- is refused as the header says."""
    b, s = sc.big(), sc.small()
    d = device(b)
    try:
        call_big(d, "planes")
        d.load_library(s.lib)
        got = small_planes(d)
        lists, _ = small_lists()
        beyond = lr.as_planes([(s.rows[0] - 1, 6), (s.rows[0], 6)])                  # the second row exists in BIG's replay only
        with pytest.raises(_lib.RamxError, match=r"\(-103\).*outside the resident replay \(28 rows"):
            d.plane_gram([beyond, lists[1], lists[2]])
        with pytest.raises(_lib.RamxError, match=r"\(-103\).*outside the resident replay \(0 rows"):
            d.plane_gram([lists[0], lr.as_planes([(0, 6)]), lists[2]])               # BIG's family 1 had 40 rows, SMALL's has none
        with pytest.raises(_lib.RamxError, match=r"\(-103\).*4 families, the resident replay has 3"):
            d.plane_gram(b.planes)
        cos = d.plane_gram(lists)                                                    # a refused list leaves the planes resident
    finally:
        d.close()
    check("planes", got)
    assert_same_result(list(cos), list(got[1]), "after the refusals")


# ---------------------------------------------------------------------------------------------------- d. the loop

# what moves a whole-set direction from one kernel route to another (tests/test_gpu_direction_routes.py): the run info's
# (persistent, packed_rows > 0, lanes_per_flank > 1) says which one ran
ROUTES = {"streaming": ({"RAMX_NO_PERSISTENT": "1"}, (0, False, False)),
          "packed_rows": ({"RAMX_NO_CP_DEVICE": "1"}, (1, True, False)),
          "cell_parallel": ({}, (1, False, True))}


def set_route(monkeypatch, env):
    for k in ROUTE_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def run_direction(d, w):
    """One right direction on an open device -> (info, consensus, lengths, scores, the final DP rows of flank 0 and of the last
    flank, the one beside the padding lanes of its tile: peek_state refuses a lane that holds no flank)."""
    from repeatafterme_amd.device import resolve_flanks
    flanks, idx = resolve_flanks(1, w.cores, w.p.bandwidth, w.p.L)
    assert len(idx) == w.cores.n
    d.begin_direction(flanks, to_extend_params(w.p))
    info = d.run_direction()
    cons, th, tp = d.download()
    ext = (th > 0) & (tp >= 0)
    return info, cons, np.where(ext, tp + 1, 0), np.where(ext, th, 0), [d.peek_state(i) for i in (0, w.cores.n - 1)]


def assert_direction_is_the_oracles(got, w, tag):
    info, cons, lengths, scores, _ = got
    o = w.o
    assert (info.ret, info.rows_executed) == (o.ret, o.rows_executed), (tag, info.ret, info.rows_executed, o.ret, o.rows_executed)
    assert np.array_equal(cons, o.col_base[:o.rows_executed]), f"{tag}: consensus"
    assert np.array_equal(lengths, o.right_len) and np.array_equal(scores, o.score), f"{tag}: lengths and scores"


def route_of(info):
    return (info.persistent, info.packed_rows > 0, info.lanes_per_flank > 1)


@pytest.mark.parametrize("route,other", [("streaming", "cell_parallel"), ("packed_rows", "streaming"), ("cell_parallel", "packed_rows")])
def test_a_small_direction_after_a_big_one(route, other, monkeypatch):
    """700 flanks at W = 40, L = 200 on one route, then on the same Device 70 flanks at W = 14, L = 40 on the same route and on
    another: the return value, the executed rows, the consensus, the lengths and the scores are the oracle's, and the final DP
    rows of the first and the last flank are those of a Device that has run nothing before."""
    big, small = sc.loop_world("big"), sc.loop_world("small")
    env, want = ROUTES[route]
    set_route(monkeypatch, env)
    d = device(big)
    try:
        got = run_direction(d, big)
        assert route_of(got[0]) == want, (route, route_of(got[0]))
        assert_direction_is_the_oracles(got, big, f"big on {route}")
        d.load_library(small.seq)
        after = {}
        for r in (route, other):
            set_route(monkeypatch, ROUTES[r][0])
            after[r] = run_direction(d, small)
    finally:
        d.close()
    for r, res in after.items():
        assert route_of(res[0]) == ROUTES[r][1], (r, route_of(res[0]))
        assert_direction_is_the_oracles(res, small, f"small on {r} after big on {route}")
        set_route(monkeypatch, ROUTES[r][0])
        f = device(small)
        try:
            alone = run_direction(f, small)
        finally:
            f.close()
        for (ca, ha, pa), (cb, hb, pb) in zip(res[4], alone[4]):
            assert np.array_equal(ca, cb) and (ha, pa) == (hb, pb), f"small on {r} after big on {route}: final DP rows"


def test_a_small_batch_after_a_big_one():
    """The family route (ramx_dev_run_families) on the process-wide session: a batch of the BIG loop's family and two others,
    then a batch of the SMALL one alone; every family equals its oracle run."""
    from oracle import pyoracle as po
    from repeatafterme_amd.extend import extend_batch
    from repeatafterme_amd.synth import synth_family
    big, small = sc.loop_world("big"), sc.loop_world("small")
    mids = [synth_family(n, big.L, big.W, K=100, seed=80 + n, both_sides=True, minus_frac=0.3, n_run_frac=0.1) for n in (130, 33)]
    worlds = [(big.cores, big.seq, big.p)] + [(fs.cores, np.ascontiguousarray(fs.sequence, np.int8), big.p) for fs in mids]
    for group in (worlds, [(small.cores, small.seq, small.p)]):
        batch = [(c.copy(), seq, new_master(p.L)) for c, seq, p in group]
        infos = extend_batch(1, batch, to_extend_params(group[0][2]))
        for i, ((c, seq, p), (got_c, _, got_m)) in enumerate(zip(group, batch)):
            oc, om = c.copy(), new_master(p.L)
            o = po.oracle_extend(1, oc, seq, om, p)
            assert (infos[i].ret, infos[i].rows_executed) == (o.ret, o.rows_executed) and o.ret > 0, (len(group), i)
            assert np.array_equal(got_m, om) and np.array_equal(got_c.right_len, oc.right_len) and np.array_equal(got_c.score, oc.score), (len(group), i)


# ---------------------------------------------------------------------------------------------------- e. seam 1, every sink set

SINK_SELECT = (2, 50, 1024)                                  # min_count, min_permille, max_variants
SUBFAM_ARGS = SINK_SELECT + (1.0, sc.SUBFAM_K, 8, 2, 3)      # ... min_mlog10p, K, max_iter, min_members, max_replays
BIG_SELECT = (4, 100, 256)
BIG_SUBFAM = BIG_SELECT + (3.0, 4, 8, 4, 2)


def seam1_world(which):
    """(cores, sequence, parameters) of BIG's first family or of SMALL's largest, with an early stop so that the kept consensus
    is shorter than the executed rows"""
    from oracle import pyoracle as po
    w = sc.big() if which == "big" else sc.small()
    seq, cores = w.fams[0]
    p = po.Params.named("14p43g", bandwidth=w.p.bandwidth, L=w.p.L, cappenalty=w.p.cappenalty, when_to_stop=12)
    return cores, seq, p


def seam1_call(direction, cores, seq, master, p, select, subfam):
    from repeatafterme_amd.extend import extend_alignment
    res = extend_alignment(direction, cores, seq, master, to_extend_params(p), profile=True, align=True, refine=3, copies=True,
                           linkage=select, subfam=subfam, cpg=3)
    return dict(zip(("info", "profile", "align", "refine", "copies", "linkage", "subfam", "cpg"), res))


def test_seam_1_with_every_sink_small_after_big():
    """extend_alignment with the profile, alignment, refinement, copies, linkage, subfamily and CpG sinks set, both directions, on
    BIG's large family and then, in the same process, on SMALL's: SMALL's records are the restatements', and so are its
    tsd_flat, period_flat and term_flat after the same calls on BIG."""
    import copystats_ref as cr
    import dinuc_ref as dr
    import period_ref as per
    import pileup_ref as pr
    import term_ref as tr
    import tsd_ref as ts
    from oracle import pyoracle as po
    from repeatafterme_amd.extend import period_flat, term_flat, tsd_flat
    from test_gpu_profile import check_against_oracle
    done = {}
    for which in ("big", "small"):
        cores, seq, p = seam1_world(which)
        c, m = cores.copy(), new_master(p.L)
        args = (BIG_SELECT, BIG_SUBFAM) if which == "big" else (SINK_SELECT, SUBFAM_ARGS)
        recs = {direction: seam1_call(direction, c, seq, m, p, *args) for direction in (1, 0)}
        sites = (tsd_flat(c, seq, TsdParams(**sc.TSD)), period_flat(c, seq, 2, PeriodParams(**sc.PERIOD)), term_flat(c, seq, TermParams(**sc.TERM)))
        done[which] = (c, m, recs, sites)
        assert all(recs[k]["info"].ret > 0 and len(recs[k]["profile"].cols) > 0 for k in (1, 0)), which
    cores, seq, p = seam1_world("small")
    c, m, recs, (tsd, period, term) = done["small"]
    oc, om = cores.copy(), new_master(p.L)
    for direction in (1, 0):
        before = oc.copy()
        o = po.oracle_extend(direction, oc, seq, om, p, trace=True, row_trace=True)
        r = recs[direction]
        tag = f"small, direction {direction}"
        assert (r["info"].ret, r["info"].rows_executed) == (o.ret, o.rows_executed) and 0 < o.ret < o.rows_executed, tag
        check_against_oracle(direction, o, r["profile"], o.rows_executed, p.cappenalty, tag)
        cons = o.col_base[:o.ret].astype(np.int8)
        cols, di, idx, results = dr.pileups(direction, before, seq, p, cons, with_walks=True)
        al = r["align"]
        assert np.array_equal(al.cons, cons) and list(al.core_index) == idx, tag
        check_against_walker(al.ends, al.col_idx, al.col_ins, results, o.ret, tag)
        rcons, rcols, replays, conv = pr.refine(direction, before, seq, p, cons, 3)
        rf = r["refine"]
        same_pileup(rf.cols, cols, tag)
        assert np.array_equal(rf.refined_cons, rcons) and (rf.replays, rf.converged) == (replays, conv), tag
        same_pileup(rf.refined_cols, rcols, tag + ": refined")
        stats = cr.stats_of(direction, before, idx, results, seq, p.bandwidth, cons, not direction)
        assert np.array_equal(r["copies"].stats, stats), tag
        same_ends(r["copies"].ends, results, tag)
        pl = lr.planes_of(direction, before, idx, results, seq, p.bandwidth, cons)
        planes = lr.select(cons, cols, *SINK_SELECT)
        lk = r["linkage"]
        same_pileup(lk.cols, cols, tag + ": linkage")
        assert np.array_equal(lk.planes, planes) and np.array_equal(lk.co, lr.gram(pl, planes)) and len(planes) > 0, tag
        sf = r["subfam"]
        assert np.array_equal(sf.planes, planes), tag
        linked = [(l["p"], l["q"]) for l in lr.link_pairs(planes, lr.gram(pl, planes), SUBFAM_ARGS[3])]
        init, _ = sr.components(planes, linked, SUBFAM_ARGS[4])
        want = sr.iterate(pl, planes, init, len(idx), max_iter=SUBFAM_ARGS[5])
        assert (sf.iterations, sf.converged) == (want["iterations"], want["converged"]), tag
        for k in ("labels", "patterns", "cnt", "size", "dist"):
            assert np.array_equal(getattr(sf, k), want[k]), (tag, k)
        assert [(g.group, g.size) for g in sf.groups] == [(k, int(n)) for k, n in enumerate(want["size"]) if n >= SUBFAM_ARGS[6]], tag
        ccons, ccols, cdi, creplays, cconv, n_cpg = dr.refine_cpg(direction, before, seq, p, cons, 3)
        cg = r["cpg"]
        assert np.array_equal(cg.refined_cons, ccons) and (cg.replays, cg.converged, cg.n_cpg) == (creplays, cconv, n_cpg), tag
        same_pileup(cg.refined_cols, ccols, tag + ": cpg")
        assert np.array_equal(cg.refined_di, cdi), tag
    assert np.array_equal(m, om) and np.array_equal(c.left_len, oc.left_len) and np.array_equal(c.right_len, oc.right_len)
    sites = ts.sites_of(oc)
    assert [tuple(int(r[k]) for k in ("k", "mm", "dl", "dr")) for r in tsd] == ts.tsd_all(seq, sites, **sc.TSD)
    segs = per.segments_of(oc, 2)
    assert [tuple(int(r[k]) for k in ("period", "score", "start", "end", "agree", "disagree")) for r in period] == per.records(seq, segs, **sc.PERIOD)
    want = [tr.site_records(seq, site, **sc.TERM) for site in sites]
    assert [tuple(tuple(int(r[j][k]) for k in tr.FIELDS) for j in (0, 1)) for r in term] == want


# ---------------------------------------------------------------------------------------------------- f. a batch of the CLI

from test_gpu_cli_all_outputs import inputs        # noqa: E402,F401  (the module's fixture: the three families as a .2bit and their ranges)


def test_a_batch_in_which_every_family_names_every_field(inputs):      # noqa: F811
    """The three families of tests/test_gpu_cli_all_outputs.py in one -batch list, the largest first, every line with all sixteen
    fields: every file is the one -ranges writes for that family alone in a process of its own (f0's are pinned there)."""
    import test_gpu_cli_all_outputs as ao
    tmp = inputs
    fields = [(ext, field) for _, ext, field in ao.CLASSIC + ao.ANALYSIS if field] + [("term", 16)]
    sizes = {k: sum(1 for _ in open(tmp / f"fam{k}.tsv")) for k in range(3)}
    order = sorted(range(3), key=lambda k: -sizes[k])
    with open(tmp / "all.list", "w") as fh:
        for k in order:
            fh.write("\t".join([f"fam{k}.tsv", f"s{k}.log"] + [f"s{k}.{ext}" for ext, _ in sorted(fields, key=lambda x: x[1])]) + "\n")
    r = subprocess.run([_lib.CLI_PATH] + ao.COMMON + ["-batch", "all.list"], cwd=tmp, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    flags = {ext: flag for flag, ext, field in ao.CLASSIC + ao.ANALYSIS if field}
    flags["term"] = "-outterm"
    for k in range(3):
        alone = [x for ext, _ in fields for x in (flags[ext], f"o{k}.{ext}")]
        r1 = subprocess.run([_lib.CLI_PATH] + ao.COMMON + ["-ranges", f"fam{k}.tsv"] + alone, cwd=tmp, capture_output=True, text=True)
        assert r1.returncode == 0 and r1.stderr == "", r1.stderr
        assert ao.without_duration(open(tmp / f"s{k}.log").read()) == ao.without_duration(r1.stdout), k
        for ext, _ in fields:
            a, b = open(tmp / f"s{k}.{ext}", "rb").read(), open(tmp / f"o{k}.{ext}", "rb").read()
            assert a == b and len(a) > 0, (k, ext)
