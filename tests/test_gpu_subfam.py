"""The split of an extension's copies into subfamilies on the device (C-ABI ramx_dev_subfamilies, ramx_dev_subfam_masks) against
the restatement of tests/subfam_ref.py: labels, mask words, counts, sizes, patterns, iterations and converged are integers,
everything is exact.  The families are those of tests/linkage_ref.py and tests/test_gpu_linkage.py.  The kernels' edges: 64
flanks a mask word (1, 63, 64, 65 flanks), 64 tiles a round of the count kernel's lanes (33 and 65 tiles), 64 variants a block
of the assign kernel (1, 63, 64, 65, 130 variants)."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import PLANE_COVER, new_master

import linkage_ref as lr
import pileup_ref as pr
import subfam_ref as sr
import test_gpu_pileup as tp
import test_gpu_replay_long as rl
from helpers import to_extend_params

pytestmark = pytest.mark.gpu

FIELDS = ("labels", "masks", "cnt", "size", "patterns")


def same(got, want, tag):
    assert (got.iterations, got.converged) == (want["iterations"], want["converged"]), f"{tag}: {got.iterations} {got.converged}"
    for k in FIELDS:
        g, w = getattr(got, k), want[k]
        assert g.shape == w.shape and np.array_equal(g, w), f"{tag}: {k}: {np.argwhere(g != w)[:8].tolist() if g.shape == w.shape else g.shape}"


def open_case(c, direction):
    """-> (Device with the case's planes resident, n flanks)"""
    from repeatafterme_amd.device import Device, resolve_flanks
    d = Device(0)
    d.load_library(c["seq"])
    flanks, idx = resolve_flanks(direction, c["fs"].cores, c["p"].bandwidth, c["p"].L)
    assert list(idx) == c["idx"]
    d.planes(flanks, to_extend_params(c["p"]), c["cons"])
    return d, len(idx)


def linked_init(d_planes, co, K):
    """The library's own path from a Gram matrix to the initial patterns, compared with the restatement's."""
    from repeatafterme_amd.device import link_components, link_pairs
    links, found = link_pairs(d_planes, co, float(lr.CLI_SCORE))
    assert found == len(links)
    init, comp = link_components(d_planes, links, K)
    want, wcomp = sr.components(d_planes, [(int(l["p"]), int(l["q"])) for l in links], K)
    assert np.array_equal(init, want) and np.array_equal(comp, wcomp)
    return init


@pytest.mark.parametrize("direction", [1, 0])
def test_the_planted_family(direction):
    """K = 1, 2, 4, 8 from the linked pairs (one, two, and -- in the right direction, which has the unplanted pair -- three
    patterns), and eight patterns of random bits."""
    c = lr.planted_case(direction)
    d, n = open_case(c, direction)
    try:
        co = d.plane_gram(c["sel"])
        assert np.array_equal(co, c["co"])
        var, _ = sr.variants_of(c["sel"])
        seen = set()
        for K in (1, 2, 4, 8):
            init = linked_init(c["sel"], co, K)
            seen.add(init.shape[1])
            res = d.subfamilies(c["sel"], init, masks=True)
            want = sr.iterate(c["planes"], c["sel"], init, n)
            same(res, want, f"dir={direction} K={K}")
            assert res.converged == 1 and res.iterations == (1 if K == 1 else 2)
            if K >= 2:
                assert res.size[1] >= 20 and res.size[0] >= 30
        assert seen == ({1, 2, 3} if direction else {1, 2})
        init = sr.random_init(len(var), 8, 11)
        res = d.subfamilies(c["sel"], init, masks=True)
        same(res, sr.iterate(c["planes"], c["sel"], init, n), f"dir={direction} random")
        assert (res.size > 0).sum() >= 3
    finally:
        d.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_flank_counts_at_the_mask_word_edge(n):
    """One flank; a word one short, full, and one flank in a second word: the padding lanes belong to no group."""
    c = lr.shape_case(n, 14, 60, "14p43g", 1, "foreign")
    rows = len(c["cons"])
    planes = sr.list_with(rows, 40, first_row=3)
    init = sr.copy_init(c["planes"], planes, 8, n, n)
    d, nf = open_case(c, 1)
    try:
        res = d.subfamilies(planes, init, masks=True)
        labels_all = d._subfam_labels
    finally:
        d.close()
    assert nf == n and res.masks.shape == (8, (n + 63) // 64)
    same(res, sr.iterate(c["planes"], planes, init, n), f"n={n}")
    assert (labels_all[n:] == -1).all() and res.size.sum() == n
    if n > 1:
        assert (res.size > 0).sum() >= 2


@functools.lru_cache(maxsize=None)
def many_tiles():
    """4,160 flanks (65 tiles), W = 5, a foreign consensus of about 20 columns -> (fs, seq, p, cons, idx, planes)"""
    from repeatafterme_amd.synth import synth_family
    n, L, W = 4160, 24, 5
    fs = synth_family(n, L, W, K=20, seed=78, both_sides=True, minus_frac=0.4, n_run_frac=0.1)
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    p = tp.params("14p43g", W, L, when_to_stop=20)
    o = po.oracle_extend(1, fs.cores.copy(), seq, new_master(L), p, trace=True)
    cons = tp.foreign(o.col_base[:o.rows_executed], at=10, k=2)
    cols, idx, results = pr.pileup(1, fs.cores, seq, p, cons, with_walks=True)
    assert len(idx) == n and len(cons) >= 15
    return fs, seq, p, cons, cols, lr.planes_of(1, fs.cores, idx, results, seq, W, cons)


def test_tile_counts_past_one_round_of_the_count_kernel():
    """65 tiles, and the first 2,112 flanks (33 tiles) and the first 4,096 (64 tiles) as families of their own, all in one call
    along the same consensus: the count kernel's lanes go round once with idle lanes, once exactly, and twice."""
    from repeatafterme_amd.device import Device, resolve_flanks
    fs, seq, p, cons, cols, whole = many_tiles()
    rows, L = len(cons), p.L
    (fl, nx), _ = resolve_flanks(1, fs.cores, p.bandwidth, L)
    counts = [2112, 4160, 4096]
    flanks, first, count = rl.lay_out([(fl, k, 0) for k in counts], hole_before=1)
    planes = lr.select(cons, cols, 40, 20)
    var, _ = sr.variants_of(planes)
    assert len(var) >= 8
    init = sr.random_init(len(var), 5, 3)
    d = Device(0)
    try:
        d.load_library(seq)
        d.planes(flanks, to_extend_params(p), np.stack([np.resize(cons, L)] * 3), rows=[rows] * 3, fam_first=first, fam_count=count)
        res = d.subfamilies([planes] * 3, [init] * 3, masks=True)
    finally:
        d.close()
    assert any(v >> 4096 for v in whole.values())                               # the 65th tile has bits of its own
    for f, k in enumerate(counts):
        cut = {key: v & ((1 << k) - 1) for key, v in whole.items()}
        same(res[f], sr.iterate(cut, planes, init, k), f"{k} flanks")
        assert res[f].masks.shape == (5, (k + 63) // 64) and (res[f].size > 0).sum() >= 3
    assert not np.array_equal(res[0].cnt, res[1].cnt)


def test_variant_counts_at_the_block_edge_on_one_resident_replay():
    """1, 63, 64, 65 and 130 variants of one family's full list of 8 planes a row: a block of one, one short, full, a second
    block of one variant, and three blocks with a partial last -- with three and with eight patterns, the call repeated."""
    c = lr.shape_case(*tp.SHAPES[4], 1, "foreign")
    rows = len(c["cons"])
    d, n = open_case(c, 1)
    try:
        for V in (1, 63, 64, 65, 130):
            planes = sr.list_with(rows, V, first_row=2)
            assert len(sr.variants_of(planes)[0]) == V
            for K in (3, 8):
                init = sr.copy_init(c["planes"], planes, K, n, 100 + V)
                if V == 1:
                    init[0, K - 1] = 1
                res = d.subfamilies(planes, init, masks=True)
                same(res, sr.iterate(c["planes"], planes, init, n), f"V={V} K={K}")
                assert res.size.sum() == n and (V == 1 or (res.size > 0).sum() >= 2)
    finally:
        d.close()


def test_three_families_with_an_empty_one_in_the_middle():
    """Their own consensus and list each; the middle family has no flank, hence no tile: it is answered on the host."""
    from repeatafterme_amd.device import Device, resolve_flanks
    p = tp.params("20p43g", 14, 120, cappenalty=-10, when_to_stop=25)
    fams = tp._three_families()
    fams = [fams[1], fams[0], fams[2]]                                          # the small one in the middle, without its flanks
    lib = np.concatenate([fs.sequence for fs in fams])
    offs = np.cumsum([0] + [len(fs.sequence) for fs in fams])
    cons = np.zeros((3, 120), np.int8)
    rows, parts, want = [], [], []
    for f, fs in enumerate(fams):
        o = po.oracle_extend(1, fs.cores.copy(), fs.sequence, new_master(120), p, trace=True)
        c = tp.foreign(o.col_base[:o.ret], at=8, k=5)
        rows.append(len(c))
        cons[f, :len(c)] = c
        cols, idx, results = pr.pileup(1, fs.cores, fs.sequence, p, c, with_walks=True)
        (fl, nx), _ = resolve_flanks(1, fs.cores, 14, 120)
        n = 0 if f == 1 else len(idx)
        want.append((lr.planes_of(1, fs.cores, idx, results, fs.sequence, 14, c), n))
        parts.append((fl, n, offs[f]))
    flanks, first, count = rl.lay_out(parts, hole_before=2)
    assert count[1] == 0 and rows[1] >= 2 and min(rows[0], rows[2]) > 20
    lists = [sr.list_with(rows[0], 20, 1), sr.list_with(rows[1], 9, 0), sr.list_with(rows[2], 70, 4)]
    inits = [sr.copy_init(want[f][0], x, 4, max(want[f][1], 4), 7 + f) for f, x in enumerate(lists)]
    d = Device(0)
    try:
        d.load_library(lib)
        d.planes(flanks, to_extend_params(p), cons, rows=rows, fam_first=first, fam_count=count)
        res = d.subfamilies(lists, inits, masks=True)
        labels_all = d._subfam_labels.copy()
    finally:
        d.close()
    for f in (0, 2):
        pl, n = want[f]
        same(res[f], sr.iterate(pl, lists[f], inits[f], n), f"family {f}")
    e = res[1]
    assert len(e.labels) == 0 and e.masks.shape == (4, 0) and not e.cnt.any() and not e.size.any() and (e.iterations, e.converged) == (1, 1)
    assert np.array_equal(e.patterns, inits[1])
    inside = np.zeros(len(labels_all), bool)
    for f in (0, 2):
        inside[first[f]:first[f] + count[f]] = True
    assert (labels_all[~inside] == -1).all() and (labels_all[inside] >= 0).all()


def test_a_family_without_tiles_before_another_in_the_gram_and_in_the_split():
    """The layout of tests/test_gpu_dist.py: three families, one of them with rows = 0, a family without flanks, a tile that
    belongs to no family -- here the family without flanks stands third, with a list of its own, before the last family.  The
    Gram call writes nothing for it (and takes none of its planes' offsets); the split answers it on the host, its counts
    placed by its planes' offsets; the family behind it gets the restatement's answers from both."""
    from repeatafterme_amd.device import Device, resolve_flanks
    p = tp.params("20p43g", 14, 120, cappenalty=-10, when_to_stop=25)
    fams = tp._three_families()
    lib = np.concatenate([fs.sequence for fs in fams])
    offs = np.cumsum([0] + [len(fs.sequence) for fs in fams])
    cons = np.zeros((4, 120), np.int8)
    rows, parts, want = [], [], []
    for f, fs in enumerate(fams):
        o = po.oracle_extend(1, fs.cores.copy(), fs.sequence, new_master(120), p, trace=True)
        c = tp.foreign(o.col_base[:o.ret], at=8, k=5) if f else o.col_base[:0]               # family 0: rows = 0
        cols, idx, results = pr.pileup(1, fs.cores, fs.sequence, p, c, with_walks=True)
        (fl, nx), _ = resolve_flanks(1, fs.cores, 14, 120)
        if f == 2:                                                                            # before it: a family without flanks
            cons[len(rows), :len(c)] = c
            rows.append(len(c)); parts.append((fl, 0, offs[f])); want.append(({}, 0))
        cons[len(rows), :len(c)] = c
        rows.append(len(c)); parts.append((fl, nx, offs[f]))
        want.append((lr.planes_of(1, fs.cores, idx, results, fs.sequence, 14, c), len(idx)))
    flanks, first, count = rl.lay_out(parts, hole_before=1)
    assert rows[0] == 0 and count[2] == 0 and rows[2] == rows[3] > 10 and rows[1] > 10 and min(count[0], count[1], count[3]) > 0
    K = 3
    lists = [lr.as_planes([]), sr.list_with(rows[1], 9, 1), sr.list_with(rows[2], 12, 2), sr.list_with(rows[3], 20, 3)]
    inits = [np.zeros((0, K), np.uint8), sr.copy_init(want[1][0], lists[1], K, want[1][1], 5), sr.random_init(12, K, 6),
             sr.copy_init(want[3][0], lists[3], K, want[3][1], 7)]
    assert inits[2].any()
    d = Device(0)
    try:
        d.load_library(lib)
        d.planes(flanks, to_extend_params(p), cons, rows=rows, fam_first=first, fam_count=count)
        cos = d.plane_gram(lists)
        res = d.subfamilies(lists, inits, masks=True)
    finally:
        d.close()
    assert cos[0].shape == (0, 0) and cos[2].shape == (len(lists[2]),) * 2 and (cos[2] == -1).all()    # nothing written
    e = res[2]
    assert e.cnt.shape == (K, len(lists[2])) and not e.cnt.any() and e.size.shape == (K,) and not e.size.any()
    assert (e.iterations, e.converged) == (1, 1) and np.array_equal(e.patterns, inits[2])
    assert len(e.labels) == 0 and e.masks.shape == (K, 0)
    for f in (1, 3):
        pl, n = want[f]
        assert np.array_equal(cos[f], lr.gram(pl, lists[f])) and cos[f].any(), f
        same(res[f], sr.iterate(pl, lists[f], inits[f], n), f"family {f}")


def test_one_assignment_only_and_an_init_whose_group_empties():
    c = lr.planted_case(0)
    d, n = open_case(c, 0)
    try:
        co = d.plane_gram(c["sel"])
        init = linked_init(c["sel"], co, 4)
        # max_iter = 1: the first assignment's labels and counts, the initial patterns, not converged
        one = d.subfamilies(c["sel"], init, max_iter=1, masks=True)
        more = d.subfamilies(c["sel"], init, max_iter=8, masks=True)
        same(one, sr.iterate(c["planes"], c["sel"], init, n, max_iter=1), "max_iter=1")
        same(more, sr.iterate(c["planes"], c["sel"], init, n, max_iter=8), "max_iter=8")
        assert (one.iterations, one.converged) == (1, 0) and np.array_equal(one.patterns, init)
        assert more.converged == 1 and more.iterations > 1
        two = d.subfamilies(c["sel"], init, max_iter=2, masks=True)
        same(two, sr.iterate(c["planes"], c["sel"], init, n, max_iter=2), "max_iter=2")
        # a pattern that carries every class of every row is further from every copy than the consensus: its group is empty
        # after the first assignment and keeps the pattern, while the planted group moves on
        rows = len(c["cons"])
        planes = sr.list_with(rows, 70, first_row=5)
        V = len(sr.variants_of(planes)[0])
        bad = np.zeros((V, 3), np.uint8)
        bad[:, 1] = 1
        bad[:, 2] = sr.copy_init(c["planes"], planes, 2, n, 1)[:, 1]
        res = d.subfamilies(planes, bad, masks=True)
        want = sr.iterate(c["planes"], planes, bad, n)
        same(res, want, "emptied")
        assert res.size[1] == 0 and res.patterns[:, 1].all() and res.size[2] > 0
    finally:
        d.close()


def test_state_and_argument_errors_and_what_the_call_leaves():
    """All refused on the host, before a launch; the call repeated gives the same; the resident planes are untouched."""
    from repeatafterme_amd import _lib
    from repeatafterme_amd.device import Device, resolve_flanks
    c = lr.planted_case(1)
    ep = to_extend_params(c["p"])
    sel = c["sel"]
    var, _ = sr.variants_of(sel)
    init = sr.random_init(len(var), 4, 2)
    d = Device(0)
    try:
        d.load_library(c["seq"])
        flanks, idx = resolve_flanks(1, c["fs"].cores, c["p"].bandwidth, c["p"].L)
        with pytest.raises(_lib.RamxError, match=r"\(-104\)"):                               # before any planes
            d.subfamilies(sel, init)
        d.planes(flanks, ep, c["cons"])
        full = lr.all_planes(min(len(c["cons"]), 200))
        before = d.plane_gram(full, bits=True)
        first = d.subfamilies(sel, init, masks=True)
        # a variant whose row's cover plane is not in the list
        r0 = int(sel[var[0]]["row"])
        holed = sel[[not (int(x["row"]) == r0 and int(x["cls"]) == PLANE_COVER) for x in sel]]
        assert len(holed) == len(sel) - 1
        with pytest.raises(_lib.RamxError, match=r"\(-103\).*cover plane"):
            d.subfamilies(holed, init)
        for K in (0, 9):
            with pytest.raises(_lib.RamxError, match=r"\(-103\).*K = %d" % K):
                d.subfamilies(sel, np.zeros((len(var), max(K, 1)), np.uint8), K=K)
        with pytest.raises(_lib.RamxError, match=r"\(-103\).*max_iter"):
            d.subfamilies(sel, init, max_iter=0)
        with pytest.raises(_lib.RamxError, match=r"\(-103\).*not strictly increasing"):
            d.subfamilies(sel[::-1].copy(), init)
        with pytest.raises(_lib.RamxError, match=r"\(-103\).*2 families, the resident replay has 1"):
            d.subfamilies([sel, sel], [init, init])
        rows = len(c["cons"])
        for bad in ((rows, 0), (0, 8)):
            with pytest.raises(_lib.RamxError, match=r"\(-103\).*outside the resident replay \(%d rows" % rows):
                d.subfamilies(lr.as_planes([bad]), np.zeros((1, 4), np.uint8))
        again = d.subfamilies(sel, init, masks=True)
        after = d.plane_gram(full, bits=True)
        d.copy_stats(flanks, ep, c["cons"])
        with pytest.raises(_lib.RamxError, match=r"\(-104\)"):                               # a later replay dropped them
            d.subfamilies(sel, init)
    finally:
        d.close()
    same(first, sr.iterate(c["planes"], sel, init, len(idx)), "first")
    for k in FIELDS:
        assert np.array_equal(getattr(first, k), getattr(again, k)), k
    assert (first.iterations, first.converged) == (again.iterations, again.converged)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert np.array_equal(before[0], lr.gram(c["planes"], full))
