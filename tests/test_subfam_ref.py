"""The CPU restatement of the split into subfamilies (tests/subfam_ref.py): ramx_link_components of libramx.so through ctypes
against it; the identities of the counts against the Gram matrix on the shapes the GPU tests use; hand-made bit tables for the
update at exactly half and the tie of the assignment; and the planted family that the GPU and CLI tests rest on, asserted here on
the restatement first.  No GPU; everything is integers and exact."""
import ctypes
import os
import re

import numpy as np
import pytest

from repeatafterme_amd import _lib
from repeatafterme_amd.datamodel import LINK_DTYPE, PLANE_COVER

import linkage_ref as lr
import subfam_ref as sr
import test_gpu_pileup as tp
from helpers import ROOT

CASES = [(sh, d) for sh in tp.SHAPES for d in (1, 0)]

# seven variants on six rows (row 2 has two), every row with its cover plane: the variants are list entries 0 2 4 6 7 9 11
LIST = lr.as_planes([(0, 1), (0, 6), (1, 2), (1, 6), (2, 5), (2, 6), (2, 7), (3, 0), (3, 6), (4, 3), (4, 6), (5, 1), (5, 6)])
VAR = [0, 2, 4, 6, 7, 9, 11]


def test_header_declares_and_library_exports_the_entries():
    txt = open(os.path.join(ROOT, "include", "ramx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ramx_link_components", "ramx_dev_subfamilies", "ramx_dev_subfam_masks", "ramx_dev_subfam_ms", "ramx_set_subfam_sink"):
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} is not declared in include/ramx.h"
        assert hasattr(lib, name), f"{name} is not exported by libramx.so"
        assert name in _lib.EXPORTS
    assert re.search(r"#define\s+RAMX_SUBFAM_MAX\s+8", txt)
    assert sr.variants_of(LIST)[0] == VAR


def c_components(planes, pairs, K):
    from repeatafterme_amd.device import link_components
    links = np.zeros(len(pairs), LINK_DTYPE)
    for i, (p, q) in enumerate(pairs):
        links[i]["p"], links[i]["q"] = p, q
    return link_components(planes, links, K)


def both(pairs, K):
    init, comp = sr.components(LIST, pairs, K)
    got_init, got_comp = c_components(LIST, pairs, K)
    assert got_init.shape == init.shape and np.array_equal(got_init, init), (pairs, K)
    assert np.array_equal(got_comp, comp), (pairs, K)
    assert not init[:, 0].any()                                 # pattern 0 is the consensus itself
    return init, comp


def test_components_of_the_library_against_the_restatement():
    v = VAR
    # no pairs: one pattern
    init, comp = both([], 4)
    assert init.shape == (7, 1) and not comp.any()
    # one pair
    init, comp = both([(v[1], v[5])], 4)
    assert init.shape == (7, 2) and list(comp) == [0, 1, 0, 0, 0, 1, 0]
    # two components of equal size: the one with the lowest member first
    init, comp = both([(v[2], v[6]), (v[0], v[4])], 4)
    assert init.shape == (7, 3) and list(comp) == [1, 0, 2, 0, 1, 0, 2]
    # a chain a - b - c is one component, and the larger one comes first whatever its members
    init, comp = both([(v[3], v[4]), (v[4], v[6]), (v[0], v[1])], 4)
    assert init.shape == (7, 3) and list(comp) == [2, 2, 0, 1, 1, 0, 1]
    # more components than K - 1: the first K - 1 are kept, the variants of the others start in no pattern
    three = [(v[0], v[1]), (v[2], v[3]), (v[4], v[5])]
    init, comp = both(three, 3)
    assert init.shape == (7, 3) and list(comp) == [1, 1, 2, 2, 0, 0, 0]
    init, comp = both(three, 2)
    assert init.shape == (7, 2) and list(comp) == [1, 1, 0, 0, 0, 0, 0]
    init, comp = both(three, 1)
    assert init.shape == (7, 1) and not comp.any()
    init, comp = both(three, 8)
    assert init.shape == (7, 4) and list(comp) == [1, 1, 2, 2, 3, 3, 0]
    # a pair given twice and in either order; K at its limits
    both([(v[5], v[1]), (v[1], v[5])], 8)
    for K in (0, 9):
        with pytest.raises(_lib.RamxError):
            c_components(LIST, [], K)
    with pytest.raises(_lib.RamxError):                         # a cover plane is no variant
        c_components(LIST, [(1, 2)], 4)


@pytest.mark.parametrize("shape,direction", CASES)
def test_identities_against_the_gram_matrix(shape, direction):
    c = lr.shape_case(*shape, direction, "kept")
    pl, n = c["planes"], len(c["idx"])
    planes = lr.select(c["cons"], c["cols"], 2, 50)
    co = lr.gram(pl, planes)
    var, cov = sr.variants_of(planes)
    linked = [(l["p"], l["q"]) for l in lr.link_pairs(planes, co, 1.0)]
    for init in (sr.components(planes, linked, 4)[0], sr.random_init(len(var), 8, 5)):
        res = sr.iterate(pl, planes, init, n)
        K = init.shape[1]
        assert np.array_equal(res["cnt"].sum(axis=0), np.diag(co)) and res["size"].sum() == n
        assert res["labels"].min() >= 0 and res["labels"].max() < K and res["masks"].shape == (K, (n + 63) // 64)
        assert np.array_equal(res["dist"][np.arange(n), res["labels"]], res["dist"].min(axis=1))
        assert 1 <= res["iterations"] <= 8 and (res["converged"] or res["iterations"] == 8)
        if res["converged"] and K > 1:
            # a converged family's patterns are their own update
            assert np.array_equal(sr.update(planes, res["patterns"], res["cnt"], res["size"]), res["patterns"])


def test_the_update_at_exactly_half():
    planes = lr.as_planes([(0, 1), (0, 6), (1, 2), (1, 6)])
    #            copies  0 1 2 3 4 5 6 7
    pl = {(0, 1): int("00110000"[::-1], 2), (0, 6): int("11110000"[::-1], 2),      # group 0: 2 of 4 carry it: exactly half
          (1, 2): int("11100000"[::-1], 2), (1, 6): int("11111000"[::-1], 2)}      # group 0: 3 of 5
    labels = np.array([0, 0, 0, 0, 0, 1, 1, 1], np.int32)
    cnt, size = sr.counts(pl, planes, labels, 2)
    assert cnt.tolist() == [[2, 4, 3, 5], [0, 0, 0, 0]] and size.tolist() == [5, 3]
    pats = np.array([[1, 1], [0, 1]], np.uint8)
    new = sr.update(planes, pats, cnt, size)
    # half is no majority; 3 of 5 is; group 1 covers neither column: 0 > 0 fails
    assert new.tolist() == [[0, 0], [1, 0]]
    # an empty group keeps its pattern
    assert sr.update(planes, pats, cnt, np.array([5, 0], np.int32)).tolist() == [[0, 1], [1, 1]]


def test_the_tie_of_the_assignment_goes_to_the_lowest_pattern():
    planes = lr.as_planes([(0, 1), (0, 6), (1, 2), (1, 6)])
    #            copies  0 1 2 3 4
    pl = {(0, 1): int("11000"[::-1], 2), (0, 6): int("11110"[::-1], 2),
          (1, 2): int("10100"[::-1], 2), (1, 6): int("11101"[::-1], 2)}
    pats = np.array([[0, 1, 1], [0, 1, 1]], np.uint8)            # patterns 1 and 2 are equal: never 2
    d = sr.distances(pl, planes, pats, 5)
    # copy 0 carries both, copy 1 the first only (1 : 1, a tie), copy 2 the second only (a tie), copy 3 covers row 0 only
    # (0 : 1), copy 4 covers row 1 only and carries nothing
    assert d.tolist() == [[2, 0, 0], [1, 1, 1], [1, 1, 1], [0, 1, 1], [0, 1, 1]]
    assert sr.assign(d).tolist() == [1, 0, 0, 0, 0]
    # a copy that covers nothing is at distance 0 from everything
    pl0 = {k: v & 0b01111 for k, v in pl.items()}
    pl0[(1, 6)] &= 0b01111
    assert sr.distances(pl0, planes, pats, 5)[4].tolist() == [0, 0, 0] and sr.assign(sr.distances(pl0, planes, pats, 5))[4] == 0


def planted_split(direction, K=4, max_iter=8):
    c = lr.planted_case(direction)
    linked = [(l["p"], l["q"]) for l in lr.link_pairs(c["sel"], c["co"], lr.CLI_SCORE)]
    init, comp = sr.components(c["sel"], linked, K)
    return c, init, comp, sr.iterate(c["planes"], c["sel"], init, len(c["idx"]), max_iter)


@pytest.mark.parametrize("direction", [1, 0])
def test_the_planted_family(direction):
    """Every copy that covers columns 8, 30 and 55 and carries all three planted bases gets one common non-zero label (1: the
    planted columns are the largest component); every copy that covers all three and carries none gets 0 -- in the right
    direction unless it carries a variant of the unplanted pair, which is a component of its own and takes it into group 2."""
    c, init, comp, res = planted_split(direction)
    pl, n = c["planes"], len(c["idx"])
    where = {(int(x["row"]), int(x["cls"])): k for k, x in enumerate(c["sel"])}
    var, _ = sr.variants_of(c["sel"])
    planted = [var.index(where[rc]) for rc in c["planted"]]
    # the planted variants are one component, and it is the first pattern: the largest (three variants)
    assert len(set(comp[planted])) == 1 and comp[planted[0]] == 1
    # the right direction has the unplanted pair (0, del) x (1, ins) as a component of its own
    extra = [var.index(where[rc]) for rc in lr.UNPLANTED_PAIR if rc in where]
    if direction == 1:
        assert len(extra) == 2 and comp[extra[0]] == comp[extra[1]] == 2 and init.shape[1] == 3
    else:
        assert init.shape[1] == 2
    cover_all = pl[(8, PLANE_COVER)] & pl[(30, PLANE_COVER)] & pl[(55, PLANE_COVER)]
    carry = [pl[rc] for rc in c["planted"]]
    all3, none = cover_all & carry[0] & carry[1] & carry[2], cover_all & ~(carry[0] | carry[1] | carry[2])
    lab_all = {int(res["labels"][i]) for i in range(n) if all3 >> i & 1}
    lab_none = {int(res["labels"][i]) for i in range(n) if none >> i & 1}
    print(f"dir={direction} K'={init.shape[1]} iterations={res['iterations']} converged={res['converged']} size={res['size'].tolist()} "
          f"all three: {bin(all3).count('1')} copies -> {lab_all}; none: {bin(none).count('1')} copies -> {lab_none}")
    assert bin(all3).count("1") >= 15 and bin(none).count("1") >= 30
    assert lab_all == {1}
    if direction == 0:
        assert lab_none == {0}
    else:
        # as worded the claim fails here: 5 of the 36 copies that carry no planted base carry the unplanted pair instead -- column
        # 0 deleted AND bases inserted before column 1 -- and follow it into group 2; every other one gets 0 (one of the two
        # alone is a tie, which goes to the lowest)
        other = pl[lr.UNPLANTED_PAIR[0]] & pl[lr.UNPLANTED_PAIR[1]]
        for i in range(n):
            if none >> i & 1:
                assert int(res["labels"][i]) == (2 if other >> i & 1 else 0), i
        assert lab_none == {0, 2}
    assert res["converged"] == 1 and res["patterns"][planted, 1].all()
