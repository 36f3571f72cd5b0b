"""The CPU restatement of the co-segregation of variants (tests/linkage_ref.py) on the shapes the GPU tests use, both directions:
the identities of the Gram matrix against the pileup of the same consensus; the two host C functions of libramx.so
(ramx_select_planes, ramx_link_pairs) through ctypes against the restatement; and the planted family that the GPU and CLI tests
rest on, asserted here on the restatement first.  No GPU.

The numeric bound of ramx_link_pairs.  expected is one multiplication and one division of exact integers: 1e-9 relative holds
with room.  mlog10p is compared within 1e-9 * max(1, |exact|): relative from 1 upwards, as the project's 1e-9 for Kimura, and
absolute below 1, where the exact value goes to 0 (P = 1 is exactly 0 on both sides) and a pure relative bound fails: the
table n = 150, n_p = n_q = 75, n_pq = 1 has the exact value 4.7e-45 and the C code gives 2.7e-14.  The C code sums the tail in log space with lgamma; the largest
deviation from the exact rational value measured over this file's tables (n up to 300, 3,918 tables: 2.6e-13, so the bound holds as it stands) is printed by
test_pair_statistic_of_the_library_on_tables and recorded in DESIGN.md 4.11."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from repeatafterme_amd import _lib
from repeatafterme_amd.datamodel import LINK_DTYPE, PILEUP_DTYPE, PLANE_COVER, PLANE_DTYPE

import linkage_ref as lr
import test_gpu_pileup as tp
from helpers import ROOT

CASES = [(sh, d) for sh in tp.SHAPES for d in (1, 0)]
TOL = 1e-9


def close(got, want):
    return abs(got - want) <= TOL * max(1.0, abs(want))


def test_the_structs():
    assert PLANE_DTYPE.itemsize == 8 == ctypes.sizeof(_lib.Plane) and LINK_DTYPE.itemsize == 40 == ctypes.sizeof(_lib.Link)
    assert [LINK_DTYPE.fields[k][1] for k in LINK_DTYPE.names] == [0, 4, 8, 12, 16, 20, 24, 32]
    assert [n for n, _ in _lib.Link._fields_] == list(LINK_DTYPE.names)


def test_header_declares_and_library_exports_the_entries():
    txt = open(os.path.join(ROOT, "include", "ramx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ramx_dev_planes", "ramx_dev_plane_gram", "ramx_select_planes", "ramx_link_pairs", "ramx_set_linkage_sink"):
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} is not declared in include/ramx.h"
        assert hasattr(lib, name), f"{name} is not exported by libramx.so"
        assert name in _lib.EXPORTS
    assert re.search(r"#define\s+RAMX_LINKAGE_MAX_PLANES\s+2048", txt)


@pytest.mark.parametrize("shape,direction", CASES)
def test_identities_against_the_pileup(shape, direction):
    c = lr.shape_case(*shape, direction, "kept")
    pl, cols, rows = c["planes"], c["cols"], len(c["cons"])
    # whatever is at most 2048 planes whole, else the first 256 rows' worth
    planes = lr.all_planes(min(rows, 256))
    co = lr.gram(pl, planes)
    assert np.array_equal(co, co.T)
    diag = np.diag(co).reshape(-1, 8)
    r = slice(0, len(diag))
    assert np.array_equal(diag[:, :5], cols["match"][r]) and np.array_equal(diag[:, 5], cols["del"][r])
    assert np.array_equal(diag[:, 6], cols["cover"][r]) and np.array_equal(diag[:, 7], cols["ins_open"][r])
    assert (co <= np.minimum.outer(np.diag(co), np.diag(co))).all()
    for (row, cls), s in pl.items():
        assert s & ~pl[(row, PLANE_COVER)] == 0, (row, cls)
    # matched classes and the deletion partition the cover
    for row in range(rows):
        parts = [pl[(row, k)] for k in range(6)]
        assert sum(bin(x).count("1") for x in parts) == bin(pl[(row, PLANE_COVER)]).count("1")
    if shape[0] >= 37:
        assert cols["del"].sum() > 0 and cols["ins_open"].sum() > 0 and len(lr.select(c["cons"], cols, 2, 50)) > 0


def c_select(cons, cols, *args):
    from repeatafterme_amd.device import select_planes
    return select_planes(cons, cols, *args)


def col(base, cover, match, dele=0, ins_open=0):
    c = np.zeros(1, PILEUP_DTYPE)
    c["base"], c["cover"], c["match"][0][:len(match)], c["del"], c["ins_open"] = base, cover, match, dele, ins_open
    return c


def pairs_of(planes):
    return [(int(x["row"]), int(x["cls"])) for x in planes]


def test_selection_rules():
    cons = np.array([0, 1, 2, 3, 0], np.int8)
    cols = np.concatenate([
        col(0, 41, [30, 4, 3, 0, 4]),                      # C: 4 of 41 is below 100 per mille; G: below min_count
        col(1, 40, [4, 32, 0, 0, 4]),                      # A: 4 >= 4 and 4000 >= 4000; N has 4 too and is never a candidate
        col(2, 30, [0, 0, 4, 0, 0], dele=20, ins_open=6),  # the consensus base itself never; del and ins
        col(3, 0, [0, 0, 0, 0, 0]),                        # no cover
        col(0, 50, [9, 9, 9, 9, 0], dele=9, ins_open=9)])  # five candidates of 9 (A is the consensus base: four)... and ins
    want = [(1, 0), (1, 6), (2, 5), (2, 6), (2, 7), (4, 1), (4, 2), (4, 3), (4, 5), (4, 6), (4, 7)]
    assert pairs_of(lr.select(cons, cols, 4, 100, 1024)) == want == pairs_of(c_select(cons, cols, 4, 100, 1024))
    # the count threshold at its edge: 4 qualifies at 4, not at 5; the share at its edge: 4 of 40 at 100 / 101 per mille
    for mc, mp in ((5, 100), (4, 101), (4, 99), (3, 0), (1, 0), (0, 0), (4, 1000), (21, 0), (20, 666), (20, 667)):
        assert pairs_of(lr.select(cons, cols, mc, mp, 1024)) == pairs_of(c_select(cons, cols, mc, mp, 1024)), (mc, mp)
    assert (1, 0) in pairs_of(c_select(cons, cols, 4, 100, 1024)) and (1, 0) not in pairs_of(c_select(cons, cols, 4, 101, 1024))
    assert (0, 1) in pairs_of(c_select(cons, cols, 4, 97, 1024)) and (0, 1) not in pairs_of(c_select(cons, cols, 4, 98, 1024))
    assert (1, 0) not in pairs_of(c_select(cons, cols, 5, 100, 1024))
    assert (2, 5) in pairs_of(c_select(cons, cols, 20, 666, 1024)) and (2, 5) not in pairs_of(c_select(cons, cols, 20, 667, 1024))
    assert all(cls != 4 and (cls == PLANE_COVER or cls != cons[r]) for r, cls in pairs_of(c_select(cons, cols, 0, 0, 1024)))
    # the cap: the largest counts, ties to the lower (row, cls): 20 (2, del), then the 9s of row 4 in class order, 6 (2, ins) last
    counts = {1: [(2, 5), (2, 6)], 2: [(2, 5), (2, 6), (4, 1), (4, 6)], 4: [(2, 5), (2, 6), (4, 1), (4, 2), (4, 3), (4, 6)],
              6: [(2, 5), (2, 6), (4, 1), (4, 2), (4, 3), (4, 5), (4, 6), (4, 7)],
              7: [(2, 5), (2, 6), (2, 7), (4, 1), (4, 2), (4, 3), (4, 5), (4, 6), (4, 7)], 8: want, 0: []}
    for cap, w in counts.items():
        assert pairs_of(lr.select(cons, cols, 4, 100, cap)) == w == pairs_of(c_select(cons, cols, 4, 100, cap)), cap


@pytest.mark.parametrize("shape,direction", CASES)
def test_selection_of_the_library_on_the_shapes(shape, direction):
    c = lr.shape_case(*shape, direction, "kept")
    for args in ((4, 100, 1024), (1, 0, 1024), (2, 50, 5), (1, 0, 1)):
        assert pairs_of(c_select(c["cons"], c["cols"], *args)) == pairs_of(lr.select(c["cons"], c["cols"], *args)), args


def check_links(planes, co, tag):
    from repeatafterme_amd.device import link_pairs
    got, found = link_pairs(planes, co, 0.0)
    want = lr.link_pairs(planes, co, 0.0)
    assert found == len(got) == len(want), tag
    worst = 0.0
    for g, w in zip(got, want):
        assert tuple(int(g[k]) for k in ("p", "q", "n", "n_p", "n_q", "n_pq")) == tuple(w[k] for k in ("p", "q", "n", "n_p", "n_q", "n_pq")), tag
        assert close(float(g["expected"]), float(w["expected"])), (tag, g, w)
        assert close(float(g["mlog10p"]), w["mlog10p"]), (tag, g, w)
        worst = max(worst, abs(float(g["mlog10p"]) - w["mlog10p"]) / max(1.0, abs(w["mlog10p"])))
    return worst, want


@pytest.mark.parametrize("shape,direction", CASES)
def test_pair_statistic_of_the_library_on_the_shapes(shape, direction):
    c = lr.shape_case(*shape, direction, "kept")
    planes = lr.select(c["cons"], c["cols"], 2, 50, 1024)
    co = lr.gram(c["planes"], planes)
    _, want = check_links(planes, co, (shape, direction))
    from repeatafterme_amd.device import link_pairs
    # the threshold cuts, the order stays (p, q), and the count goes on beyond cap
    for cut in (0.5, 1.0, 3.0):
        got, found = link_pairs(planes, co, cut, cap=2)
        keep = [w for w in want if w["mlog10p"] >= cut and abs(w["mlog10p"] - cut) > 1e-6]
        near = [w for w in want if abs(w["mlog10p"] - cut) <= 1e-6]
        assert near or (found == len(keep) and [(int(g["p"]), int(g["q"])) for g in got] == [(w["p"], w["q"]) for w in keep[:2]])


def test_pair_statistic_of_the_library_on_tables():
    """2 x 2 tables as Gram matrices of two variants and their two cover planes: n up to 300, every margin pattern of a grid,
    every n_pq the margins allow."""
    planes = lr.as_planes([(0, 1), (0, 6), (1, 2), (1, 6)])
    worst, tables = 0.0, 0
    for n in (1, 2, 3, 7, 20, 70, 150, 299, 300):
        marg = sorted({0, 1, 2, n // 10, n // 3, n // 2, n - n // 3, n - 1, n})
        for n_p in marg:
            for n_q in marg:
                for n_pq in range(max(0, n_p + n_q - n), min(n_p, n_q) + 1):
                    co = np.array([[n_p, n_p, n_pq, n_p], [n_p, n, n_q, n], [n_pq, n_q, n_q, n_q], [n_p, n, n_q, n]], np.int32)
                    w, want = check_links(planes, co, (n, n_p, n_q, n_pq))
                    assert len(want) == 1 and want[0]["expected"] == Fraction(n_p * n_q, n)
                    worst, tables = max(worst, w), tables + 1
    print(f"ramx_link_pairs: largest deviation of mlog10p from the exact value over {tables} tables: {worst:.3e} (in units of max(1, exact))")
    assert tables > 3000 and worst <= 1e-10
    # no covering copy, no shared copy: 0
    from repeatafterme_amd.device import link_pairs
    z = np.zeros((4, 4), np.int32)
    got, found = link_pairs(planes, z)
    assert found == 1 and got[0]["mlog10p"] == 0.0 and got[0]["expected"] == 0.0
    # variants on the same row are not paired; a row without its cover plane is not tested
    assert link_pairs(lr.as_planes([(0, 1), (0, 3), (0, 6)]), np.ones((3, 3), np.int32))[1] == 0
    assert link_pairs(lr.as_planes([(0, 1), (1, 3), (1, 6)]), np.ones((3, 3), np.int32))[1] == 0


@pytest.mark.parametrize("direction", [1, 0])
def test_the_planted_family(direction):
    """Two lineages under one consensus: every third flank carries another base at columns 8, 30 and 55.  The three planted pairs
    score at or above 6, every other pair at or below 1 -- but for ONE measured exception in the right direction, named below --
    and no pair lies within 1e-6 of the CLI test's threshold 3.

    Measured on the restatement (count >= 4, 100 per mille).  Left: 8 variants, 28 pairs, the planted pairs at 7.63, 7.99, 9.59,
    the best other pair 0.84.  Right: 9 variants, 35 pairs, the planted pairs at 6.63, 7.40, 7.40.  The ninth variant is (1, ins):
    bases inserted before column 1 in exactly 7 of 70 copies (100 per mille, which 1000 * count >= min_permille * cover admits).
    All 7 also delete column 0 (9 of 70 copies do; 2 of them insert nothing), so the pair (0, del) x (1, ins) has n = 70, n_p = 9,
    n_q = 7, n_pq = 7 and scores 7.52: a real co-occurrence that nobody planted, an artefact of how the alignment opens.  The
    statistic reports it, and so does this test: the pair is asserted to be there with these counts, and every remaining pair of
    the right direction is at or below 1 (the best one 0.31)."""
    c = lr.planted_case(direction)
    sel, pairs = c["sel"], c["pairs"]
    assert len(c["cons"]) == 70
    variants = [x for x in pairs_of(sel) if x[1] != PLANE_COVER]
    assert set(c["planted"]) <= set(variants)
    where = {x: k for k, x in enumerate(pairs_of(sel))}
    planted = {where[x] for x in c["planted"]}
    got = sorted(l["mlog10p"] for l in pairs if l["p"] in planted and l["q"] in planted)
    others = sorted(l["mlog10p"] for l in pairs if not (l["p"] in planted and l["q"] in planted))
    print(f"planted family dir={direction}: {len(variants)} variants, {len(pairs)} pairs, planted {[round(x, 2) for x in got]}, "
          f"best others {[round(x, 2) for x in others[-2:]]}")
    # the planted copies are the ones that carry the variants: every third flank
    n = len(c["idx"])
    third = sum(1 << k for k in range(0, n, lr.PLANTED_EVERY))
    for x in c["planted"]:
        s = c["planes"][x]
        assert bin(s & third).count("1") >= 0.8 * bin(s).count("1") and bin(s & third).count("1") >= 0.7 * bin(third).count("1")
    # the library on the same matrix
    check_links(sel, c["co"], f"planted dir={direction}")
    assert pairs_of(c_select(c["cons"], c["cols"], 4, 100, 1024)) == pairs_of(sel)
    assert len(got) == 3 and min(got) >= 6
    assert all(abs(l["mlog10p"] - lr.CLI_SCORE) > 1e-6 for l in pairs)
    # the measured exception: the right direction's deleted column 0 with the insertion before column 1
    named = [l for l in pairs if (pairs_of(sel)[l["p"]], pairs_of(sel)[l["q"]]) == lr.UNPLANTED_PAIR]
    if direction:
        assert len(variants) == 9 and len(pairs) == 35 and len(named) == 1
        assert tuple(named[0][k] for k in ("n", "n_p", "n_q", "n_pq")) == (70, 9, 7, 7) and abs(named[0]["mlog10p"] - 7.5224) < 1e-3
    else:
        assert len(variants) == 8 and len(pairs) == 28 and not named
    rest = [l["mlog10p"] for l in pairs if not (l["p"] in planted and l["q"] in planted) and l not in named]
    assert len(rest) == len(pairs) - 3 - len(named) and max(rest) <= 1


def test_renderer():
    c = lr.planted_case(0)
    text = lr.render_linkage({1: (c["sel"][:0], np.zeros((0, 0), np.int32)), 0: (c["sel"], c["co"])}, 3)
    lines = text.splitlines()
    assert lines[0].split("\t") == ["dir", "row_a", "var_a", "count_a", "row_b", "var_b", "count_b", "n", "n_a", "n_b", "n_ab", "expected",
                                    "mlog10p"]
    assert len(lines) == 1 + 1 + 3 + 1 and lines[1] == "#right\tvariants=0\tpairs=0\tlinked=0" and lines[5] == "#left\tvariants=8\tpairs=28\tlinked=3"
    assert [(x.split("\t")[0], x.split("\t")[1], x.split("\t")[4]) for x in lines[2:5]] == [("left", "8", "30"), ("left", "8", "55"), ("left", "30", "55")]
    assert all(x.split("\t")[2] in "ACGT" and re.fullmatch(r"\d+\.\d{4}", x.split("\t")[12]) for x in lines[2:5])
    lr.same_linkage_text(text, text)
    with pytest.raises(AssertionError):
        lr.same_linkage_text(text, text.replace("\t30\t", "\t31\t", 1))
    with pytest.raises(AssertionError):
        lr.same_linkage_text(text, text.replace("variants=8", "variants=9"))
    with pytest.raises(AssertionError):
        lr.same_linkage_text(text, re.sub(r"(\d+\.\d{4})$", "1.0000", text.rstrip("\n").rsplit("\n", 2)[0]) + "\n" + "\n".join(lines[-1:]) + "\n")
