"""The CPU restatement of the per-copy statistics (tests/copystats_ref.py) on the shapes the GPU tests use, both directions,
along the kept and along a foreign consensus: the per-copy identity, the sums over the copies against the pileup of the same
consensus, the CpG columns in both row orders, and the two host C functions of libramx.so (ramx_copy_kimura,
ramx_family_divergence) against the Python formula.  The preconditions of the GPU tests are asserted here, on the reference's
side, so that no test passes on empty ground.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from repeatafterme_amd import _lib
from repeatafterme_amd.datamodel import COPY_STATS_DTYPE, COPY_STATS_FIELDS

import copystats_ref as cr
import test_gpu_pileup as tp
from helpers import ROOT

CASES = [(sh, d, what) for sh in tp.SHAPES for d in (1, 0) for what in ("kept", "foreign")]


def test_the_struct_is_48_bytes():
    assert COPY_STATS_DTYPE.itemsize == 48 and ctypes.sizeof(_lib.CopyStats) == 48
    assert COPY_STATS_DTYPE.names == COPY_STATS_FIELDS == ("cols", "match", "ts", "tv", "n_match", "del", "del_open", "ins", "ins_open",
                                                          "cpg_cols", "cpg_ts", "score")
    assert [COPY_STATS_DTYPE.fields[k][1] for k in COPY_STATS_FIELDS] == list(range(0, 48, 4))
    assert [n.rstrip("_") for n, _ in _lib.CopyStats._fields_] == list(COPY_STATS_FIELDS)


def test_header_declares_and_library_exports_the_entries():
    txt = open(os.path.join(ROOT, "include", "ramx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ramx_dev_copy_stats", "ramx_copy_kimura", "ramx_family_divergence", "ramx_set_copies_sink"):
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} is not declared in include/ramx.h"
        assert hasattr(lib, name), f"{name} is not exported by libramx.so"
        assert name in _lib.EXPORTS
    fields = re.search(r"typedef struct ramx_copy_stats\s*\{(.*?)\}", txt, flags=re.S).group(1)
    assert tuple(re.findall(r"int32_t\s+(\w+);", fields)) == COPY_STATS_FIELDS


def check_identity_and_sums(c, tag):
    st, cols, cons, results = c["stats"], c["cols"], c["cons"], c["results"]
    assert len(st) == len(results), tag
    # the per-copy identity, and what a copy without an alignment looks like
    assert np.array_equal(st["match"] + st["ts"] + st["tv"] + st["n_match"] + st["del"], st["cols"]), tag
    for s, res in zip(st, results):
        assert s["cols"] == res["end_row"] + 1 and s["score"] == res["score"], tag
        if res["end_row"] < 0:
            assert not np.frombuffer(s.tobytes(), np.uint8).any(), tag
        assert 0 <= s["del_open"] <= s["del"] and 0 <= s["ins_open"] <= s["ins"] and 0 <= s["cpg_ts"] <= min(s["cpg_cols"], s["ts"]), tag
        assert (s["del_open"] > 0) == (s["del"] > 0) and (s["ins_open"] > 0) == (s["ins"] > 0), tag
    # the sums over the copies against the pileup of the same consensus
    assert st["cols"].sum() == cols["cover"].sum(), tag
    assert st["del"].sum() == cols["del"].sum(), tag
    assert st["ins"].sum() == cols["ins_bases"].sum() and st["ins_open"].sum() == cols["ins_open"].sum(), tag
    assert (st["match"] + st["ts"] + st["tv"] + st["n_match"]).sum() == cols["match"].sum(), tag
    assert st["n_match"].sum() == cols["match"][:, 4].sum(), tag
    assert st["match"].sum() == sum(int(cols["match"][r, int(cons[r])]) for r in range(len(cons))), tag


@pytest.mark.parametrize("shape,direction,what", CASES)
def test_identity_and_sums_against_the_pileup(shape, direction, what):
    check_identity_and_sums(cr.shape_case(*shape, direction, what), f"{shape} dir={direction} {what}")


@pytest.mark.parametrize("shape", tp.SHAPES)
def test_preconditions_of_the_gpu_tests(shape):
    """What the GPU tests of these shapes rest on, counted on the restatement."""
    tot = {(d, what): {k: int(cr.shape_case(*shape, d, what)["stats"][k].sum()) for k in COPY_STATS_FIELDS}
           for d in (1, 0) for what in ("kept", "foreign")}
    none = {k: sum(r["end_row"] < 0 for r in cr.shape_case(*shape, *k)["results"]) for k in tot}
    tails = sum(r["tail_ins"] > 0 for k in tot for r in cr.shape_case(*shape, *k)["results"])
    assert tails == 0                                                  # these shapes do not hold one: TAIL_FAMILY does
    if shape[0] >= 37:
        for k, t in tot.items():
            assert all(t[f] > 0 for f in ("ts", "tv", "del", "ins", "ins_open")), (shape, k, t)
        assert any(t["del_open"] < t["del"] for t in tot.values())
        assert any(t["cpg_ts"] > 0 for t in tot.values())
        assert any(t["n_match"] > 0 for (d, _), t in tot.items() if d == 1)
    if shape[:3] == (37, 14, 60):
        assert (tot[(1, "foreign")]["del_open"], tot[(1, "foreign")]["del"]) == (52, 56)
    if shape[:3] == (64, 20, 60):
        assert none[(0, "foreign")] == 1
    if shape[:3] == (130, 40, 60):
        assert none[(1, "foreign")] == 2


@pytest.mark.parametrize("direction", [1, 0])
def test_inserted_bases_behind_the_last_column_are_counted_nowhere(direction):
    c = cr.tail_case(direction)
    tails = [r["tail_ins"] for r in c["results"]]
    assert sum(t > 0 for t in tails) >= 6                              # the family does hold such paths
    check_identity_and_sums(c, f"tail dir={direction}")
    for s, res in zip(c["stats"], c["results"]):                       # every consumed position: matched, inserted or the tail
        if res["end_row"] >= 0:
            matched = int(s["match"] + s["ts"] + s["tv"] + s["n_match"])
            assert matched + int(s["ins"]) + res["tail_ins"] == res["end_idx"] - res["start_idx"] + 1


def test_cpg_columns_in_both_row_orders():
    """CGACGTTCG read 5'->3': CG at the first two and at the last two columns, and one inside."""
    cons = np.array([1, 2, 0, 1, 2, 3, 3, 1, 2], np.int8)
    fwd = cr.cpg_columns(cons, False)
    assert fwd == [True, True, False, True, True, False, False, True, True]
    # the same rows read outward from the core (a left extension): reading order is GCTTGCAGC, and no column is in a CpG but
    # where a C is followed, in reading order, by a G -- here nowhere
    assert cr.cpg_columns(cons, True) == [False] * 9
    # the left extension of that sequence: rows are the reading order reversed
    rev = cr.cpg_columns(cons[::-1].copy(), True)
    assert rev == fwd[::-1]
    # a lone C at the last column, a lone G at the first: the neighbour that would complete them does not exist
    assert cr.cpg_columns(np.array([2, 0, 1], np.int8), False) == [False, False, False]
    assert cr.cpg_columns(np.array([1, 0, 2], np.int8), True) == [False, False, False]
    assert cr.cpg_columns(np.array([1], np.int8), False) == [False] and cr.cpg_columns(np.zeros(0, np.int8), True) == []


def test_cpg_counters_follow_the_row_order():
    """The same walks counted in both row orders: only the CpG counters move, and they do move."""
    sh = tp.SHAPES[1]
    c = cr.shape_case(*sh, 1, "foreign")
    a = cr.stats_of(1, c["fs"].cores, c["idx"], c["results"], c["seq"], sh[1], c["cons"], False)
    b = cr.stats_of(1, c["fs"].cores, c["idx"], c["results"], c["seq"], sh[1], c["cons"], True)
    assert np.array_equal(a, c["stats"])
    for k in COPY_STATS_FIELDS:
        assert np.array_equal(a[k], b[k]) == (k not in ("cpg_cols", "cpg_ts")), k


def rec(**kw):
    s = np.zeros(1, COPY_STATS_DTYPE)
    for k, v in kw.items():
        s[k] = v
    return s


EDGE = [rec(), rec(n_match=5, cols=7, **{"del": 2}),                                   # sites = 0
        rec(match=10, ts=10), rec(ts=1, tv=1), rec(ts=3),                              # a <= 0 (a = 0, a < 0)
        rec(match=10, tv=10), rec(tv=4), rec(match=1, tv=3),                           # b <= 0 (b = 0, b < 0)
        rec(match=100), rec(match=90, ts=7, tv=3), rec(match=1), rec(match=2, ts=0, tv=1), rec(match=2 ** 31 - 1, ts=1)]


def test_kimura_of_the_library_is_the_formula():
    from repeatafterme_amd.device import copy_kimura
    recs = list(EDGE) + [cr.shape_case(*sh, d, what)["stats"][i:i + 1] for sh, d, what in CASES[4:] for i in (0, 17, 36)]
    defined = 0
    for s in recs:
        want, got = cr.kimura(s[0]), copy_kimura(s)
        if want is None:
            assert got == -1.0, s
        else:
            assert got >= 0 and abs(got - want) <= 1e-9, (s, got, want)
            defined += 1
    assert [cr.kimura(s[0]) is None for s in EDGE] == [True] * 8 + [False] * 5 and defined > 50
    assert cr.kimura(EDGE[8][0]) == 0.0 and math.copysign(1, cr.kimura(EDGE[8][0])) == 1 == math.copysign(1, copy_kimura(EDGE[8]))
    assert abs(cr.kimura(EDGE[9][0]) - (-0.5 * math.log(0.83 * math.sqrt(0.94)) * 100)) < 1e-9


def test_family_divergence_of_the_library_is_the_formula():
    from repeatafterme_amd.device import family_divergence_of
    edge = np.concatenate(EDGE)
    sets = [edge, edge[:2], edge[:0]] + [cr.shape_case(*sh, d, what)["stats"] for sh, d, what in CASES]
    for st in sets:
        for min_sites in (-3, 0, 1, 2, 4, 25, 101, 10 ** 6):
            want, used = cr.family_divergence(st, min_sites)
            got, got_used = family_divergence_of(st, min_sites)
            assert got_used == used and abs(got - want) <= 1e-9, (min_sites, got, want)
    # the cut: match=1 and (2, 0, 1) have 1 and 3 sites
    assert family_divergence_of(edge, 1)[1] == 5 and family_divergence_of(edge, 2)[1] == 4 and family_divergence_of(edge, 4)[1] == 3
    assert family_divergence_of(edge[:2], 1) == (0.0, 0) and family_divergence_of(edge[:0]) == (0.0, 0)
    assert family_divergence_of(edge, 0) == family_divergence_of(edge, 1) == family_divergence_of(edge, -3)


def test_renderer():
    c = cr.shape_case(*tp.SHAPES[1], 1, "foreign")
    names = [f"s{n}:1-2_+" for n in range(c["fs"].cores.n)]
    text = cr.render_copies({1: (names, c["idx"], c["results"], c["stats"]), 0: (names, c["idx"][:2], c["results"][:2], c["stats"][:2])})
    lines = text.splitlines()
    assert lines[0].split("\t") == ["dir", "copy", "end_row", "start", "end", "score", "cols", "match", "ts", "tv", "n", "del", "del_open",
                                    "ins", "ins_open", "cpg_cols", "cpg_ts", "kimura"]
    n = len(c["idx"])
    assert len(lines) == 1 + n + 1 + 2 + 1 and all(len(x.split("\t")) == 18 for x in lines[1:n + 1])
    div, used = cr.family_divergence(c["stats"])
    assert lines[n + 1] == f"#right\tcopies={n}\tused={used}\tkimura={div:.4f}" and lines[-1].startswith("#left\tcopies=2\t")
    cr.same_copies_text(text, text)
    with pytest.raises(AssertionError):
        cr.same_copies_text(text, text.replace("\t52\t", "\t53\t", 1) if "\t52\t" in text else text + "x\n")
    assert cr.render_block(1, names, [0], [dict(end_row=-1, start_idx=0, end_idx=-1)], np.zeros(1, COPY_STATS_DTYPE)).splitlines()[0].endswith("\tNA")
