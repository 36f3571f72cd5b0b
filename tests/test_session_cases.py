"""The inputs of tests/test_gpu_session_reuse.py (tests/session_cases.py) against the list of things they are there for, counted
on the oracle and the restatements alone: SMALL is smaller than BIG in every extent a device buffer is sized or strided by, it
holds the corners a stale buffer would show in, none of its expected results is trivial, and BIG's numbers are not SMALL's.
No GPU."""
import numpy as np

import session_cases as sc
import subfam_ref as sr
import window_ref as wr


def test_small_is_smaller_than_big_in_every_extent():
    b, s = sc.extents(sc.big(), sc.BIG_W, sc.BIG_L), sc.extents(sc.small(), sc.SMALL_W, sc.SMALL_L)
    assert set(b) == set(s)
    for k in b:
        assert 0 < s[k] < b[k], (k, s[k], b[k])
    # the names the buffers go by: flanks and tiles, rows, L, window words, stream words, families, planes, variants, sites
    assert set(b) >= {"padded_flanks", "tiles", "maxrows", "L", "KW", "term_SW", "period_SW", "families", "planes", "variants", "sites"}
    assert (b["KW"], s["KW"]) == (wr.window_words(300, 40), wr.window_words(30, 5)) == (59, 17)
    # BIG runs past one block row of the sum kernels (256 columns) and past one tile group of lanes
    big = sc.big()
    assert big.loop[1].rows_executed > 256 and big.rows[0] > 256 and big.fams[0][1].n % 64 != 0
    lw = {w: sc.extents_of_loop(w) for w in ("big", "small")}
    for k in lw["big"]:
        assert 0 < lw["small"][k] < lw["big"][k], k


def test_small_holds_the_corners():
    s = sc.small()
    flanks, first, count = sc.small_layout()
    arr, npad = flanks
    assert (npad, first, count, s.rows) == (256, [0, 192, 192], [70, 0, 3], [28, 0, 17])
    owner = np.full(npad // 64, -1)
    for f in range(3):
        owner[first[f] // 64:first[f] // 64 + (count[f] + 63) // 64] = f
    assert list(owner) == [0, 0, -1, 2]                                             # the tile of no family lies between families
    assert count[1] == 0 and s.rows[1] == 0                                          # the family without flanks runs no row
    assert len(set(s.rows)) == 3 and min(r for r in s.rows if r) < max(s.rows)       # rows beyond a family's count exist
    empty = [arr[i].t_lo > arr[i].t_hi for i in range(npad)]
    assert all(empty[70:192]) and all(empty[195:]) and not all(empty[:70]) and not all(empty[192:195])      # padding lanes, the hole
    # copies end at several rows, some before the consensus' last, and some have no alignment at all
    t = sc.small_truth()
    ends = sorted({int(r["end_row"]) for r in t["walks"][0][1]})
    assert ends[0] == -1 and len(ends) >= 8 and ends[-1] < s.rows[0] - 1
    # the sites: one of length 0, one from in front of the library, one to behind it; window lengths off the word sizes
    lo, hi = s.sites["lo"], s.sites["hi"]
    assert lo[0] == hi[0] + 1 and lo[1] < 0 and hi[2] >= len(s.lib)
    T = [int((h + 1 - l) // 2) for l, h in zip(lo, hi)]
    assert T == [0, 27, 21] and all(v % 8 and v % 32 for v in T[1:])
    words, bounds = sc.small_windows()
    assert words.shape == (17, 256) and (words[:, 70:192] == wr.PAD_WORD).all() and (words[:, :70] != wr.PAD_WORD).any()


def test_small_expectations_are_not_trivial():
    s, t = sc.small(), sc.small_truth()
    for f in (0, 2):
        cols, di = t["cols"][f], t["di"][f]
        assert cols["cover"].sum() > 0 and cols["del"].sum() > 0 and cols["ins_open"].sum() > 0, f
        assert di["adjacent"].sum() > 0 and di["di"].sum() > 0, f
        total, counts, row_best, row_idx, last = t["profile"][f]
        assert total.any() and row_best.any() and (last >= 0).any(), f
        assert t["stats"][f]["cols"].sum() > 0 and t["stats"][f]["match"].sum() > 0, f
        planes, gram = t["planes"][f], t["gram"][f]
        assert len(sr.variants_of(planes)[0]) >= 1 and None not in sr.variants_of(planes)[1], f
        off = gram - np.diag(np.diag(gram))
        assert off.any(), f                                                          # a pair of planes with a common copy
    assert t["profile"][0][1][:, 0].max() > 0                                        # capped flanks occur
    assert not np.array_equal(t["stats"][0], t["stats_reversed"][0])                 # the row order shows in the CpG counters
    assert (t["subfam"][0]["size"] > 0).sum() >= 2 and t["subfam"][0]["iterations"] > 1
    cons, cols, replays, conv = t["refine"][0]
    assert replays > 1 and not np.array_equal(cons, s.cons[0, :s.rows[0]])           # the refinement moves the consensus
    assert t["refine_cpg"][0][3] > 1 and t["refine_cpg"][0][5] > 0                   # ... and the CpG-aware one calls sites
    # every site-window analysis finds a record and misses one
    assert [r[0] > 0 for r in t["tsd"]] == [True, False, False]
    assert [r[0] > 0 for r in t["period"]] == [False, True, False]
    assert [(d[0] > 0, v[0] > 0) for d, v in t["term"]] == [(False, False), (True, False), (False, True)]


def test_big_is_not_small():
    """What BIG leaves in the leading rows and columns of a buffer is not what SMALL is to find there (BIG's side from the
    oracle's loop alone)."""
    b, s, t = sc.big(), sc.small(), sc.small_truth()
    o = b.loop[1]
    rows = s.rows[0]
    total, counts, row_best, row_idx, last = t["profile"][0]
    assert not np.array_equal(o.col_base[:rows], s.cons[0, :rows]) and not np.array_equal(b.cons[0, :rows], s.cons[0, :rows])
    assert (o.col_sums[:rows] != total).any(axis=1).all()                            # every leading column's totals
    assert (o.row_best[:rows, :70] != row_best).mean() > 0.9 and (o.row_best[:rows, :70] != 0).mean() > 0.9
    assert o.rows_executed > rows and (o.row_best[rows:s.rows[0] + 8, :256] != 0).any()      # behind SMALL's rows: not 0 either
    # BIG's first tiles hold flanks where SMALL has padding lanes and its tile of no family
    assert b.fams[0][1].n >= 256
    # the libraries and the sites are others
    assert not np.array_equal(b.lib[:len(s.lib)], s.lib)
    assert (b.sites["hi"] + 1 - b.sites["lo"]).max() > 2000 and (b.sites["hi"] + 1 - b.sites["lo"])[:3].tolist() != [0, 55, 42]


def test_loop_worlds():
    big, small = sc.loop_world("big"), sc.loop_world("small")
    assert big.o.rows_executed > small.o.rows_executed > 10 and big.o.ret > 0 and small.o.ret > 0
    assert not np.array_equal(big.o.col_base[:small.o.rows_executed], small.o.col_base[:small.o.rows_executed])
