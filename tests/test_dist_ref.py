"""The contract of include/ramx_dist.h on the CPU: the restatement of tests/dist_ref.py on hand-made paths with a literal record
for every rule, its identities against the pileup and the per-copy statistics on the shared families, and the three host
functions of the library (ramx_select_copies, ramx_dist_kimura, ramx_dist_summary) through ctypes against the restatement."""
import math

import numpy as np
import pytest

from repeatafterme_amd.datamodel import ALN_END_DTYPE, COPY_DIST_DTYPE, COPY_DIST_FIELDS, CoreSet

import dist_ref as dr
import linkage_ref as lr
import test_gpu_pileup as tp

A, C_, G, T, N = 0, 1, 2, 3, 99
W = 5


def hand_family(bases):
    """One forward-strand core per list of bases: copy i reads bases[i][t] at flank position t of a right extension.  -> (cores,
    sequence); every copy has 100 positions of its own."""
    n = len(bases)
    seq = np.full(100 * n + 100, N, np.int8)
    pos = np.array([100 * i + 9 for i in range(n)], np.int64)
    for i, b in enumerate(bases):
        seq[100 * i + 10:100 * i + 10 + len(b)] = b
    cores = CoreSet(pos - 5, pos, np.array([100 * i for i in range(n)], np.int64), np.array([100 * i + 99 for i in range(n)], np.int64),
                    *(np.zeros(n, np.int8) for _ in range(3)))
    return cores, seq


def path(text):
    """"M D M I M" -> a walk() result: rows in order for M and D, flank positions in order for M and I."""
    ops, row, t = [], 0, 0
    for x in text.split():
        if x == "I":
            ops.append(("I", t)); t += 1
        elif x == "M":
            ops.append(("M", row, t)); row += 1; t += 1
        else:
            ops.append(("D", row)); row += 1
    tail = 0
    for op in reversed(ops):
        if op[0] != "I":
            break
        tail += 1
    return dict(end_row=row - 1, ops=ops, tail_ins=tail)


NO_ALIGNMENT = dict(end_row=-1, ops=[], tail_ins=0)


def records(bases, paths, rows):
    cores, seq = hand_family(bases)
    maps = dr.maps_of(1, cores, list(range(len(bases))), paths, seq, W, np.zeros(rows, np.int8))
    return maps, dr.matrix(maps, range(len(bases)))


def rec(m, a, b):
    return tuple(int(m[a, b][f]) for f in COPY_DIST_FIELDS)          # cover, sites, ts, tv, del_one, del_both


def test_a_literal_record_for_every_rule():
    bases = [[A, C_, G, T, A, C_],        # 0: six bases
             [A, N, G, T, A, C_],         # 1: N at row 1
             [A, C_, T, A],               # 2: row 2 deleted (reads A C . T A . -> rows 0 1 3 4), ends at row 4
             [A, T, A, C_],               # 3: rows 1 and 2 deleted
             [G, T, A],                   # 4: ends at row 2
             [A, C_, G, T, A, C_]]        # 5: no alignment
    paths = [path("M M M M M M"), path("M M M M M M"), path("M M D M M"), path("M D D M M M"), path("M M M"), NO_ALIGNMENT]
    maps, m = records(bases, paths, 6)
    assert maps[2] == {0: A, 1: C_, 2: 5, 3: T, 4: A} and maps[3] == {0: A, 1: 5, 2: 5, 3: T, 4: A, 5: C_} and maps[5] == {}
    assert rec(m, 0, 1) == (6, 5, 0, 0, 0, 0)         # N against a base: cover but not sites
    assert rec(m, 0, 2) == (5, 4, 0, 0, 1, 0)         # deleted against a base: del_one; rows above copy 2's end_row count nowhere
    assert rec(m, 1, 3) == (6, 4, 0, 0, 2, 0)         # deleted against N (row 1) and against a base (row 2): del_one both times
    assert rec(m, 2, 3) == (5, 3, 0, 0, 1, 1)         # row 2 deleted in both; row 1 in one
    assert rec(m, 0, 4) == (3, 3, 3, 0, 0, 0)         # rows above copy 4's end_row count nowhere; A/G, C/T and G/A: three transitions
    assert rec(m, 2, 4) == (3, 2, 2, 0, 1, 0)
    assert rec(m, 0, 5) == rec(m, 5, 5) == (0, 0, 0, 0, 0, 0)      # a copy without an alignment
    # the diagonal: a copy with itself
    assert rec(m, 0, 0) == (6, 6, 0, 0, 0, 0) and rec(m, 1, 1) == (6, 5, 0, 0, 0, 0) and rec(m, 3, 3) == (6, 4, 0, 0, 0, 2)
    for f in COPY_DIST_FIELDS:
        assert np.array_equal(m[f], m[f].T)


def test_each_ordered_base_pair_is_a_transition_or_a_transversion():
    ts = {(A, G), (G, A), (C_, T), (T, C_)}
    for x in (A, C_, G, T):
        for y in (A, C_, G, T):
            maps, m = records([[x], [y]], [path("M"), path("M")], 1)
            want = (1, 1, 0, 0, 0, 0) if x == y else (1, 1, 1, 0, 0, 0) if (x, y) in ts else (1, 1, 0, 1, 0, 0)
            assert rec(m, 0, 1) == rec(m, 1, 0) == want, (x, y)
    # lower-case codes 4..7 are the same bases
    maps, m = records([[A + 4], [G]], [path("M"), path("M")], 1)
    assert rec(m, 0, 1) == (1, 1, 1, 0, 0, 0)


def test_inserted_bases_and_tail_insertions_change_nothing():
    plain = records([[A, C_, G, T], [A, T, G, A]], [path("M M M M"), path("M M M M")], 4)[1]
    # copy 1 reads T G inserted between rows 0 and 1 and two more bases behind its last row
    ins = records([[A, C_, G, T], [A, T, G, T, G, A, C_, C_]], [path("M M M M"), path("M I I M M M I I")], 4)[1]
    assert rec(plain, 0, 1) == rec(ins, 0, 1) == (4, 4, 1, 1, 0, 0)        # C/T at row 1, T/A at row 3
    assert rec(ins, 1, 1) == (4, 4, 0, 0, 0, 0)


def test_rows_behind_the_consensus_are_cut():
    maps, m = records([[A, C_, G, T], [A, C_, G, T]], [path("M M M M"), path("M M M M")], 2)
    assert rec(m, 0, 1) == (2, 2, 0, 0, 0, 0)


CASES = [(sh, d, what) for sh in tp.SHAPES[1:5] for d in (1, 0) for what in ("kept", "foreign")]


def comb2(x):
    x = np.asarray(x, np.int64)
    return x * (x - 1) // 2


@pytest.mark.parametrize("sh,direction,what", CASES)
def test_identities_against_the_pileup_and_the_copy_statistics(sh, direction, what):
    c = dr.shape_case(*sh, direction, what)
    m, cols, stats = c["dist"], c["cols"], c["stats"]
    iu = np.triu_indices(len(m), 1)
    up = {f: int(m[f][iu].astype(np.int64).sum()) for f in COPY_DIST_FIELDS}
    mt = cols["match"].astype(np.int64)
    assert up["sites"] == int(comb2(mt[:, :4].sum(axis=1)).sum())
    assert up["sites"] - up["ts"] - up["tv"] == int(comb2(mt[:, :4]).sum())
    assert up["ts"] == int((mt[:, 0] * mt[:, 2] + mt[:, 1] * mt[:, 3]).sum())
    assert up["del_both"] == int(comb2(cols["del"]).sum())
    dg = m[np.arange(len(m)), np.arange(len(m))]
    assert np.array_equal(dg["cover"], stats["cols"]) and np.array_equal(dg["sites"], stats["match"] + stats["ts"] + stats["tv"])
    assert np.array_equal(dg["del_both"], stats["del"]) and not (dg["ts"] | dg["tv"] | dg["del_one"]).any()
    assert np.array_equal(dr.matrix_of_one_word(c["maps"], range(len(m)), len(c["cons"])), m)      # the second restatement agrees
    # the planes of the linkage restatement say the same of one pair
    pl, a, b = lr.shape_case(*sh, direction, what)["planes"], 0, len(m) - 1
    both = lambda r, k: (pl[(r, k)] >> a) & (pl[(r, k)] >> b) & 1
    assert int(m[a, b]["cover"]) == sum(both(r, 6) for r in range(len(c["cons"])))
    assert int(m[a, b]["del_both"]) == sum(both(r, 5) for r in range(len(c["cons"])))


def ends_of(end_rows):
    e = np.zeros(len(end_rows), ALN_END_DTYPE)
    e["end_row"] = end_rows
    return e


def test_select_copies_of_the_library_is_the_restatement():
    from repeatafterme_amd.device import select_copies
    rng = np.random.default_rng(5)
    sets = [[9, 9, 4, -1, 9, 4, 20], [], [-1, -1], [0], [3] * 10, list(rng.integers(-1, 40, 300)), [7] * 2100]
    for er in sets:
        for rows in (0, 1, 10, 30):
            for min_cols in (-2, 0, 1, 5, 10, 11, 41):
                for cap in (-1, 0, 1, 2, 3, 5, 256, 2048, 5000):
                    got = select_copies(ends_of(er), rows, min_cols, cap)
                    assert list(got) == dr.select([int(x) for x in er], rows, min_cols, cap), (er[:8], rows, min_cols, cap)
    assert list(select_copies(ends_of(sets[0]), 10, 0, 3)) == [0, 1, 4]                    # ties go to the lower index
    assert list(select_copies(ends_of(sets[0]), 10, 0, 5)) == [0, 1, 2, 4, 6]              # ... also at the shorter length
    assert len(select_copies(ends_of(sets[6]), 10, 1, 5000)) == 2048                       # the clamp


EDGE = [(0, 0, 0), (10, 5, 0), (10, 0, 5), (10, 4, 2), (10, 0, 6), (100, 0, 0), (100, 10, 5), (100, 1, 0), (7, 1, 1), (2 ** 30, 3, 4)]


def one(sites, ts, tv):
    r = np.zeros(1, COPY_DIST_DTYPE)
    r["cover"], r["sites"], r["ts"], r["tv"] = sites, sites, ts, tv
    return r


def test_kimura_of_the_library_is_the_formula():
    from repeatafterme_amd.device import dist_kimura
    recs = [one(*e) for e in EDGE] + [dr.shape_case(*sh, d, what)["dist"][i, j:j + 1] for sh, d, what in CASES[:4] for i, j in ((0, 1), (5, 30), (36, 2))]
    defined = 0
    for s in recs:
        want, got = dr.kimura(s[0]), dist_kimura(s)
        if want is None:
            assert got == -1.0, s
        else:
            assert got >= 0 and abs(got - want) <= 1e-9, (s, got, want)
            defined += 1
    assert [dr.kimura(one(*e)[0]) is None for e in EDGE] == [True] * 5 + [False] * 5 and defined > 10
    assert dr.kimura(one(100, 0, 0)[0]) == 0.0 and math.copysign(1, dist_kimura(one(100, 0, 0))) == 1
    assert abs(dr.kimura(one(100, 10, 5)[0]) - (-0.5 * math.log(0.75 * math.sqrt(0.9)) * 100)) < 1e-9


def same_summary(m, min_sites):
    from repeatafterme_amd.device import dist_summary
    s, w = dist_summary(m, min_sites), dr.summary(m, min_sites)
    assert (s.n, s.pairs, s.used, s.medoid) == (w["n"], w["pairs"], w["used"], w["medoid"]), (min_sites, s, w)
    assert abs(s.mean - w["mean"]) <= 1e-9 and abs(s.medoid_mean - w["medoid_mean"]) <= 1e-9
    return s


def square(n, ts_of):
    m = np.zeros((n, n), COPY_DIST_DTYPE)
    for a in range(n):
        for b in range(n):
            m[a, b] = (100, 100, 0 if a == b else ts_of(min(a, b), max(a, b)), 0, 0, 0)
    return m


def test_summary_of_the_library_is_the_restatement():
    for n in (0, 1, 2):
        s = same_summary(square(n, lambda a, b: 10), 1)
        assert (s.pairs, s.used, s.medoid) == ((0, 0, -1) if n < 2 else (1, 1, 0))
    s = same_summary(square(4, lambda a, b: 50), 1)                       # all pairs undefined
    assert s.used == 0 and s.medoid == -1 and s.mean == 0.0 and s.medoid_mean == 0.0
    s = same_summary(square(4, lambda a, b: 10), 1)                       # a medoid tie: the lowest
    assert s.used == 6 and s.medoid == 0
    s = same_summary(square(4, lambda a, b: 5 if 3 in (a, b) else 20), 1)
    assert s.medoid == 3
    s = same_summary(square(4, lambda a, b: 5 if (a, b) == (1, 2) else 50), 1)     # one used pair: its first copy
    assert s.used == 1 and s.medoid == 1
    for sh, d, what in CASES[:6]:
        m = dr.shape_case(*sh, d, what)["dist"]
        for min_sites in (-3, 0, 1, 20, 40, 10 ** 6):
            same_summary(m, min_sites)
    assert same_summary(dr.shape_case(*CASES[0][0], *CASES[0][1:])["dist"], 10 ** 6).used == 0


def test_the_text_round_trips():
    c = dr.shape_case(*CASES[0][0], *CASES[0][1:])
    sel = dr.select([r["end_row"] for r in c["results"]], len(c["cons"]), 20, 12)
    m = dr.matrix(c["maps"], sel)
    names = {n: f"copy{n}" for n in c["idx"]}
    ci = np.asarray(c["idx"])
    text = dr.render_dist({1: (ci, sel, m), 0: (ci[::-1], sel, m)}, names, 20)
    got = dr.parse_dist(text)
    assert set(got) == {"right", "left", "both"} and len(got["right"][0]) == len(sel) * (len(sel) - 1) // 2
    assert got["right"][1]["selected"] == str(len(sel)) and got["right"][1]["copies"] == str(len(ci))
    a, b, r, k = got["right"][0][0]
    assert (a, b) == (names[c["idx"][sel[0]]], names[c["idx"][sel[1]]]) and r == rec(m, 0, 1)
    dr.same_dist_text(text, text)
    with pytest.raises(AssertionError):
        dr.same_dist_text(text, text.replace("\t" + str(r[0]) + "\t", "\t" + str(r[0] + 1) + "\t", 1))
