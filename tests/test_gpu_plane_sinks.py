"""The three sinks of seam 1 that answer from the resident planes (linkage, subfamilies, distance) through both of their callers,
as tests/test_gpu_sink_paths.py does for the first five and with its helpers: the same families run one at a time through
extend_alignment and together through extend_batch, both directions, the three sinks set at once.  Every record the batch hands
over is the single call's, byte for byte; the split of the ordinary families is the restatement's (tests/subfam_ref.py); the
corners are literal.

Six planted families (tests/linkage_ref.py: bandwidth 20, L = 80, matrix 14p43g, when_to_stop = 30), in this order in the batch.
The restatement runs along the consensus the loop keeps on the library with the variants planted (the oracle's).  That is
linkage_ref.planted_case for families 0 and 5; where every second flank is planted the loop keeps the planted base at some of the
columns (half the flanks carry each), so planted_case, which walks along the consensus of the family as generated, is not what a
sink can return for families 2, 3 and 4.  Both tables are below and a CPU test asserts them: PLANTED_TABLE, planted_case's, and
TABLE, the kept consensus', which says what the subfamily sink's per-K calls have to keep apart: to the right families 0 and 5
have three patterns and share a call with everything else between them, 3 and 4 share the call for one; to the left families 0,
4 and 5 have two.
  0: 70 flanks, columns (8, 30, 55) of every third     the planted family of the other tests
  1: family 0 with no core extendable in either direction
  2: 50 flanks, columns (12, 40) of every second        shares K with family 0 in both directions; other V and P
  3: 40 flanks, columns (20, 50) of every second        the other K in each direction
  4: 64 flanks, column 20 of every second               exactly one tile; variants but one pattern to the right
  5: 130 flanks, columns (5, 33, 60) of every fourth    three tiles, the last uneven"""
import dataclasses
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import new_master

import linkage_ref as lr
import pileup_ref as pr
import subfam_ref as sr
from helpers import to_extend_params
from test_gpu_sink_paths import HUGE_MINIMPROVEMENT, all_none, assert_same_record

gpu = pytest.mark.gpu

W, L, MATRIX, STOP = 20, 80, "14p43g", 30
# (synth spec (n, L, W, K, seed), planted columns, every); None: family 0 without an extendable core
SPECS = (((70, L, W, 70, 7), (8, 30, 55), 3), None, ((50, L, W, 70, 11), (12, 40), 2), ((40, L, W, 70, 24), (20, 50), 2),
         ((64, L, W, 70, 31), (20,), 2), ((130, L, W, 70, 13), (5, 33, 60), 4))
EMPTY = 1
PLANTED = (0, 2, 3, 4, 5)
SELECT = (4, 100, 1024)                      # linkage: min_count, min_permille, max_variants
MIN_MEMBERS = 6
SUBFAM = SELECT + (3.0, 4, 8, MIN_MEMBERS, 10)   # ... min_mlog10p, K, max_iter, min_members, max_replays
DISTS = ((1, 256), (20, 40))                 # the default, and one that cuts families 0 and 5 to 40 copies
SINKS = ("linkage", "subfam", "dist")
# "nothing kept" as in test_gpu_sink_paths.py: 130 flanks times an entry below 100 stays far under 10**6, and 81 * 10**6 fits an
# int32
KINDS = {"ordinary": dict(when_to_stop=STOP), "nothing_kept": dict(when_to_stop=STOP, minimprovement=HUGE_MINIMPROVEMENT)}
# {family: ((right: P, V, K, sizes, iterations), (left: the same))} of the restatement at SELECT, score 3, cap 4, along
# planted_case's consensus.  Two assignments everywhere but in family 4: one pattern ends with the first (include/ramx.h), and
# its left split takes three
PLANTED_TABLE = {0: ((17, 9, 3, [40, 25, 5], 2), (16, 8, 2, [44, 26], 2)),
         2: ((21, 11, 3, [27, 5, 18], 2), (30, 15, 2, [34, 16], 2)),
         3: ((22, 12, 2, [27, 13], 2), (26, 13, 3, [17, 8, 15], 2)),
         4: ((6, 3, 1, [64], 1), (6, 3, 2, [55, 9], 3)),
         5: ((10, 5, 3, [85, 32, 13], 2), (10, 5, 2, [95, 35], 2))}
# the same along the consensus the loop keeps, and the columns at which that differs from planted_case's
TABLE = {0: ((17, 9, 3, [40, 25, 5], 2), (16, 8, 2, [44, 26], 2)),
         2: ((19, 10, 2, [45, 5], 2), (30, 15, 1, [50], 1)),
         3: ((21, 11, 1, [40], 1), (26, 13, 3, [21, 8, 11], 2)),
         4: ((7, 4, 1, [64], 1), (6, 3, 2, [57, 7], 2)),
         5: ((10, 5, 3, [85, 32, 13], 2), (10, 5, 2, [95, 35], 2))}
MOVED = {0: [], 2: [40], 3: [20, 50], 4: [20], 5: []}
# with 9 members a group of family 3's left split is dropped from the middle: its kept groups are 0 and 2
GAP_MEMBERS, GAP_FAMILY = 9, 3


def planted_args(f):
    (spec, columns, every) = SPECS[f]
    return (spec, MATRIX, STOP), columns, every


@functools.lru_cache(maxsize=None)
def families():
    """-> [(cores, sequence)]; nobody writes to either"""
    out = []
    for f, s in enumerate(SPECS):
        fs, seq, _, _, _ = lr.planted_family(*planted_args(0 if s is None else f))
        cores = fs.cores.copy()
        if s is None:
            cores.left_ext[:] = 0
            cores.right_ext[:] = 0
        out.append((cores, seq))
    return out


def n_flanks(f, direction):
    c = families()[f][0]
    return int((c.right_ext if direction else c.left_ext).sum())


def params(kind):
    return po.Params.named(MATRIX, bandwidth=W, L=L, **KINDS[kind])


def split(c):
    linked = [(l["p"], l["q"]) for l in lr.link_pairs(c["sel"], c["co"], SUBFAM[3])]
    init, _ = sr.components(c["sel"], linked, SUBFAM[4])
    return sr.iterate(c["planes"], c["sel"], init, len(c["idx"]), SUBFAM[5])


@functools.lru_cache(maxsize=None)
def restated(f, direction):
    """-> (family f walked along the consensus the oracle keeps on its planted library: cons, idx, planes, sel, co as in
    lr.planted_case; what sr.iterate makes of it), on the CPU"""
    fs, seq, p, _, _ = lr.planted_family(*planted_args(f))
    o = po.oracle_extend(direction, fs.cores.copy(), seq, new_master(L), p, trace=True)
    cons = o.col_base[:o.ret].copy()
    cols, idx, results = pr.pileup(direction, fs.cores, seq, p, cons, with_walks=True)
    pl = lr.planes_of(direction, fs.cores, idx, results, seq, W, cons)
    sel = lr.select(cons, cols, *SELECT)
    c = dict(cons=cons, idx=idx, planes=pl, sel=sel, co=lr.gram(pl, sel))
    return c, split(c)


def same_as_table(c, res, row, where):
    P, V, K, sizes, iterations = row
    assert len(c["cons"]) == 70, where
    assert (len(c["sel"]), len(sr.variants_of(c["sel"])[0]), res["patterns"].shape) == (P, V, (V, K)), where
    assert res["size"].tolist() == sizes and (res["iterations"], res["converged"]) == (iterations, 1), where


def test_the_restatement_sees_the_cases():
    """On the CPU: both tables are what the restatement gives, every case keeps 70 columns and converges, and the kept consensus
    is planted_case's but at the columns of MOVED, all of them planted ones.  Along the kept consensus, in each direction 1, 2
    and 3 patterns all occur and a number of at least 2 is shared by families with different V and P, with the family without a
    flank between the first two of them: by two to the right, where 1 is shared as well, by three to the left.  With MIN_MEMBERS the last
    group of families 0 and 2 is dropped to the right; with GAP_MEMBERS the middle one of family 3 to the left."""
    for f in PLANTED:
        for k, direction in enumerate((1, 0)):
            pc = lr.planted_case(direction, *planted_args(f))
            same_as_table(pc, split(pc), PLANTED_TABLE[f][k], ("planted_case", f, direction))
            c, res = restated(f, direction)
            same_as_table(c, res, TABLE[f][k], (f, direction))
            assert len(c["idx"]) == SPECS[f][0][0] == n_flanks(f, direction) and c["idx"] == pc["idx"], (f, direction)
            assert [r for r in range(70) if c["cons"][r] != pc["cons"][r]] == MOVED[f] and set(MOVED[f]) <= set(SPECS[f][1]), (f, direction)
            if not MOVED[f]:
                assert np.array_equal(c["sel"], pc["sel"]) and np.array_equal(c["co"], pc["co"]) and c["planes"] == pc["planes"]
    for k in range(2):
        Ks = {f: TABLE[f][k][2] for f in PLANTED}
        assert set(Ks.values()) == {1, 2, 3}
        shared = [K for K in (1, 2, 3) if sum(x == K for x in Ks.values()) >= 2]
        assert len(shared) == (2, 1)[k] and max(shared) >= 2, Ks
        for K in shared:
            sharers = [f for f in PLANTED if Ks[f] == K]
            assert len({TABLE[f][k][0] for f in sharers}) == len({TABLE[f][k][1] for f in sharers}) == len(sharers)
        sharers = [f for f in PLANTED if Ks[f] == max(shared)]
        assert sharers[0] < EMPTY < sharers[1] and len(sharers) == (2, 3)[k], Ks
    kept = lambda f, k, m: [g for g, s in enumerate(TABLE[f][k][3]) if s >= m]
    assert kept(0, 0, MIN_MEMBERS) == [0, 1] and kept(2, 0, MIN_MEMBERS) == [0] and kept(5, 0, MIN_MEMBERS) == [0, 1, 2]
    assert kept(GAP_FAMILY, 1, GAP_MEMBERS) == [0, 2] and kept(4, 1, GAP_MEMBERS) == [0]


@dataclasses.dataclass
class Run:
    infos: list            # [family][k]
    recs: list             # [family][k] {sink: record}


@functools.lru_cache(maxsize=None)
def single(kind, select):
    from repeatafterme_amd.extend import extend_alignment
    ep = to_extend_params(params(kind))
    run = Run([], [])
    for cores, seq in families():
        res = [extend_alignment(d, cores.copy(), seq, new_master(L), ep, linkage=SELECT, subfam=SUBFAM, dist=select) for d in (1, 0)]
        run.infos.append([r[0] for r in res])
        run.recs.append([dict(zip(SINKS, r[1:])) for r in res])
    return run


def batch_call(direction, kind, **sinks):
    """extend_batch over the six families as generated -> (infos, {sink: [record per family]})"""
    from repeatafterme_amd.extend import extend_batch
    res = extend_batch(direction, [(c.copy(), seq, new_master(L)) for c, seq in families()], to_extend_params(params(kind)), **sinks)
    return res[0], dict(zip([s for s in SINKS if s in sinks], res[1:]))


@functools.lru_cache(maxsize=None)
def batch(kind, select):
    run = Run([[] for _ in SPECS], [[] for _ in SPECS])
    for direction in (1, 0):
        infos, got = batch_call(direction, kind, linkage=SELECT, subfam=SUBFAM, dist=select)
        for f in range(len(SPECS)):
            run.infos[f].append(infos[f])
            run.recs[f].append({s: got[s][f] for s in SINKS})
    return run


@gpu
@pytest.mark.parametrize("select", DISTS, ids=["dist_default", "dist_cut"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_both_callers_agree(kind, select):
    s, b = single(kind, select), batch(kind, select)
    for f in range(len(SPECS)):
        for k, direction in enumerate((1, 0)):
            where = (kind, select, f, direction)
            si, bi = s.infos[f][k], b.infos[f][k]
            assert (bi.ret, bi.rows_executed) == (si.ret, si.rows_executed), where
            for sink in SINKS:
                rs, rb = s.recs[f][k][sink], b.recs[f][k][sink]
                assert rs.family == 0 and rb.family == f and rs.direction == rb.direction == direction, where + (sink,)
                assert_same_record(rb, rs, where + (sink,))
            fl = b.recs[f][k]["subfam"].flanks
            assert len(fl) == n_flanks(f, direction) and np.all((fl["start"] >= 0) & (fl["start"] < len(families()[f][1]))), where
    if kind == "ordinary":
        for f in (0, 5):
            for k, direction in enumerate((1, 0)):
                cut, whole = batch(kind, DISTS[1]).recs[f][k]["dist"], batch(kind, DISTS[0]).recs[f][k]["dist"]
                print(f"family {f} dir {direction}: {len(whole.copies)} copies by default, {len(cut.copies)} with {DISTS[1]}")
                assert 0 < len(cut.copies) <= DISTS[1][1] < len(whole.copies) <= n_flanks(f, direction)
                assert cut.dist.shape == (len(cut.copies),) * 2 and cut.dist["cover"].any()


@gpu
def test_the_ordinary_batch_is_the_restatement():
    """What tests/test_gpu_subfam_cli.py::test_the_subfamily_sink asserts of one family, of the families that share a call."""
    b = batch("ordinary", DISTS[0])
    for f in PLANTED:
        for k, direction in enumerate((1, 0)):
            c, res = restated(f, direction)
            info, lk, sf = b.infos[f][k], b.recs[f][k]["linkage"], b.recs[f][k]["subfam"]
            where = (f, direction)
            assert info.ret == len(c["cons"]) and np.array_equal(sf.cons, c["cons"]) and list(sf.core_index) == c["idx"], where
            assert np.array_equal(lk.planes, c["sel"]) and np.array_equal(lk.co, c["co"]) and np.array_equal(sf.planes, c["sel"]), where
            for key in ("labels", "patterns", "cnt", "size", "dist"):
                assert getattr(sf, key).shape == res[key].shape and np.array_equal(getattr(sf, key), res[key]), where + (key,)
            assert (sf.iterations, sf.converged) == (res["iterations"], res["converged"]), where
            assert [g.group for g in sf.groups] == [g for g, n in enumerate(res["size"]) if n >= MIN_MEMBERS], where
            for g in sf.groups:
                assert g.size == res["size"][g.group] and 0 < len(g.refined_cons) == len(g.refined_cols), where + (g.group,)
                assert g.refined_cols["cover"][0] <= g.size


@gpu
def test_a_group_dropped_from_the_middle():
    """The left direction with GAP_MEMBERS: family 3 keeps groups 0 and 2, and both callers hand over the same records."""
    from repeatafterme_amd.extend import extend_alignment
    args = SUBFAM[:6] + (GAP_MEMBERS,) + SUBFAM[7:]
    _, got = batch_call(0, "ordinary", subfam=args)
    for f in PLANTED:
        _, res = restated(f, 0)
        assert [g.group for g in got["subfam"][f].groups] == [g for g, n in enumerate(res["size"]) if n >= GAP_MEMBERS], f
    assert [g.group for g in got["subfam"][GAP_FAMILY].groups] == [0, 2]
    for f in (GAP_FAMILY, 4):
        cores, seq = families()[f]
        _, sf = extend_alignment(0, cores.copy(), seq, new_master(L), to_extend_params(params("ordinary")), subfam=args)
        assert_same_record(got["subfam"][f], sf, (f,))


def corner_is_literal(info, rec, n, where):
    """No kept column (a family without a flank among them): what include/ramx.h and include/ramx_dist.h say, and where they are
    silent what the sinks have always handed over."""
    assert info.ret == 0 and info.rows_executed > 0, where
    lk, sf, ds = rec["linkage"], rec["subfam"], rec["dist"]
    assert len(lk.cons) == 0 and len(lk.cols) == 0 and len(lk.planes) == 0 and lk.co.shape == (0, 0), where
    assert len(sf.cons) == 0 and len(sf.flanks) == n and len(sf.core_index) == n and len(sf.planes) == 0, where
    assert sf.patterns.shape == (0, 1) and sf.cnt.shape == (1, 0) and sf.size.tolist() == [n], where
    assert sf.labels.shape == (n,) and not sf.labels.any() and sf.dist.shape == (n, 1) and not sf.dist.any(), where
    assert sf.groups == [] and (sf.iterations, sf.converged) == (1, 1), where
    assert len(ds.cons) == 0 and len(ds.core_index) == n and len(ds.ends) == n and all_none(ds.ends), where
    assert ds.copies.shape == (0,) and ds.dist.shape == (0, 0), where


@gpu
@pytest.mark.parametrize("caller", [single, batch], ids=["single", "batch"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_the_corners_are_literal(kind, caller):
    run = caller(kind, DISTS[0])
    for f in range(len(SPECS)) if kind == "nothing_kept" else (EMPTY,):
        for k, direction in enumerate((1, 0)):
            n = n_flanks(f, direction)
            assert n == (0 if f == EMPTY else SPECS[f][0][0])
            corner_is_literal(run.infos[f][k], run.recs[f][k], n, (kind, f, direction))


@gpu
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("sink", SINKS)
def test_sinks_do_not_disturb_each_other(kind, sink):
    """One batch call with a sink alone hands over the records of the call with all three, for every family."""
    b = batch(kind, DISTS[0])
    arg = dict(linkage=SELECT, subfam=SUBFAM, dist=DISTS[0])[sink]
    for k, direction in enumerate((1, 0)):
        infos, got = batch_call(direction, kind, **{sink: arg})
        assert list(got) == [sink]
        for f in range(len(SPECS)):
            assert (infos[f].ret, infos[f].rows_executed) == (b.infos[f][k].ret, b.infos[f][k].rows_executed)
            assert got[sink][f].family == f
            assert_same_record(got[sink][f], b.recs[f][k][sink], (kind, sink, f, direction))
