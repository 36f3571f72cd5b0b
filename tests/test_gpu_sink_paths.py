"""The five sinks of seam 1 (profile, alignment, refinement, copies, linkage) through both of their callers: the same families
run one at a time through extend_alignment and together through extend_batch, both directions, all five sinks set at once.
Every record the batch hands over is the single call's, byte for byte, and the corners are what include/ramx.h documents: a
family without an extendable core, and ret = 0 after rows were executed.  Ordinary families are tied to independent
restatements elsewhere (align_ref.py, pileup_ref.py, copystats_ref.py, linkage_ref.py); this file does not repeat that.  The
sinks that answer from the resident planes (linkage again, subfamilies, distance) have tests/test_gpu_plane_sinks.py, on families
that share a ramx_dev_subfamilies call.

Four families (bandwidth 5, L = 30, matrix 14p43g, about 20 recoverable columns), in this order in the batch:
  0: 70 flanks          two tiles, the second uneven
  1: 10 cores, none extendable in either direction
  2: 5 flanks
  3: 600 flanks         above one workgroup: the batch runs it on its own with family = 3, the single call takes the
                        direction route instead of the family route"""
import dataclasses
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import new_master
from repeatafterme_amd.synth import synth_family

from helpers import to_extend_params

pytestmark = pytest.mark.gpu

W, L = 5, 30
SIZES = (70, 10, 5, 600)
EMPTY = 1                            # the family without an extendable core
SELECT = (2, 20, 64)                 # linkage: min_count, min_permille, max_variants -- low enough that 70 flanks have variants
REPLAYS = 3
SINKS = ("profile", "align", "refine", "copies", "linkage")
NONE = (-1, -1, 0, 0, 0)
END_FIELDS = ("end_row", "end_idx", "score", "start_idx", "tail_ins")
# "nothing kept": row r becomes the new maximum iff its column score >= max + (r - max_row) * minimprovement.  No column of
# 600 flanks can score 600 * (the matrix' largest entry, < 100) = 60000, so with this value ret = 0 on every family, while
# 31 * 10**6 still fits an int32.
HUGE_MINIMPROVEMENT = 10 ** 6
# the loop stops 7 rows after its last maximum, so rows_executed lies above ret and (with about 20 kept columns) below L
KINDS = {"ordinary": dict(when_to_stop=7), "nothing_kept": dict(when_to_stop=7, minimprovement=HUGE_MINIMPROVEMENT)}


@functools.lru_cache(maxsize=None)
def families():
    fams = [synth_family(n, L, W, K=20, seed=70 + i, both_sides=True) for i, n in enumerate(SIZES)]
    fams[EMPTY].cores.left_ext[:] = 0
    fams[EMPTY].cores.right_ext[:] = 0
    for fs in fams:
        fs.sequence.setflags(write=False)
    return fams


def params(kind):
    return po.Params.named("14p43g", bandwidth=W, L=L, **KINDS[kind])


@functools.lru_cache(maxsize=None)
def oracle(kind):
    """-> [family][k] the oracle's Result of direction (1, 0)[k], on the CPU"""
    out = []
    for fs in families():
        c, m = fs.cores.copy(), new_master(L)
        out.append([po.oracle_extend(d, c, fs.sequence, m, params(kind)) for d in (1, 0)])
    return out


def batch_call(direction, batch, ep, sinks):
    """extend_batch with the named sinks set -> (infos, {sink: [record per family]})"""
    from repeatafterme_amd.extend import _RefineSink, extend_batch
    kw = dict(profile="profile" in sinks, align="align" in sinks, copies="copies" in sinks, linkage=SELECT if "linkage" in sinks else None)
    if "refine" in sinks:
        with _RefineSink(REPLAYS) as rs:
            res = extend_batch(direction, batch, ep, **kw)
        by_family = {rf.family: rf for rf in rs.got}
        assert len(by_family) == len(rs.got) == len(batch)
    else:
        res = extend_batch(direction, batch, ep, **kw)
    res = res if isinstance(res, tuple) else (res,)
    got = dict(zip([s for s in SINKS if s in sinks and s != "refine"], res[1:]))
    if "refine" in sinks:
        got["refine"] = [by_family[f] for f in range(len(batch))]
    return res[0], got


@dataclasses.dataclass
class Run:
    infos: list            # [family][k]
    recs: list             # [family][k] {sink: record}
    cores: list            # [family] the cores after both directions
    masters: list


@functools.lru_cache(maxsize=None)
def single(kind):
    from repeatafterme_amd.extend import extend_alignment
    ep = to_extend_params(params(kind))
    run = Run([], [], [], [])
    for fs in families():
        c, m = fs.cores.copy(), new_master(L)
        res = [extend_alignment(d, c, fs.sequence, m, ep, profile=True, align=True, refine=REPLAYS, copies=True, linkage=SELECT) for d in (1, 0)]
        run.infos.append([r[0] for r in res])
        run.recs.append([dict(zip(SINKS, r[1:])) for r in res])
        run.cores.append(c)
        run.masters.append(m)
    return run


def fresh_batch():
    return [(fs.cores.copy(), fs.sequence, new_master(L)) for fs in families()]


@functools.lru_cache(maxsize=None)
def batch(kind):
    ep = to_extend_params(params(kind))
    b = fresh_batch()
    run = Run([[] for _ in b], [[] for _ in b], [c for c, _, _ in b], [m for _, _, m in b])
    for direction in (1, 0):
        infos, got = batch_call(direction, b, ep, SINKS)
        for f in range(len(b)):
            run.infos[f].append(infos[f])
            run.recs[f].append({s: got[s][f] for s in SINKS})
    return run


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def assert_same_record(a, b, where):
    """every field of two records of one kind but `family`: arrays byte for byte, a list of records (Subfamilies.groups) record by
    record"""
    assert type(a) is type(b), where
    for fld in dataclasses.fields(a):
        if fld.name == "family":
            continue
        x, y = getattr(a, fld.name), getattr(b, fld.name)
        if isinstance(x, np.ndarray):
            assert same_bytes(x, y), where + (fld.name,)
        elif isinstance(x, list):
            assert isinstance(y, list) and len(x) == len(y), where + (fld.name, len(x))
            for i, (p, q) in enumerate(zip(x, y)):
                assert_same_record(p, q, where + (fld.name, i))
        else:
            assert x == y, where + (fld.name, x, y)


def all_none(ends):
    return all(np.all(ends[k] == v) for k, v in zip(END_FIELDS, NONE))


def n_extendable(f, direction):
    c = families()[f].cores
    return int((c.right_ext if direction else c.left_ext).sum())


def test_the_oracle_sees_the_cases():
    """On the CPU: the ordinary set keeps different numbers of columns in at least two families, the other set keeps none
    anywhere while rows are executed."""
    for k in range(2):
        kept = {o[k].ret for f, o in enumerate(oracle("ordinary")) if f != EMPTY}
        assert len(kept) >= 2 and min(kept) > 0, kept
        assert all(o[k].ret < o[k].rows_executed < L for f, o in enumerate(oracle("ordinary")) if f != EMPTY)
    for o in oracle("nothing_kept"):
        for k in range(2):
            assert o[k].ret == 0 and 0 < o[k].rows_executed < L


@pytest.mark.parametrize("kind", list(KINDS))
def test_both_callers_agree(kind):
    s, b, want = single(kind), batch(kind), oracle(kind)
    for f, fs in enumerate(families()):
        for k, direction in enumerate((1, 0)):
            where = (kind, f, direction)
            si, bi = s.infos[f][k], b.infos[f][k]
            assert (bi.ret, bi.rows_executed) == (si.ret, si.rows_executed) == (want[f][k].ret, want[f][k].rows_executed), where
            for sink in SINKS:
                rs, rb = s.recs[f][k][sink], b.recs[f][k][sink]
                assert rs.family == 0 and rb.family == f and rs.direction == rb.direction == direction, where + (sink,)
                assert_same_record(rb, rs, where + (sink,))
            # the flanks' positions are in the family's own library, in both
            for sink in ("align", "copies"):
                fl = b.recs[f][k][sink].flanks
                assert len(fl) == n_extendable(f, direction) and np.all((fl["start"] >= 0) & (fl["start"] < len(fs.sequence))), where
        assert np.array_equal(b.masters[f], s.masters[f]) and np.array_equal(b.masters[f], want[f][1].master), (kind, f)
        for key in ("left_len", "right_len", "score"):
            assert same_bytes(getattr(b.cores[f], key), getattr(s.cores[f], key)), (kind, f, key)
            assert np.array_equal(getattr(b.cores[f], key), getattr(want[f][1], key)), (kind, f, key)
    if kind == "ordinary":
        for k in range(2):
            assert len({b.infos[f][k].ret for f in range(len(SIZES)) if f != EMPTY}) >= 2


@pytest.mark.parametrize("caller", [single, batch], ids=["single", "batch"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_a_family_without_an_extendable_core(kind, caller):
    """include/ramx.h: rows_executed profile columns of zeros with base A, no flank anywhere, one converged replay, no plane."""
    run = caller(kind)
    for k in range(2):
        info, rec = run.infos[EMPTY][k], run.recs[EMPTY][k]
        assert info.ret == 0 and info.rows_executed > 0
        pr = rec["profile"]
        assert pr.ret == 0 and len(pr.core_index) == 0 and len(pr.last_uncapped_row) == 0                 # n_flanks == 0
        assert len(pr.cols) == info.rows_executed and not pr.cols.view(np.uint8).any()                     # base A = 0, the rest 0
        al, cp = rec["align"], rec["copies"]
        for a in (al.cons, al.flanks, al.core_index, al.ends, al.col_idx, al.col_ins, cp.cons, cp.flanks, cp.core_index, cp.ends, cp.stats):
            assert a.size == 0
        rf = rec["refine"]
        assert (rf.replays, rf.converged) == (1, 1) and len(rf.cons) == 0 and len(rf.refined_cons) == 0
        lk = rec["linkage"]
        assert len(lk.planes) == 0 and lk.co.size == 0 and len(lk.cons) == 0


@pytest.mark.parametrize("caller", [single, batch], ids=["single", "batch"])
def test_nothing_kept(caller):
    """include/ramx.h for ret = 0 with rows executed, asserted on what the GPU returned: no flank has an alignment, no column,
    zero records, nothing refined, no plane; the profile still has rows_executed columns, none of them kept."""
    run = caller("nothing_kept")
    for f in range(len(SIZES)):
        for k, direction in enumerate((1, 0)):
            info, rec, n = run.infos[f][k], run.recs[f][k], n_extendable(f, direction)
            assert info.ret == 0 and info.rows_executed > 0, (f, direction)
            pr = rec["profile"]
            assert pr.ret == 0 and len(pr.cols) == info.rows_executed and len(pr.core_index) == n
            if n:
                assert pr.cols["total"].any(), (f, direction)          # the replay did run over the executed rows
            al = rec["align"]
            assert len(al.ends) == n and all_none(al.ends) and al.col_idx.size == 0 and al.col_ins.size == 0 and len(al.cons) == 0
            cp = rec["copies"]
            assert len(cp.stats) == n and not cp.stats.view(np.uint8).any() and len(cp.ends) == n and all_none(cp.ends)
            rf = rec["refine"]
            assert len(rf.cons) == 0 and len(rf.refined_cons) == 0 and len(rf.refined_cols) == 0
            assert len(rec["linkage"].planes) == 0 and rec["linkage"].co.size == 0


def test_the_ordinary_records_are_not_trivial():
    """What the agreement above compares is there: alignments end somewhere, copies have columns, variants were selected, and
    the largest family's refinement replayed."""
    b = batch("ordinary")
    for f in (0, 2, 3):
        for k in range(2):
            rec = b.recs[f][k]
            assert (rec["align"].ends["end_row"] >= 0).any() and rec["copies"].stats["cols"].any(), (f, k)
            assert rec["refine"].cols["cover"].sum() > 0 and rec["profile"].cols["total"].any(), (f, k)
    assert all(len(b.recs[f][k]["linkage"].planes) > 0 for f in (0, 3) for k in range(2))


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("sink", SINKS)
def test_sinks_do_not_disturb_each_other(kind, sink):
    """One batch call with a sink alone hands over the record of the call with all five (family 0)."""
    ep = to_extend_params(params(kind))
    b, fam = batch(kind), fresh_batch()
    for k, direction in enumerate((1, 0)):
        infos, got = batch_call(direction, fam, ep, (sink,))
        assert list(got) == [sink]
        assert (infos[0].ret, infos[0].rows_executed) == (b.infos[0][k].ret, b.infos[0][k].rows_executed)
        assert got[sink][0].family == 0
        assert_same_record(got[sink][0], b.recs[0][k][sink], (kind, sink, direction))
