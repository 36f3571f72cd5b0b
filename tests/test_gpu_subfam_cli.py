"""`RAMExtend -outsubfam` and the subfamily sink of seam 1 on the planted family of tests/linkage_ref.py, written to a .2bit as
the other CLI tests do: the TSV equals the rendering of the restatement (tests/subfam_ref.py) on the oracle's kept consensus, with
every kept group's consensus from ramx_dev_refine through the Python mirror on that group's flanks; every other output is what it
is without the option; the twelfth field of a -batch line gives the same file; extend_alignment hands over the same split; and a
collective refuses the sink."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd import _lib
from repeatafterme_amd.datamodel import new_master
from repeatafterme_amd.loader import load_sequence_subset_minimal, write_ranges, write_twobit

import align_ref as ar
import linkage_ref as lr
import pileup_ref as pr
import subfam_ref as sr
from helpers import make_genome, to_extend_params
from test_gpu_align_cli import fa_records, run_cli
from test_gpu_linkage_cli import COMMON, write_planted

pytestmark = pytest.mark.gpu

MIN_MEMBERS, REPLAYS = 4, 10


def refine_groups(dev, direction, cores, p, cons, labels, K, min_members=MIN_MEMBERS, replays=REPLAYS):
    """Every group of at least min_members copies as a family of its own through Device.refine, from the kept consensus
    -> {group: (refined consensus, replays, converged)}"""
    from repeatafterme_amd.device import resolve_flanks
    (fl, nx), idx = resolve_flanks(direction, cores, p.bandwidth, p.L)
    assert nx == len(labels)
    out = {}
    for k in range(K):
        members = [i for i in range(nx) if int(labels[i]) == k]
        if len(members) < max(min_members, 1):
            continue
        sub = (_lib.Flank * len(members))()
        for j, i in enumerate(members):
            sub[j] = fl[i]
        r = dev.refine((sub, len(members)), to_extend_params(p), cons, max_replays=replays)
        out[k] = (r.cons[0, :int(r.rows[0])].copy(), int(r.replays[0]), int(r.converged[0]))
    return out


def expected(twobit, ranges, names, K=4, score=3, max_iter=8, min_members=MIN_MEMBERS):
    """-> (the file as the helper renders it, {direction: (restatement's result, refined)})"""
    from repeatafterme_amd.device import Device
    fs = load_sequence_subset_minimal(twobit, ranges, 80 + 20)
    p = po.Params.named("14p43g", bandwidth=20, L=80, when_to_stop=30)
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    cores, master = fs.cores, new_master(80)
    blocks, results_of = {}, {}
    dev = Device(0)
    try:
        dev.load_library(seq)
        for direction in (1, 0):
            before = cores.copy()
            o = po.oracle_extend(direction, cores, seq, master, p, trace=True)
            cons = o.col_base[:o.ret]
            cols, idx, results = pr.pileup(direction, before, seq, p, cons, with_walks=True)
            pl = lr.planes_of(direction, before, idx, results, seq, 20, cons)
            sel = lr.select(cons, cols, 4, 100, 1024)
            linked = [(l["p"], l["q"]) for l in lr.link_pairs(sel, lr.gram(pl, sel), score)]
            init, _ = sr.components(sel, linked, K)
            res = sr.iterate(pl, sel, init, len(idx), max_iter)
            refined = refine_groups(dev, direction, before, p, cons, res["labels"], init.shape[1], min_members)
            blocks[direction] = (names, idx, sel, res, refined)
            results_of[direction] = (res, refined, sel)
            if direction:
                ar.overlap_avoidance(fs)
    finally:
        dev.close()
    return sr.render_subfam(blocks), results_of


@pytest.fixture(scope="module")
def planted_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("subfam")
    recs, rows = write_planted(tmp)
    write_twobit(str(tmp / "g.2bit"), recs)
    write_ranges(str(tmp / "g.tsv"), rows)
    base = ["-twobit", "g.2bit", "-ranges", "g.tsv"] + COMMON
    outs = lambda tag: ["-cons", f"{tag}.cons", "-outtsv", f"{tag}.tsv", "-outfa", f"{tag}.fa", "-outlinkage", f"{tag}.linkage",
                        "-outcopies", f"{tag}.copies"]
    plain = run_cli(base + outs("p"), tmp)
    with_new = run_cli(base + outs("n") + ["-outsubfam", "n.subfam"], tmp)
    names = {n: v[0] for n, v in fa_records(tmp / "n.fa").items()}
    want, results_of = expected(str(tmp / "g.2bit"), str(tmp / "g.tsv"), names)
    return tmp, base, plain, with_new, want, results_of, names


def test_outsubfam_is_the_rendering_and_changes_nothing_else(planted_run):
    tmp, base, plain, with_new, want, results_of, names = planted_run
    assert with_new == plain.replace("p.", "n.")
    for ext in ("cons", "tsv", "fa", "linkage", "copies"):
        assert open(tmp / f"n.{ext}").read() == open(tmp / f"p.{ext}").read(), ext
    got = open(tmp / "n.subfam").read()
    assert got == want
    assert got.startswith(sr.SUBFAM_HEADER)
    # right: the consensus, the planted group and the unplanted pair's; left: the consensus and the planted group
    heads = [l.split("\t") for l in got.splitlines() if l.startswith("group\t")]
    assert [(h[1], h[2]) for h in heads] == [("right", "0"), ("right", "1"), ("right", "2"), ("left", "0"), ("left", "1")]
    for h in heads:
        if h[2] == "1":
            assert [x.split(":")[0] for x in h[6].split(",")] == ["8", "30", "55"] and int(h[3]) >= 20 and h[7] != "NA"
    assert sum(l.startswith("copy\t") for l in got.splitlines()) == 2 * 70
    # the planted group's own consensus carries the planted bases where the family's carries its own
    for direction in (1, 0):
        res, refined, sel = results_of[direction]
        c = lr.planted_case(direction)
        assert len(refined[1][0]) == len(refined[0][0]) == len(c["cons"])
        for (row, cls) in c["planted"]:
            assert refined[1][0][row] == cls and refined[0][0][row] == c["cons"][row]
    # the flag alone writes the same file; the options move the split as the restatement says
    run_cli(base + ["-outsubfam", "o.subfam"], tmp)
    assert open(tmp / "o.subfam").read() == got
    run_cli(base + ["-outsubfam", "q.subfam", "-subfamk", "2", "-subfammin", "30", "-subfamiter", "1"], tmp)
    want_q, _ = expected(str(tmp / "g.2bit"), str(tmp / "g.tsv"), names, K=2, max_iter=1, min_members=30)
    assert open(tmp / "q.subfam").read() == want_q and want_q != want and "\tNA\tNA\tNA\t-\n" in want_q
    bad = subprocess.run([_lib.CLI_PATH] + base + ["-outsubfam", "x.subfam", "-subfamk", "9"], cwd=tmp, capture_output=True, text=True)
    assert bad.returncode != 0 and "-subfamk" in bad.stderr and not os.path.exists(tmp / "x.subfam")


def restated(direction):
    """The split of lr.planted_case(direction) and its kept groups' refinement -> (restatement's result, refined)"""
    from repeatafterme_amd.device import Device
    fs, seq, p, _, _ = lr.planted_family()
    c = lr.planted_case(direction)
    linked = [(l["p"], l["q"]) for l in lr.link_pairs(c["sel"], c["co"], lr.CLI_SCORE)]
    init, _ = sr.components(c["sel"], linked, 4)
    res = sr.iterate(c["planes"], c["sel"], init, len(c["idx"]))
    dev = Device(0)
    try:
        dev.load_library(seq)
        refined = refine_groups(dev, direction, fs.cores, p, c["cons"], res["labels"], init.shape[1])
    finally:
        dev.close()
    return res, refined


def test_the_subfamily_sink():
    """extend_alignment(subfam=...) alone and beside the linkage sink: the Subfamilies comes last, and everything in it is the
    restatement's along the kept consensus."""
    from repeatafterme_amd.extend import extend_alignment
    fs, seq, p, cons, _ = lr.planted_family()
    ep = to_extend_params(p)
    for direction in (1, 0):
        c = lr.planted_case(direction)
        res, refined = restated(direction)
        info0, lk0 = extend_alignment(direction, fs.cores.copy(), seq, new_master(p.L), ep, linkage=True)
        m1 = new_master(p.L)
        info1, lk1, sf = extend_alignment(direction, fs.cores.copy(), seq, m1, ep, linkage=True, subfam=True)
        assert info0.ret == info1.ret == len(c["cons"]) and np.array_equal(lk0.co, lk1.co) and np.array_equal(lk0.planes, lk1.planes)
        assert (sf.direction, sf.family) == (direction, 0) and np.array_equal(sf.cons, c["cons"]) and np.array_equal(sf.planes, c["sel"])
        assert list(sf.core_index) == c["idx"]
        for k in ("labels", "patterns", "cnt", "size", "dist"):
            assert getattr(sf, k).shape == res[k].shape and np.array_equal(getattr(sf, k), res[k]), k
        assert (sf.iterations, sf.converged) == (res["iterations"], res["converged"])
        assert [g.group for g in sf.groups] == sorted(refined)
        for g in sf.groups:
            rc, replays, conv = refined[g.group]
            assert g.size == res["size"][g.group] and np.array_equal(g.refined_cons, rc) and (g.replays, g.converged) == (replays, conv)
            assert g.refined_cols["cover"][0] <= g.size and len(g.refined_cols) == len(rc)
        # one pattern only: every copy in group 0, one assignment; a group needs more members than there are copies: none is kept
        _, one = extend_alignment(direction, fs.cores.copy(), seq, new_master(p.L), ep, subfam=(4, 100, 1024, 3.0, 1, 8, 1000, 10))
        assert one.patterns.shape[1] == 1 and not one.labels.any() and one.size.tolist() == [70] and (one.iterations, one.converged) == (1, 1)
        assert one.groups == []


def test_the_sink_answers_a_family_without_an_extendable_core_on_the_host():
    from repeatafterme_amd.extend import extend_alignment
    fs, seq, p, _, _ = lr.planted_family()
    cores = fs.cores.copy()
    cores.right_ext[:] = 0
    info, sf = extend_alignment(1, cores, seq, new_master(p.L), to_extend_params(p), subfam=True)
    assert info.ret == 0 and len(sf.labels) == 0 and sf.patterns.shape == (0, 1) and sf.size.tolist() == [0] and sf.groups == []
    assert (sf.iterations, sf.converged) == (1, 1) and len(sf.planes) == 0


def test_the_sink_is_refused_under_a_collective():
    """With an allreduce callback set on seam 1's session (the single-rank stand-in for a communicator) the subfamily sink fails
    the direction with RAMX_ERR_UNSUPPORTED, as the linkage sink does; with the callback taken away again it works."""
    import ctypes as C
    from repeatafterme_amd.extend import extend_alignment
    fs, seq, p, _, _ = lr.planted_family()
    ep = to_extend_params(p)
    L = _lib.lib()
    L.ramx_default_device.restype = C.c_void_p
    dev = L.ramx_default_device()
    assert dev
    cb = _lib.ALLREDUCE_CB(lambda ptr, user: None)
    _lib.check(L.ramx_dev_set_allreduce_cb(dev, cb, None), "ramx_dev_set_allreduce_cb")
    try:
        plain = extend_alignment(1, fs.cores.copy(), seq, new_master(p.L), ep)
        with pytest.raises(_lib.RamxError, match=r"\(-106\).*subfamily sink.*counts of every rank"):
            extend_alignment(1, fs.cores.copy(), seq, new_master(p.L), ep, subfam=True)
    finally:
        _lib.check(L.ramx_dev_set_allreduce_cb(dev, _lib.ALLREDUCE_CB(), None), "ramx_dev_set_allreduce_cb")
    info, sf = extend_alignment(1, fs.cores.copy(), seq, new_master(p.L), ep, subfam=True)
    assert info.ret == plain.ret == 70 and sf.size.sum() == 70


def test_outsubfam_in_a_batch_is_the_twelfth_field(tmp_path):
    """Two families in one -batch list with their subfamily files in the twelfth field ("-" in the six before it): the files of
    the stand-alone runs, the other outputs those of a batch without the field; the bare flag with -batch is refused.  The
    families get different numbers of patterns, so the batch splits them in calls of their own."""
    recs, rows = write_planted(tmp_path, "f0_")
    recs1, rows1 = make_genome(14)
    write_twobit(str(tmp_path / "all.2bit"), recs + [("f1_" + n, s) for n, s in recs1])
    write_ranges(str(tmp_path / "fam0.tsv"), rows)
    write_ranges(str(tmp_path / "fam1.tsv"), [("f1_" + r[0],) + tuple(r[1:]) for r in rows1])
    common = ["-twobit", "all.2bit"] + COMMON
    with open(tmp_path / "batch.list", "w") as fh:
        for k in range(2):
            fh.write("\t".join([f"fam{k}.tsv", f"b{k}.log", f"b{k}.cons", f"b{k}.tsv", f"b{k}.fa", "-", "-", "-", "-", "-", "-", f"b{k}.subfam"]) + "\n")
    r = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "batch.list"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(tmp_path / "-")
    with open(tmp_path / "plain.list", "w") as fh:
        for k in range(2):
            fh.write("\t".join([f"fam{k}.tsv", f"q{k}.log", f"q{k}.cons", f"q{k}.tsv", f"q{k}.fa"]) + "\n")
    q = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "plain.list"], cwd=tmp_path, capture_output=True, text=True)
    assert q.returncode == 0, q.stderr
    for k in range(2):
        for ext in ("cons", "tsv", "fa"):
            assert open(tmp_path / f"b{k}.{ext}").read() == open(tmp_path / f"q{k}.{ext}").read(), (k, ext)
        run_cli(common + ["-ranges", f"fam{k}.tsv", "-outsubfam", f"s{k}.subfam"], tmp_path)
        assert open(tmp_path / f"s{k}.subfam").read() == open(tmp_path / f"b{k}.subfam").read(), k
    groups = [sum(l.startswith("group\tright") for l in open(tmp_path / f"b{k}.subfam")) for k in range(2)]
    assert groups[0] == 3 and groups[1] >= 1
    bad = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "batch.list", "-outsubfam", "x.subfam"], cwd=tmp_path, capture_output=True, text=True)
    assert bad.returncode != 0 and "twelfth field" in bad.stderr and not os.path.exists(tmp_path / "x.subfam")
