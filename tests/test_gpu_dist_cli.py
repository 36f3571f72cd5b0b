"""`RAMExtend -outdist` and the distance sink of seam 1 on the planted family of tests/linkage_ref.py, written to a .2bit as the
other CLI tests do: the sink's records are the restatement's, the TSV equals the rendering of the sink's records (integers and
names exactly, the %.4f fields within one unit of their last printed digit) including the block of both directions, every other
output is what it is without the option, the seventeenth field of a -batch line gives the same file, and tools/extend_stk.py
hands the file through."""
import os
import subprocess
import sys

import numpy as np
import pytest

from repeatafterme_amd import _lib
from repeatafterme_amd.datamodel import new_master
from repeatafterme_amd.loader import load_sequence_subset_minimal, write_ranges, write_twobit

import align_ref as ar
import dist_ref as dr
import linkage_ref as lr
from helpers import make_genome, to_extend_params
from test_gpu_align_cli import fa_records, run_cli
from test_gpu_linkage_cli import COMMON, write_planted

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sink_blocks(twobit, ranges, select):
    """Both directions through extend_alignment(dist=select), with the overlap avoidance between them as the command line runs
    them -> {direction: (core_index, selected flanks, matrix)}"""
    from oracle import pyoracle as po
    from repeatafterme_amd.extend import extend_alignment
    fs = load_sequence_subset_minimal(twobit, ranges, 80 + 20)
    ep = to_extend_params(po.Params.named("14p43g", bandwidth=20, L=80, when_to_stop=30))
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    master, blocks = new_master(80), {}
    for direction in (1, 0):
        info, ds = extend_alignment(direction, fs.cores, seq, master, ep, dist=select)
        assert (ds.direction, ds.family) == (direction, 0) and len(ds.cons) == info.ret
        blocks[direction] = (ds.core_index, ds.copies, ds.dist)
        if direction:
            ar.overlap_avoidance(fs)
    return blocks


@pytest.fixture(scope="module")
def planted_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dist")
    recs, rows = write_planted(tmp)
    write_twobit(str(tmp / "g.2bit"), recs)
    write_ranges(str(tmp / "g.tsv"), rows)
    base = ["-twobit", "g.2bit", "-ranges", "g.tsv"] + COMMON
    outs = lambda tag: ["-cons", f"{tag}.cons", "-outtsv", f"{tag}.tsv", "-outfa", f"{tag}.fa", "-outpileup", f"{tag}.pileup",
                        "-outcopies", f"{tag}.copies", "-outlinkage", f"{tag}.linkage", "-outterm", f"{tag}.term"]
    plain = run_cli(base + outs("p"), tmp)
    with_new = run_cli(base + outs("n") + ["-outdist", "n.dist"], tmp)
    names = {n: v[0] for n, v in fa_records(tmp / "n.fa").items()}
    return tmp, base, plain, with_new, names


def test_the_sink_after_real_extensions_is_the_restatement():
    """extend_alignment(dist=...) alone and beside the copies sink: the Dist comes last, its selection and records are the
    restatement's along the kept consensus, and equal the direct calls on a session of one's own."""
    from repeatafterme_amd.device import Device, resolve_flanks, select_copies
    from repeatafterme_amd.extend import extend_alignment
    fs, seq, p, cons, _ = lr.planted_family()
    ep = to_extend_params(p)
    for direction in (1, 0):
        c = lr.planted_case(direction)
        maps = dr.maps_of(direction, fs.cores, c["idx"], c["results"], seq, p.bandwidth, c["cons"])
        er = [r["end_row"] for r in c["results"]]
        info0, cp0 = extend_alignment(direction, fs.cores.copy(), seq, new_master(p.L), ep, copies=True)
        info1, cp1, ds1 = extend_alignment(direction, fs.cores.copy(), seq, new_master(p.L), ep, copies=True, dist=True)
        info2, ds2 = extend_alignment(direction, fs.cores.copy(), seq, new_master(p.L), ep, dist=(60, 9))
        assert info0.ret == info1.ret == info2.ret == len(c["cons"]) and np.array_equal(cp0.stats, cp1.stats)
        assert np.array_equal(ds1.cons, c["cons"]) and list(ds1.core_index) == c["idx"] and list(ds1.ends["end_row"]) == er
        for ds, sel in ((ds1, dr.select(er, len(c["cons"]), 1, 256)), (ds2, dr.select(er, len(c["cons"]), 60, 9))):
            assert list(ds.copies) == sel and np.array_equal(ds.dist, dr.matrix(maps, sel))
        assert len(ds1.copies) == 70 and len(ds2.copies) == 9
        d = Device(0)
        try:
            d.load_library(seq)
            flanks, idx = resolve_flanks(direction, fs.cores, p.bandwidth, p.L)
            res = d.planes(flanks, ep, c["cons"])
            sel = select_copies(res.ends[:len(idx)], len(c["cons"]), 60, 9)
            assert np.array_equal(sel, ds2.copies) and np.array_equal(d.copy_dist(sel), ds2.dist)
        finally:
            d.close()


def test_outdist_is_the_rendering_and_changes_nothing_else(planted_run):
    tmp, base, plain, with_new, names = planted_run
    assert with_new == plain.replace("p.", "n.")
    for ext in ("cons", "tsv", "fa", "pileup", "copies", "linkage", "term"):
        assert open(tmp / f"n.{ext}").read() == open(tmp / f"p.{ext}").read(), ext
    got = open(tmp / "n.dist").read()
    blocks = sink_blocks(str(tmp / "g.2bit"), str(tmp / "g.tsv"), (20, 256))
    dr.same_dist_text(got, dr.render_dist(blocks, names, 20))
    parsed = dr.parse_dist(got)
    assert got.startswith(dr.DIST_HEADER) and got.count("\n#") == 3 and set(parsed) == {"right", "left", "both"}
    n_both, cores, m = dr.both_block(blocks)
    assert len(cores) > 30 and parsed["both"][1]["selected"] == str(len(cores)) and parsed["both"][1]["medoid"] != "NA"
    a, b, rec, k = parsed["both"][0][0]
    r1 = next(x for x in parsed["right"][0] if x[:2] == (a, b))[2]
    r0 = next(x for x in parsed["left"][0] if set(x[:2]) == {a, b})[2]
    assert rec == tuple(x + y for x, y in zip(r1, r0))
    # the flag alone writes the same file
    run_cli(base + ["-outdist", "o.dist"], tmp)
    assert open(tmp / "o.dist").read() == got


def test_distmin_and_distmax_reach_the_record(planted_run):
    tmp, base, _, _, names = planted_run
    run_cli(base + ["-outdist", "q.dist", "-distmin", "60", "-distmax", "9"], tmp)
    got = open(tmp / "q.dist").read()
    blocks = sink_blocks(str(tmp / "g.2bit"), str(tmp / "g.tsv"), (60, 9))
    dr.same_dist_text(got, dr.render_dist(blocks, names, 60))
    parsed = dr.parse_dist(got)
    assert parsed["right"][1]["selected"] == "9" and len(parsed["right"][0]) == 36 and parsed["right"][1]["copies"] == "70"
    for bad in ("1", "0", "-4", "2049"):
        r = subprocess.run([_lib.CLI_PATH] + base + ["-outdist", "x.dist", "-cons", "x.cons", "-distmax", bad], cwd=tmp, capture_output=True, text=True)
        assert r.returncode != 0 and "-distmax" in r.stderr and not os.path.exists(tmp / "x.dist") and not os.path.exists(tmp / "x.cons"), bad
    for ok in ("2", "2048"):
        run_cli(base + ["-outdist", "y.dist", "-distmax", ok], tmp)
    assert dr.parse_dist(open(tmp / "y.dist").read())["right"][1]["selected"] == "70"


def test_outdist_in_a_batch_is_the_seventeenth_field(tmp_path):
    """Three families in one -batch list: a line with all seventeen fields, one that stops at the sixteenth and one that gives only
    the seventeenth ("-" in the eleven before it); every file is byte-equal to the single-family run's, and the bare flag with
    -batch is refused."""
    recs, rows = write_planted(tmp_path, "f0_")
    recs1, rows1 = make_genome(14)
    write_twobit(str(tmp_path / "all.2bit"), recs + [("f1_" + n, s) for n, s in recs1])
    write_ranges(str(tmp_path / "fam0.tsv"), rows)
    write_ranges(str(tmp_path / "fam1.tsv"), [("f1_" + r[0],) + tuple(r[1:]) for r in rows1])
    write_ranges(str(tmp_path / "fam2.tsv"), rows)
    common = ["-twobit", "all.2bit"] + COMMON
    flags = ["-outprofile", "-outaln", "-outpileup", "-outrefined", "-outcopies", "-outlinkage", "-outsubfam", "-outtsd", "-outcpg", "-outperiod",
             "-outterm", "-outdist"]
    exts = [f[4:] for f in flags]
    first5 = lambda k: [f"fam{k}.tsv", f"b{k}.log", f"b{k}.cons", f"b{k}.tsv", f"b{k}.fa"]
    with open(tmp_path / "batch.list", "w") as fh:
        fh.write("\t".join(first5(0) + [f"b0.{e}" for e in exts]) + "\n")
        fh.write("\t".join(first5(1) + [f"b1.{e}" for e in exts[:-1]]) + "\n")
        fh.write("\t".join(first5(2) + ["-"] * 11 + ["b2.dist"]) + "\n")
    r = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "batch.list"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(tmp_path / "-") and not os.path.exists(tmp_path / "b1.dist") and not os.path.exists(tmp_path / "b2.term")
    wanted = {0: exts, 1: exts[:-1], 2: ["dist"]}
    for k in range(3):
        args = ["-cons", f"s{k}.cons", "-outtsv", f"s{k}.tsv", "-outfa", f"s{k}.fa"]
        for f, e in zip(flags, exts):
            if e in wanted[k]:
                args += [f, f"s{k}.{e}"]
        run_cli(common + ["-ranges", f"fam{k}.tsv"] + args, tmp_path)
        for e in ["cons", "tsv", "fa"] + wanted[k]:
            assert open(tmp_path / f"s{k}.{e}").read() == open(tmp_path / f"b{k}.{e}").read(), (k, e)
    assert open(tmp_path / "b0.dist").read() == open(tmp_path / "b2.dist").read() and open(tmp_path / "b0.dist").read().count("\n#") == 3
    bad = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "batch.list", "-outdist", "x.dist"], cwd=tmp_path, capture_output=True, text=True)
    assert bad.returncode != 0 and "seventeenth field" in bad.stderr and not os.path.exists(tmp_path / "x.dist")


def test_the_dist_sink_in_a_batch():
    """extend_batch(dist=...) on the planted family beside a second one: one Dist per family, last in the tuple, equal to the
    single run's."""
    from repeatafterme_amd.extend import extend_alignment, extend_batch
    from repeatafterme_amd.synth import synth_family
    fs, seq, p, _, _ = lr.planted_family()
    other = synth_family(37, 80, 20, K=50, seed=3, both_sides=True, minus_frac=0.4, n_run_frac=0.1)
    ep = to_extend_params(p)
    for direction in (1, 0):
        batch = [(fs.cores.copy(), seq, new_master(80)), (other.cores.copy(), other.sequence, new_master(80))]
        infos, dss = extend_batch(direction, batch, ep, dist=(20, 40))
        assert len(dss) == 2 and [ds.family for ds in dss] == [0, 1]
        for k, (cores, s) in enumerate(((fs.cores, seq), (other.cores, other.sequence))):
            s_info, s_ds = extend_alignment(direction, cores.copy(), s, new_master(80), ep, dist=(20, 40))
            assert s_info.ret == infos[k].ret and np.array_equal(s_ds.copies, dss[k].copies) and np.array_equal(s_ds.dist, dss[k].dist)
        assert len(dss[0].copies) == 40 and 2 < len(dss[1].copies) <= 37


def test_the_sink_is_refused_under_a_collective():
    """With an allreduce callback set on seam 1's session (the single-rank stand-in for a communicator, as
    tests/test_gpu_linkage_cli.py uses it) the loop runs, and the distance sink fails the direction with RAMX_ERR_UNSUPPORTED."""
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
        with pytest.raises(_lib.RamxError, match=r"\(-106\).*dist sink"):
            extend_alignment(1, fs.cores.copy(), seq, new_master(p.L), ep, dist=True)
    finally:
        _lib.check(L.ramx_dev_set_allreduce_cb(dev, _lib.ALLREDUCE_CB(), None), "ramx_dev_set_allreduce_cb")
    info, ds = extend_alignment(1, fs.cores.copy(), seq, new_master(p.L), ep, dist=True)
    assert info.ret == plain.ret == 70 and len(ds.copies) == 70


def test_extend_stk_dist(tmp_path):
    """tools/extend_stk.py -dist: <id>-dist.tsv per family is the stand-alone run's file, through -batch and one by one."""
    from repeatafterme_amd import stockholm as stk
    import test_gpu_batch_cli as tb
    fams = tb._families(tmp_path, [60, 61])
    mdiv = [12.5, 17.0]
    with open(tmp_path / "in.stk", "w") as fh:
        for k, rows in enumerate(fams):
            fh.write(f"# STOCKHOLM 1.0\n#=GF ID    fam{k}\n#=GF DE    Source:gsa, mDiv={mdiv[k]:.2f}, all.2bit:1\n")
            for (name, s, e, lf, rf, o) in rows:
                fh.write(f"{name}:{s + 1}-{e}_{o} {'' if lf else '.' * 12}{'ACGT' * 3}{'' if rf else '.' * 12}\n")
            fh.write("//\n")
    tool = [sys.executable, os.path.join(ROOT, "tools", "extend_stk.py"), "-assembly", "all.2bit", "-input", "in.stk", "-L", "400", "-bandwidth", "40"]
    r = subprocess.run(tool + ["-outdir", "out", "-dist"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    one = subprocess.run(tool + ["-outdir", "one", "-dist", "-one_by_one"], cwd=tmp_path, capture_output=True, text=True)
    assert one.returncode == 0, one.stdout + one.stderr
    checked = 0
    for k, rows in enumerate(fams):
        if sum(1 for row in rows if row[3] or row[4]) <= 3:
            continue
        matrix, minimp = stk.choose_scoring(mdiv[k])
        run_cli(["-twobit", "all.2bit", "-L", "400", "-bandwidth", "40", "-matrix", matrix, "-minimprovement", str(minimp), "-vvv",
                 "-ranges", f"out/fam{k}-linup.tsv", "-outdist", f"s{k}.dist"], tmp_path)
        want = open(tmp_path / f"s{k}.dist").read()
        assert want.count("\n#") == 3 and open(tmp_path / "out" / f"fam{k}-dist.tsv").read() == want == open(tmp_path / "one" / f"fam{k}-dist.tsv").read()
        checked += 1
    assert checked >= 1
