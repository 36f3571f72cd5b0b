"""`RAMExtend -outlinkage` and the linkage sink of seam 1 on the planted family of tests/linkage_ref.py, written to a .2bit as
the other CLI tests do: the TSV equals the rendering of the restatement on the oracle's kept consensus (integers and names
exactly, the two %.4f fields within one unit of their last printed digit), every other output is what it is without the option,
the eleventh field of a -batch line gives the same file, and extend_alignment / extend_batch hand over the same planes and
counts."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd import _lib
from repeatafterme_amd.datamodel import PLANE_COVER, new_master
from repeatafterme_amd.loader import load_sequence_subset_minimal, write_ranges, write_twobit

import align_ref as ar
import linkage_ref as lr
import pileup_ref as pr
from helpers import make_genome, to_extend_params
from test_gpu_align_cli import run_cli

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_planted(tmp_path, prefix=""):
    """The planted family as a genome of one record per copy and its ranges -> the options the runs share."""
    fs, seq, p, _, _ = lr.planted_family()
    n, win = fs.cores.n, len(seq) // fs.cores.n
    recs, rows = [], []
    for i in range(n):
        lo = int(min(fs.cores.left_pos[i], fs.cores.right_pos[i])) - i * win
        hi = int(max(fs.cores.left_pos[i], fs.cores.right_pos[i])) - i * win
        recs.append((f"{prefix}c{i}", seq[i * win:(i + 1) * win]))
        rows.append((f"{prefix}c{i}", lo, hi + 1, 1, 1, "-" if fs.cores.orient[i] else "+"))
    return recs, rows


COMMON = ["-bandwidth", "20", "-matrix", "14p43g", "-L", "80", "-stopafter", "30"]


def expected(twobit, ranges, count=4, permille=100, score=3):
    """-> (the file as the helper renders it, {direction: (planes, co, pairs)})"""
    fs = load_sequence_subset_minimal(twobit, ranges, 80 + 20)
    p = po.Params.named("14p43g", bandwidth=20, L=80, when_to_stop=30)
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    cores, master = fs.cores, new_master(80)
    blocks = {}
    for direction in (1, 0):
        before = cores.copy()
        o = po.oracle_extend(direction, cores, seq, master, p, trace=True)
        cons = o.col_base[:o.ret]
        cols, idx, results = pr.pileup(direction, before, seq, p, cons, with_walks=True)
        pl = lr.planes_of(direction, before, idx, results, seq, 20, cons)
        sel = lr.select(cons, cols, count, permille, 1024)
        blocks[direction] = (sel, lr.gram(pl, sel))
        if direction:
            ar.overlap_avoidance(fs)
    return lr.render_linkage(blocks, score), blocks


@pytest.fixture(scope="module")
def planted_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("linkage")
    recs, rows = write_planted(tmp)
    write_twobit(str(tmp / "g.2bit"), recs)
    write_ranges(str(tmp / "g.tsv"), rows)
    base = ["-twobit", "g.2bit", "-ranges", "g.tsv"] + COMMON
    outs = lambda tag: ["-cons", f"{tag}.cons", "-outtsv", f"{tag}.tsv", "-outfa", f"{tag}.fa", "-outpileup", f"{tag}.pileup",
                        "-outcopies", f"{tag}.copies"]
    plain = run_cli(base + outs("p"), tmp)
    with_new = run_cli(base + outs("n") + ["-outlinkage", "n.linkage"], tmp)
    want, blocks = expected(str(tmp / "g.2bit"), str(tmp / "g.tsv"))
    return tmp, base, plain, with_new, want, blocks


def test_outlinkage_is_the_rendering_and_changes_nothing_else(planted_run):
    tmp, base, plain, with_new, want, blocks = planted_run
    assert with_new == plain.replace("p.", "n.")
    for ext in ("cons", "tsv", "fa", "pileup", "copies"):
        assert open(tmp / f"n.{ext}").read() == open(tmp / f"p.{ext}").read(), ext
    got = open(tmp / "n.linkage").read()
    lr.same_linkage_text(got, want)
    assert got.startswith(lr.LINKAGE_HEADER) and got.count("\n#") == 2
    # the flag alone writes the same file; the three options move the selection and the cut as the restatement says
    run_cli(base + ["-outlinkage", "o.linkage"], tmp)
    assert open(tmp / "o.linkage").read() == got
    run_cli(base + ["-outlinkage", "q.linkage", "-linkcount", "6", "-linkfrac", "150", "-linkscore", "1"], tmp)
    want_q, _ = expected(str(tmp / "g.2bit"), str(tmp / "g.tsv"), 6, 150, 1)
    lr.same_linkage_text(open(tmp / "q.linkage").read(), want_q)
    assert want_q != want


@pytest.mark.parametrize("direction", [1, 0])
def test_the_planted_pairs_are_the_only_lines_of_each_block(planted_run, direction):
    """The left block holds the three planted pairs and nothing else.  The right block holds them and a fourth line, first in (p, q)
    order: column 0 deleted with bases inserted before column 1 at 7.5224, the measured exception that
    tests/test_linkage_ref.py::test_the_planted_family names and counts."""
    tmp, _, _, _, _, _ = planted_run
    tag = "right" if direction else "left"
    lines = [l.split("\t") for l in open(tmp / "n.linkage").read().splitlines() if l.startswith(tag + "\t")]
    print(tag, [(l[1], l[2], l[4], l[5], l[12]) for l in lines])
    assert {(l[1], l[4]) for l in lines} >= {("8", "30"), ("8", "55"), ("30", "55")}
    if direction:
        assert len(lines) == 4 and lines[0][1:7] == ["0", "del", "9", "1", "ins", "7"] and lines[0][7:11] == ["70", "9", "7", "7"]
        assert lines[0][12] == "7.5224"
        lines = lines[1:]
    assert len(lines) == 3 and {(l[1], l[4]) for l in lines} == {("8", "30"), ("8", "55"), ("30", "55")}


def test_the_linkage_sink(planted_run):
    """extend_alignment(linkage=...) alone and beside the copies sink: the Linkage comes last, and its planes and counts are the
    restatement's along the kept consensus."""
    from repeatafterme_amd.extend import extend_alignment
    fs, seq, p, cons, _ = lr.planted_family()
    ep = to_extend_params(p)
    for direction in (1, 0):
        c = lr.planted_case(direction)
        c0, m0 = fs.cores.copy(), new_master(p.L)
        info0, cp0 = extend_alignment(direction, c0, seq, m0, ep, copies=True)
        c1, m1 = fs.cores.copy(), new_master(p.L)
        info1, cp1, lk1 = extend_alignment(direction, c1, seq, m1, ep, copies=True, linkage=True)
        c2, m2 = fs.cores.copy(), new_master(p.L)
        info2, lk2 = extend_alignment(direction, c2, seq, m2, ep, linkage=(6, 150, 4))
        assert info0.ret == info1.ret == info2.ret == len(c["cons"]) and np.array_equal(m0, m1) and np.array_equal(cp0.stats, cp1.stats)
        assert (lk1.direction, lk1.family) == (direction, 0) and np.array_equal(lk1.cons, c["cons"])
        assert np.array_equal(lk1.planes, c["sel"]) and np.array_equal(lk1.co, c["co"])
        for k in ("cover", "match", "del", "ins_open"):
            assert np.array_equal(lk1.cols[k], c["cols"][k]), k
        sel2 = lr.select(c["cons"], c["cols"], 6, 150, 4)
        assert 0 < sum(int(x["cls"]) != PLANE_COVER for x in sel2) <= 4
        assert np.array_equal(lk2.planes, sel2) and np.array_equal(lk2.co, lr.gram(c["planes"], sel2))


def test_the_sink_is_refused_under_a_collective():
    """With an allreduce callback set on seam 1's session (the single-rank stand-in for a communicator, as tests/test_gpu_sharded.py
    uses it) the loop runs, and the linkage sink fails the direction with RAMX_ERR_UNSUPPORTED: the selection needs the counts of
    every rank.  Without the sink the same call succeeds; with the callback taken away again the sink works."""
    import ctypes as C
    from repeatafterme_amd.extend import extend_alignment
    fs, seq, p, _, _ = lr.planted_family()
    ep = to_extend_params(p)
    L = _lib.lib()
    L.ramx_default_device.restype = C.c_void_p
    dev = L.ramx_default_device()
    assert dev
    cb = _lib.ALLREDUCE_CB(lambda ptr, user: None)                                 # one rank: the sums are already the total
    _lib.check(L.ramx_dev_set_allreduce_cb(dev, cb, None), "ramx_dev_set_allreduce_cb")
    try:
        plain = extend_alignment(1, fs.cores.copy(), seq, new_master(p.L), ep)
        with pytest.raises(_lib.RamxError, match=r"\(-106\).*linkage sink.*counts of every rank"):
            extend_alignment(1, fs.cores.copy(), seq, new_master(p.L), ep, linkage=True)
    finally:
        _lib.check(L.ramx_dev_set_allreduce_cb(dev, _lib.ALLREDUCE_CB(), None), "ramx_dev_set_allreduce_cb")
    info, lk = extend_alignment(1, fs.cores.copy(), seq, new_master(p.L), ep, linkage=True)
    assert info.ret == plain.ret == 70 and np.array_equal(lk.co, lr.planted_case(1)["co"])


def test_outlinkage_in_a_batch_is_the_eleventh_field(tmp_path):
    """Two families in one -batch list, the planted one with its linkage file in the eleventh field ("-" in the five before it)
    and a second one whose line names one too; the bare flag with -batch is refused."""
    recs, rows = write_planted(tmp_path, "f0_")
    recs1, rows1 = make_genome(14)
    write_twobit(str(tmp_path / "all.2bit"), recs + [("f1_" + n, s) for n, s in recs1])
    write_ranges(str(tmp_path / "fam0.tsv"), rows)
    write_ranges(str(tmp_path / "fam1.tsv"), [("f1_" + r[0],) + tuple(r[1:]) for r in rows1])
    common = ["-twobit", "all.2bit"] + COMMON
    with open(tmp_path / "batch.list", "w") as fh:
        for k in range(2):
            fh.write("\t".join([f"fam{k}.tsv", f"b{k}.log", f"b{k}.cons", f"b{k}.tsv", f"b{k}.fa", "-", "-", "-", "-", "-", f"b{k}.linkage"]) + "\n")
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
        assert not os.path.exists(tmp_path / f"q{k}.linkage")
        run_cli(common + ["-ranges", f"fam{k}.tsv", "-outlinkage", f"s{k}.linkage"], tmp_path)
        assert open(tmp_path / f"s{k}.linkage").read() == open(tmp_path / f"b{k}.linkage").read(), k
    want, blocks = expected(str(tmp_path / "all.2bit"), str(tmp_path / "fam0.tsv"))
    lr.same_linkage_text(open(tmp_path / "b0.linkage").read(), want)
    assert open(tmp_path / "b1.linkage").read().count("\n#") == 2
    bad = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "batch.list", "-outlinkage", "x.linkage"], cwd=tmp_path, capture_output=True, text=True)
    assert bad.returncode != 0 and "eleventh field" in bad.stderr and not os.path.exists(tmp_path / "x.linkage")


def test_the_linkage_sink_in_a_batch():
    """extend_batch(linkage=True) on the planted family beside a second one: one Linkage per family, last in the tuple, equal to
    the single run's."""
    from repeatafterme_amd.extend import extend_alignment, extend_batch
    from repeatafterme_amd.synth import synth_family
    fs, seq, p, _, _ = lr.planted_family()
    other = synth_family(37, 80, 20, K=50, seed=3, both_sides=True, minus_frac=0.4, n_run_frac=0.1)
    ep = to_extend_params(p)
    for direction in (1, 0):
        c = lr.planted_case(direction)
        batch = [(fs.cores.copy(), seq, new_master(80)), (other.cores.copy(), other.sequence, new_master(80))]
        infos, lks = extend_batch(direction, batch, ep, linkage=True)
        assert len(lks) == 2 and [lk.family for lk in lks] == [0, 1]
        assert np.array_equal(lks[0].planes, c["sel"]) and np.array_equal(lks[0].co, c["co"]) and np.array_equal(lks[0].cons, c["cons"])
        s_info, s_lk = extend_alignment(direction, other.cores.copy(), other.sequence, new_master(80), ep, linkage=True)
        assert s_info.ret == infos[1].ret and np.array_equal(s_lk.planes, lks[1].planes) and np.array_equal(s_lk.co, lks[1].co)
        assert np.array_equal(lks[1].co, lks[1].co.T)


def test_extend_stk_linkage(tmp_path):
    """tools/extend_stk.py -linkage: <id>-linkage.tsv per family is the stand-alone run's file, through -batch and one by one, on
    the synthetic genome the tool's other tests use (the ce10-fam*.stk inputs have no genome in the repository)."""
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
    r = subprocess.run(tool + ["-outdir", "out", "-linkage"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    one = subprocess.run(tool + ["-outdir", "one", "-linkage", "-one_by_one"], cwd=tmp_path, capture_output=True, text=True)
    assert one.returncode == 0, one.stdout + one.stderr
    checked = 0
    for k, rows in enumerate(fams):
        if sum(1 for row in rows if row[3] or row[4]) <= 3:
            continue
        matrix, minimp = stk.choose_scoring(mdiv[k])
        run_cli(["-twobit", "all.2bit", "-L", "400", "-bandwidth", "40", "-matrix", matrix, "-minimprovement", str(minimp), "-vvv",
                 "-ranges", f"out/fam{k}-linup.tsv", "-outlinkage", f"s{k}.linkage"], tmp_path)
        want = open(tmp_path / f"s{k}.linkage").read()
        assert want.count("\n#") == 2 and open(tmp_path / "out" / f"fam{k}-linkage.tsv").read() == want == open(tmp_path / "one" / f"fam{k}-linkage.tsv").read()
        for line in (l for l in want.splitlines() if l.startswith("#")):
            tag, variants, pairs, linked = line[1:].split("\t")
            said = f"  - Linked variants [{tag}]: {linked.split('=')[1]} of {pairs.split('=')[1]} pairs among {variants.split('=')[1]} variants"
            assert said in r.stdout and said in one.stdout, said
        checked += 1
    assert checked >= 1
