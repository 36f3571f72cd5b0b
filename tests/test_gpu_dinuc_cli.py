"""`RAMExtend -outcpg / -outdinuc / -cpgscore`: on the planted family of tests/cpg_cases.py the files equal the renderers of
tests/dinuc_ref.py on the oracle's consensus, the planted CpGs come back through -outcpg where -outrefined loses them, every
other output is what it is without the options, the fourteenth field of a -batch line gives the same file, and
tools/extend_stk.py -cpg writes it per family."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd import _lib
from repeatafterme_amd.datamodel import new_master
from repeatafterme_amd.loader import load_sequence_subset_minimal, write_ranges, write_twobit

import align_ref as ar
import cpg_cases as cc
import dinuc_ref as dr
import pileup_ref as pr
from helpers import make_genome

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["-bandwidth", str(cc.W), "-matrix", cc.MATRIX, "-L", str(cc.L), "-stopafter", "30"]


def run_cli(args, cwd):
    r = subprocess.run([_lib.CLI_PATH] + args, cwd=cwd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return "\n".join(l for l in r.stdout.splitlines() if not l.startswith("Program duration is"))


def write_planted(tmp_path, stem="planted", prefix="c"):
    """The planted family as a genome of one contig per copy and its ranges file."""
    fs, _, _ = cc.planted_family()
    n = fs.cores.n
    win = len(fs.sequence) // n
    recs = [(f"{prefix}{i}", fs.sequence[i * win:(i + 1) * win].astype(np.int64)) for i in range(n)]
    rows = []
    for i in range(n):
        a, b = sorted((int(fs.cores.left_pos[i]) - i * win, int(fs.cores.right_pos[i]) - i * win))
        rows.append((f"{prefix}{i}", a, b + 1, 1, 1, "-" if fs.cores.orient[i] else "+"))
    write_twobit(str(tmp_path / f"{stem}.2bit"), recs)
    write_ranges(str(tmp_path / f"{stem}.tsv"), rows)
    return recs, rows


def expected(twobit, ranges, matrix, W, L, stopafter, max_replays, cpg_ts=0):
    """-> (the -outcpg text, the -outdinuc text, the -outrefined text) of the restatements on the loader's flank set"""
    fs = load_sequence_subset_minimal(twobit, ranges, L + W)
    p = po.Params.named(matrix, bandwidth=W, L=L, when_to_stop=stopafter)
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    cores, master = fs.cores, new_master(L)
    cpg, blocks, refined = {}, {}, {}
    for direction in (1, 0):
        before = cores.copy()
        o = po.oracle_extend(direction, cores, seq, master, p, trace=True)
        kept = o.col_base[:o.ret]
        cons, cols, di, replays, conv, n_cpg = dr.refine_cpg(direction, before, seq, p, kept, max_replays, cpg_ts)
        cpg[direction], blocks[direction] = (cons, replays, conv, n_cpg), di
        rc, _, rr, rv = pr.refine(direction, before, seq, p, kept, max_replays)
        refined[direction] = (rc, rr, rv)
        if direction:
            ar.overlap_avoidance(fs)
    return dr.render_cpg(cpg), dr.render_dinuc(blocks), pr.render_refined(refined)


def planted_sites_called(fasta):
    """How many planted sites read CG in the two records of a consensus FASTA (both in reading order): -> (right, left)"""
    lines = fasta.splitlines()
    right, left = lines[1], lines[3]
    assert lines[0].startswith(">right-extension") and lines[2].startswith(">left-extension") and min(len(right), len(left)) >= cc.K
    at_left = len(left) - cc.K                          # the left ancestor ends at the core
    return (sum(right[c:c + 2] == "CG" for c in cc.site_columns()), sum(left[at_left + c:at_left + c + 2] == "CG" for c in cc.site_columns()))


def test_the_planted_family(tmp_path):
    write_planted(tmp_path)
    outs = lambda tag: ["-cons", str(tmp_path / f"{tag}.cons"), "-outtsv", str(tmp_path / f"{tag}.tsv"), "-outfa", str(tmp_path / f"{tag}.fa"),
                        "-outrefined", str(tmp_path / f"{tag}.refined")]
    base = ["-twobit", str(tmp_path / "planted.2bit"), "-ranges", str(tmp_path / "planted.tsv")] + COMMON
    plain = run_cli(base + outs("p"), tmp_path)
    with_new = run_cli(base + outs("n") + ["-outcpg", str(tmp_path / "n.cpg"), "-outdinuc", str(tmp_path / "n.dinuc")], tmp_path)
    # stdout and every other output: byte for byte what they are without the options
    assert with_new == plain.replace(str(tmp_path / "p."), str(tmp_path / "n."))
    for ext in ("cons", "tsv", "fa", "refined"):
        assert open(tmp_path / f"n.{ext}").read() == open(tmp_path / f"p.{ext}").read(), ext
    cpg, dinuc, refined = expected(str(tmp_path / "planted.2bit"), str(tmp_path / "planted.tsv"), cc.MATRIX, cc.W, cc.L, 30, 10)
    assert open(tmp_path / "n.cpg").read() == cpg
    assert open(tmp_path / "n.dinuc").read() == dinuc
    assert open(tmp_path / "n.refined").read() == refined
    # what the feature is for: the planted sites come back through -outcpg where -outrefined loses them
    assert planted_sites_called(cpg) == (8, 8)
    assert all(n < cc.N_SITES // 2 for n in planted_sites_called(refined))
    # -outcpg alone, -refine 1 and -cpgscore
    run_cli(base + ["-outcpg", str(tmp_path / "r1.cpg"), "-refine", "1"], tmp_path)
    assert open(tmp_path / "r1.cpg").read() == expected(str(tmp_path / "planted.2bit"), str(tmp_path / "planted.tsv"), cc.MATRIX, cc.W, cc.L, 30, 1)[0]
    run_cli(base + ["-outcpg", str(tmp_path / "h.cpg"), "-cpgscore", "-18"], tmp_path)
    harsh = expected(str(tmp_path / "planted.2bit"), str(tmp_path / "planted.tsv"), cc.MATRIX, cc.W, cc.L, 30, 10, cpg_ts=-18)[0]
    assert open(tmp_path / "h.cpg").read() == harsh and planted_sites_called(harsh) == (0, 0)
    run_cli(base + ["-outdinuc", str(tmp_path / "o.dinuc")], tmp_path)
    assert open(tmp_path / "o.dinuc").read() == dinuc


def test_in_a_batch_equals_single_runs(tmp_path):
    """The fourteenth field of a -batch line, alone ("-" before it) and beside others; shorter lines keep working."""
    records, fams = [], []
    for k, seed in enumerate((14, 7)):
        recs, rows = make_genome(seed)
        records += [(f"f{k}_" + name, seq) for name, seq in recs]
        fams.append([(f"f{k}_" + r[0],) + tuple(r[1:]) for r in rows])
    recs, rows = write_planted(tmp_path, prefix="f2_c")
    records += recs
    fams.append(rows)
    write_twobit(str(tmp_path / "all.2bit"), records)
    common = ["-twobit", "all.2bit"] + COMMON + ["-cappenalty", "-10", "-refine", "4"]
    tails = [["-"] * 8 + ["b0.cpg"], ["-", "-", "-", "b1.refined"], ["-", "-", "-", "b2.refined", "-", "-", "-", "-", "b2.cpg"]]
    with open(tmp_path / "batch.list", "w") as fh:
        for k, rows in enumerate(fams):
            write_ranges(str(tmp_path / f"fam{k}.tsv"), rows)
            fh.write("\t".join([f"fam{k}.tsv", f"b{k}.log", f"b{k}.cons", f"b{k}.tsv", f"b{k}.fa"] + tails[k]) + "\n")
    r = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "batch.list"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(tmp_path / "b1.cpg") and not os.path.exists(tmp_path / "b0.refined")
    for k in range(3):
        s = subprocess.run([_lib.CLI_PATH] + common + ["-ranges", f"fam{k}.tsv", "-cons", f"s{k}.cons", "-outtsv", f"s{k}.tsv", "-outfa", f"s{k}.fa",
                                                       "-outrefined", f"s{k}.refined", "-outcpg", f"s{k}.cpg"],
                           cwd=tmp_path, capture_output=True, text=True)
        assert s.returncode == 0, s.stderr
        for ext in ("tsv", "fa") + (("refined",) if k else ()) + (("cpg",) if k != 1 else ()):
            assert open(tmp_path / f"s{k}.{ext}").read() == open(tmp_path / f"b{k}.{ext}").read(), (k, ext)
    assert planted_sites_called(open(tmp_path / "b2.cpg").read()) == (8, 8)
    assert all(n < cc.N_SITES // 2 for n in planted_sites_called(open(tmp_path / "b2.refined").read()))
    # with -batch the single-family options are refused
    for flag in ("-outcpg", "-outdinuc"):
        bad = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "batch.list", flag, "x.out"], cwd=tmp_path, capture_output=True, text=True)
        assert bad.returncode != 0 and "fourteenth field" in bad.stderr


def test_extend_stk_cpg(tmp_path):
    """tools/extend_stk.py -cpg: <id>-cpg-cons.fa per family is the stand-alone run's file, through -batch and one by one; without
    the flag there is none."""
    from repeatafterme_amd import stockholm as stk
    recs, rows = write_planted(tmp_path, stem="all")
    mdiv = 14.0
    with open(tmp_path / "in.stk", "w") as fh:
        fh.write(f"# STOCKHOLM 1.0\n#=GF ID    fam0\n#=GF DE    Source:gsa, mDiv={mdiv:.2f}, all.2bit:1\n")
        for (name, s, e, lf, rf, o) in rows:
            fh.write(f"{name}:{s + 1}-{e}_{o} {'ACGT' * 3}\n")
        fh.write("//\n")
    tool = [sys.executable, os.path.join(ROOT, "tools", "extend_stk.py"), "-assembly", "all.2bit", "-input", "in.stk", "-L", str(cc.L), "-bandwidth", str(cc.W)]
    r = subprocess.run(tool + ["-outdir", "out", "-cpg"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    one = subprocess.run(tool + ["-outdir", "one", "-cpg", "-one_by_one"], cwd=tmp_path, capture_output=True, text=True)
    assert one.returncode == 0, one.stdout + one.stderr
    plain = subprocess.run(tool + ["-outdir", "plain"], cwd=tmp_path, capture_output=True, text=True)
    assert plain.returncode == 0 and not os.path.exists(tmp_path / "plain" / "fam0-cpg-cons.fa")
    matrix, minimp = stk.choose_scoring(mdiv)
    run_cli(["-twobit", "all.2bit", "-L", str(cc.L), "-bandwidth", str(cc.W), "-matrix", matrix, "-minimprovement", str(minimp), "-vvv",
             "-ranges", "out/fam0-linup.tsv", "-outcpg", "s.cpg"], tmp_path)
    want = open(tmp_path / "s.cpg").read()
    assert want.count(">") == 2 and " cpg=" in want
    assert open(tmp_path / "out" / "fam0-cpg-cons.fa").read() == want == open(tmp_path / "one" / "fam0-cpg-cons.fa").read()
    for ext in ("ext-cons.fa", "repam-ranges.tsv", "repam-repseq.fa"):
        assert open(tmp_path / "out" / f"fam0-{ext}").read() == open(tmp_path / "plain" / f"fam0-{ext}").read(), ext
