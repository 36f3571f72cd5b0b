"""`RAMExtend -outpileup / -outrefined / -refine`: the files equal the renderers of tests/pileup_ref.py on the oracle's
consensus, every other output is what it is without the options, and the eighth and ninth field of a -batch line give the same
files."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd import _lib
from repeatafterme_amd.datamodel import new_master
from repeatafterme_amd.loader import load_sequence_subset_minimal, write_ranges, write_twobit

import align_ref as ar
import pileup_ref as pr
from helpers import make_genome

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def run_cli(args, cwd):
    r = subprocess.run([_lib.CLI_PATH] + args, cwd=cwd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return "\n".join(l for l in r.stdout.splitlines() if not l.startswith("Program duration is"))


def expected(twobit, ranges, matrix, W, L, stopafter, max_replays, cap=None):
    """(pileup text with the refined blocks, pileup text without, refined FASTA, replays per direction)"""
    fs = load_sequence_subset_minimal(twobit, ranges, L + W)
    kw = dict(cappenalty=cap) if cap is not None else {}
    p = po.Params.named(matrix, bandwidth=W, L=L, when_to_stop=stopafter, **kw)
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    cores, master = fs.cores, new_master(L)
    blocks, plain, refined = {}, {}, {}
    for direction in (1, 0):
        before = cores.copy()
        o = po.oracle_extend(direction, cores, seq, master, p, trace=True)
        kept = o.col_base[:o.ret]
        cols = pr.pileup(direction, before, seq, p, kept)
        cons, rcols, replays, conv = pr.refine(direction, before, seq, p, kept, max_replays)
        blocks[direction] = (cols, rcols if replays > 1 else None)
        plain[direction] = (cols, None)
        refined[direction] = (cons, replays, conv)
        if direction:
            ar.overlap_avoidance(fs)
    return pr.render_pileup(blocks), pr.render_pileup(plain), pr.render_refined(refined), [refined[d][1] for d in (1, 0)]


def check(tmp_path, twobit, ranges, extra, matrix, W, L, stopafter, cap=None):
    outs = lambda tag: ["-cons", str(tmp_path / f"{tag}.cons"), "-outtsv", str(tmp_path / f"{tag}.tsv"), "-outfa", str(tmp_path / f"{tag}.fa"),
                        "-outaln", str(tmp_path / f"{tag}.a2m")]
    base = ["-twobit", twobit, "-ranges", ranges] + extra
    plain = run_cli(base + outs("p"), tmp_path)
    with_new = run_cli(base + outs("n") + ["-outpileup", str(tmp_path / "n.pileup"), "-outrefined", str(tmp_path / "n.refined")], tmp_path)
    # stdout and every other output: byte for byte what they are without the options
    assert with_new == plain.replace(str(tmp_path / "p."), str(tmp_path / "n."))
    for ext in ("cons", "tsv", "fa", "a2m"):
        assert open(tmp_path / f"n.{ext}").read() == open(tmp_path / f"p.{ext}").read(), ext
    both, alone, fasta, replays = expected(twobit, ranges, matrix, W, L, stopafter, 10, cap)
    assert open(tmp_path / "n.pileup").read() == both
    assert open(tmp_path / "n.refined").read() == fasta
    # the pileup alone: no replay beyond the first, no refined block; -refine without -outrefined changes nothing
    run_cli(base + ["-outpileup", str(tmp_path / "o.pileup"), "-refine", "3"], tmp_path)
    assert open(tmp_path / "o.pileup").read() == alone
    # -refine 1 is "pileup only"
    run_cli(base + ["-outrefined", str(tmp_path / "r1.refined"), "-refine", "1"], tmp_path)
    assert open(tmp_path / "r1.refined").read() == expected(twobit, ranges, matrix, W, L, stopafter, 1, cap)[2]
    return both, fasta, replays


def test_on_the_reference_test_family(tmp_path):
    both, fasta, replays = check(tmp_path, os.path.join(G, "inputs", "extension-test2.2bit"), os.path.join(G, "inputs", "extension-test2.tsv"),
                                 [], "20p43g", 14, 10000, 100)
    assert len(both.splitlines()) > 20 and fasta.count(">") == 2


def test_on_a_synthetic_genome(tmp_path):
    recs, rows = make_genome(14)
    write_twobit(str(tmp_path / "g.2bit"), recs)
    write_ranges(str(tmp_path / "g.tsv"), rows)
    extra = ["-bandwidth", "14", "-matrix", "25p43g", "-L", "300", "-stopafter", "20"]
    both, fasta, replays = check(tmp_path, str(tmp_path / "g.2bit"), str(tmp_path / "g.tsv"), extra, "25p43g", 14, 300, 20)
    body = [l.split("\t") for l in both.splitlines()[1:]]
    assert replays == [1, 2] and {l[0] for l in body} == {"right", "left", "left-refined"}     # the left consensus moves once
    assert sum(int(l[9]) for l in body) > 0 and sum(int(l[10]) for l in body) > 0


def test_in_a_batch_equals_single_runs(tmp_path):
    """The eighth and ninth field of a -batch line, alone ("-" before them) and beside the others; shorter lines keep working."""
    records, fams = [], []
    for k, seed in enumerate((14, 7, 9)):
        recs, rows = make_genome(seed)
        records += [(f"f{k}_" + name, seq) for name, seq in recs]
        fams.append([(f"f{k}_" + r[0],) + tuple(r[1:]) for r in rows])
    write_twobit(str(tmp_path / "all.2bit"), records)
    common = ["-twobit", "all.2bit", "-bandwidth", "14", "-matrix", "25p43g", "-L", "300", "-stopafter", "20", "-cappenalty", "-10", "-refine", "4"]
    tails = [["-", "-", "b0.pileup", "b0.refined"], ["b1.profile", "b1.a2m", "-", "b1.refined"], ["-", "b2.a2m"]]
    with open(tmp_path / "batch.list", "w") as fh:
        for k, rows in enumerate(fams):
            write_ranges(str(tmp_path / f"fam{k}.tsv"), rows)
            fh.write("\t".join([f"fam{k}.tsv", f"b{k}.log", f"b{k}.cons", f"b{k}.tsv", f"b{k}.fa"] + tails[k]) + "\n")
    r = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "batch.list"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(tmp_path / "b1.pileup") and not os.path.exists(tmp_path / "b2.refined") and not os.path.exists(tmp_path / "b0.a2m")
    for k in range(3):
        s = subprocess.run([_lib.CLI_PATH] + common + ["-ranges", f"fam{k}.tsv", "-cons", f"s{k}.cons", "-outtsv", f"s{k}.tsv", "-outfa", f"s{k}.fa",
                                                       "-outaln", f"s{k}.a2m", "-outpileup", f"s{k}.pileup", "-outrefined", f"s{k}.refined"],
                           cwd=tmp_path, capture_output=True, text=True)
        assert s.returncode == 0, s.stderr
        for ext in ("tsv", "fa"):
            assert open(tmp_path / f"s{k}.{ext}").read() == open(tmp_path / f"b{k}.{ext}").read()
        if k != 2:
            assert open(tmp_path / f"s{k}.refined").read() == open(tmp_path / f"b{k}.refined").read(), k
        if k == 0:
            assert open(tmp_path / "s0.pileup").read() == open(tmp_path / "b0.pileup").read()
            assert len(open(tmp_path / "b0.pileup").read().splitlines()) > 10
        if k:
            assert open(tmp_path / f"s{k}.a2m").read() == open(tmp_path / f"b{k}.a2m").read(), k
    # with -batch the single-family options are refused
    bad = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "batch.list", "-outpileup", "x.pileup"], cwd=tmp_path, capture_output=True, text=True)
    assert bad.returncode != 0 and "eighth field" in bad.stderr
