"""`RAMExtend -outcopies` and the copies sink of seam 1: the TSV equals the rendering of tests/copystats_ref.py on the oracle's
kept consensus (integers and ids exactly, the Kimura fields within one unit of their last printed digit), every other output is
what it is without the option, the tenth field of a -batch line gives the same file, and extend_alignment / extend_batch hand
over the same records beside the other sinks."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd import _lib
from repeatafterme_amd.datamodel import COPY_STATS_FIELDS, new_master
from repeatafterme_amd.loader import load_sequence_subset_minimal, write_ranges, write_twobit

import align_ref as ar
import copystats_ref as cr
import test_gpu_align as ta
import test_gpu_pileup as tp
from helpers import make_genome, to_extend_params
from test_gpu_align_cli import fa_records, run_cli

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def expected_text(twobit, ranges, matrix, W, L, stopafter, names, cap=None):
    """The file as the helper renders it: the oracle's two directions with the overlap avoidance between them, the restatement on
    every extendable core along the kept consensus, rows reversed on the left.  -> (text, the records of both directions)"""
    fs = load_sequence_subset_minimal(twobit, ranges, L + W)
    p = po.Params.named(matrix, bandwidth=W, L=L, when_to_stop=stopafter, **(dict(cappenalty=cap) if cap is not None else {}))
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    cores, master = fs.cores, new_master(L)
    blocks = {}
    for direction in (1, 0):
        before = cores.copy()
        o = po.oracle_extend(direction, cores, seq, master, p, trace=True)
        stats, idx, results = cr.copy_stats(direction, before, seq, p, o.col_base[:o.ret], with_walks=True)
        blocks[direction] = (names, idx, results, stats)
        if direction:
            ar.overlap_avoidance(fs)
    return cr.render_copies(blocks), np.concatenate([blocks[1][3], blocks[0][3]])


def check_outcopies(tmp_path, twobit, ranges, extra, matrix, W, L, stopafter):
    outs = lambda tag: ["-cons", str(tmp_path / f"{tag}.cons"), "-outtsv", str(tmp_path / f"{tag}.tsv"), "-outfa", str(tmp_path / f"{tag}.fa"),
                        "-outaln", str(tmp_path / f"{tag}.a2m"), "-outpileup", str(tmp_path / f"{tag}.pileup")]
    base = ["-twobit", twobit, "-ranges", ranges] + extra
    plain = run_cli(base + outs("p"), tmp_path)
    with_new = run_cli(base + outs("n") + ["-outcopies", str(tmp_path / "n.copies")], tmp_path)
    # stdout and every other output: byte for byte what they are without the option
    assert with_new == plain.replace(str(tmp_path / "p."), str(tmp_path / "n."))
    for ext in ("cons", "tsv", "fa", "a2m", "pileup"):
        assert open(tmp_path / f"n.{ext}").read() == open(tmp_path / f"p.{ext}").read(), ext
    fa = fa_records(tmp_path / "n.fa")
    got = open(tmp_path / "n.copies").read()
    want, stats = expected_text(twobit, ranges, matrix, W, L, stopafter, {n: v[0] for n, v in fa.items()})
    cr.same_copies_text(got, want)
    # the flag alone writes the same file
    run_cli(base + ["-outcopies", str(tmp_path / "o.copies")], tmp_path)
    assert open(tmp_path / "o.copies").read() == got
    return got, stats


def test_outcopies_on_the_reference_test_family(tmp_path):
    got, stats = check_outcopies(tmp_path, os.path.join(G, "inputs", "extension-test2.2bit"), os.path.join(G, "inputs", "extension-test2.tsv"),
                                 [], "20p43g", 14, 10000, 100)
    lines = got.splitlines()
    assert lines[0].split("\t")[:3] == ["dir", "copy", "end_row"] and sum(l.startswith("#") for l in lines) == 2
    # the copies of this family are identical over their extensions: every divergence is 0, printed as such (the synthetic
    # family of the batch test is the one with substitutions and gaps)
    assert len(lines) >= 1 + 5 + 2 and (stats["cols"] > 0).sum() >= 4 and stats["match"].sum() > 0
    assert {l.split("\t")[-1] for l in lines[1:] if not l.startswith("#")} == {"0.0000"} and lines[-1].endswith("\tkimura=0.0000")


def _batch_families(tmp_path):
    records, fams = [], []
    for k, seed in enumerate((14, 7)):
        recs, rows = make_genome(seed)
        records += [(f"f{k}_" + name, seq) for name, seq in recs]
        fams.append([(f"f{k}_" + r[0],) + tuple(r[1:]) for r in rows])
    write_twobit(str(tmp_path / "all.2bit"), records)
    for k, rows in enumerate(fams):
        write_ranges(str(tmp_path / f"fam{k}.tsv"), rows)
    return ["-twobit", "all.2bit", "-bandwidth", "14", "-matrix", "25p43g", "-L", "300", "-stopafter", "20", "-cappenalty", "-10"]


def test_outcopies_in_a_batch_is_the_tenth_field(tmp_path):
    """A synthetic family whose paths hold insertions and deletions, through the tenth field of its -batch line ("-" in the four
    before it), beside a family whose line stops at the fifth; the bare flag with -batch is refused."""
    common = _batch_families(tmp_path)
    tails = [["-", "-", "-", "-", "b0.copies"], []]
    with open(tmp_path / "batch.list", "w") as fh:
        for k in range(2):
            fh.write("\t".join([f"fam{k}.tsv", f"b{k}.log", f"b{k}.cons", f"b{k}.tsv", f"b{k}.fa"] + tails[k]) + "\n")
    r = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "batch.list"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(tmp_path / "b1.copies") and not os.path.exists(tmp_path / "-")
    # the other files of both families are those of a batch without the tenth field
    with open(tmp_path / "plain.list", "w") as fh:
        for k in range(2):
            fh.write("\t".join([f"fam{k}.tsv", f"q{k}.log", f"q{k}.cons", f"q{k}.tsv", f"q{k}.fa"]) + "\n")
    q = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "plain.list"], cwd=tmp_path, capture_output=True, text=True)
    assert q.returncode == 0, q.stderr
    for k in range(2):
        for ext in ("cons", "tsv", "fa"):
            assert open(tmp_path / f"b{k}.{ext}").read() == open(tmp_path / f"q{k}.{ext}").read(), (k, ext)
    fa = fa_records(tmp_path / "b0.fa")
    got = open(tmp_path / "b0.copies").read()
    want, stats = expected_text(str(tmp_path / "all.2bit"), str(tmp_path / "fam0.tsv"), "25p43g", 14, 300, 20, {n: v[0] for n, v in fa.items()},
                                cap=-10)
    assert stats["del"].sum() > 0 and stats["ins"].sum() > 0 and stats["ts"].sum() > 0 and (stats["cols"] > 0).sum() > 2
    cr.same_copies_text(got, want)
    # ... and of the stand-alone run
    run_cli(common + ["-ranges", "fam0.tsv", "-outcopies", "s0.copies"], tmp_path)
    assert open(tmp_path / "s0.copies").read() == got
    bad = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "batch.list", "-outcopies", "x.copies"], cwd=tmp_path, capture_output=True, text=True)
    assert bad.returncode != 0 and "tenth field" in bad.stderr and not os.path.exists(tmp_path / "x.copies")


def same_copies(cp, direction, family, cores, seq, p, kept, tag):
    want, widx, results = cr.copy_stats(direction, cores, seq, p, kept, with_walks=True)
    assert (cp.direction, cp.family) == (direction, family), tag
    assert np.array_equal(cp.cons, kept) and list(cp.core_index) == widx and len(cp.flanks) == len(widx), tag
    for k in COPY_STATS_FIELDS:
        assert np.array_equal(cp.stats[k], want[k]), (tag, k)
    tp.same_ends(cp.ends, results, tag)
    return want


def test_the_copies_sink_beside_the_other_sinks():
    """extend_alignment(copies=True) alone and with profile, align and refine: the Copies come last, the other results are what
    they are without it, and the records are the restatement's along the kept consensus."""
    from repeatafterme_amd.extend import extend_alignment
    c = cr.shape_case(*tp.SHAPES[2], 1, "kept")
    fs, seq, p = c["fs"], c["seq"], c["p"]
    ep = to_extend_params(p)
    seen = 0
    for direction in (1, 0):
        c0, m0 = fs.cores.copy(), new_master(p.L)
        info0, prof0, al0, rf0 = extend_alignment(direction, c0, seq, m0, ep, profile=True, align=True, refine=3)
        c1, m1 = fs.cores.copy(), new_master(p.L)
        info1, prof1, al1, rf1, cp1 = extend_alignment(direction, c1, seq, m1, ep, profile=True, align=True, refine=3, copies=True)
        c2, m2 = fs.cores.copy(), new_master(p.L)
        info2, cp2 = extend_alignment(direction, c2, seq, m2, ep, copies=True)
        assert info0.ret == info1.ret == info2.ret > 0 and np.array_equal(m0, m1) and np.array_equal(m0, m2)
        for key in ("left_len", "right_len", "score"):
            assert np.array_equal(getattr(c0, key), getattr(c1, key)) and np.array_equal(getattr(c0, key), getattr(c2, key)), key
        assert np.array_equal(prof0.cols, prof1.cols) and np.array_equal(rf0.cols, rf1.cols) and np.array_equal(rf0.refined_cons, rf1.refined_cons)
        for key in ("cons", "ends", "col_idx", "col_ins"):
            assert np.array_equal(getattr(al0, key), getattr(al1, key)), key
        kept = al1.cons
        want = same_copies(cp1, direction, 0, fs.cores, seq, p, kept, f"dir={direction} beside the others")
        same_copies(cp2, direction, 0, fs.cores, seq, p, kept, f"dir={direction} alone")
        assert np.array_equal(cp1.ends, al1.ends) and np.array_equal(cp1.flanks, al1.flanks)
        seen += int(want["ts"].sum() > 0 and want["del"].sum() > 0)
    assert seen == 2


def test_the_copies_sink_in_a_batch():
    """extend_batch(copies=True) with profile and align on three families that keep different numbers of columns: one Copies per
    family, last in the tuple, equal to the single runs' and to the restatement."""
    from repeatafterme_amd.extend import extend_alignment, extend_batch
    p = ta.params("20p43g", 14, 120, -10, when_to_stop=25)
    ep = to_extend_params(p)
    fams = ta._three_families()
    batch = [(fs.cores.copy(), fs.sequence, new_master(120)) for fs in fams]
    single = [(fs.cores.copy(), new_master(120)) for fs in fams]
    for direction in (1, 0):
        before = [b[0].copy() for b in batch]
        infos, profs, als, cps = extend_batch(direction, batch, ep, profile=True, align=True, copies=True)
        only = extend_batch(direction, [(b.copy(), fs.sequence, new_master(120)) for b, fs in zip(before, fams)], ep, copies=True)
        assert len(cps) == 3 and len(only) == 2 and len(only[1]) == 3 and len({i.ret for i in infos}) > 1
        for f, fs in enumerate(fams):
            tag = f"family {f} dir={direction}"
            kept = als[f].cons
            assert len(kept) == infos[f].ret
            want = same_copies(cps[f], direction, f, before[f], np.ascontiguousarray(fs.sequence, np.int8), p, kept, tag)
            assert np.array_equal(cps[f].flanks, als[f].flanks) and np.array_equal(cps[f].ends, als[f].ends), tag
            assert np.array_equal(only[1][f].stats, cps[f].stats), tag
            s_info, s_cp = extend_alignment(direction, single[f][0], fs.sequence, single[f][1], ep, copies=True)
            assert s_info.ret == infos[f].ret and np.array_equal(s_cp.stats, cps[f].stats) and np.array_equal(s_cp.flanks, cps[f].flanks), tag
            assert f == 0 or want["cols"].sum() > 0


def test_extend_stk_copies(tmp_path):
    """tools/extend_stk.py -copies: <id>-copies.tsv per family is the stand-alone run's file, through -batch and one by one, and
    every direction's divergence is printed beside the matrix the ladder picks for it."""
    import sys
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
    r = subprocess.run(tool + ["-outdir", "out", "-copies"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    one = subprocess.run(tool + ["-outdir", "one", "-copies", "-one_by_one"], cwd=tmp_path, capture_output=True, text=True)
    assert one.returncode == 0, one.stdout + one.stderr
    plain = subprocess.run(tool + ["-outdir", "plain"], cwd=tmp_path, capture_output=True, text=True)
    assert plain.returncode == 0 and "Extension divergence" not in plain.stdout and not os.path.exists(tmp_path / "plain" / "fam0-copies.tsv")
    checked = 0
    for k, rows in enumerate(fams):
        if sum(1 for row in rows if row[3] or row[4]) <= 3:
            continue
        matrix, minimp = stk.choose_scoring(mdiv[k])
        run_cli(["-twobit", "all.2bit", "-L", "400", "-bandwidth", "40", "-matrix", matrix, "-minimprovement", str(minimp), "-vvv",
                 "-ranges", f"out/fam{k}-linup.tsv", "-outcopies", f"s{k}.copies"], tmp_path)
        want = open(tmp_path / f"s{k}.copies").read()
        assert want.count("\n") > 3 and open(tmp_path / "out" / f"fam{k}-copies.tsv").read() == want == open(tmp_path / "one" / f"fam{k}-copies.tsv").read()
        for ext in ("ext-cons.fa", "repam-ranges.tsv", "repam-repseq.fa"):
            assert open(tmp_path / "out" / f"fam{k}-{ext}").read() == open(tmp_path / "plain" / f"fam{k}-{ext}").read(), (k, ext)
        for line in (l for l in want.splitlines() if l.startswith("#")):
            tag, copies, used, kim = line[1:].split("\t")
            div = float(kim.split("=")[1])
            said = f"  - Extension divergence [{tag}]: {div:.2f} % over {used.split('=')[1]} of {copies.split('=')[1]} copies: " \
                   f"matrix {stk.choose_scoring(div)[0]} (used: {matrix})"
            assert said in r.stdout and said in one.stdout, said
        checked += 1
    assert checked >= 1
