"""`RAMExtend -outperiod`: on a planted family whose right extension runs into a (CA)n every row of the file equals the
restatement (tests/period_ref.py) on the oracle's extents, the summary lines equal its summary and the modal period of the right
part is 2; -periodwhole adds the third part; the fifteenth field of a -batch line gives the same file; the bare flag with -batch
and bad parameters are refused before anything runs; the Python wrapper and tools/extend_stk.py -period."""
import os
import subprocess
import sys

import numpy as np
import pytest

from repeatafterme_amd import _lib
from repeatafterme_amd.datamodel import new_master
from repeatafterme_amd.loader import write_ranges, write_twobit

import period_ref as pr
from helpers import to_extend_params
from test_gpu_align_cli import run_cli
from test_gpu_tsd_cli import ranges_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, W = 300, 14
COMMON = ["-bandwidth", str(W), "-matrix", "20p43g", "-L", str(L)]
COLUMNS = ["core", "seqid", "start", "end", "strand", "part", "length", "period", "units", "score", "region_start", "region_end",
           "agree", "disagree", "unit"]
PARTS = ["left", "right", "whole"]


def parse_period(path):
    """-> (the #period fields, {part: #part fields}, {part: #consensus fields}, rows)"""
    params, part, cons, rows = None, {}, {}, []
    for line in open(path).read().splitlines():
        f = line.split("\t")
        if line.startswith("#"):
            kv = dict(x.split("=") for x in f[1:])
            if f[0] == "#period":
                params = kv
                continue
            assert f[0] in ("#part", "#consensus")
            name = kv.pop("part")
            (part if f[0] == "#part" else cons)[name] = {k: int(v) for k, v in kv.items()}
        elif f[0] == "core":
            assert f == COLUMNS
        else:
            rows.append(dict(zip(COLUMNS, f)))
    return params, part, cons, rows


def check_file(path, tsv_path, genome, cores_after, master, rets, parts, params=None):
    """Every row against the restatement on the extents of cores_after (one record at offset 0: library positions are the
    file's coordinates minus one), the region and its first bases against the genome, the summary lines against the rows."""
    params = {**pr.DEFAULT, **(params or {})}
    head, part, cons, rows = parse_period(path)
    assert head == {k: str(v) for k, v in params.items()}
    tsv = [l.split("\t") for l in open(tsv_path).read().splitlines()]
    M = cores_after.n
    assert len(rows) == M * len(parts) and len(tsv) == M and list(part) == parts and list(cons) == parts
    letters = "ACGT"
    for w, name in enumerate(parts):
        segs = pr.segments_of(cores_after, w)
        want = pr.records(genome, segs, **params)
        mine = rows[w::len(parts)]
        for i, (r, t, (lo, hi), rec) in enumerate(zip(mine, tsv, segs, want)):
            assert [r["seqid"], r["start"], r["end"], r["strand"]] == t[:4] and int(r["core"]) == i and r["part"] == name
            assert int(r["length"]) == hi + 1 - lo
            got = tuple(int(r[k]) for k in ("period", "score", "agree", "disagree"))
            assert got == (rec[0], rec[1], rec[4], rec[5]), (name, i, r, rec)
            if rec[0]:
                a, b = lo + rec[2], lo + rec[3] + rec[0]
                assert (int(r["region_start"]), int(r["region_end"])) == (a + 1, b + 1)
                assert r["units"] == "%.2f" % ((rec[3] - rec[2] + 1 + rec[0]) / rec[0])
                assert r["unit"] == "".join(letters[genome[p] & 3] for p in range(a, a + min(rec[0], 32)))
            else:
                assert (r["units"], r["region_start"], r["region_end"], r["unit"]) == ("0.00", "0", "0", "-")
        assert part[name] == pr.summary(want, segs)
    p = len(master) // 2 - 1                    # the master holds L rows to the left of the core and L to the right
    left = master[p - rets[0]:p]                # in reading order: the rows run outward from the core
    right = master[p + 1:p + 1 + rets[1]]
    seqs = {"left": left, "right": right, "whole": np.concatenate((left, right))}
    for name in parts:
        rec = pr.record_of_codes(seqs[name], **params)
        assert cons[name] == dict(length=len(seqs[name]), period=rec[0], score=rec[1], start=rec[2], end=rec[3], agree=rec[4], disagree=rec[5]), name
    return part


def test_outperiod_on_the_planted_family(tmp_path):
    e = pr.planted_expectation()
    write_twobit(str(tmp_path / "g.2bit"), [("chrP", e["seq"])])
    write_ranges(str(tmp_path / "fam.tsv"), ranges_of("chrP", e["cores"]))
    base = ["-twobit", "g.2bit", "-ranges", "fam.tsv"] + COMMON
    outs = lambda tag: ["-outtsv", str(tmp_path / f"{tag}.tsv"), "-cons", str(tmp_path / f"{tag}.cons"), "-outfa", str(tmp_path / f"{tag}.fa")]      # noqa: E731
    plain = run_cli(base + outs("p"), tmp_path)
    with_new = run_cli(base + outs("n") + ["-outperiod", "n.period"], tmp_path)
    assert with_new == plain.replace(str(tmp_path / "p."), str(tmp_path / "n."))
    for ext in ("tsv", "cons", "fa"):
        assert open(tmp_path / f"n.{ext}").read() == open(tmp_path / f"p.{ext}").read(), ext
    rets = [e["rets"][0], e["rets"][1]]
    part = check_file(tmp_path / "n.period", tmp_path / "n.tsv", e["seq"], e["after"], e["master"], rets, PARTS[:2])
    # the planted family's modal period through the CLI
    assert part["right"]["mode"] == 2 and 2 * part["right"]["mode_count"] >= pr.PLANTED["M"] and part["left"]["n_tract"] == 0
    # with the whole element as a third part; the first two are what they were
    run_cli(base + ["-outperiod", "w.period", "-periodwhole", "-outtsv", "w.tsv"], tmp_path)
    part3 = check_file(tmp_path / "w.period", tmp_path / "w.tsv", e["seq"], e["after"], e["master"], rets, PARTS)
    assert part3["whole"]["mode"] == 2 and {k: part3[k] for k in PARTS[:2]} == part
    # the one-byte library of the reference gives the same file, and other parameters another
    r = subprocess.run([_lib.CLI_PATH] + base + ["-outperiod", "b.period"], cwd=tmp_path, capture_output=True, text=True, env=dict(os.environ, RAMX_CLI_BYTES="1"))
    assert r.returncode == 0 and open(tmp_path / "b.period").read() == open(tmp_path / "n.period").read()
    run_cli(base + ["-outperiod", "s.period", "-outtsv", "s.tsv", "-periodmax", "1", "-periodmm", "1", "-periodmin", "8"], tmp_path)
    other = check_file(tmp_path / "s.period", tmp_path / "s.tsv", e["seq"], e["after"], e["master"], rets, PARTS[:2], dict(pmax=1, mm=1, min_score=8))
    assert other["right"]["mode"] in (0, 1) and other["right"]["n_simple"] == 0
    for flag, value, word in (("-periodmax", "8193", "pmax"), ("-periodmax", "0", "pmax"), ("-periodmm", "16", "mm"), ("-periodmm", "0", "mm"),
                              ("-periodmin", "0", "min_score")):
        bad = subprocess.run([_lib.CLI_PATH] + base + ["-outperiod", "x.period", "-outtsv", "x.tsv", flag, value], cwd=tmp_path, capture_output=True, text=True)
        assert bad.returncode != 0 and word in bad.stderr and not os.path.exists(tmp_path / "x.period") and not os.path.exists(tmp_path / "x.tsv"), flag


def test_outperiod_in_a_batch_is_the_fifteenth_field(tmp_path):
    fams = [pr.planted_family(M=14, seed=21), pr.planted_family(M=9, seed=22)]
    write_twobit(str(tmp_path / "all.2bit"), [(f"chr{i}", f[0]) for i, f in enumerate(fams)])
    for i, f in enumerate(fams):
        write_ranges(str(tmp_path / f"fam{i}.tsv"), ranges_of(f"chr{i}", f[1]))
    common = ["-twobit", "all.2bit"] + COMMON
    tails = [["-"] * 9 + ["b0.period"], [], ["-"] * 9 + ["b2.period"]]
    order = [0, 1, 1]                 # the family in the middle asks for nothing
    with open(tmp_path / "batch.list", "w") as fh:
        for j, i in enumerate(order):
            fh.write("\t".join([f"fam{i}.tsv", f"b{j}.log", f"b{j}.cons", f"b{j}.tsv", f"b{j}.fa"] + tails[j]) + "\n")
    r = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "batch.list", "-periodwhole"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(tmp_path / "b1.period") and not os.path.exists(tmp_path / "-")
    for j, i in ((0, 0), (2, 1)):
        run_cli(common + ["-ranges", f"fam{i}.tsv", "-outperiod", f"s{j}.period", "-periodwhole"], tmp_path)
        got = open(tmp_path / f"b{j}.period").read()
        assert got == open(tmp_path / f"s{j}.period").read()
        head, part, cons, rows = parse_period(tmp_path / f"b{j}.period")
        assert len(rows) == 3 * (14, 9)[i] and part["right"]["mode"] == 2 and part["whole"]["mode"] == 2
    # the other files are those of a batch without the field
    with open(tmp_path / "plain.list", "w") as fh:
        for j, i in enumerate(order):
            fh.write("\t".join([f"fam{i}.tsv", f"q{j}.log", f"q{j}.cons", f"q{j}.tsv", f"q{j}.fa"]) + "\n")
    q = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "plain.list"], cwd=tmp_path, capture_output=True, text=True)
    assert q.returncode == 0 and q.stdout == r.stdout
    for j in range(3):
        for ext in ("cons", "tsv", "fa"):
            assert open(tmp_path / f"b{j}.{ext}").read() == open(tmp_path / f"q{j}.{ext}").read(), (j, ext)
    bad = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "batch.list", "-outperiod", "x.period"], cwd=tmp_path, capture_output=True, text=True)
    assert bad.returncode != 0 and "fifteenth field" in bad.stderr and not os.path.exists(tmp_path / "x.period")


def test_the_wrapper_in_a_batch():
    """extend_batch(period=...) hands every family's records of the direction it ran behind its RunInfos."""
    from repeatafterme_amd.datamodel import PeriodParams
    from repeatafterme_amd.extend import extend_batch
    from oracle import pyoracle as po
    p = pr.planted_expectation()["p"]
    fams = [pr.planted_family(M=14, seed=21)[:2], pr.planted_family(M=9, seed=22)[:2]]
    batch = [(c.copy(), s, new_master(p.L)) for s, c in fams]
    infos, recs = extend_batch(1, batch, to_extend_params(p), period=PeriodParams(64, 3, 16))
    assert len(infos) == 2 and [len(r) for r in recs] == [14, 9]
    for (s, c0), (c, _, m), rec in zip(fams, batch, recs):
        oc, om = c0.copy(), new_master(p.L)
        po.oracle_extend(1, oc, s, om, p)
        assert np.array_equal(c.right_len, oc.right_len)
        want = pr.records(s, pr.segments_of(oc, 1), pmax=64)
        assert [tuple(int(r[k]) for k in ("period", "score", "start", "end", "agree", "disagree")) for r in rec] == want


def test_extend_stk_period(tmp_path):
    """tools/extend_stk.py -period: <id>-period.tsv per family is the stand-alone run's file, through -batch and one by one, and
    the modal period of each part is printed; without the flag there is neither."""
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
    r = subprocess.run(tool + ["-outdir", "out", "-period"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    one = subprocess.run(tool + ["-outdir", "one", "-period", "-one_by_one"], cwd=tmp_path, capture_output=True, text=True)
    assert one.returncode == 0, one.stdout + one.stderr
    plain = subprocess.run(tool + ["-outdir", "plain"], cwd=tmp_path, capture_output=True, text=True)
    assert plain.returncode == 0 and "Tandem periodicity" not in plain.stdout and not os.path.exists(tmp_path / "plain" / "fam0-period.tsv")
    checked = 0
    for k, rows in enumerate(fams):
        if sum(1 for row in rows if row[3] or row[4]) <= 3:
            continue
        matrix, minimp = stk.choose_scoring(mdiv[k])
        run_cli(["-twobit", "all.2bit", "-L", "400", "-bandwidth", "40", "-matrix", matrix, "-minimprovement", str(minimp), "-vvv",
                 "-ranges", f"out/fam{k}-linup.tsv", "-outperiod", f"s{k}.period"], tmp_path)
        want = open(tmp_path / f"s{k}.period").read()
        assert want.count("\n") > 7 and open(tmp_path / "out" / f"fam{k}-period.tsv").read() == want == open(tmp_path / "one" / f"fam{k}-period.tsv").read()
        for ext in ("ext-cons.fa", "repam-ranges.tsv", "repam-repseq.fa"):
            assert open(tmp_path / "out" / f"fam{k}-{ext}").read() == open(tmp_path / "plain" / f"fam{k}-{ext}").read(), (k, ext)
        _, part, _, _ = parse_period(tmp_path / f"s{k}.period")
        for name in PARTS[:2]:
            h = part[name]
            said = f"  - Tandem periodicity [{name}]: period {h['mode']} in {h['mode_count']} of {h['n']} copies ({h['n_tract']} with a tract)"
            assert said in r.stdout and said in one.stdout, said
        checked += 1
    assert checked >= 1
