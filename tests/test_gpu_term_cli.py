"""`RAMExtend -outterm`: on the two planted families every row of the file equals ramx_term_flat and the restatement
(tests/term_ref.py) on the oracle's extents, the #family line equals its summary with the verdict spelled out, the #consensus
lines equal ramx_term_pair on the kept columns; every -term* flag reaches the record; the sixteenth field of a -batch line gives
the same file; the bare flag with -batch and bad parameters are refused before anything runs; the fifteen other files of a run
with every output do not change; tools/extend_stk.py -term."""
import os
import subprocess
import sys

import numpy as np
import pytest

from repeatafterme_amd import _lib
from repeatafterme_amd.datamodel import TERM_VERDICTS, TermParams
from repeatafterme_amd.extend import term_flat, term_pair
from repeatafterme_amd.loader import write_ranges, write_twobit

import term_ref as tr
from test_gpu_align_cli import run_cli
from test_gpu_tsd_cli import ranges_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, W = 400, 14
COMMON = ["-bandwidth", str(W), "-matrix", "20p43g", "-L", str(L)]
COLUMNS = ["core", "seqid", "start", "end", "strand", "orientation", "T", "score", "a_start", "a_end", "b_start", "b_end", "five_start",
           "five_end", "three_start", "three_end", "matches", "columns", "identity", "anchored"]
ORIENT = ["direct", "inverted"]
FLAGS = dict(tmax="-termmax", match="-termmatch", mismatch="-termmismatch", gap="-termgap", min_score="-termmin", slack="-termslack")


def parse_term(path):
    """-> (the #term fields, the #family fields, {orientation: #consensus fields}, rows)"""
    params, fam, cons, rows = None, None, {}, []
    for line in open(path).read().splitlines():
        f = line.split("\t")
        if line.startswith("#"):
            kv = dict(x.split("=") for x in f[1:])
            if f[0] == "#term":
                params = {k: int(v) for k, v in kv.items()}
            elif f[0] == "#family":
                fam = kv
            else:
                assert f[0] == "#consensus"
                name = kv.pop("orientation")
                cons[name] = {k: int(v) for k, v in kv.items()}
        elif f[0] == "core":
            assert f == COLUMNS
        else:
            rows.append(dict(zip(COLUMNS, f)))
    return params, fam, cons, rows


def check_file(path, tsv_path, e, params=None):
    """Every row against ramx_term_flat and the restatement on the extents of the oracle's cores (one record at offset 0:
    library positions are the file's coordinates minus one), the summary line against the rows, the consensus lines against
    ramx_term_pair and the restatement on the kept columns."""
    p = {**tr.DEFAULT, **(params or {})}
    head, fam, cons, rows = parse_term(path)
    assert head == p
    tsv = [l.split("\t") for l in open(tsv_path).read().splitlines()]
    after, sites = e["after"], e["sites"]
    M = after.n
    assert len(rows) == 2 * M and len(tsv) == M and list(cons) == ORIENT
    want = [tr.site_records(e["seq"], s, **p) for s in sites]
    flat = term_flat(after, e["seq"], TermParams(**p))
    assert [(tuple(int(r[0][k]) for k in tr.FIELDS), tuple(int(r[1][k]) for k in tr.FIELDS)) for r in flat] == want
    for i, (site, t, recs) in enumerate(zip(sites, tsv, want)):
        lo, hi = site[0], site[1]
        for o, name in enumerate(ORIENT):
            r, rec = rows[2 * i + o], dict(zip(tr.FIELDS, recs[o]))
            assert [r["seqid"], r["start"], r["end"], r["strand"]] == t[:4] and int(r["core"]) == i and r["orientation"] == name
            assert {k: int(r[k]) for k in tr.FIELDS} == rec, (i, name, r, rec)
            if rec["score"] > 0:
                five = (lo + rec["a_start"] + 1, lo + rec["a_end"] + 1)
                three = (hi + 1 - rec["T"] + rec["b_start"] + 1, hi + 1 - rec["T"] + rec["b_end"] + 1) if o == 0 else \
                    (hi - rec["b_end"] + 1, hi - rec["b_start"] + 1)
                anchored = rec["a_start"] <= p["slack"] and (rec["b_end"] >= rec["T"] - 1 - p["slack"] if o == 0 else rec["b_start"] <= p["slack"])
                assert r["identity"] == "%.3f" % (rec["matches"] / rec["columns"])
            else:
                five = three = (0, 0)
                anchored = False
                assert r["identity"] == "0.000"
            assert (int(r["five_start"]), int(r["five_end"]), int(r["three_start"]), int(r["three_end"])) == five + three
            assert int(r["anchored"]) == int(anchored)
    s = tr.summary(want, slack=p["slack"])
    verdict = fam.pop("verdict")
    assert {k: int(v) for k, v in fam.items()} == {k: v for k, v in s.items() if k != "verdict"} and verdict == TERM_VERDICTS[s["verdict"]]
    # the consensus: the outermost kept columns of the left direction in reading order, and the last ones of the right direction
    master, rets = e["master"], e["rets"]
    mid = len(master) // 2 - 1                  # the master holds L rows to the left of the core and L to the right
    w = min(p["tmax"], rets[0], rets[1])
    a = master[mid - rets[0]:mid - rets[0] + w]
    right = master[mid + 1:mid + 1 + rets[1]]
    b = right[len(right) - w:]
    c = tr.revcomp(right)[:w]
    for name, partner in zip(ORIENT, (b, c)):
        rec = tr.pair(tr.classes(a), tr.classes(partner), **p)
        assert cons[name] == dict(zip(tr.FIELDS, rec)), name
        assert tuple(int(term_pair(a, partner, TermParams(**p))[k]) for k in tr.FIELDS) == rec
    return s


@pytest.mark.parametrize("kind,verdict", [("TIR", 2), ("LTR", 1)])
def test_outterm_on_the_planted_families(tmp_path, kind, verdict):
    e = tr.planted_expectation(kind)
    write_twobit(str(tmp_path / "g.2bit"), [("chrP", e["seq"])])
    write_ranges(str(tmp_path / "fam.tsv"), ranges_of("chrP", e["cores"]))
    base = ["-twobit", "g.2bit", "-ranges", "fam.tsv"] + COMMON
    outs = lambda tag: ["-outtsv", str(tmp_path / f"{tag}.tsv"), "-cons", str(tmp_path / f"{tag}.cons"), "-outfa", str(tmp_path / f"{tag}.fa")]      # noqa: E731
    plain = run_cli(base + outs("p"), tmp_path)
    with_new = run_cli(base + outs("n") + ["-outterm", "n.term"], tmp_path)
    assert with_new == plain.replace(str(tmp_path / "p."), str(tmp_path / "n."))
    for ext in ("tsv", "cons", "fa"):
        assert open(tmp_path / f"n.{ext}").read() == open(tmp_path / f"p.{ext}").read(), ext
    s = check_file(tmp_path / "n.term", tmp_path / "n.tsv", e)
    assert s["verdict"] == verdict
    assert abs((s["inverted_median"] if kind == "TIR" else s["direct_median"]) - (60 if kind == "TIR" else 150)) <= 3
    if kind == "LTR":
        return
    # the one-byte library of the reference gives the same file
    r = subprocess.run([_lib.CLI_PATH] + base + ["-outterm", "b.term"], cwd=tmp_path, capture_output=True, text=True, env=dict(os.environ, RAMX_CLI_BYTES="1"))
    assert r.returncode == 0 and open(tmp_path / "b.term").read() == open(tmp_path / "n.term").read()
    # every -term* flag reaches the records
    other = dict(tmax=100, match=3, mismatch=4, gap=6, min_score=30, slack=1)
    run_cli(base + ["-outterm", "s.term", "-outtsv", "s.tsv"] + [x for k, v in other.items() for x in (FLAGS[k], str(v))], tmp_path)
    check_file(tmp_path / "s.term", tmp_path / "s.tsv", e, other)
    for flag, value, word in (("-termmax", "1025", "tmax"), ("-termmax", "0", "tmax"), ("-termmatch", "16", "match"), ("-termmismatch", "0", "mismatch"),
                              ("-termgap", "32", "gap"), ("-termmin", "0", "min_score"), ("-termslack", "16", "slack")):
        bad = subprocess.run([_lib.CLI_PATH] + base + ["-outterm", "x.term", "-outtsv", "x.tsv", flag, value], cwd=tmp_path, capture_output=True, text=True)
        assert bad.returncode != 0 and word in bad.stderr and not os.path.exists(tmp_path / "x.term") and not os.path.exists(tmp_path / "x.tsv"), flag


def test_outterm_in_a_batch_is_the_sixteenth_field(tmp_path):
    fams = [tr.planted_expectation("TIR"), tr.planted_expectation("LTR")]
    write_twobit(str(tmp_path / "all.2bit"), [(f"chr{i}", f["seq"]) for i, f in enumerate(fams)])
    for i, f in enumerate(fams):
        write_ranges(str(tmp_path / f"fam{i}.tsv"), ranges_of(f"chr{i}", f["cores"]))
    common = ["-twobit", "all.2bit"] + COMMON
    # a line with all sixteen fields, one that stops at field 15, one that gives only field 16
    tails = [["-"] * 7 + ["b0.tsd", "-", "b0.period", "b0.term"], ["-"] * 7 + ["b1.tsd", "-", "b1.period"], ["-"] * 10 + ["b2.term"]]
    order = [0, 1, 1]
    with open(tmp_path / "batch.list", "w") as fh:
        for j, i in enumerate(order):
            fh.write("\t".join([f"fam{i}.tsv", f"b{j}.log", f"b{j}.cons", f"b{j}.tsv", f"b{j}.fa"] + tails[j]) + "\n")
    r = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "batch.list"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(tmp_path / "b1.term") and not os.path.exists(tmp_path / "-") and not os.path.exists(tmp_path / "b2.period")
    for j, i in ((0, 0), (2, 1)):
        run_cli(common + ["-ranges", f"fam{i}.tsv", "-outterm", f"s{j}.term", "-outtsd", f"s{j}.tsd", "-outperiod", f"s{j}.period"], tmp_path)
        assert open(tmp_path / f"b{j}.term").read() == open(tmp_path / f"s{j}.term").read()
        _, fam, _, rows = parse_term(tmp_path / f"b{j}.term")
        assert len(rows) == 2 * fams[i]["cores"].n and fam["verdict"] == ("TIR", "LTR")[i]
    # the other files are those of a batch without the field
    with open(tmp_path / "plain.list", "w") as fh:
        for j, i in enumerate(order):
            fh.write("\t".join([f"fam{i}.tsv", f"q{j}.log", f"q{j}.cons", f"q{j}.tsv", f"q{j}.fa"] + (tails[j][:10] if j < 2 else [])).replace("b", "q") + "\n")
    q = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "plain.list"], cwd=tmp_path, capture_output=True, text=True)
    assert q.returncode == 0 and q.stdout == r.stdout
    # (the log's duration line is the wall clock in whole seconds since the program began: two runs differ where a second ends)
    text = lambda name: "".join(l for l in open(tmp_path / name).read().splitlines(True) if not l.startswith("Program duration is"))   # noqa: E731
    for j in range(3):
        for ext in ("cons", "tsv", "fa", "log") + (("tsd", "period") if j < 2 else ()):
            assert text(f"b{j}.{ext}") == text(f"q{j}.{ext}").replace(f"q{j}.", f"b{j}."), (j, ext)
    assert open(tmp_path / "b0.tsd").read() == open(tmp_path / "s0.tsd").read() and open(tmp_path / "b0.period").read() == open(tmp_path / "s0.period").read()
    bad = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "batch.list", "-outterm", "x.term"], cwd=tmp_path, capture_output=True, text=True)
    assert bad.returncode != 0 and "sixteenth field" in bad.stderr and not os.path.exists(tmp_path / "x.term")


def test_the_other_fifteen_outputs_do_not_change(tmp_path):
    """A run with every output: the eleven analysis files, -cons, -outtsv, -outfa and stdout are byte for byte those of the same
    run without -outterm."""
    e = tr.planted_expectation("TIR")
    write_twobit(str(tmp_path / "g.2bit"), [("chrP", e["seq"])])
    write_ranges(str(tmp_path / "fam.tsv"), ranges_of("chrP", e["cores"]))
    base = ["-twobit", "g.2bit", "-ranges", "fam.tsv", "-periodwhole", "-addflanking", "7"] + COMMON
    names = ["profile", "aln", "pileup", "refined", "copies", "cpg", "dinuc", "linkage", "subfam", "tsd", "period", "cons", "tsv", "fa"]
    flag = lambda n: "-cons" if n == "cons" else "-out" + n                                                      # noqa: E731
    outs = lambda tag: [x for n in names for x in (flag(n), str(tmp_path / f"{tag}.{n}"))]                      # noqa: E731
    without = run_cli(base + outs("p"), tmp_path)
    with_new = run_cli(base + outs("n") + ["-outterm", "n.term"], tmp_path)
    assert with_new == without.replace(str(tmp_path / "p."), str(tmp_path / "n."))
    for n in names:
        assert open(tmp_path / f"n.{n}", "rb").read() == open(tmp_path / f"p.{n}", "rb").read(), n
    assert len(names) + 1 == 15 and os.path.getsize(tmp_path / "n.term") > 0
    check_file(tmp_path / "n.term", tmp_path / "n.tsv", e)


def test_extend_stk_term(tmp_path):
    """tools/extend_stk.py -term: <id>-term.tsv per family is the stand-alone run's file, through -batch and one by one, and the
    verdict is printed; without the flag there is neither."""
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
    r = subprocess.run(tool + ["-outdir", "out", "-term"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    one = subprocess.run(tool + ["-outdir", "one", "-term", "-one_by_one"], cwd=tmp_path, capture_output=True, text=True)
    assert one.returncode == 0, one.stdout + one.stderr
    plain = subprocess.run(tool + ["-outdir", "plain"], cwd=tmp_path, capture_output=True, text=True)
    assert plain.returncode == 0 and "Terminal repeats" not in plain.stdout and not os.path.exists(tmp_path / "plain" / "fam0-term.tsv")
    checked = 0
    for k, rows in enumerate(fams):
        if sum(1 for row in rows if row[3] or row[4]) <= 3:
            continue
        matrix, minimp = stk.choose_scoring(mdiv[k])
        run_cli(["-twobit", "all.2bit", "-L", "400", "-bandwidth", "40", "-matrix", matrix, "-minimprovement", str(minimp), "-vvv",
                 "-ranges", f"out/fam{k}-linup.tsv", "-outterm", f"s{k}.term"], tmp_path)
        want = open(tmp_path / f"s{k}.term").read()
        assert want.count("\n") > 6 and open(tmp_path / "out" / f"fam{k}-term.tsv").read() == want == open(tmp_path / "one" / f"fam{k}-term.tsv").read()
        for ext in ("ext-cons.fa", "repam-ranges.tsv", "repam-repseq.fa"):
            assert open(tmp_path / "out" / f"fam{k}-{ext}").read() == open(tmp_path / "plain" / f"fam{k}-{ext}").read(), (k, ext)
        _, h, _, _ = parse_term(tmp_path / f"s{k}.term")
        said = (f"  - Terminal repeats: {h['verdict']} (direct: {h['direct_anchored']} of {h['n']} copies anchored, median "
                f"{h['direct_median']} bp; inverted: {h['inverted_anchored']}, median {h['inverted_median']} bp)")
        assert said in r.stdout and said in one.stdout, said
        checked += 1
    assert checked >= 1
