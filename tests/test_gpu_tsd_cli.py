"""`RAMExtend -outtsd`: on a planted family every record of the file equals the restatement (tests/tsd_ref.py) on the run's own
-outtsv ranges and the header's mode is the planted length; the thirteenth field of a -batch line gives the same file; the bare
flag with -batch is refused; and a run without the option is what it was: stdout and the classic outputs of the golden case."""
import os
import subprocess

import numpy as np
import pytest

from repeatafterme_amd import _lib
from repeatafterme_amd.loader import write_ranges, write_twobit

import tsd_ref as tr
from test_gpu_align_cli import run_cli
from test_gpu_cli import CASES, STEM, _norm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
L, W = 300, 14
COMMON = ["-bandwidth", str(W), "-matrix", "20p43g", "-L", str(L)]
COLUMNS = ["core", "seqid", "start", "end", "strand", "ext_left", "ext_right", "tsd_len", "mismatches", "shift_left", "shift_right",
           "left_word", "right_word"]


def ranges_of(name, cores):
    rows = []
    for i in range(cores.n):
        a, b = sorted((int(cores.left_pos[i]), int(cores.right_pos[i])))
        rows.append((name, a, b + 1, 1, 1, "-" if cores.orient[i] else "+"))
    return rows


def parse_tsd(path):
    head, rows = {}, []
    for line in open(path).read().splitlines():
        f = line.split("\t")
        if line.startswith("#"):
            head[f[0][1:]] = dict(kv.split("=") for kv in f[1:] if "=" in kv) if f[0] != "#hist" else {int(a): int(b) for a, b in (kv.split(":") for kv in f[1:])}
        elif f[0] == "core":
            assert f == COLUMNS
        else:
            rows.append(dict(zip(COLUMNS, f)))
    return head, rows


def check_file(path, tsv_path, genome, k, M):
    """Every record against the restatement on the -outtsv ranges (1-based, closed; the core's window reaches L + W beyond it),
    the words against the genome, the header against the records."""
    head, rows = parse_tsd(path)
    tsv = [l.split("\t") for l in open(tsv_path).read().splitlines()]
    assert len(rows) == len(tsv) == M
    letters = "ACGT"
    recs = []
    for r, t in zip(rows, tsv):
        assert [r["seqid"], r["start"], r["end"], r["strand"]] == t[:4]
        meta = dict(kv.split("=") for kv in t[4].split(","))
        assert int(r["core"]) == int(meta["n"]) and r["ext_left"] == meta["extended_left"] and r["ext_right"] == meta["extended_right"]
        lo, hi = int(t[1]) - 1, int(t[2]) - 1
        a0, a1 = (int(x) for x in meta["anchor_range"].split("-"))
        # anchor_range is window-relative: the window begins L + W in front of the core (or at the record's beginning)
        core_lo = lo + (int(meta["extended_right"]) if r["strand"] == "-" else int(meta["extended_left"]))
        win_lo = core_lo - (min(a0, a1) - 1)
        core_hi = hi - (int(meta["extended_left"]) if r["strand"] == "-" else int(meta["extended_right"]))
        site = (lo, hi, win_lo, min(core_hi + L + W, len(genome) - 1))
        want = tr.tsd(genome, site)
        got = (int(r["tsd_len"]), int(r["mismatches"]), int(r["shift_left"]), int(r["shift_right"]))
        assert got == want, (r, want)
        if got[0]:
            lw = "".join(letters[genome[p]] for p in range(lo + got[2] - got[0], lo + got[2]))
            rw = "".join(letters[genome[p]] for p in range(hi + 1 + got[3], hi + 1 + got[3] + got[0]))
            assert (r["left_word"], r["right_word"]) == (lw, rw)
        else:
            assert (r["left_word"], r["right_word"]) == ("-", "-")
        recs.append(got)
    hist, mode, count, null = tr.summary(recs)
    assert head["tsd"] == dict(slack="3", kmin="4", kmax="20", mm_div="10")
    assert head["hist"] == {i: v for i, v in enumerate(hist) if v}
    assert int(head["mode"]["mode"]) == mode == k and int(head["mode"]["mode_count"]) == count and 2 * count >= M
    assert abs(float(head["mode"]["null"]) - float(null[mode])) <= 5e-5
    assert int(head["rows"]["left_rows"]) > 100 and int(head["rows"]["right_rows"]) > 100
    assert len(head["termini"]["five"]) == 32 and len(head["termini"]["three"]) == 32 and int(head["termini"]["tir"]) >= 0
    return recs


def test_outtsd_on_the_planted_family(tmp_path):
    e = tr.planted_expectation()
    write_twobit(str(tmp_path / "g.2bit"), [("chrP", e["seq"])])
    write_ranges(str(tmp_path / "fam.tsv"), ranges_of("chrP", e["cores"]))
    base = ["-twobit", "g.2bit", "-ranges", "fam.tsv"] + COMMON
    outs = lambda tag: ["-outtsv", str(tmp_path / f"{tag}.tsv"), "-cons", str(tmp_path / f"{tag}.cons"), "-outfa", str(tmp_path / f"{tag}.fa")]      # noqa: E731
    plain = run_cli(base + outs("p"), tmp_path)
    with_new = run_cli(base + outs("n") + ["-outtsd", "n.tsd"], tmp_path)
    assert with_new == plain.replace(str(tmp_path / "p."), str(tmp_path / "n."))
    for ext in ("tsv", "cons", "fa"):
        assert open(tmp_path / f"n.{ext}").read() == open(tmp_path / f"p.{ext}").read(), ext
    recs = check_file(tmp_path / "n.tsd", tmp_path / "n.tsv", e["seq"], tr.PLANTED["k"], tr.PLANTED["M"])
    # the loader sorts the ranges as the planted family has them: the records are the oracle's
    assert recs == e["records"]
    # the one-byte library of the reference gives the same file, and other parameters another
    r = subprocess.run([_lib.CLI_PATH] + base + ["-outtsd", "b.tsd"], cwd=tmp_path, capture_output=True, text=True, env=dict(os.environ, RAMX_CLI_BYTES="1"))
    assert r.returncode == 0 and open(tmp_path / "b.tsd").read() == open(tmp_path / "n.tsd").read()
    run_cli(base + ["-outtsd", "s.tsd", "-tsdslack", "0", "-tsdmin", "5", "-tsdmax", "5", "-tsdmm", "0"], tmp_path)
    head, rows = parse_tsd(tmp_path / "s.tsd")
    assert head["tsd"] == dict(slack="0", kmin="5", kmax="5", mm_div="0")
    want = tr.tsd_all(e["seq"], e["sites"], slack=0, kmin=5, kmax=5, mm_div=0)
    assert [(int(x["tsd_len"]), int(x["mismatches"]), int(x["shift_left"]), int(x["shift_right"])) for x in rows] == want
    assert 0 < sum(w[0] == 5 for w in want) < sum(r_[0] == 5 for r_ in recs)
    bad = subprocess.run([_lib.CLI_PATH] + base + ["-outtsd", "x.tsd", "-tsdslack", "8"], cwd=tmp_path, capture_output=True, text=True)
    assert bad.returncode != 0 and "slack" in bad.stderr and not os.path.exists(tmp_path / "x.tsd")


def test_outtsd_in_a_batch_is_the_thirteenth_field(tmp_path):
    fams = [tr.planted_family(M=14, k=5, seed=21, div=0.05), tr.planted_family(M=9, k=8, seed=22, div=0.05)]
    write_twobit(str(tmp_path / "all.2bit"), [(f"chr{i}", f[0]) for i, f in enumerate(fams)])
    for i, f in enumerate(fams):
        write_ranges(str(tmp_path / f"fam{i}.tsv"), ranges_of(f"chr{i}", f[1]))
    common = ["-twobit", "all.2bit"] + COMMON
    tails = [["-"] * 7 + ["b0.tsd"], [], ["-"] * 7 + ["b2.tsd"]]
    order = [0, 1, 1]                 # the family in the middle asks for nothing
    with open(tmp_path / "batch.list", "w") as fh:
        for j, i in enumerate(order):
            fh.write("\t".join([f"fam{i}.tsv", f"b{j}.log", f"b{j}.cons", f"b{j}.tsv", f"b{j}.fa"] + tails[j]) + "\n")
    r = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "batch.list"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(tmp_path / "b1.tsd") and not os.path.exists(tmp_path / "-")
    for j, i in ((0, 0), (2, 1)):
        check_file(tmp_path / f"b{j}.tsd", tmp_path / f"b{j}.tsv", fams[i][0], (5, 8)[i], (14, 9)[i])
        run_cli(common + ["-ranges", f"fam{i}.tsv", "-outtsd", f"s{j}.tsd"], tmp_path)
        assert open(tmp_path / f"s{j}.tsd").read() == open(tmp_path / f"b{j}.tsd").read()
    # the other files are those of a batch without the field
    with open(tmp_path / "plain.list", "w") as fh:
        for j, i in enumerate(order):
            fh.write("\t".join([f"fam{i}.tsv", f"q{j}.log", f"q{j}.cons", f"q{j}.tsv", f"q{j}.fa"]) + "\n")
    q = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "plain.list"], cwd=tmp_path, capture_output=True, text=True)
    assert q.returncode == 0 and q.stdout == r.stdout
    for j in range(3):
        for ext in ("cons", "tsv", "fa"):
            assert open(tmp_path / f"b{j}.{ext}").read() == open(tmp_path / f"q{j}.{ext}").read(), (j, ext)
        strip = lambda t: [l for l in t.splitlines() if not l.startswith("Program duration")]       # noqa: E731
        assert strip(open(tmp_path / f"b{j}.log").read().replace(f"b{j}.", "")) == strip(open(tmp_path / f"q{j}.log").read().replace(f"q{j}.", ""))
    bad = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "batch.list", "-outtsd", "x.tsd"], cwd=tmp_path, capture_output=True, text=True)
    assert bad.returncode != 0 and "thirteenth field" in bad.stderr and not os.path.exists(tmp_path / "x.tsd")


def test_a_run_without_the_option_is_the_golden_case(tmp_path):
    case = [c for c in CASES if c.startswith("t2")][0]
    argv = open(os.path.join(G, "cli", case, "argv")).read().split()
    stem = STEM["t2"]
    cmd = [_lib.CLI_PATH, "-twobit", f"inputs/{stem}.2bit", "-ranges", f"inputs/{stem}.tsv", "-cons", str(tmp_path / "cons"),
           "-outtsv", str(tmp_path / "tsv"), "-outfa", str(tmp_path / "fa")] + argv
    r = subprocess.run(cmd, cwd=G, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert _norm(r.stdout.replace(str(tmp_path) + "/", "")) == _norm(open(os.path.join(G, "cli", case, "stdout")).read())
    for f in ("cons", "tsv", "fa"):
        ref_f = os.path.join(G, "cli", case, f)
        if os.path.exists(ref_f):
            assert open(tmp_path / f).read() == open(ref_f).read(), f
    # ... and with it: the same stdout, the same three files, and the file itself
    keep = {f: open(tmp_path / f).read() for f in ("cons", "tsv", "fa") if os.path.exists(tmp_path / f)}
    w = subprocess.run(cmd + ["-outtsd", str(tmp_path / "tsd")], cwd=G, capture_output=True, text=True)
    assert w.returncode == 0, w.stderr
    assert _norm(w.stdout) == _norm(r.stdout)
    assert keep == {f: open(tmp_path / f).read() for f in keep}
    head, rows = parse_tsd(tmp_path / "tsd")
    assert len(rows) == len(keep["tsv"].splitlines()) > 0 and [x["start"] for x in rows] == [l.split("\t")[1] for l in keep["tsv"].splitlines()]


def test_extend_stk_tsd(tmp_path):
    """tools/extend_stk.py -tsd: <id>-tsd.tsv per family is the stand-alone run's file, through -batch and one by one, and the
    modal length is printed; without the flag there is neither."""
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
    r = subprocess.run(tool + ["-outdir", "out", "-tsd"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    one = subprocess.run(tool + ["-outdir", "one", "-tsd", "-one_by_one"], cwd=tmp_path, capture_output=True, text=True)
    assert one.returncode == 0, one.stdout + one.stderr
    plain = subprocess.run(tool + ["-outdir", "plain"], cwd=tmp_path, capture_output=True, text=True)
    assert plain.returncode == 0 and "Target-site duplication" not in plain.stdout and not os.path.exists(tmp_path / "plain" / "fam0-tsd.tsv")
    checked = 0
    for k, rows in enumerate(fams):
        if sum(1 for row in rows if row[3] or row[4]) <= 3:
            continue
        matrix, minimp = stk.choose_scoring(mdiv[k])
        run_cli(["-twobit", "all.2bit", "-L", "400", "-bandwidth", "40", "-matrix", matrix, "-minimprovement", str(minimp), "-vvv",
                 "-ranges", f"out/fam{k}-linup.tsv", "-outtsd", f"s{k}.tsd"], tmp_path)
        want = open(tmp_path / f"s{k}.tsd").read()
        assert want.count("\n") > 7 and open(tmp_path / "out" / f"fam{k}-tsd.tsv").read() == want == open(tmp_path / "one" / f"fam{k}-tsd.tsv").read()
        for ext in ("ext-cons.fa", "repam-ranges.tsv", "repam-repseq.fa"):
            assert open(tmp_path / "out" / f"fam{k}-{ext}").read() == open(tmp_path / "plain" / f"fam{k}-{ext}").read(), (k, ext)
        head, _ = parse_tsd(tmp_path / f"s{k}.tsd")
        said = f"  - Target-site duplication: {head['mode']['mode']} bp in {head['mode']['mode_count']} copies ({head['mode']['null']} expected by chance)"
        assert said in r.stdout and said in one.stdout, said
        checked += 1
    assert checked >= 1
