"""`RAMExtend -outxfam`, alone and with -batch, and `tools/extend_stk.py -xfam`: the file byte for byte against a writer of the
test's own fed by the restatement (tests/xfam_ref.py) on the consensi of the CPU oracle, on the families of
xfam_ref.planted_families -- fragments of one element that extend into each other -- and on the planted LTR family of
tests/term_ref.py; every -xfam* option at both ends of its range; and a -batch list with all seventeen fields, whose files the
flag leaves as they are."""
import os
import subprocess
import sys

import numpy as np
import pytest

from repeatafterme_amd import _lib
from repeatafterme_amd.loader import write_ranges, write_twobit

import term_ref as tr
import xfam_ref as xr
from test_gpu_align_cli import run_cli
from test_gpu_tsd_cli import ranges_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["-bandwidth", "14", "-matrix", "25p43g", "-L", "1500"]
HEADER = ("#family_a\tranges_a\tside_a\tfamily_b\tranges_b\tside_b\torient\tscore\ta_from\ta_to\tlen_a\tb_from\tb_to\tlen_b\tmatches\tcolumns\t"
          "identity\tlink\n")
CODE = np.full(256, 99, np.int8)
for _k, _ch in enumerate("ACGTacgt"):
    CODE[ord(_ch)] = _k


def render(seqs, owner, labels, names, sides, K=16, params=None, link=None, within=True):
    """The file and the summary line from the restatement: records with a score in pair order, then the groups."""
    nf = len(labels)
    recs, pairs, counts, group = xr.compare(seqs, owner, nf, K=K, within=within, params=params, link=link)
    out, n_rec, n_link = [HEADER], 0, 0
    for (a, b, inv), r, c in zip(pairs, recs, counts):
        if r[0] <= 0:
            continue
        score, a0, a1, b0, b1, m, cols, _ = r
        la, lb = len(seqs[a]), len(seqs[b])
        if inv:                                                            # B's own reading coordinates
            b0, b1 = lb - 1 - b1, lb - 1 - b0
        lk = int(c == 1 and owner[a] != owner[b])
        permille = (1000 * m * 2 + cols) // (2 * cols)                     # three decimals, a half rounded up
        out.append("\t".join(str(x) for x in (labels[owner[a]], names[a], sides[a], labels[owner[b]], names[b], sides[b], "-" if inv else "+",
                                               score, a0, a1, la, b0, b1, lb, m, cols, f"{permille // 1000}.{permille % 1000:03d}", lk)) + "\n")
        n_rec += 1
        n_link += lk
    big = 0
    for g in sorted(set(group)):
        members = [f for f in range(nf) if group[f] == g]
        big += len(members) > 1
        out.append(f"#group\t{labels[g]}\t{len(members)}\t{','.join(str(labels[f]) for f in members)}\n")
    return "".join(out), f"xfam: {len(pairs)} candidates, {n_rec} records, {n_link} links, {big} groups with more than one family"


def batch_want(which, **kw):
    """The planted families `which` as a batch: sequence 2 f and 2 f + 1 are the left and right extension of the f-th of them."""
    P = xr.planted_families()
    seqs = [s for f in which for s in P["seqs"][2 * f:2 * f + 2]]
    owner = [k // 2 for k in range(len(seqs))]
    names = [f"fam{xr.PLANT_NAMES[f]}.tsv" for f in which for _ in (0, 1)]
    return render(seqs, owner, list(range(len(which))), names, ["left", "right"] * len(which), **kw)


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("xfam")
    P = xr.planted_families()
    fams = P["families"]
    write_twobit(str(tmp / "g.2bit"), [("g1", fams[0]["seq"]), ("g2", fams[3]["seq"])])
    for f in fams:
        write_ranges(str(tmp / f"fam{f['name']}.tsv"), ranges_of("g2" if f["name"] == "C" else "g1", f["cores"]))
    with open(tmp / "all.list", "w") as fh:
        for f in fams:
            fh.write(f"fam{f['name']}.tsv\t{f['name']}.log\t{f['name']}.cons\n")
    with open(tmp / "two.list", "w") as fh:
        for n in "AC":
            fh.write(f"fam{n}.tsv\t{n}2.log\n")
    return tmp


def run_batch(tmp, lst, out, extra=()):
    r = subprocess.run([_lib.CLI_PATH, "-twobit", "g.2bit"] + COMMON + ["-batch", lst, "-outxfam", out] + list(extra), cwd=tmp,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return open(tmp / out).read(), r.stdout


def test_the_planted_batch_byte_for_byte(planted):
    got, stdout = run_batch(planted, "all.list", "x.tsv")
    want, summary = batch_want(range(4))
    assert got == want
    assert summary in stdout.splitlines() and summary == "xfam: 8 candidates, 8 records, 8 links, 1 groups with more than one family"
    assert got.count("\n#group") == 2 and "#group\t0\t3\t0,1,2\n#group\t3\t1\t3\n" in got
    # the consensi are the oracle's, so are the extension lengths in the file
    P = xr.planted_families()
    first = got.splitlines()[1].split("\t")
    assert (first[0], first[1], first[2], first[3], first[4], first[5], first[6]) == ("0", "famA.tsv", "left", "1", "famB.tsv", "left", "+")
    assert int(first[10]) == P["families"][0]["bp"][0] and int(first[13]) == P["families"][1]["bp"][0]
    # an inverted record is reported in B's own reading coordinates, b_from <= b_to
    inv = [ln.split("\t") for ln in got.splitlines()[1:] if not ln.startswith("#") and ln.split("\t")[6] == "-"]
    assert len(inv) == 5 and all(0 <= int(f[11]) <= int(f[12]) < int(f[13]) for f in inv)
    # the exact mode gives the same file here: the 16-mer filter hides none of the plant
    got0, stdout0 = run_batch(planted, "all.list", "x0.tsv", ["-xfamseed", "0"])
    assert got0 == got and "xfam: 56 candidates, 8 records, 8 links, 1 groups with more than one family" in stdout0.splitlines()
    got16, _ = run_batch(planted, "all.list", "x16.tsv", ["-xfamseed", "16"])
    assert got16 == got


def test_every_option_at_its_low_end(planted):
    low = ["-xfamseed", "8", "-xfammatch", "1", "-xfammismatch", "1", "-xfamgap", "1", "-xfammin", "1", "-xfamcols", "0", "-xfamident", "0"]
    got, stdout = run_batch(planted, "two.list", "lo.tsv", low)
    want, summary = batch_want((0, 3), K=8, params=dict(match=1, mismatch=1, gap=1, min_score=1), link=dict(min_columns=0, min_permille=0))
    assert got == want and summary in stdout.splitlines()
    assert got.count("\n") > 4 and "#group\t0\t2\t0,1\n" in got         # every chance hit links at these thresholds


def test_every_option_at_its_high_end(planted):
    high = ["-xfamseed", "16", "-xfammatch", "15", "-xfammismatch", "15", "-xfamgap", "31", "-xfammin", "5000", "-xfamcols", "300", "-xfamident", "1000"]
    got, stdout = run_batch(planted, "all.list", "hi.tsv", high)
    want, summary = batch_want(range(4), K=16, params=dict(match=15, mismatch=15, gap=31, min_score=5000), link=dict(min_columns=300, min_permille=1000))
    assert got == want and summary in stdout.splitlines()
    assert got.count("\n") == 1 + 2 + 4 and got.count("\n#group") == 4    # two records reach 5,000, and no link is left


@pytest.mark.parametrize("flag,bad", [("-xfamseed", "7"), ("-xfamseed", "17"), ("-xfamseed", "-1"), ("-xfammatch", "0"), ("-xfammatch", "16"),
                                      ("-xfammismatch", "0"), ("-xfammismatch", "16"), ("-xfamgap", "0"), ("-xfamgap", "32"), ("-xfammin", "0"),
                                      ("-xfamcols", "-1"), ("-xfamident", "-1"), ("-xfamident", "1001")])
def test_an_option_outside_its_range_is_refused_at_start_up(planted, flag, bad):
    r = subprocess.run([_lib.CLI_PATH, "-twobit", "g.2bit"] + COMMON + ["-ranges", "famA.tsv", "-cons", "bad.cons", "-outxfam", "bad.tsv", flag, bad],
                       cwd=planted, capture_output=True, text=True)
    assert r.returncode != 0 and "xfam" in r.stderr and not os.path.exists(planted / "bad.tsv") and not os.path.exists(planted / "bad.cons")


def test_a_single_family_meets_its_own_other_end(tmp_path):
    """The planted LTR family: the element begins and ends with the same 150 bases, both extensions reach them, and the direct
    record between the family's left and right extension is that repeat at consensus level.  It never links."""
    e = tr.planted_expectation("LTR")
    write_twobit(str(tmp_path / "g.2bit"), [("chrP", e["seq"])])
    write_ranges(str(tmp_path / "fam.tsv"), ranges_of("chrP", e["cores"]))
    base = ["-twobit", "g.2bit", "-ranges", "fam.tsv", "-bandwidth", "14", "-matrix", "20p43g", "-L", "400"]
    plain = run_cli(base + ["-cons", "p.cons", "-outtsv", "p.tsv"], tmp_path)
    with_new = run_cli(base + ["-cons", "n.cons", "-outtsv", "n.tsv", "-outxfam", "n.xfam"], tmp_path)
    Lm, m = e["p"].L, e["master"]
    seqs = [np.array(m[Lm - e["rets"][0]:Lm], np.int8), np.array(m[Lm + 1:Lm + 1 + e["rets"][1]], np.int8)]
    want, summary = render(seqs, [0, 0], [0], ["fam.tsv"] * 2, ["left", "right"])
    assert open(tmp_path / "n.xfam").read() == want
    lines = with_new.splitlines()
    assert summary in lines and summary.startswith("xfam: ") and " 0 links, 0 groups" in summary
    lines.remove(summary)
    assert "\n".join(lines) == plain.replace("p.", "n.")
    for ext in ("cons", "tsv"):
        assert open(tmp_path / f"n.{ext}").read() == open(tmp_path / f"p.{ext}").read()
    rows = [ln.split("\t") for ln in want.splitlines()[1:] if not ln.startswith("#")]
    direct = [f for f in rows if f[:7] == ["0", "fam.tsv", "left", "0", "fam.tsv", "right", "+"]]
    assert len(direct) == 1 and 140 <= int(direct[0][15]) <= 160 and direct[0][17] == "0" and want.endswith("#group\t0\t1\t0\n")


def test_extend_stk_xfam_across_two_scoring_groups(tmp_path):
    """tools/extend_stk.py -xfam on a Stockholm file of the planted families A and B, which fall into two scoring groups and so
    into two RAMExtend processes: xfam.tsv compares the combined consensi after both have finished, and joins the two."""
    P = xr.planted_families()
    write_twobit(str(tmp_path / "g.2bit"), [("g1", P["families"][0]["seq"])])
    with open(tmp_path / "in.stk", "w") as fh:
        for f, mdiv in ((P["families"][0], 24.0), (P["families"][1], 20.0)):
            fh.write(f"# STOCKHOLM 1.0\n#=GF ID    fam{f['name']}\n#=GF DE    Source:gsa, mDiv={mdiv:.2f}, g.2bit:1\n")
            for (name, s, e_, _, _, o) in ranges_of("g1", f["cores"]):           # the copies' own core bases: the reference is their majority
                fh.write(f"{name}:{s + 1}-{e_}_{o} {''.join('ACGT'[c] for c in f['seq'][s:e_])}\n")
            fh.write("//\n")
    tool = [sys.executable, os.path.join(ROOT, "tools", "extend_stk.py"), "-assembly", "g.2bit", "-input", "in.stk", "-L", "1500", "-bandwidth", "14",
            "-min_aligning_seqs", "2", "-outdir", "out", "-xfam"]      # (six diverged copies: -minimprovement 18 and 20 let them extend)
    r = subprocess.run(tool, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(tmp_path / "out" / "batch-25p43g-18.list") and os.path.exists(tmp_path / "out" / "batch-20p43g-20.list")
    ids = ["famA", "famB"]
    files = [os.path.join("out", f"{i}-combined-cons.fa") for i in ids]
    seqs = []
    for path in files:
        text = "".join(ln.strip() for ln in open(tmp_path / path) if not ln.startswith(">"))
        seqs.append(CODE[np.frombuffer(text.encode(), np.uint8)])
    assert all(len(s) > 1100 for s in seqs)
    want, summary = render(seqs, [0, 1], ids, files, ["all", "all"], within=False)
    assert open(tmp_path / "out" / "xfam.tsv").read() == want
    assert summary in r.stdout.splitlines() and " 1 groups with more than one family" in summary and "#group\tfamA\t2\tfamA,famB\n" in want


def test_a_list_with_all_seventeen_fields_keeps_its_files(tmp_path):
    import test_gpu_batch_cli as tb
    tb._families(tmp_path, [60, 61])
    common = ["-twobit", "all.2bit", "-bandwidth", "20", "-matrix", "14p43g", "-L", "80", "-stopafter", "30"]
    exts = ["log", "cons", "tsv", "fa", "profile", "aln", "pileup", "refined", "copies", "linkage", "subfam", "tsd", "cpg", "period", "term", "dist"]
    for tag in "pn":
        with open(tmp_path / f"{tag}.list", "w") as fh:
            for k in range(2):
                fh.write("\t".join([f"fam{k}.tsv"] + [f"{tag}{k}.{e}" for e in exts]) + "\n")
    assert len(exts) + 1 == 17
    plain = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "p.list"], cwd=tmp_path, capture_output=True, text=True)
    with_new = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "n.list", "-outxfam", "n.xfam"], cwd=tmp_path, capture_output=True, text=True)
    assert plain.returncode == 0 and with_new.returncode == 0, plain.stderr + with_new.stderr
    drop = lambda text: [ln for ln in text.splitlines() if not ln.startswith("Program duration is")]          # noqa: E731
    for k in range(2):
        for e in exts:
            a, b = open(tmp_path / f"p{k}.{e}").read(), open(tmp_path / f"n{k}.{e}").read()
            assert drop(a.replace(f"p{k}.", f"n{k}.")) == drop(b), (k, e)
    out = with_new.stdout.splitlines()
    extra = [ln for ln in out if ln.startswith("xfam: ")]
    assert len(extra) == 1 and drop("\n".join(ln for ln in out if ln not in extra)) == drop(plain.stdout)
    text = open(tmp_path / "n.xfam").read()
    assert text.startswith(HEADER) and text.count("\n#group") >= 1
