"""Every output of `RAMExtend` at once, pinned byte for byte.  The other tests/test_gpu_*_cli.py check each analysis output on
its own; what the plumbing they share can break is the combination: -outpileup with and without -outrefined decides the replays
handed to the refine sink, -outcpg and -outdinuc share one sink, and a batch in which only some families name a file takes the
"not wanted" paths of every sink and writer.

Three families in one .2bit, all run with L = 300, bandwidth 14 and 20p43g:
  f0  the planted family of tests/linkage_ref.py, one record per copy ("-" strand copies among them); the record of copy 0 begins
      at its core (offset 0, and the -addflanking clamp at the library's first base), copy 1 is not extendable to the left and
      copy 2 not to the right (the "*" fields)
  f1  tsd_ref.planted_family(M=14, k=5, seed=21, div=0.05)
  f2  period_ref.planted_family(M=9, seed=22)
Case A runs f0 alone with every flag (the eleven analysis files, -periodwhole, -cons, -outtsv, -outfa, -addflanking 7), on the
packed library and with RAMX_CLI_BYTES=1.  Case B is a -batch of the three: f0 names all fifteen fields, f1 only fields 6, 9, 12
and 15, f2 gives five fields.  Case C is every bare -outX flag together with -batch.

The fixtures under tests/golden/cli_outputs/ (gzip where large) were written by the RAMExtend of commit fc8b7a0 ("Add tandem
periodicity of the extended copies (-outperiod)"), the last one before the analysis outputs moved to ramx_cli_outputs.c, by
running this file with RAMX_RECORD_CLI_OUTPUTS=<directory>; nothing else writes them."""
import gzip
import os
import subprocess

import pytest

from repeatafterme_amd import _lib
from repeatafterme_amd.loader import write_ranges, write_twobit

import linkage_ref as lr
import period_ref as pr
import tsd_ref as tr
from test_gpu_tsd_cli import ranges_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "cli_outputs")
RECORD = os.environ.get("RAMX_RECORD_CLI_OUTPUTS")
COMMON = ["-twobit", "all.2bit", "-bandwidth", "14", "-matrix", "20p43g", "-L", "300", "-addflanking", "7", "-periodwhole"]
# flag, extension of its file, 1-based field of a -batch line (None: the flag writes one family only)
CLASSIC = [("-cons", "cons", 3), ("-outtsv", "tsv", 4), ("-outfa", "fa", 5)]
ANALYSIS = [("-outprofile", "profile", 6), ("-outaln", "aln", 7), ("-outpileup", "pileup", 8), ("-outrefined", "refined", 9),
            ("-outcopies", "copies", 10), ("-outlinkage", "linkage", 11), ("-outsubfam", "subfam", 12), ("-outtsd", "tsd", 13),
            ("-outcpg", "cpg", 14), ("-outperiod", "period", 15), ("-outdinuc", "dinuc", None)]
GZIP_FROM = 8192


def fixture(name, data):
    """Compare `data` (str) with the fixture `name`; when recording, write it instead (once: a second use compares)."""
    path = os.path.join(RECORD or FIX, name)
    if RECORD and not os.path.exists(path) and not os.path.exists(path + ".gz"):
        os.makedirs(RECORD, exist_ok=True)
        raw = data.encode()
        if len(raw) >= GZIP_FROM:
            with open(path + ".gz", "wb") as fh, gzip.GzipFile(fileobj=fh, mode="wb", mtime=0, filename="") as gz:
                gz.write(raw)
        else:
            with open(path, "wb") as fh:
                fh.write(raw)
        return
    want = gzip.open(path + ".gz", "rb").read() if os.path.exists(path + ".gz") else open(path, "rb").read()
    assert data.encode() == want, name


def without_duration(text):
    return "\n".join(l for l in text.splitlines() if not l.startswith("Program duration is"))


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("all_outputs")
    fs, seq, _, _, _ = lr.planted_family()
    n, win = fs.cores.n, len(seq) // fs.cores.n
    recs, rows, strands = [], [], set()
    for i in range(n):
        lo = int(min(fs.cores.left_pos[i], fs.cores.right_pos[i])) - i * win
        hi = int(max(fs.cores.left_pos[i], fs.cores.right_pos[i])) - i * win
        cut = lo if i == 0 else 0                                     # copy 0: its record begins at its core
        recs.append((f"f0_c{i:02d}", seq[i * win + cut:(i + 1) * win]))
        strand = "-" if fs.cores.orient[i] else "+"
        strands.add(strand)
        rows.append((f"f0_c{i:02d}", lo - cut, hi + 1 - cut, 0 if i == 1 else 1, 0 if i == 2 else 1, strand))
    assert strands == {"+", "-"} and rows[0][1] == 0
    t_seq, t_cores, _ = tr.planted_family(M=14, k=5, seed=21, div=0.05)
    p_seq, p_cores, _ = pr.planted_family(M=9, seed=22)
    assert t_cores.orient.any() and p_cores.orient.any()
    write_twobit(str(tmp / "all.2bit"), recs + [("f1_chrT", t_seq), ("f2_chrP", p_seq)])
    write_ranges(str(tmp / "fam0.tsv"), rows)
    write_ranges(str(tmp / "fam1.tsv"), ranges_of("f1_chrT", t_cores))
    write_ranges(str(tmp / "fam2.tsv"), ranges_of("f2_chrP", p_cores))
    return tmp


def single_flags(tag):
    return [x for flag, ext, _ in CLASSIC + ANALYSIS for x in (flag, f"{tag}.{ext}")]


def test_case_a_every_flag_at_once(inputs):
    tmp = inputs
    runs = {}
    for tag, env in (("a", {}), ("y", {"RAMX_CLI_BYTES": "1"})):
        r = subprocess.run([_lib.CLI_PATH] + COMMON + ["-ranges", "fam0.tsv"] + single_flags(tag), cwd=tmp, capture_output=True, text=True,
                           env=dict(os.environ, **env))
        assert r.returncode == 0 and r.stderr == "", r.stderr
        runs[tag] = {ext: open(tmp / f"{tag}.{ext}").read() for _, ext, _ in CLASSIC + ANALYSIS}
        runs[tag]["stdout"] = without_duration(r.stdout)
    assert runs["a"] == runs["y"]
    for name, text in runs["a"].items():
        fixture(f"f0.{name}", text)
    # the inputs reach the corners they were built for
    tsv = runs["a"]["tsv"].splitlines()
    assert any("\t-\t" in l for l in tsv) and any("extended_left=*" in l for l in tsv) and any("extended_right=*" in l for l in tsv)
    assert any(l.startswith("f0_c00\t1\t") for l in tsv) and "flanking=7" in runs["a"]["fa"]
    assert ">f0_c00:2-" in runs["a"]["fa"]            # the reference's clamp at the library's first base begins at 1, not 0


def test_case_b_a_batch_of_three(inputs):
    tmp = inputs
    wanted = {0: [3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15], 1: [3, 4, 5, 6, 9, 12, 15], 2: [3, 4, 5]}
    exts = {field: ext for _, ext, field in CLASSIC + ANALYSIS if field}
    with open(tmp / "batch.list", "w") as fh:
        for k, fields in wanted.items():
            line = [f"fam{k}.tsv", f"b{k}.log"] + [f"b{k}.{exts[f]}" if f in fields else "-" for f in range(3, max(fields) + 1)]
            fh.write("\t".join(line) + "\n")
    r = subprocess.run([_lib.CLI_PATH] + COMMON + ["-batch", "batch.list"], cwd=tmp, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    fixture("batch.stdout", r.stdout)
    assert not os.path.exists(tmp / "-")
    for k, fields in wanted.items():
        fixture(f"f{k}.log", without_duration(open(tmp / f"b{k}.log").read()))
        for field, ext in exts.items():
            if field in fields:
                # the all-fields family: the very fixtures of Case A, the run of that family alone
                fixture(f"f{k}.{ext}", open(tmp / f"b{k}.{ext}").read())
            else:
                assert not os.path.exists(tmp / f"b{k}.{ext}"), (k, ext)
        assert not os.path.exists(tmp / f"b{k}.dinuc")


def test_case_c_the_bare_flags_are_refused_with_a_batch(inputs):
    tmp = inputs
    with open(tmp / "refuse.list", "w") as fh:
        fh.write("\t".join(["fam2.tsv", "r.log", "r.cons", "r.tsv", "r.fa"]) + "\n")
    said = []
    for flag, ext, _ in ANALYSIS:
        r = subprocess.run([_lib.CLI_PATH] + COMMON + ["-batch", "refuse.list", flag, f"x.{ext}"], cwd=tmp, capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == "" and r.stderr.count("\n") == 1, (flag, r.stderr)
        said.append(f"{flag}\t{r.returncode}\t{r.stderr}")
        assert not [f for f in os.listdir(tmp) if f.startswith(("x.", "r."))], flag
    fixture("refusals.txt", "".join(said))
