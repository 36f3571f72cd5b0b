"""`RAMExtend -outprofile` against the reference binary's own -vvvv / -vvvvv logs (tests/golden/cli/*/vvvv.gz): every TSV
line -- the four candidate totals, the chosen base, curr_ext_score, total_edges / num_extending / num_out_of_seq, the
new-maximum mark and the number of **CAPPED** lines under the chosen base -- must be what the reference printed for
that row, in both directions."""
import gzip
import os
import re
import subprocess

import pytest

from repeatafterme_amd import _lib
from repeatafterme_amd.loader import write_ranges, write_twobit

from helpers import make_genome

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
VERBOSE = sorted(c for c in os.listdir(os.path.join(G, "cli")) if os.path.exists(os.path.join(G, "cli", c, "vvvv.gz")))
HEADER = "dir row base total_A total_C total_G total_T score margin n_flanks n_uncapped n_new_high n_out_of_seq new_max kept".split()

_ROW = re.compile(r"^(RIGHT|LEFT) ROW (\d+) with '([ACGT])': n = \d+")
_TOTAL = re.compile(r"^  Total Score for '([ACGT])' = (-?\d+)")
_DONE = re.compile(r"^ROW (\d+) complete, '([ACGT])' chosen as the consensus. curr_ext_score = (-?\d+)")
_EDGES = re.compile(r"total_edges = (\d+), num_extending = (\d+), num_out_of_seq = (\d+)")
_EXT = re.compile(r"^Extended (right|left ): (\d+) bp")


def parse_log(text):
    """-> {"right": [row dict ...], "left": [...]} from a reference -vvvv log, rows in the order they were printed."""
    out = {"right": [], "left": []}
    cur, direction, cand = None, None, None
    for line in text.splitlines():
        m = _ROW.match(line)
        if m:
            direction, cand = m.group(1).lower(), m.group(3)
            if cur is None or cur["row"] != int(m.group(2)) or cur["dir"] != direction:
                cur = dict(dir=direction, row=int(m.group(2)), totals={}, capped={b: 0 for b in "ACGT"}, new_max=0)
            continue
        if cur is not None and "**CAPPED**" in line:
            cur["capped"][cand] += 1
            continue
        m = _TOTAL.match(line)
        if m and cur is not None:
            cur["totals"][m.group(1)] = int(m.group(2))
            continue
        m = _DONE.match(line)
        if m:
            if cur is None or cur["row"] != int(m.group(1)):      # a direction without an extendable core prints no candidate lines
                cur = dict(dir=direction, row=int(m.group(1)), totals={b: 0 for b in "ACGT"}, capped={b: 0 for b in "ACGT"}, new_max=0)
            cur["base"], cur["score"] = m.group(2), int(m.group(3))
            out[cur["dir"]].append(cur)
            continue
        m = _EDGES.search(line)
        if m and cur is not None:
            cur["n_flanks"], cur["n_new_high"], cur["n_out_of_seq"] = (int(x) for x in m.groups())
            continue
        if "**This row is now the new max**" in line and cur is not None:
            cur["new_max"] = 1
            continue
        m = _EXT.match(line)
        if m:
            d = m.group(1).strip()
            for row in out[d]:
                row["kept"] = int(row["row"] < int(m.group(2)))
            cur = None
            direction = "left" if d == "right" else direction
        if line.startswith("extend_alignment(left)"):
            direction = "left"
        if line.startswith("extend_alignment(right)"):
            direction = "right"
    return out


def expected_lines(parsed):
    lines = []
    for d in ("right", "left"):
        for r in parsed[d]:
            t = [r["totals"][b] for b in "ACGT"]
            bi = "ACGT".index(r["base"])
            margin = t[bi] - max(x for k, x in enumerate(t) if k != bi)
            lines.append([d, r["row"], r["base"]] + t + [r["score"], margin, r["n_flanks"], r["n_flanks"] - r["capped"][r["base"]],
                                                         r["n_new_high"], r["n_out_of_seq"], r["new_max"], r["kept"]])
    return [[str(x) for x in l] for l in lines]


def _golden(case):
    return gzip.open(os.path.join(G, "cli", case, "vvvv.gz"), "rb").read().decode()


def _argv(case, keep_verbose=False):
    argv = open(os.path.join(G, "cli", case, "argv")).read().split()
    stem = open(os.path.join(G, "cli", case, "stem")).read().strip()
    if not keep_verbose:
        argv = [a for a in argv if not re.fullmatch(r"-v+", a)]
    return ["-twobit", f"inputs/{stem}.2bit", "-ranges", f"inputs/{stem}.tsv"] + argv


def _read_tsv(path):
    rows = [l.split("\t") for l in open(path).read().splitlines()]
    assert rows[0] == HEADER
    return rows[1:]


@pytest.mark.parametrize("case", VERBOSE)
def test_golden_log_parser_is_sane(case):
    """No GPU: in every golden log the rows of a direction count up from 0, the chosen base is the first strict maximum of
    the four totals (A when none is positive) and curr_ext_score is that maximum."""
    parsed = parse_log(_golden(case))
    assert len(VERBOSE) == 9
    assert parsed["right"] and parsed["left"]
    n_capped = n_out = 0
    for d in ("right", "left"):
        assert [r["row"] for r in parsed[d]] == list(range(len(parsed[d])))
        for r in parsed[d]:
            t = [r["totals"][b] for b in "ACGT"]
            best, base = 0, 0
            for k, v in enumerate(t):
                if v > best:
                    best, base = v, k
            assert ("ACGT"[base], best) == (r["base"], r["score"]), (case, d, r["row"])
            assert "kept" in r and "n_flanks" in r
            n_capped += sum(r["capped"].values())
            n_out += r["n_out_of_seq"]
    assert n_capped == _golden(case).count("**CAPPED**")      # every such line was attributed to a row and a candidate
    if case in ("g2_vvvv_w3", "ov_vvvv", "ov_v5"):
        assert n_out > 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", VERBOSE)
def test_outprofile_equals_reference_log(case, tmp_path):
    r = subprocess.run([_lib.CLI_PATH] + _argv(case) + ["-outprofile", str(tmp_path / "profile.tsv")], cwd=G, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got, want = _read_tsv(tmp_path / "profile.tsv"), expected_lines(parse_log(_golden(case)))
    assert len(got) == len(want), (len(got), len(want))
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"line {k}: {a} != {b}"


@pytest.mark.gpu
def test_outprofile_with_verbose_rows_and_outmat(tmp_path):
    """-vvvv kept: stdout is still the reference's, byte for byte, and the TSV is the one of the quiet run; the same with -outmat."""
    case = "ov_vvvv"
    want_tsv = expected_lines(parse_log(_golden(case)))
    r = subprocess.run([_lib.CLI_PATH] + _argv(case, keep_verbose=True) + ["-outprofile", str(tmp_path / "v.tsv")], cwd=G, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    norm = lambda txt: ["<v>" if l.startswith("RAMExtend Version") else "<t>" if l.startswith("Program duration is") else l for l in txt.splitlines()]
    assert norm(r.stdout) == norm(_golden(case))
    assert _read_tsv(tmp_path / "v.tsv") == want_tsv
    r = subprocess.run([_lib.CLI_PATH] + _argv(case) + ["-outprofile", str(tmp_path / "m.tsv"), "-outmat", str(tmp_path / "mat")], cwd=G, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert _read_tsv(tmp_path / "m.tsv") == want_tsv and os.path.getsize(tmp_path / "mat") > 0


@pytest.mark.gpu
def test_outprofile_in_a_batch_equals_single_runs(tmp_path):
    """Six-field -batch lines: every family's profile file equals the one of a run of that family alone; five-field
    lines keep working."""
    records, fams = [], []
    for k, seed in enumerate((40, 41, 42)):
        recs, rows = make_genome(seed)
        records += [(f"f{k}_{name}", seq) for name, seq in recs]
        fams.append([(f"f{k}_{r[0]}",) + tuple(r[1:]) for r in rows])
    write_twobit(str(tmp_path / "all.2bit"), records)
    common = ["-twobit", "all.2bit", "-bandwidth", "14", "-matrix", "25p43g", "-L", "300", "-stopafter", "20", "-cappenalty", "-10"]
    with open(tmp_path / "batch.list", "w") as fh:
        for k, rows in enumerate(fams):
            write_ranges(str(tmp_path / f"fam{k}.tsv"), rows)
            cols = [f"fam{k}.tsv", f"b{k}.log", f"b{k}.cons", f"b{k}.tsv", f"b{k}.fa"] + ([f"b{k}.profile"] if k != 1 else [])
            fh.write("\t".join(cols) + "\n")
    r = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "batch.list"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(tmp_path / "b1.profile")
    for k in range(3):
        s = subprocess.run([_lib.CLI_PATH] + common + ["-ranges", f"fam{k}.tsv", "-cons", f"s{k}.cons", "-outtsv", f"s{k}.tsv",
                                                       "-outprofile", f"s{k}.profile"], cwd=tmp_path, capture_output=True, text=True)
        assert s.returncode == 0, s.stderr
        assert open(tmp_path / f"s{k}.tsv").read() == open(tmp_path / f"b{k}.tsv").read()
        if k != 1:
            single = open(tmp_path / f"s{k}.profile").read()
            assert single == open(tmp_path / f"b{k}.profile").read(), k
            assert len(single.splitlines()) > 20
