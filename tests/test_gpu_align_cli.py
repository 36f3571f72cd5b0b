"""`RAMExtend -outaln`: the A2M text equals the rendering of the CPU walker's paths (tests/align_ref.py) on the oracle's
consensus; every record, degapped and upper-cased, is the flank's own stretch of bases; and every other output is what it is
without the option."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd import _lib
from repeatafterme_amd.datamodel import new_master
from repeatafterme_amd.loader import load_sequence_subset_minimal, write_ranges, write_twobit

import align_ref as ar
from helpers import make_genome

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def run_cli(args, cwd):
    r = subprocess.run([_lib.CLI_PATH] + args, cwd=cwd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return "\n".join(l for l in r.stdout.splitlines() if not l.startswith("Program duration is"))


def fa_records(path):
    """-outfa: {core number: (record name up to the two spaces, sequence)}"""
    lines = open(path).read().splitlines()
    out = {}
    for head, seq in zip(lines[0::2], lines[1::2]):
        name, meta = head[1:].split("  ")
        out[int(dict(kv.split("=") for kv in meta.split(","))["n"])] = (name, seq)
    return out


def expected_text(twobit, ranges, matrix, W, L, stopafter, names):
    """The file as the helper renders it: the oracle's two directions with the overlap avoidance between them, the walker on
    every extendable core along the kept consensus."""
    fs = load_sequence_subset_minimal(twobit, ranges, L + W)
    p = po.Params.named(matrix, bandwidth=W, L=L, when_to_stop=stopafter)
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    cores, master = fs.cores, new_master(L)
    text, flanks = "", {}
    for direction in (1, 0):
        before = cores.copy()
        o = po.oracle_extend(direction, cores, seq, master, p, trace=True)
        cons = o.col_base[:o.ret]
        idx, results = ar.walk_family(direction, before, seq, p, cons)
        text += ar.render_block(direction, cons, names, idx, results, before, seq, W)
        flanks["right" if direction else "left"] = [(n, ar.Flank(direction, before, n, W), r) for n, r in zip(idx, results)]
        if direction:
            ar.overlap_avoidance(fs)
    return text, flanks, seq, cores


def check_outaln(tmp_path, twobit, ranges, extra, matrix, W, L, stopafter):
    outs = lambda tag: ["-cons", str(tmp_path / f"{tag}.cons"), "-outtsv", str(tmp_path / f"{tag}.tsv"), "-outfa", str(tmp_path / f"{tag}.fa")]
    base = ["-twobit", twobit, "-ranges", ranges] + extra
    plain = run_cli(base + outs("p"), tmp_path)
    with_aln = run_cli(base + outs("a") + ["-outaln", str(tmp_path / "a.a2m")], tmp_path)
    # stdout and every other output: byte for byte what they are without the option
    assert with_aln == plain.replace(str(tmp_path / "p."), str(tmp_path / "a."))
    for ext in ("cons", "tsv", "fa"):
        assert open(tmp_path / f"a.{ext}").read() == open(tmp_path / f"p.{ext}").read(), ext
    fa = fa_records(tmp_path / "a.fa")
    got = open(tmp_path / "a.a2m").read()
    want, flanks, seq, cores = expected_text(twobit, ranges, matrix, W, L, stopafter, {n: v[0] for n, v in fa.items()})
    assert got == want
    parsed = ar.parse_outaln(got)
    assert list(parsed) == ["right", "left"]
    n_records = n_aligned = 0
    for d in ("right", "left"):
        ret, cons, records = parsed[d]
        assert len(cons) == ret and len(records) == len(flanks[d])
        for (name, meta, body), (n, fl, res) in zip(records, flanks[d]):
            n_records += 1
            assert name == fa[n][0] and meta["dir"] == d
            assert sum(ch == "-" or ch.isupper() for ch in body) == ret and all(ch == "-" or ch.isalpha() for ch in body)
            start, end = int(meta["start"]), int(meta["end"])
            stretch = "".join(ar._char(fl.base(t, seq)).upper() for t in range(start, end + 1)) if int(meta["end_row"]) >= 0 else ""
            degapped = body.replace("-", "").upper()
            assert degapped == (stretch if d == "right" else stretch[::-1]), (d, n)
            if int(meta["end_row"]) >= 0 and start == 0:
                n_aligned += 1
                # the extension stretch of the same core's -outfa record: its last (right) or first (left) end + 1 bases
                ext_len = int((cores.right_len if d == "right" else cores.left_len)[n])
                assert ext_len == end + 1
                assert degapped == (fa[n][1][len(fa[n][1]) - ext_len:] if d == "right" else fa[n][1][:ext_len]).upper(), (d, n)
    return n_records, n_aligned


@pytest.mark.parametrize("W", [14, 40])
def test_outaln_on_the_reference_test_family(W, tmp_path):
    extra = [] if W == 14 else ["-bandwidth", "40"]
    n_records, n_aligned = check_outaln(tmp_path, os.path.join(G, "inputs", "extension-test2.2bit"), os.path.join(G, "inputs", "extension-test2.tsv"),
                                        extra, "20p43g", W, 10000, 100)
    assert n_records >= 5 and n_aligned >= 4


def _genome_family(tmp_path, seed, prefix=""):
    recs, rows = make_genome(seed)
    return [(prefix + name, seq) for name, seq in recs], [(prefix + r[0],) + tuple(r[1:]) for r in rows]


def test_outaln_on_a_synthetic_genome(tmp_path):
    recs, rows = _genome_family(tmp_path, 14)                      # a family whose paths hold some thirty insertions and deletions
    write_twobit(str(tmp_path / "g.2bit"), recs)
    write_ranges(str(tmp_path / "g.tsv"), rows)
    extra = ["-bandwidth", "14", "-matrix", "25p43g", "-L", "300", "-stopafter", "20"]
    n_records, n_aligned = check_outaln(tmp_path, str(tmp_path / "g.2bit"), str(tmp_path / "g.tsv"), extra, "25p43g", 14, 300, 20)
    assert n_records > 4 and n_aligned > 2
    bodies = [b for d in ar.parse_outaln(open(tmp_path / "a.a2m").read()).values() for _, _, b in d[2]]
    assert any(ch.islower() for b in bodies for ch in b) and any("-" in b.strip("-") for b in bodies)


def test_outaln_with_profile_verbose_rows_and_outmat(tmp_path):
    """Beside -outprofile, -vvvv and -outmat the file is the one of the quiet run."""
    base = ["-twobit", os.path.join(G, "inputs", "extension-test2.2bit"), "-ranges", os.path.join(G, "inputs", "extension-test2.tsv"),
            "-bandwidth", "5", "-L", "30"]
    run_cli(base + ["-outaln", str(tmp_path / "q.a2m")], tmp_path)
    quiet = open(tmp_path / "q.a2m").read()
    assert quiet.count(">") > 4
    plain_v = run_cli(base + ["-vvvv"], tmp_path)
    with_v = run_cli(base + ["-vvvv", "-outaln", str(tmp_path / "v.a2m"), "-outprofile", str(tmp_path / "v.profile")], tmp_path)
    assert with_v == plain_v and open(tmp_path / "v.a2m").read() == quiet
    assert len(open(tmp_path / "v.profile").read().splitlines()) > 10
    run_cli(base + ["-outaln", str(tmp_path / "m.a2m"), "-outmat", str(tmp_path / "mat")], tmp_path)
    assert open(tmp_path / "m.a2m").read() == quiet and os.path.getsize(tmp_path / "mat") > 0


def test_outaln_in_a_batch_equals_single_runs(tmp_path):
    """The seventh field of a -batch line, alone ("-" in the sixth) and beside the sixth; shorter lines keep working."""
    records, fams = [], []
    for k, seed in enumerate((14, 7, 9)):
        recs, rows = _genome_family(tmp_path, seed, prefix=f"f{k}_")
        records += recs
        fams.append(rows)
    write_twobit(str(tmp_path / "all.2bit"), records)
    common = ["-twobit", "all.2bit", "-bandwidth", "14", "-matrix", "25p43g", "-L", "300", "-stopafter", "20", "-cappenalty", "-10"]
    tails = [["-", "b0.a2m"], ["b1.profile", "b1.a2m"], []]
    with open(tmp_path / "batch.list", "w") as fh:
        for k, rows in enumerate(fams):
            write_ranges(str(tmp_path / f"fam{k}.tsv"), rows)
            fh.write("\t".join([f"fam{k}.tsv", f"b{k}.log", f"b{k}.cons", f"b{k}.tsv", f"b{k}.fa"] + tails[k]) + "\n")
    r = subprocess.run([_lib.CLI_PATH] + common + ["-batch", "batch.list"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(tmp_path / "b0.profile") and not os.path.exists(tmp_path / "b2.a2m") and os.path.exists(tmp_path / "b1.profile")
    for k in range(3):
        s = subprocess.run([_lib.CLI_PATH] + common + ["-ranges", f"fam{k}.tsv", "-cons", f"s{k}.cons", "-outtsv", f"s{k}.tsv", "-outfa", f"s{k}.fa",
                                                       "-outaln", f"s{k}.a2m", "-outprofile", f"s{k}.profile"], cwd=tmp_path, capture_output=True, text=True)
        assert s.returncode == 0, s.stderr
        for ext in ("tsv", "fa"):
            assert open(tmp_path / f"s{k}.{ext}").read() == open(tmp_path / f"b{k}.{ext}").read()
        if k != 2:
            single = open(tmp_path / f"s{k}.a2m").read()
            assert single == open(tmp_path / f"b{k}.a2m").read(), k
            assert single.count(">") > 4
        if k == 1:
            assert open(tmp_path / "s1.profile").read() == open(tmp_path / "b1.profile").read()
