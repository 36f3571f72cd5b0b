#!/usr/bin/env python3
"""Extend every family of a Stockholm file with ONE RAMExtend process per scoring group.

The reference's wrapper (util/extend-stk.pl) starts one RAMExtend per family (:349-364).  This driver performs the
same per-family preparation (repeatafterme_amd/stockholm.py), then hands all families that share a matrix /
-minimprovement to `RAMExtend -batch`, which extends them in one launch per direction.  Per family it leaves what the
wrapper's -onlyextend mode leaves (extend-stk.pl:391-427):

    <id>-linup.tsv  <id>-repam.log  <id>-repam-ranges.tsv  <id>-ext-cons.fa  <id>-repam-repseq.fa  <id>-combined-cons.fa

and, with -profile, <id>-profile.tsv: the per-column support of both extensions (RAMExtend -outprofile) -- how many copies
still carry the extension at every column, which the wrapper can only approximate through -minimprovement; with -aln,
<id>-aln.a2m: every extendable copy aligned to the kept consensus of both extensions (RAMExtend -outaln), which the wrapper
rebuilds with an external aligner from -cons and -outfa (extend-stk.pl:553-556); with --refine N, <id>-pileup.tsv and
<id>-refined-cons.fa: the per-column composition of both extensions and their consensus re-called from it over at most N
replays (RAMExtend -outpileup / -outrefined / -refine), the wrapper's `alignAndCallConsensus.pl -refine 10` step (:553-555);
with -copies, <id>-copies.tsv: every copy's divergence from the kept consensus of both extensions (RAMExtend -outcopies), and
per direction the family's mean Kimura divergence over the extension beside the matrix the wrapper's ladder would pick for it
-- the check that the matrix chosen from the seed alignment was the right one for the extended part; with -linkage,
<id>-linkage.tsv: the pairs of variant columns of both extensions whose variants travel together in the copies (RAMExtend
-outlinkage) -- the sign that the family is two subfamilies under one consensus.
<id>-cpg-cons.fa: with -cpg, the consensus of both extensions re-called with the CpG-aware rule (RAMExtend -outcpg; the replays are
--refine's, 10 without it) -- a CG that most copies have deaminated to TG / CA / TA comes back as CG.
<id>-tsd.tsv: with -tsd, the target-site duplication of every extended copy and the family's modal length (RAMExtend -outtsd).
<id>-period.tsv: with -period, the tandem periodicity of every copy's left and right extension -- did the extension run into a
simple repeat or a satellite? -- and the family's modal period per part (RAMExtend -outperiod).
<id>-term.tsv: with -term, the terminal repeats of every extended copy -- its first bases repeated at its end, directly (LTR) or
as their reverse complement (TIR) -- and the family's verdict (RAMExtend -outterm).
<id>-dist.tsv: with -dist, the pairwise divergence between the extended copies (RAMExtend -outdist).
xfam.tsv: with -xfam, after every scoring group has finished (a -outxfam per process would miss the pairs across groups), the
overlaps between the families' combined consensi -- left extension + reference + right extension, so the core is included --
and the groups of families that belong together, in the format of RAMExtend -outxfam with the family id in place of the index.

(the re-alignment and Stockholm rewriting that follow in the wrapper belong to RepeatModeler and are out of scope).
"""
import argparse
import os
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from repeatafterme_amd import stockholm as stk          # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_EXE = os.path.join(HERE, "..", "repeatafterme_amd", "RAMExtend")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-assembly", required=True, help="genome .2bit")
    ap.add_argument("-input", required=True, help="Stockholm file with one or more seed alignments")
    ap.add_argument("-outdir", default=".", help="where the per-family files go")
    ap.add_argument("-bandwidth", type=int, default=40)                 # extend-stk.pl:197
    ap.add_argument("-min_aligning_seqs", type=int, default=3)          # extend-stk.pl:192
    ap.add_argument("-L", type=int, default=20000)                      # extend-stk.pl:352
    ap.add_argument("-ramextend", default=DEFAULT_EXE)
    ap.add_argument("-profile", action="store_true", help="also write <id>-profile.tsv per family (RAMExtend -outprofile)")
    ap.add_argument("-aln", action="store_true", help="also write <id>-aln.a2m per family (RAMExtend -outaln)")
    ap.add_argument("--refine", type=int, default=0, metavar="N",
                    help="also write <id>-pileup.tsv and <id>-refined-cons.fa per family (RAMExtend -outpileup / -outrefined / -refine N)")
    ap.add_argument("-copies", action="store_true", help="also write <id>-copies.tsv per family (RAMExtend -outcopies) and print "
                    "each extension's divergence with the matrix it would call for")
    ap.add_argument("-linkage", action="store_true", help="also write <id>-linkage.tsv per family (RAMExtend -outlinkage)")
    ap.add_argument("-tsd", action="store_true", help="also write <id>-tsd.tsv per family (RAMExtend -outtsd) and print the modal "
                    "target-site duplication of the extended copies")
    ap.add_argument("-period", action="store_true", help="also write <id>-period.tsv per family (RAMExtend -outperiod) and print the "
                    "modal period of the copies' extensions")
    ap.add_argument("-term", action="store_true", help="also write <id>-term.tsv per family (RAMExtend -outterm) and print the "
                    "family's verdict (none, LTR, TIR) and the median lengths of the anchored repeats")
    ap.add_argument("-dist", action="store_true", help="also write <id>-dist.tsv per family (RAMExtend -outdist): the pairwise "
                    "divergence between the extended copies")
    ap.add_argument("-xfam", action="store_true", help="also write <outdir>/xfam.tsv: the overlaps between the combined consensi of "
                    "all families and the groups of families they join")
    ap.add_argument("-cpg", action="store_true", help="also write <id>-cpg-cons.fa per family (RAMExtend -outcpg)")
    ap.add_argument("-one_by_one", action="store_true", help="start one RAMExtend per family, as the wrapper does")
    a = ap.parse_args(argv)

    seeds = stk.read_stockholm(a.input)
    if not seeds:
        sys.exit(f"No seed alignments found in {a.input}!")
    os.makedirs(a.outdir, exist_ok=True)
    groups = {}
    for seed in seeds:
        fid = seed.name
        print(f"Working on {fid}..")
        rows, extendable = stk.ranges_for(seed)
        tdiv = stk.family_divergence(seed)
        matrix, minimp = stk.choose_scoring(tdiv, a.min_aligning_seqs)
        base = os.path.join(a.outdir, fid)
        with open(base + "-linup.tsv", "w") as fh:
            for r in rows:
                fh.write("%s\t%d\t%d\t%d\t%d\t%s\n" % r)
        print(f"  - Consensus length [recalculated]: {len(stk.reference_sequence(seed))}")
        print(f"  - Divergence: {tdiv:.2f} %")
        print(f"  - Instances: {len(seed.rows)}")
        if extendable > 3:                                              # extend-stk.pl:351
            groups.setdefault((matrix, minimp), []).append((seed, base))
        else:
            print(f"  **Too few extendable sequences ({extendable}) for RAMExtend**")

    finished = []
    for (matrix, minimp), fams in groups.items():
        finished += fams
        common = ["-twobit", a.assembly, "-L", str(a.L), "-bandwidth", str(a.bandwidth), "-matrix", matrix, "-vvv",
                  "-minimprovement", str(minimp)]
        print(f"  - Running RAMExtend [bandwidth={a.bandwidth}, matrix={matrix}, minimprovement={minimp}] on "
              f"{len(fams)} families..")
        if a.one_by_one:
            for seed, base in fams:
                with open(base + "-repam.log", "w") as log:
                    rc = subprocess.run([a.ramextend] + common + ["-ranges", base + "-linup.tsv", "-outtsv",
                                        base + "-repam-ranges.tsv", "-outfa", base + "-repam-repseq.fa", "-cons",
                                        base + "-ext-cons.fa"] + (["-outprofile", base + "-profile.tsv"] if a.profile else []) +
                                       (["-outaln", base + "-aln.a2m"] if a.aln else []) +
                                       (["-outpileup", base + "-pileup.tsv", "-outrefined", base + "-refined-cons.fa", "-refine",
                                         str(a.refine)] if a.refine > 0 else []) +
                                       (["-outcopies", base + "-copies.tsv"] if a.copies else []) +
                                       (["-outlinkage", base + "-linkage.tsv"] if a.linkage else []) +
                                       (["-outtsd", base + "-tsd.tsv"] if a.tsd else []) +
                                       (["-outcpg", base + "-cpg-cons.fa"] if a.cpg else []) +
                                       (["-outperiod", base + "-period.tsv"] if a.period else []) +
                                       (["-outterm", base + "-term.tsv"] if a.term else []) +
                                       (["-outdist", base + "-dist.tsv"] if a.dist else []),
                                       stdout=log, stderr=subprocess.STDOUT).returncode
                if rc:
                    sys.exit(f"  RAMExtend failed! [{rc}] see {base}-repam.log")
        else:
            lst = os.path.join(a.outdir, f"batch-{matrix}-{minimp}.list")
            with open(lst, "w") as fh:
                for seed, base in fams:
                    # fields six to seventeen are optional (the twelfth, the subfamily file, is never asked for here): "-" holds the place of one that is not asked for before one that is
                    opt = [base + "-profile.tsv" if a.profile else "-", base + "-aln.a2m" if a.aln else "-",
                           base + "-pileup.tsv" if a.refine > 0 else "-", base + "-refined-cons.fa" if a.refine > 0 else "-",
                           base + "-copies.tsv" if a.copies else "-", base + "-linkage.tsv" if a.linkage else "-", "-",
                           base + "-tsd.tsv" if a.tsd else "-", base + "-cpg-cons.fa" if a.cpg else "-",
                           base + "-period.tsv" if a.period else "-", base + "-term.tsv" if a.term else "-",
                           base + "-dist.tsv" if a.dist else "-"]
                    while opt and opt[-1] == "-":
                        opt.pop()
                    fh.write("\t".join([base + "-linup.tsv", base + "-repam.log", base + "-ext-cons.fa",
                                        base + "-repam-ranges.tsv", base + "-repam-repseq.fa"] + opt) + "\n")
            rc = subprocess.run([a.ramextend] + common + (["-refine", str(a.refine)] if a.refine > 0 else []) + ["-batch", lst]).returncode
            if rc:
                sys.exit(f"  RAMExtend -batch failed! [{rc}]")
        for seed, base in fams:                                         # extend-stk.pl:397-417
            reference = stk.reference_sequence(seed)
            found_right = False
            out = [">combined\n"]
            if os.path.exists(base + "-ext-cons.fa"):
                for line in open(base + "-ext-cons.fa"):
                    if line.startswith(">left-extension"):
                        continue
                    if line.startswith(">right-extension"):
                        found_right = True
                        out.append(reference + "\n")
                        continue
                    out.append(line)
            if not found_right:
                out.append(reference + "\n")
            with open(base + "-combined-cons.fa", "w") as fh:
                fh.writelines(out)
            t = [l.strip() for l in open(base + "-repam.log") if l.startswith("Extended ")]
            print(f"RAMExtend Results [{seed.name}]: " + "  ".join(t))
            if a.copies and os.path.exists(base + "-copies.tsv"):
                for line in open(base + "-copies.tsv"):                 # the summary line of each direction
                    if not line.startswith("#"):
                        continue
                    tag, copies, used, kim = line[1:].rstrip("\n").split("\t")
                    div = float(kim.split("=")[1])
                    would = stk.choose_scoring(div, a.min_aligning_seqs)[0]
                    print(f"  - Extension divergence [{tag}]: {div:.2f} % over {used.split('=')[1]} of {copies.split('=')[1]} copies: "
                          f"matrix {would} (used: {matrix})" + ("" if would == matrix or used.endswith("=0") else "  **differs**"))
            if a.linkage and os.path.exists(base + "-linkage.tsv"):
                for line in open(base + "-linkage.tsv"):                # the summary line of each direction
                    if line.startswith("#"):
                        tag, variants, pairs, linked = line[1:].rstrip("\n").split("\t")
                        print(f"  - Linked variants [{tag}]: {linked.split('=')[1]} of {pairs.split('=')[1]} pairs among "
                              f"{variants.split('=')[1]} variants")
            if a.tsd and os.path.exists(base + "-tsd.tsv"):
                for line in open(base + "-tsd.tsv"):                    # the summary line
                    if line.startswith("#mode"):
                        mode, count, null = (kv.split("=")[1] for kv in line.rstrip("\n").split("\t")[1:])
                        print(f"  - Target-site duplication: {mode} bp in {count} copies ({null} expected by chance)")
            if a.period and os.path.exists(base + "-period.tsv"):
                for line in open(base + "-period.tsv"):                 # the summary line of each part
                    if line.startswith("#part"):
                        kv = dict(f.split("=") for f in line.rstrip("\n").split("\t")[1:])
                        print(f"  - Tandem periodicity [{kv['part']}]: period {kv['mode']} in {kv['mode_count']} of {kv['n']} copies "
                              f"({kv['n_tract']} with a tract)")
            if a.term and os.path.exists(base + "-term.tsv"):
                for line in open(base + "-term.tsv"):                   # the summary line
                    if line.startswith("#family"):
                        kv = dict(f.split("=") for f in line.rstrip("\n").split("\t")[1:])
                        print(f"  - Terminal repeats: {kv['verdict']} (direct: {kv['direct_anchored']} of {kv['n']} copies anchored, median "
                              f"{kv['direct_median']} bp; inverted: {kv['inverted_anchored']}, median {kv['inverted_median']} bp)")
    if a.xfam:
        print(cross_family([(seed.name, base + "-combined-cons.fa") for seed, base in finished], os.path.join(a.outdir, "xfam.tsv")))
    return 0


def cross_family(families, out_path):
    """families: (id, combined consensus FASTA) of every family that was extended -> out_path, and the summary line."""
    import numpy as np
    from repeatafterme_amd import xfam
    code = np.full(256, 99, np.int8)
    for k, ch in enumerate("ACGTacgt"):
        code[ord(ch)] = k
    seqs = []
    for _, path in families:
        text = "".join(line.strip() for line in open(path) if not line.startswith(">"))
        seqs.append(code[np.frombuffer(text.encode(), np.uint8)] if text else np.zeros(0, np.int8))
    keep = [i for i, s in enumerate(seqs) if len(s) <= 32767]                # (a longer consensus is left out and named)
    owner = list(range(len(keep)))
    rec, pairs, counts, group = xfam.compare([seqs[i] for i in keep], owner, n_families=len(keep))
    line = xfam.write_tsv(out_path, [families[i][1] for i in keep], ["all"] * len(keep), [len(seqs[i]) for i in keep], pairs, rec,
                          counts, owner, group, labels=[families[i][0] for i in keep])
    with open(out_path, "a") as fh:
        for i in range(len(seqs)):
            if i not in keep:
                fh.write(f"#skipped\t{families[i][0]}\t{families[i][1]}\tall\t{len(seqs[i])}\n")
    return line


if __name__ == "__main__":
    sys.exit(main())
