"""Reference side of the dinucleotide pileup and the CpG-aware re-call (a helper, not a test): the contract of include/ramx.h
(ramx_col_dinuc, ramx_recall_cpg, ramx_dev_refine_cpg) restated on the paths of align_ref.walk_family, and the renderers of the
`-outcpg` / `-outdinuc` text.

As in pileup_ref.py the records are counted from every flank's path (`ops`, in path order), not from col_idx / col_ins: the
device derives "no base inserted between the two columns" from col_ins[r + 1], the restatement from the path itself."""
import numpy as np

from repeatafterme_amd.datamodel import DINUC_DTYPE, PILEUP_INS

import align_ref as ar
import pileup_ref as pr

A, C, G, T = 0, 1, 2, 3


def dinuc_of(direction, cores, core_idx, results, sequence, W, cons):
    """walk() results of a family's flanks -> DINUC_DTYPE [len(cons)]."""
    rows = len(cons)
    di = np.zeros(rows, DINUC_DTYPE)
    di["base"] = np.asarray(cons, np.int32)
    if rows:
        di["next"][:-1] = np.asarray(cons[1:], np.int32)
        di["next"][-1] = -1
    for n, res in zip(core_idx, results):
        if res["end_row"] < 0:
            continue
        fl = ar.Flank(direction, cores, n, W)
        prev, between, at = None, 0, 0              # what the path put into the row before; bases inserted since; the next row
        for op in res["ops"]:
            if op[0] == "I":
                between += 1
                continue
            assert op[1] == at                      # a path goes through rows 0 .. end_row, one column move each
            cur = "D" if op[0] == "D" else pr.base_class(fl, op[2], sequence)
            if at > 0:
                d = di[at - 1]
                d["both"] += 1
                if prev == "D" or cur == "D":
                    d["gapped"] += 1
                elif between:
                    d["split"] += 1
                else:
                    d["adjacent"] += 1
                    d["di"][prev][cur] += 1
            prev, between, at = cur, 0, at + 1
        assert at == res["end_row"] + 1
    return di


def pileups(direction, cores, sequence, p, cons, with_walks=False):
    """-> (pileup, dinucleotide pileup) of one walk of the family along cons (and the walk with with_walks)."""
    sequence = np.ascontiguousarray(sequence, np.int8)
    idx, results = ar.walk_family(direction, cores, sequence, p, cons)
    cols = pr.pileup_of(direction, cores, idx, results, sequence, p.bandwidth, cons)
    di = dinuc_of(direction, cores, idx, results, sequence, p.bandwidth, cons)
    return (cols, di, idx, results) if with_walks else (cols, di)


def identities_hold(di):
    """both == adjacent + split + gapped and adjacent == sum di for every record; the last record has no pair."""
    ok = np.array_equal(di["both"], di["adjacent"] + di["split"] + di["gapped"]) and \
        np.array_equal(di["adjacent"], di["di"].sum(axis=(1, 2))) and not di["reserved"].any()
    if len(di):
        last = di[-1]
        ok = ok and last["next"] == -1 and not any(int(last[k]) for k in ("both", "adjacent", "split", "gapped")) and not last["di"].any()
    return bool(ok)


# ---------------------------------------------------------------------------------------------------- re-call

def plain_calls(cons, cols, L):
    """Pass 1, the rule of pileup_ref.recall with its bookkeeping kept: -> (out, at, before): the output as a list, per row the
    place of its base in the output (None: dropped, or beyond the cut to L columns) and the inserted columns emitted before it."""
    out, at, before = [], [], []
    for r in range(len(cons)):
        at.append(None)
        before.append(0)
        if len(out) >= L:
            continue
        c = cols[r]
        cover = int(c["cover"])
        if cover == 0:
            at[r] = len(out)
            out.append(int(cons[r]))
            continue
        for k in range(PILEUP_INS):
            s = [int(x) for x in c["ins"][k]]
            if len(out) >= L or not (2 * sum(s) > cover and max(s[:4]) > 0):
                break
            out.append(pr._plurality(s))
            before[r] += 1
        if len(out) >= L or 2 * int(c["del"]) > cover:
            continue
        m = [int(x) for x in c["match"][:4]]
        best, cur = pr._plurality(m), int(cons[r])
        at[r] = len(out)
        out.append(cur if m[best] == 0 or m[cur] == m[best] else best)
    return out, at, before


def pair_sums(D, a, b, M, cpg_ts):
    """(S_plain, S_CG) of a pair in reading order: D[x][y] copies put class x into the 5' and y into the 3' column, (a, b) are
    the plain calls, M[c][s] = matrix[c * 100 + s].  Python integers: exact."""
    mC = lambda x: cpg_ts if x == T else M(C, x)
    mG = lambda y: cpg_ts if y == A else M(G, y)
    s_plain = sum(int(D[x][y]) * (M(a, x) + M(b, y)) for x in range(4) for y in range(4))
    s_cg = sum(int(D[x][y]) * (mC(x) + mG(y)) for x in range(4) for y in range(4))
    return s_plain, s_cg


def recall_cpg(cons, cols, di, rows_reversed, matrix, cpg_ts, L, with_pairs=False):
    """-> (the new consensus (int8, at most L columns), pairs called CG); with_pairs also the tested pairs as
    (row, a, b, S_plain, S_CG, called)."""
    mat = np.asarray(matrix).reshape(-1)
    M = lambda c, s: int(mat[c * 100 + s])
    plain, at, before = plain_calls(cons, cols, L)
    out, n_cpg, pairs = list(plain), 0, []
    for r in range(len(cons) - 1):
        if at[r] is None or at[r + 1] is None or before[r + 1] > 0:
            continue
        p5, p3 = (at[r + 1], at[r]) if rows_reversed else (at[r], at[r + 1])
        a, b = plain[p5], plain[p3]                 # the plain calls: pass 2 never reads what it wrote
        if a not in (C, T) or b not in (G, A):
            continue
        D = np.asarray(di[r]["di"]).T if rows_reversed else np.asarray(di[r]["di"])
        s_plain, s_cg = pair_sums(D, a, b, M, cpg_ts)
        called = (a, b) == (C, G) or s_cg > s_plain
        pairs.append((r, a, b, s_plain, s_cg, called))
        if called:
            assert out[p5] == plain[p5] and out[p3] == plain[p3]          # tested pairs are disjoint
            out[p5], out[p3] = C, G
            n_cpg += 1
    res = (np.asarray(out, np.int8), n_cpg)
    return res + (pairs,) if with_pairs else res


def refine_cpg(direction, cores, sequence, p, cons, max_replays, cpg_ts=0):
    """The loop of pileup_ref.refine with the CpG-aware re-call, rows_reversed = not direction.
    -> (consensus, its pileup, its dinucleotide pileup, replays, converged, n_cpg of the last re-call)"""
    assert max_replays >= 1
    cons = np.asarray(cons, np.int8)
    i = 0
    while True:
        cols, di = pileups(direction, cores, sequence, p, cons)
        nxt, n_cpg = recall_cpg(cons, cols, di, not direction, p.matrix, cpg_ts, p.L)
        i += 1
        if np.array_equal(nxt, cons):
            return cons, cols, di, i, 1, n_cpg
        if i == max_replays:
            return cons, cols, di, i, 0, n_cpg
        cons = nxt


# ---------------------------------------------------------------------------------------------------- text

DINUC_HEADER = "dir\trow\tbase\tnext\tboth\tadjacent\tsplit\tgapped\t" + "\t".join(x + y for x in "ACGTN" for y in "ACGTN") + "\n"


def render_dinuc(blocks):
    """blocks: {1: di, 0: di} -> the `-outdinuc` file: header, the right block, the left block (rows as the device has them)."""
    out = [DINUC_HEADER]
    for d in (1, 0):
        if d in blocks:
            for r, c in enumerate(blocks[d]):
                f = ["right" if d else "left", str(r), "ACGT"[int(c["base"])], "-" if c["next"] < 0 else "ACGT"[int(c["next"])]] + \
                    [str(int(c[k])) for k in ("both", "adjacent", "split", "gapped")] + [str(int(x)) for x in c["di"].ravel()]
                out.append("\t".join(f) + "\n")
    return "".join(out)


def render_cpg(results):
    """results: {1: (consensus, replays, converged, n_cpg), 0: ...} -> the `-outcpg` FASTA; the left one reads as the sequence does."""
    out = []
    for d in (1, 0):
        if d in results:
            cons, replays, conv, n_cpg = results[d]
            s = "".join("ACGT"[int(b)] for b in cons)
            out.append(f">{'right' if d else 'left'}-extension-cpg {len(cons)} bp replays={replays} converged={conv} cpg={n_cpg}\n")
            out.append((s if d else s[::-1]) + "\n")
    return "".join(out)
