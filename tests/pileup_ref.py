"""Reference side of the pileup and the consensus refinement (a helper, not a test): the contract of include/ramx.h
(ramx_col_pileup, ramx_recall_consensus, ramx_dev_refine) restated on the paths of align_ref.walk_family, and the renderers of
the `-outpileup` / `-outrefined` text.

The pileup is counted from every flank's path (`ops`, in path order), not from col_idx / col_ins: the device derives the
positions of the inserted bases from the columns and the running position, so the two sides do not share that step."""
import numpy as np

from repeatafterme_amd.datamodel import PILEUP_DTYPE, PILEUP_INS

import align_ref as ar


def base_class(flank, t, sequence):
    """A C G T -> 0..3 (lower case alike); 4: N, a position outside the flank's bounds, a position outside the library."""
    if not flank.inside(t):
        return 4
    b = flank.base(t, sequence)
    return b & 3 if 0 <= b < 8 else 4


def pileup_of(direction, cores, core_idx, results, sequence, W, cons):
    """walk() results of a family's flanks -> PILEUP_DTYPE [len(cons)]."""
    rows = len(cons)
    cols = np.zeros(rows, PILEUP_DTYPE)
    cols["base"] = np.asarray(cons, np.int32)
    for n, res in zip(core_idx, results):
        if res["end_row"] < 0:
            continue
        fl = ar.Flank(direction, cores, n, W)
        cols["cover"][:res["end_row"] + 1] += 1
        pending = []
        for op in res["ops"]:
            if op[0] == "I":
                pending.append(op[1])
                continue
            c = cols[op[1]]
            if pending:
                assert pending == list(range(pending[0], pending[0] + len(pending)))      # path order is increasing t
                c["ins_open"] += 1
                c["ins_long"] += len(pending) > PILEUP_INS
                c["ins_bases"] += len(pending)
                for k, t in enumerate(pending[:PILEUP_INS]):
                    c["ins"][k][base_class(fl, t, sequence)] += 1
            pending = []
            if op[0] == "M":
                c["match"][base_class(fl, op[2], sequence)] += 1
            else:
                c["del"] += 1
        assert len(pending) == res["tail_ins"]                                           # counted nowhere
    return cols


def pileup(direction, cores, sequence, p, cons, with_walks=False):
    sequence = np.ascontiguousarray(sequence, np.int8)
    idx, results = ar.walk_family(direction, cores, sequence, p, cons)
    cols = pileup_of(direction, cores, idx, results, sequence, p.bandwidth, cons)
    return (cols, idx, results) if with_walks else cols


def _plurality(v):
    best = 0
    for b in range(1, 4):
        if v[b] > v[best]:
            best = b
    return best


def recall(cons, cols, L):
    """One pass over the columns in order -> the new consensus (int8, at most L columns)."""
    out = []
    for r in range(len(cons)):
        c = cols[r]
        cover = int(c["cover"])
        if cover == 0:
            out.append(int(cons[r]))
            continue
        for k in range(PILEUP_INS):
            s = [int(x) for x in c["ins"][k]]
            if not (2 * sum(s) > cover and max(s[:4]) > 0):
                break
            out.append(_plurality(s))
        if 2 * int(c["del"]) > cover:
            continue
        m = [int(x) for x in c["match"][:4]]
        best, cur = _plurality(m), int(cons[r])
        out.append(cur if m[best] == 0 or m[cur] == m[best] else best)
    return np.asarray(out[:L], np.int8)


def refine(direction, cores, sequence, p, cons, max_replays):
    """-> (consensus, its pileup, replays, converged)"""
    assert max_replays >= 1
    cons = np.asarray(cons, np.int8)
    i = 0
    while True:
        cols = pileup(direction, cores, sequence, p, cons)
        nxt = recall(cons, cols, p.L)
        i += 1
        if np.array_equal(nxt, cons):
            return cons, cols, i, 1
        if i == max_replays:
            return cons, cols, i, 0
        cons = nxt


# ---------------------------------------------------------------------------------------------------- text

PILEUP_HEADER = "dir\trow\tbase\tcover\tA\tC\tG\tT\tN\tdel\tins_open\tins_long\tins_bases\t" + \
    "\t".join(f"i{k}_{b}" for k in range(PILEUP_INS) for b in "ACGTN") + "\n"


def render_pileup_block(tag, cols):
    """The lines of one block of `-outpileup`: tag is right / left / right-refined / left-refined."""
    lines = []
    for r, c in enumerate(cols):
        f = [tag, str(r), "ACGT"[int(c["base"])], str(int(c["cover"]))] + [str(int(x)) for x in c["match"]] + \
            [str(int(c[k])) for k in ("del", "ins_open", "ins_long", "ins_bases")] + [str(int(x)) for x in c["ins"].ravel()]
        lines.append("\t".join(f))
    return "".join(line + "\n" for line in lines)


def render_pileup(blocks):
    """blocks: {1: (kept cols, refined cols or None), 0: ...} -> the file: header, right, right-refined, left, left-refined."""
    out = [PILEUP_HEADER]
    for d in (1, 0):
        if d in blocks:
            name = "right" if d else "left"
            kept, refined = blocks[d]
            out.append(render_pileup_block(name, kept))
            if refined is not None:
                out.append(render_pileup_block(name + "-refined", refined))
    return "".join(out)


def render_refined(results):
    """results: {1: (consensus, replays, converged), 0: ...} -> the `-outrefined` FASTA; the left one reads as the sequence does."""
    out = []
    for d in (1, 0):
        if d in results:
            cons, replays, conv = results[d]
            s = "".join("ACGT"[int(b)] for b in cons)
            out.append(f">{'right' if d else 'left'}-extension-refined {len(cons)} bp replays={replays} converged={conv}\n")
            out.append((s if d else s[::-1]) + "\n")
    return "".join(out)


# ---------------------------------------------------------------------------------------------------- shared cases

# (flanks, L, W, K, seed), matrix: the families the fixed-point and restoration findings were made on; all with
# both_sides=True, minus_frac=0.4, n_run_frac=0.1, the loop's consensus taken with when_to_stop=1000
FAMILIES = [((37, 60, 14, 50, 41), "25p43g"), ((70, 80, 20, 70, 7), "14p43g"), ((37, 60, 40, 50, 3), "18p43g")]


def plant_edits(cons):
    """One dropped column, one substituted base and one spurious column, each at a column whose two neighbours differ from it and
    from each other: the dropped one nearest K/6, the substitution nearest K/2, the spurious one before the column nearest 5K/6
    (its base differs from both neighbours).  The two edits that change the length sit at opposite ends on purpose: 11 columns
    apart across a low-complexity stretch (family 3, direction 1, columns 26 and 37) they settle into another fixed point, the
    dropped base re-called on the far side of the stretch -- those two edits are not isolated.  -> (edited, (a, b, c))"""
    K = len(cons)
    ok = [r for r in range(1, K - 1) if len({int(cons[r - 1]), int(cons[r]), int(cons[r + 1])}) == 3]
    a, b, c = (min(ok, key=lambda r: abs(r - at)) for at in (K // 6, K // 2, 5 * K // 6))
    assert a + 2 < b and b + 2 < c
    e = [int(x) for x in cons]
    e.insert(c, next(v for v in range(4) if v not in (e[c - 1], e[c])))
    e[b] = next(v for v in range(4) if v not in (e[b - 1], e[b], e[b + 1]))
    del e[a]
    return np.asarray(e, np.int8), (a, b, c)
