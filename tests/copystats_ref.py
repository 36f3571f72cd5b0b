"""Reference side of the per-copy statistics (a helper, not a test): the contract of include/ramx.h (ramx_copy_stats,
ramx_copy_kimura, ramx_family_divergence) restated on the paths of align_ref.walk_family, and the renderer of the `-outcopies`
text.

The records are counted from every flank's path (`ops`, in path order), not from col_idx / col_ins: the device counts a
deletion's opening and the insertion runs from the columns, so the two sides do not share that step."""
import functools
import math

import numpy as np

from repeatafterme_amd.datamodel import COPY_STATS_DTYPE

import align_ref as ar
from pileup_ref import base_class

FIELDS = COPY_STATS_DTYPE.names


def cpg_columns(cons, rows_reversed):
    """Column r lies in a CpG: it is the C and the next column in reading order is G, or the G and the previous one is C."""
    rows, step = len(cons), -1 if rows_reversed else 1
    at = lambda r: int(cons[r]) if 0 <= r < rows else -1
    return [(at(r) == 1 and at(r + step) == 2) or (at(r) == 2 and at(r - step) == 1) for r in range(rows)]


def stats_of(direction, cores, core_idx, results, sequence, W, cons, rows_reversed):
    """walk() results of a family's flanks -> COPY_STATS_DTYPE [len(results)]."""
    out = np.zeros(len(results), COPY_STATS_DTYPE)
    cpg = cpg_columns(cons, rows_reversed)
    purine = (0, 2)
    for i, (n, res) in enumerate(zip(core_idx, results)):
        if res["end_row"] < 0:
            continue
        fl = ar.Flank(direction, cores, n, W)
        s = out[i]
        s["cols"], s["score"] = res["end_row"] + 1, res["score"]
        prev, pending = None, 0
        for op in res["ops"]:
            if op[0] == "I":
                pending += 1
            else:
                if pending:
                    s["ins"] += pending
                    s["ins_open"] += 1
                pending = 0
                if op[0] == "D":
                    s["del"] += 1
                    s["del_open"] += prev != "D"          # the first move, after a matched column, or after inserted bases
                else:
                    r, b, c = op[1], base_class(fl, op[2], sequence), int(cons[op[1]])
                    if b == 4:
                        s["n_match"] += 1
                    else:
                        kind = "match" if b == c else "ts" if (b in purine) == (c in purine) else "tv"
                        s[kind] += 1
                        if cpg[r]:
                            s["cpg_cols"] += 1
                            s["cpg_ts"] += kind == "ts"
            prev = op[0]
        assert pending == res["tail_ins"]                   # counted nowhere
    return out


def copy_stats(direction, cores, sequence, p, cons, rows_reversed=None, with_walks=False):
    """rows_reversed: None -> not direction, as seam 1 passes it."""
    sequence = np.ascontiguousarray(sequence, np.int8)
    if rows_reversed is None:
        rows_reversed = not direction
    idx, results = ar.walk_family(direction, cores, sequence, p, cons)
    st = stats_of(direction, cores, idx, results, sequence, p.bandwidth, cons, rows_reversed)
    return (st, idx, results) if with_walks else st


def kimura(s):
    """Percent; None: undefined."""
    sites = int(s["match"]) + int(s["ts"]) + int(s["tv"])
    if sites == 0:
        return None
    p, q = int(s["ts"]) / sites, int(s["tv"]) / sites
    a, b = 1 - 2 * p - q, 1 - 2 * q
    if a <= 0 or b <= 0:
        return None
    return -0.5 * math.log(a * math.sqrt(b)) * 100.0 + 0.0          # + 0.0: no divergence is 0, not -0


def family_divergence(stats, min_sites=1):
    """-> (mean over the copies with enough sites and a defined value, their number); 0.0 when there are none."""
    need = max(int(min_sites), 1)
    ks = [kimura(s) for s in stats if int(s["match"]) + int(s["ts"]) + int(s["tv"]) >= need]
    ks = [k for k in ks if k is not None]
    return (sum(ks) / len(ks) if ks else 0.0), len(ks)


# ---------------------------------------------------------------------------------------------------- -outcopies text

COPIES_HEADER = "dir\tcopy\tend_row\tstart\tend\tscore\tcols\tmatch\tts\ttv\tn\tdel\tdel_open\tins\tins_open\tcpg_cols\tcpg_ts\tkimura\n"


def render_block(direction, names, core_idx, results, stats):
    tag = "right" if direction else "left"
    lines = []
    for n, res, s in zip(core_idx, results, stats):
        k = kimura(s)
        f = [tag, names[n], str(res["end_row"]), str(res["start_idx"]), str(res["end_idx"])] + \
            [str(int(s[x])) for x in ("score", "cols", "match", "ts", "tv", "n_match", "del", "del_open", "ins", "ins_open",
                                      "cpg_cols", "cpg_ts")] + ["NA" if k is None else f"{k:.4f}"]
        lines.append("\t".join(f))
    div, used = family_divergence(stats, 1)
    lines.append(f"#{tag}\tcopies={len(stats)}\tused={used}\tkimura={div:.4f}")
    return "".join(line + "\n" for line in lines)


def render_copies(blocks):
    """blocks: {1: (names, core_idx, results, stats), 0: ...} -> the file: header, the right block, the left block."""
    return COPIES_HEADER + "".join(render_block(d, *blocks[d]) for d in (1, 0) if d in blocks)


def same_copies_text(got, want):
    """Integer fields and ids exactly, the kimura fields numerically within 1e-4: one unit of the last printed digit (compared
    in those units, so that the decimal text's binary rounding does not enter)."""
    g, w = got.splitlines(), want.splitlines()
    assert len(g) == len(w), (len(g), len(w))
    for k, (a, b) in enumerate(zip(g, w)):
        fa, fb = a.split("\t"), b.split("\t")
        assert len(fa) == len(fb), f"line {k}"
        assert fa[:-1] == fb[:-1], f"line {k}: {a!r} != {b!r}"
        la, lb = fa[-1], fb[-1]
        if la.startswith("kimura="):
            assert lb.startswith("kimura=")
            la, lb = la[7:], lb[7:]
        if "NA" in (la, lb) or k == 0:
            assert la == lb, f"line {k}"
        else:
            assert abs(round(float(la) * 1e4) - round(float(lb) * 1e4)) <= 1, f"line {k}: {la} != {lb}"


# ---------------------------------------------------------------------------------------------------- shared cases

@functools.lru_cache(maxsize=None)
def shape_case(n, W, L, matrix, direction, what):
    """One of the shapes of tests/test_gpu_pileup.py (same synth_family arguments and seeds), one direction, along the kept
    consensus or along foreign(...): everything the CPU and the GPU tests compare against, computed once."""
    import test_gpu_pileup as tp
    from oracle import pyoracle as po
    from repeatafterme_amd.datamodel import new_master
    from repeatafterme_amd.synth import synth_family
    from pileup_ref import pileup_of
    fs = synth_family(n, L, W, K=L // 2, seed=500 + n + W, both_sides=True, minus_frac=0.4, n_run_frac=0.1)
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    p = po.Params.named(matrix, bandwidth=W, L=L, when_to_stop=30)
    o = po.oracle_extend(direction, fs.cores.copy(), seq, new_master(L), p, trace=True)
    cons = o.col_base[:o.ret].copy() if what == "kept" else tp.foreign(o.col_base[:o.rows_executed], at=10, k=3)
    stats, idx, results = copy_stats(direction, fs.cores, seq, p, cons, with_walks=True)
    cols = pileup_of(direction, fs.cores, idx, results, seq, W, cons)
    for a in (cons, stats, cols):
        a.setflags(write=False)
    return dict(fs=fs, seq=seq, p=p, cons=cons, stats=stats, idx=idx, results=results, cols=cols)


# a small family whose paths end in inserted bases (tail_ins > 0, found on the CPU: 6 flanks of direction 1, 9 of direction 0):
# it takes a gap that pays, go + ge > 0.  Band width 7 has no instantiation of its own, and a positive gap term takes the
# row-buffer route of the forward kernel.  (flanks, L, W, K, seed), matrix, gapopen, gapextn
TAIL_FAMILY = ((10, 40, 7, 25, 43), "14p43g", 10, -7)


@functools.lru_cache(maxsize=None)
def tail_case(direction):
    from oracle import pyoracle as po
    from repeatafterme_amd.datamodel import new_master
    from repeatafterme_amd.synth import synth_family
    from pileup_ref import pileup_of
    (n, L, W, K, seed), matrix, go, ge = TAIL_FAMILY
    fs = synth_family(n, L, W, K=K, seed=seed, both_sides=True, minus_frac=0.3, n_run_frac=0.1)
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    p = po.Params.named(matrix, bandwidth=W, L=L, cappenalty=-10, when_to_stop=1000)
    p.gapopen, p.gapextn = go, ge
    o = po.oracle_extend(direction, fs.cores.copy(), seq, new_master(L), p, trace=True)
    cons = o.col_base[:o.ret].copy()
    stats, idx, results = copy_stats(direction, fs.cores, seq, p, cons, with_walks=True)
    cols = pileup_of(direction, fs.cores, idx, results, seq, W, cons)
    for a in (cons, stats, cols):
        a.setflags(write=False)
    return dict(fs=fs, seq=seq, p=p, cons=cons, stats=stats, idx=idx, results=results, cols=cols)
