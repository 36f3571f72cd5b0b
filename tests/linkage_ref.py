"""Reference side of the co-segregation of variants (a helper, not a test): the contract of include/ramx.h (ramx_plane,
ramx_dev_planes, ramx_dev_plane_gram, ramx_select_planes, ramx_link_pairs) restated on the paths of align_ref.walk_family, and
the renderer of the `-outlinkage` text.

The planes are taken from every flank's path (`ops`, in path order), not from col_idx / col_ins, as pileup_ref does; a plane is
a Python integer used as a bit set (bit i: flank i of the family), the Gram matrix the popcount of the AND, and the pair
statistic exact rational arithmetic (math.comb, fractions)."""
import functools
import math
from fractions import Fraction

import numpy as np

from repeatafterme_amd.datamodel import LINK_DTYPE, PLANE_COVER, PLANE_DTYPE, PLANE_NAMES

import align_ref as ar
from pileup_ref import base_class

CLASSES = 8


def planes_of(direction, cores, core_idx, results, sequence, W, cons):
    """walk() results of a family's flanks -> {(row, cls): bit set}, every (row, cls) of rows x 8 present."""
    rows = len(cons)
    pl = {(r, c): 0 for r in range(rows) for c in range(CLASSES)}
    for i, (n, res) in enumerate(zip(core_idx, results)):
        if res["end_row"] < 0:
            continue
        fl = ar.Flank(direction, cores, n, W)
        bit = 1 << i
        for r in range(res["end_row"] + 1):
            pl[(r, PLANE_COVER)] |= bit
        pending = 0
        for op in res["ops"]:
            if op[0] == "I":
                pending += 1
                continue
            if pending:
                pl[(op[1], 7)] |= bit
            pending = 0
            pl[(op[1], base_class(fl, op[2], sequence) if op[0] == "M" else 5)] |= bit
        assert pending == res["tail_ins"]                   # sets nothing
    return pl


def as_planes(pairs):
    out = np.zeros(len(pairs), PLANE_DTYPE)
    for k, (r, c) in enumerate(pairs):
        out[k] = (r, c)
    return out


def all_planes(rows):
    return as_planes([(r, c) for r in range(rows) for c in range(CLASSES)])


def gram(pl, planes):
    """-> int32 [P][P]"""
    sets = [pl[(int(x["row"]), int(x["cls"]))] for x in planes]
    P = len(sets)
    co = np.zeros((P, P), np.int32)
    for i, a in enumerate(sets):
        if a:
            for j in range(i, P):
                co[i, j] = co[j, i] = bin(a & sets[j]).count("1") if sets[j] else 0
    return co


def words(pl, planes, n_flanks):
    """-> uint64 [P][T]: what ramx_dev_plane_gram returns in bits"""
    T = (n_flanks + 63) // 64
    out = np.zeros((len(planes), T), np.uint64)
    for k, x in enumerate(planes):
        s = pl[(int(x["row"]), int(x["cls"]))]
        for t in range(T):
            out[k, t] = (s >> (64 * t)) & (2 ** 64 - 1)
    return out


def select(cons, cols, min_count=4, min_permille=100, max_variants=1024):
    """-> PLANE_DTYPE: the variants and the cover plane of every row that has one, sorted by (row, cls)"""
    cand = []
    for r in range(len(cons)):
        c = cols[r]
        for cls in (0, 1, 2, 3, 5, 7):
            if cls == int(cons[r]):
                continue
            count = int(c["match"][cls]) if cls < 4 else int(c["del"]) if cls == 5 else int(c["ins_open"])
            if count >= min_count and 1000 * count >= min_permille * int(c["cover"]):
                cand.append((r, cls, count))
    if len(cand) > max_variants:
        cand = sorted(cand, key=lambda x: (-x[2], x[0], x[1]))[:max(max_variants, 0)]
    keep = {(r, cls) for r, cls, _ in cand}
    keep |= {(r, PLANE_COVER) for r, _ in keep}
    return as_planes(sorted(keep))


def tail(n, n_p, n_q, k):
    """P(X >= k), X hypergeometric (n copies, n_p marked, n_q drawn), as a Fraction"""
    den = math.comb(n, n_q)
    return Fraction(sum(math.comb(n_p, x) * math.comb(n - n_p, n_q - x) for x in range(k, min(n_p, n_q) + 1)), den)


def mlog10(pv):
    """-log10 of a Fraction in (0, 1], without cancellation next to 1"""
    if pv == 1:
        return 0.0
    return -math.log1p(-float(1 - pv)) / math.log(10) if pv > Fraction(1, 2) else -math.log10(float(pv))


def link_pairs(planes, co, min_mlog10p=0.0):
    """-> list of dicts (p, q, n, n_p, n_q, n_pq, expected as a Fraction, mlog10p) in (p, q) order"""
    P = len(planes)
    where = {(int(x["row"]), int(x["cls"])): k for k, x in enumerate(planes)}
    out = []
    for p in range(P):
        for q in range(p + 1, P):
            a, b = planes[p], planes[q]
            if PLANE_COVER in (int(a["cls"]), int(b["cls"])) or a["row"] == b["row"]:
                continue
            cp, cq = where.get((int(a["row"]), PLANE_COVER)), where.get((int(b["row"]), PLANE_COVER))
            if cp is None or cq is None:
                continue
            n, n_p, n_q, n_pq = int(co[cp][cq]), int(co[p][cq]), int(co[q][cp]), int(co[p][q])
            score = 0.0 if n == 0 or n_pq == 0 else mlog10(tail(n, n_p, n_q, n_pq))
            if score >= min_mlog10p:
                out.append(dict(p=p, q=q, n=n, n_p=n_p, n_q=n_q, n_pq=n_pq, expected=Fraction(n_p * n_q, n) if n else Fraction(0),
                                mlog10p=score))
    return out


# ---------------------------------------------------------------------------------------------------- -outlinkage text

LINKAGE_HEADER = "dir\trow_a\tvar_a\tcount_a\trow_b\tvar_b\tcount_b\tn\tn_a\tn_b\tn_ab\texpected\tmlog10p\n"


def render_block(direction, planes, co, min_score=3):
    tag = "right" if direction else "left"
    tested, linked = link_pairs(planes, co), link_pairs(planes, co, min_score)
    lines = []
    for l in linked:
        a, b = planes[l["p"]], planes[l["q"]]
        lines.append("\t".join([tag, str(int(a["row"])), PLANE_NAMES[int(a["cls"])], str(int(co[l["p"]][l["p"]])),
                                str(int(b["row"])), PLANE_NAMES[int(b["cls"])], str(int(co[l["q"]][l["q"]])),
                                str(l["n"]), str(l["n_p"]), str(l["n_q"]), str(l["n_pq"]),
                                f"{float(l['expected']):.4f}", f"{l['mlog10p']:.4f}"]))
    variants = sum(int(x["cls"]) != PLANE_COVER for x in planes)
    lines.append(f"#{tag}\tvariants={variants}\tpairs={len(tested)}\tlinked={len(linked)}")
    return "".join(line + "\n" for line in lines)


def render_linkage(blocks, min_score=3):
    """blocks: {1: (planes, co), 0: ...} -> the file: header, the right block, the left block."""
    return LINKAGE_HEADER + "".join(render_block(d, *blocks[d], min_score) for d in (1, 0) if d in blocks)


def same_linkage_text(got, want):
    """Integer fields and names exactly, the two %.4f fields within one unit of their last printed digit (compared in those
    units, as copystats_ref.same_copies_text)."""
    g, w = got.splitlines(), want.splitlines()
    assert len(g) == len(w), (len(g), len(w))
    for k, (a, b) in enumerate(zip(g, w)):
        fa, fb = a.split("\t"), b.split("\t")
        if k == 0 or a.startswith("#"):
            assert a == b, f"line {k}: {a!r} != {b!r}"
            continue
        assert len(fa) == len(fb) == 13 and fa[:11] == fb[:11], f"line {k}: {a!r} != {b!r}"
        for x, y in zip(fa[11:], fb[11:]):
            assert abs(round(float(x) * 1e4) - round(float(y) * 1e4)) <= 1, f"line {k}: {x} != {y}"


# ---------------------------------------------------------------------------------------------------- shared cases

@functools.lru_cache(maxsize=None)
def shape_case(n, W, L, matrix, direction, what):
    """copystats_ref.shape_case with the family's planes."""
    import copystats_ref as cr
    c = dict(cr.shape_case(n, W, L, matrix, direction, what))
    c["planes"] = planes_of(direction, c["fs"].cores, c["idx"], c["results"], c["seq"], W, c["cons"])
    return c


# the planted family: two lineages under one consensus.  (flanks, L, W, K, seed), matrix, when_to_stop; every third flank
# carries another base at three columns
PLANTED_FAMILY = ((70, 80, 20, 70, 7), "14p43g", 30)
PLANTED_COLUMNS = (8, 30, 55)
PLANTED_EVERY = 3
CLI_SCORE = 3
# the one pair of the right direction that scores above 1 without having been planted (tests/test_linkage_ref.py,
# test_the_planted_family): column 0 deleted x bases inserted before column 1
UNPLANTED_PAIR = ((0, 5), (1, 7))


def planted_family(spec=PLANTED_FAMILY, columns=PLANTED_COLUMNS, every=PLANTED_EVERY):
    """The planted family of a spec, computed once however the spec is spelled (the defaults left out or written out)."""
    return _planted_family(spec, tuple(columns), every)


@functools.lru_cache(maxsize=None)
def _planted_family(spec, columns, every):
    """-> (fs, sequence with the variants planted, p, {direction: kept consensus}, {direction: the planted (row, cls)}).  The
    kept consensus of each direction is the oracle's on the family as generated; the base matched to `columns` (8, 30 and 55) of
    every `every`-th (third) flank is then overwritten by (cons[r] + 1) % 4, complemented on the reverse strand."""
    from oracle import pyoracle as po
    from repeatafterme_amd.datamodel import new_master
    from repeatafterme_amd.synth import synth_family
    (n, L, W, K, seed), matrix, stop = spec
    fs = synth_family(n, L, W, K=K, seed=seed, both_sides=True, minus_frac=0.4, n_run_frac=0.1)
    seq = np.ascontiguousarray(fs.sequence, np.int8).copy()
    p = po.Params.named(matrix, bandwidth=W, L=L, when_to_stop=stop)
    cons, planted = {}, {}
    walks = {}
    for d in (1, 0):
        o = po.oracle_extend(d, fs.cores.copy(), seq, new_master(L), p, trace=True)
        cons[d] = o.col_base[:o.ret].copy()
        walks[d] = ar.walk_family(d, fs.cores, seq, p, cons[d])
    for d in (1, 0):
        idx, results = walks[d]
        planted[d] = tuple((r, (int(cons[d][r]) + 1) % 4) for r in columns)
        for k in range(0, len(idx), every):
            fl = ar.Flank(d, fs.cores, idx[k], W)
            for op in results[k]["ops"]:
                if op[0] == "M" and op[1] in columns and fl.inside(op[2]):
                    write_base(fl, op[2], seq, (int(cons[d][op[1]]) + 1) % 4)
    seq.setflags(write=False)
    for d in cons:
        cons[d].setflags(write=False)
    return fs, seq, p, cons, planted


def write_base(fl, t, sequence, base):
    """Make flank position t read as `base` (the inverse of Flank.base: complemented on the reverse strand)."""
    si = fl.start + fl.sgn * t
    assert 0 <= si < len(sequence)
    for code in range(4):
        sequence[si] = code
        if fl.base(t, sequence) == base:
            return
    raise AssertionError("no code gives that base")


def planted_case(direction, spec=PLANTED_FAMILY, columns=PLANTED_COLUMNS, every=PLANTED_EVERY):
    """The planted family walked again along the kept consensus: planes, pileup, selection, Gram and pairs, computed once."""
    return _planted_case(direction, spec, tuple(columns), every)


@functools.lru_cache(maxsize=None)
def _planted_case(direction, spec, columns, every):
    from pileup_ref import pileup_of
    fs, seq, p, cons, planted = planted_family(spec, columns, every)
    c = cons[direction]
    idx, results = ar.walk_family(direction, fs.cores, seq, p, c)
    cols = pileup_of(direction, fs.cores, idx, results, seq, p.bandwidth, c)
    pl = planes_of(direction, fs.cores, idx, results, seq, p.bandwidth, c)
    sel = select(c, cols, 4, 100, 1024)
    co = gram(pl, sel)
    return dict(fs=fs, seq=seq, p=p, cons=c, idx=idx, results=results, cols=cols, planes=pl, sel=sel, co=co,
                pairs=link_pairs(sel, co), planted=planted[direction])
