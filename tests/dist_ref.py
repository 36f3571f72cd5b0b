"""Reference side of the pairwise divergence between copies (a helper, not a test): the contract of include/ramx_dist.h
(ramx_copy_dist, ramx_dev_copy_dist, ramx_select_copies, ramx_dist_kimura, ramx_dist_summary) restated on the paths of
align_ref.walk_family, and the renderer and parser of the `-outdist` text.

Every copy becomes a map row -> class (0..3 a base, 4 N, 5 deleted) from its path (`ops`, in path order, as
linkage_ref.planes_of reads it) -- not from planes --, and a pair is counted by a plain loop over the rows."""
import functools
import math

import numpy as np

from repeatafterme_amd.datamodel import COPY_DIST_DTYPE, COPY_DIST_FIELDS

import align_ref as ar
from pileup_ref import base_class

MAX_COPIES = 2048
DELETED = 5


def maps_of(direction, cores, core_idx, results, sequence, W, cons):
    """walk() results of a family's flanks -> per copy {row: class}; rows >= len(cons) never occur, a copy without an alignment
    has an empty map.  Inserted bases and tail_ins leave no trace."""
    rows = len(cons)
    out = []
    for n, res in zip(core_idx, results):
        m = {}
        if res["end_row"] >= 0:
            fl = ar.Flank(direction, cores, n, W)
            for op in res["ops"]:
                if op[0] == "I":
                    continue
                assert 0 <= op[1] <= res["end_row"] and op[1] not in m
                m[op[1]] = base_class(fl, op[2], sequence) if op[0] == "M" else DELETED
            assert sorted(m) == list(range(res["end_row"] + 1))        # covered: every row up to end_row, once
            m = {r: c for r, c in m.items() if r < rows}
        out.append(m)
    return out


def pair(ma, mb):
    """One record from two maps, by the rules of the contract."""
    cover = sites = ts = tv = del_one = del_both = 0
    for r, a in ma.items():
        if r not in mb:
            continue
        b = mb[r]
        cover += 1
        if a < 4 and b < 4:
            sites += 1
            if a != b:
                if {a, b} in ({0, 2}, {1, 3}):
                    ts += 1
                else:
                    tv += 1
        if a == DELETED and b == DELETED:
            del_both += 1
        elif a == DELETED or b == DELETED:
            del_one += 1
    return cover, sites, ts, tv, del_one, del_both


def matrix(maps, copies):
    """-> COPY_DIST_DTYPE [C][C] of the listed copies"""
    C = len(copies)
    out = np.zeros((C, C), COPY_DIST_DTYPE)
    for i in range(C):
        for j in range(i, C):
            out[i, j] = out[j, i] = pair(maps[int(copies[i])], maps[int(copies[j])])
    return out


def matrix_of_one_word(maps, copies, rows):
    """The same for rows <= 64 through one 64-bit word per copy and stream and numpy: for the 2,048 x 2,048 matrix."""
    assert rows <= 64
    C = len(copies)
    st = np.zeros((5, C), np.uint64)
    for k, i in enumerate(copies):
        for r, c in maps[int(i)].items():
            bit = np.uint64(1 << r)
            st[4, k] |= bit
            if c < 4:
                st[0, k] |= bit
                if c & 1:
                    st[1, k] |= bit
                if c & 2:
                    st[2, k] |= bit
            elif c == DELETED:
                st[3, k] |= bit

    def pop(x):
        m1, m2, m4, h = (np.uint64(k) for k in (0x5555555555555555, 0x3333333333333333, 0x0F0F0F0F0F0F0F0F, 0x0101010101010101))
        x = x - ((x >> np.uint64(1)) & m1)
        x = (x & m2) + ((x >> np.uint64(2)) & m2)
        x = (x + (x >> np.uint64(4))) & m4
        return ((x * h) >> np.uint64(56)).astype(np.int32)
    V, LO, HI, D, CV = (s[:, None] for s in st)
    v, x, y, c = V & V.T, LO ^ LO.T, HI ^ HI.T, CV & CV.T
    out = np.zeros((C, C), COPY_DIST_DTYPE)
    out["cover"], out["sites"], out["ts"], out["tv"] = pop(c), pop(v), pop(v & y & ~x), pop(v & x)
    out["del_one"], out["del_both"] = pop((D ^ D.T) & c), pop(D & D.T)
    return out


def select(end_rows, rows, min_cols=1, max_copies=256):
    """-> ascending list of the copies kept"""
    max_copies = min(max(int(max_copies), 0), MAX_COPIES)
    cols = [(min(e, rows - 1) + 1 if e >= 0 else 0) for e in end_rows]
    ok = [i for i, (e, c) in enumerate(zip(end_rows, cols)) if e >= 0 and c >= max(int(min_cols), 1)]
    if len(ok) > max_copies:
        ok = sorted(ok, key=lambda i: (-cols[i], i))[:max_copies]
    return sorted(ok)


def kimura(rec):
    """Percent; None: undefined."""
    sites = int(rec["sites"])
    if sites <= 0:
        return None
    p, q = int(rec["ts"]) / sites, int(rec["tv"]) / sites
    a, b = 1 - 2 * p - q, 1 - 2 * q
    if a <= 0 or b <= 0:
        return None
    return -0.5 * math.log(a * math.sqrt(b)) * 100.0 + 0.0


def summary(m, min_sites=1):
    """-> dict(n, pairs, used, medoid, mean, medoid_mean)"""
    n = len(m)
    need = max(int(min_sites), 1)
    val = {}
    for a in range(n):
        for b in range(a + 1, n):
            k = kimura(m[a][b]) if int(m[a][b]["sites"]) >= need else None
            if k is not None:
                val[(a, b)] = k
    medoid, best = -1, 0.0
    for a in range(n):
        mine = [k for (x, y), k in val.items() if a in (x, y)]
        if mine and (medoid < 0 or sum(mine) / len(mine) < best):
            medoid, best = a, sum(mine) / len(mine)
    return dict(n=n, pairs=n * (n - 1) // 2, used=len(val), medoid=medoid, mean=sum(val.values()) / len(val) if val else 0.0,
                medoid_mean=best)


# ---------------------------------------------------------------------------------------------------- -outdist text

DIST_HEADER = "dir\tcopy_a\tcopy_b\tcover\tsites\tts\ttv\tdel_one\tdel_both\tkimura\n"
TAGS = {1: "right", 0: "left", 2: "both"}


def render_block(tag, n_copies, names, m, min_sites=20):
    """names: the selected copies' names in list order; m their matrix"""
    lines = []
    for a in range(len(names)):
        for b in range(a + 1, len(names)):
            k = kimura(m[a][b])
            lines.append("\t".join([tag, names[a], names[b]] + [str(int(m[a][b][f])) for f in COPY_DIST_FIELDS] +
                                   ["NA" if k is None else f"{k:.4f}"]))
    s = summary(m, min_sites)
    med = "NA" if s["medoid"] < 0 else names[s["medoid"]]
    medk = "NA" if s["medoid"] < 0 else f"{s['medoid_mean']:.4f}"
    lines.append(f"#{tag}\tcopies={n_copies}\tselected={len(names)}\tpairs={s['pairs']}\tused={s['used']}\tkimura={s['mean']:.4f}"
                 f"\tmedoid={med}\tmedoid_kimura={medk}")
    return "".join(line + "\n" for line in lines)


def both_block(blocks):
    """blocks: {direction: (core_index of every flank, selected flanks, matrix)} with both directions -> (cores that are flanks
    of both, the cores selected in both in the right block's order, the field-wise sum of their records)"""
    (ci1, sel1, m1), (ci0, sel0, m0) = blocks[1], blocks[0]
    at1 = {int(ci1[i]): k for k, i in enumerate(sel1)}
    at0 = {int(ci0[i]): k for k, i in enumerate(sel0)}
    cores = [c for c in at1 if c in at0]
    m = np.zeros((len(cores), len(cores)), COPY_DIST_DTYPE)
    for a, ca in enumerate(cores):
        for b, cb in enumerate(cores):
            for f in COPY_DIST_FIELDS:
                m[a, b][f] = int(m1[at1[ca], at1[cb]][f]) + int(m0[at0[ca], at0[cb]][f])
    return len(set(int(x) for x in ci1) & set(int(x) for x in ci0)), cores, m


def render_dist(blocks, names, min_sites=20):
    """blocks as both_block takes them (one or both directions); names: core -> name.  -> the file: header, the right block, the
    left block and, with both, the block of the cores selected in both."""
    text = DIST_HEADER
    for d in (1, 0):
        if d in blocks:
            ci, sel, m = blocks[d]
            text += render_block(TAGS[d], len(ci), [names[int(ci[i])] for i in sel], m, min_sites)
    if 1 in blocks and 0 in blocks:
        n, cores, m = both_block(blocks)
        text += render_block(TAGS[2], n, [names[c] for c in cores], m, min_sites)
    return text


def parse_dist(text):
    """-> {tag: (list of (copy_a, copy_b, record tuple, kimura text), summary dict)}"""
    lines = text.splitlines()
    assert lines[0] + "\n" == DIST_HEADER
    out = {}
    for line in lines[1:]:
        f = line.split("\t")
        if line.startswith("#"):
            out.setdefault(f[0][1:], ([], {}))[1].update(dict(x.split("=", 1) for x in f[1:]))
        else:
            assert len(f) == 10
            out.setdefault(f[0], ([], {}))[0].append((f[1], f[2], tuple(int(x) for x in f[3:9]), f[9]))
    return out


def same_dist_text(got, want):
    """Integer fields and names exactly, the %.4f fields within one unit of their last printed digit (compared in those units,
    as linkage_ref.same_linkage_text)."""
    def close(x, y, where):
        if "NA" in (x, y):
            assert x == y, where
        else:
            assert abs(round(float(x) * 1e4) - round(float(y) * 1e4)) <= 1, f"{where}: {x} != {y}"
    g, w = got.splitlines(), want.splitlines()
    assert len(g) == len(w), (len(g), len(w))
    for k, (a, b) in enumerate(zip(g, w)):
        fa, fb = a.split("\t"), b.split("\t")
        assert len(fa) == len(fb), f"line {k}: {a!r} != {b!r}"
        if k == 0:
            assert a == b
        elif a.startswith("#"):
            for x, y in zip(fa, fb):
                if x.startswith(("kimura=", "medoid_kimura=")):
                    assert x.split("=")[0] == y.split("=")[0]
                    close(x.split("=")[1], y.split("=")[1], f"line {k}")
                else:
                    assert x == y, f"line {k}: {a!r} != {b!r}"
        else:
            assert fa[:9] == fb[:9], f"line {k}: {a!r} != {b!r}"
            close(fa[9], fb[9], f"line {k}")


# ---------------------------------------------------------------------------------------------------- shared cases

@functools.lru_cache(maxsize=None)
def shape_case(n, W, L, matrix_name, direction, what):
    """linkage_ref.shape_case with the family's maps and the matrix of all its copies."""
    import linkage_ref as lr
    c = dict(lr.shape_case(n, W, L, matrix_name, direction, what))
    c["maps"] = maps_of(direction, c["fs"].cores, c["idx"], c["results"], c["seq"], W, c["cons"])
    c["dist"] = matrix(c["maps"], range(len(c["idx"])))
    c["dist"].setflags(write=False)
    return c
