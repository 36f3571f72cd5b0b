"""Restatement of the cross-family contract (include/ramx_xfam.h) in plain Python (a helper, not a test): the candidates by
K-mer sets per sequence and orientation, the counting rule and the groups.  Nothing here is shared with the library; the record
of a pair comes from the restatement of the terminal repeats, tests/term_ref.py.  Pairs are tuples (a, b, inverted), records the
tuples of term_ref (score, a_start, a_end, b_start, b_end, matches, columns, T)."""
import numpy as np

import term_ref

DEFAULT = dict(match=2, mismatch=3, gap=5, min_score=80)
LINK = dict(min_columns=80, min_permille=800)


def oriented(b, inverted):
    """B' as classes: B, or B reversed with the classes below 4 complemented."""
    c = term_ref.classes(b)
    if inverted:
        c = c[::-1]
        c = np.where(c < 4, 3 - c, c).astype(np.int8)
    return c


def record(a, b, inverted, **params):
    """The record of one pair of code arrays; a zero-length side gives all zeros."""
    p = dict(DEFAULT)
    p.update(params)
    if len(a) == 0 or len(b) == 0:
        return (0,) * 8
    return term_ref.pair(term_ref.classes(a), oriented(b, inverted), **p)


def kmers(classes, K):
    """The set of K-tuples of classes below 4."""
    c = [int(x) for x in classes]
    return {tuple(c[o:o + K]) for o in range(len(c) - K + 1) if all(x < 4 for x in c[o:o + K])}


def candidates(seqs, owner, K=16, within=False):
    """All candidates in ascending (a, b, inverted) order."""
    if not (K == 0 or 8 <= K <= 16):
        raise ValueError("K")
    fwd = [kmers(term_ref.classes(s), K) if K else None for s in seqs]
    rev = [kmers(oriented(s, 1), K) if K else None for s in seqs]
    out = []
    for a in range(len(seqs)):
        for b in range(a + 1, len(seqs)):
            if owner[a] == owner[b] and not within:
                continue
            if len(seqs[a]) == 0 or len(seqs[b]) == 0:
                continue
            for inv in (0, 1):
                if K == 0 or (fwd[a] & (rev[b] if inv else fwd[b])):
                    out.append((a, b, inv))
    return out


def counts_of(records, min_columns=80, min_permille=800):
    return [int(r[0] > 0 and r[6] >= min_columns and 1000 * r[5] >= min_permille * r[6]) for r in records]


def groups(pairs, records, owner, n_families, **link):
    """(counts, group): group[f] is the smallest family of f's component under the links of counting records."""
    lk = dict(LINK)
    lk.update(link)
    counts = counts_of(records, **lk)
    adj = {f: set() for f in range(n_families)}
    for (a, b, _), c in zip(pairs, counts):
        if c and owner[a] != owner[b]:
            adj[owner[a]].add(owner[b])
            adj[owner[b]].add(owner[a])
    group = [-1] * n_families
    for f in range(n_families):
        if group[f] >= 0:
            continue
        todo = [f]
        group[f] = f
        while todo:
            x = todo.pop()
            for y in adj[x]:
                if group[y] < 0:
                    group[y] = f
                    todo.append(y)
    return counts, group


def compare(seqs, owner, n_families, K=16, within=False, params=None, link=None):
    pairs = candidates(seqs, owner, K, within)
    recs = [record(seqs[a], seqs[b], inv, **(params or {})) for a, b, inv in pairs]
    counts, group = groups(pairs, recs, owner, n_families, **(link or {}))
    return recs, pairs, counts, group


# ---- the planted families: fragments of one element that extend into each other ----

def _plant(rng, elem, copies, spacer, div):
    """A genome of diverged forward copies of elem between random spacers -> (sequence, the first base of every copy)."""
    parts, at, where = [], 0, []
    for _ in range(copies):
        copy = elem.copy()
        hit = rng.random(len(elem)) < div
        copy[hit] = (copy[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
        parts += [rng.integers(0, 4, spacer).astype(np.int8), copy]
        where.append(at + spacer)
        at += spacer + len(elem)
    parts.append(rng.integers(0, 4, spacer).astype(np.int8))
    return np.concatenate(parts).astype(np.int8), where


def _cores(seq, where, elem_len, lo, hi, spacer, minus):
    from repeatafterme_amd.datamodel import CoreSet
    a = [w + lo for w in where]
    b = [w + hi for w in where]
    n = len(where)
    return CoreSet(left_pos=b if minus else a, right_pos=a if minus else b, lower=[max(w - spacer + 1, 0) for w in where],
                   upper=[min(w + elem_len + spacer - 2, len(seq) - 1) for w in where],
                   orient=np.full(n, 1 if minus else 0, np.int8), left_ext=np.ones(n, np.int8), right_ext=np.ones(n, np.int8))


PLANT_NAMES = ("A", "B", "D", "C")
_planted = {}


def planted_families(seed=5):
    """One 1,200-base element planted 12 times at substitution rate 0.20 between 600-base spacers, and three families cut from
    it: A = offsets 300..420 of copies 0..5, B = offsets 700..820 of copies 6..11, D = B's cores given on the other strand; C is
    an unrelated 900-base element planted 6 times in a genome of its own (its cores: offsets 390..510).  Every family is extended
    by the CPU oracle in both directions (25p43g, W = 14, L = 1,500), once per process.  -> dict: families (name, sequence,
    cores before, (leftbp, rightbp), master), seqs (left and right extension of every family, index 2 f and 2 f + 1), owner."""
    if seed not in _planted:
        from oracle import pyoracle as po
        from repeatafterme_amd.datamodel import new_master
        rng = np.random.default_rng(seed)
        elem = rng.integers(0, 4, 1200).astype(np.int8)
        other = rng.integers(0, 4, 900).astype(np.int8)
        g1, w1 = _plant(rng, elem, 12, 600, 0.20)
        g2, w2 = _plant(rng, other, 6, 600, 0.20)
        plan = [("A", g1, _cores(g1, w1[:6], 1200, 300, 420, 600, False)), ("B", g1, _cores(g1, w1[6:], 1200, 700, 820, 600, False)),
                ("D", g1, _cores(g1, w1[6:], 1200, 700, 820, 600, True)), ("C", g2, _cores(g2, w2, 900, 390, 510, 600, False))]
        p = po.Params.named("25p43g", bandwidth=14, L=1500)
        fams, seqs, owner = [], [], []
        for f, (name, seq, cores) in enumerate(plan):
            c, m = cores.copy(), new_master(p.L)
            rets = {d: po.oracle_extend(d, c, seq, m, p).ret for d in (1, 0)}
            fams.append(dict(name=name, seq=seq, cores=cores, bp=(rets[0], rets[1]), master=m))
            seqs += [np.array(m[p.L - rets[0]:p.L], np.int8), np.array(m[p.L + p.l:p.L + p.l + rets[1]], np.int8)]
            owner += [f, f]
        _planted[seed] = dict(families=fams, seqs=seqs, owner=owner, p=p)
    return _planted[seed]
