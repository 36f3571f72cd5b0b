"""Brute-force restatement of the target-site duplication contract (include/ramx.h, ramx_tsd): every candidate (dl, dr, k) of
a site enumerated, its mismatches counted base by base, the best one chosen by the contract's order.  Plain Python on a
one-byte-per-base library; nothing here is shared with the code under test."""
from fractions import Fraction
from math import comb

DEFAULT = dict(slack=3, kmin=4, kmax=20, mm_div=10)


def cls(lib, site, p):
    """Class of library position p for a site (lo, hi, seq_lo, seq_hi): 0..3, or 4."""
    lo, hi, seq_lo, seq_hi = site
    if p < seq_lo or p > seq_hi or p < 0 or p >= len(lib):
        return 4
    c = int(lib[p])
    if 0 <= c <= 3:
        return c
    if 4 <= c <= 7:
        return c - 4
    return 4


def allowed(k, mm_div):
    return k // mm_div if mm_div else 0


def candidates(lib, site, slack=3, kmin=4, kmax=20, mm_div=10):
    """Every admissible candidate as (q, -(|dl| + |dr|), k, -dl, -dr, mm): the largest tuple is the best one."""
    lo, hi = site[0], site[1]
    out = []
    # (the class of every position the words can touch, looked up once)
    c = {p: cls(lib, site, p) for p in list(range(lo - slack - kmax, lo + slack)) + list(range(hi + 1 - slack, hi + 1 + slack + kmax))}
    for dl in range(-slack, slack + 1):
        for dr in range(-slack, slack + 1):
            if lo + dl > hi + 1 + dr:
                continue
            for k in range(kmin, kmax + 1):
                agree = []
                for j in range(k):
                    a, b = c[lo + dl - k + j], c[hi + 1 + dr + j]
                    agree.append(a < 4 and b < 4 and a == b)
                mm = k - sum(agree)
                if not (agree[0] and agree[-1]) or mm > allowed(k, mm_div):
                    continue
                out.append((2 * (k - 2 * mm) - abs(dl) - abs(dr), -(abs(dl) + abs(dr)), k, -dl, -dr, mm))
    return out


def tsd(lib, site, **params):
    """The record (k, mm, dl, dr) of one site; (0, 0, 0, 0) when no candidate is admissible."""
    c = candidates(lib, site, **{**DEFAULT, **params})
    if not c:
        return (0, 0, 0, 0)
    q, _, k, ndl, ndr, mm = max(c)
    return (k, mm, -ndl, -ndr)


def tsd_all(lib, sites, **params):
    return [tsd(lib, tuple(int(x) for x in s), **params) for s in sites]


def sites_of(cores):
    """(lo, hi, seq_lo, seq_hi) per core from the extents both directions left there."""
    out = []
    for i in range(cores.n):
        if cores.orient[i]:
            lo, hi = cores.right_pos[i] - cores.right_len[i], cores.left_pos[i] + cores.left_len[i]
        else:
            lo, hi = cores.left_pos[i] - cores.left_len[i], cores.right_pos[i] + cores.right_len[i]
        out.append((int(lo), int(hi), int(cores.lower[i]), int(cores.upper[i])))
    return out


def summary(records, slack=3, kmin=4, kmax=20, mm_div=10):
    """(hist [33], mode, mode_count, null [33] as Fractions)."""
    n = len(records)
    hist = [0] * 33
    for r in records:
        hist[r[0]] += 1
    mode, count = 0, 0
    for k in range(1, 33):
        if hist[k] > 0 and hist[k] >= count:
            mode, count = k, hist[k]
    null = [Fraction(0)] * 33
    for k in range(1, 33):
        pr = Fraction((2 * slack + 1) ** 2 * sum(comb(k, j) * 3 ** j for j in range(allowed(k, mm_div) + 1)), 4 ** k)
        null[k] = n * min(Fraction(1), pr)
    return hist, mode, count, null


def planted_family(M=48, k=5, seed=11, elem_len=420, core_half=60, spacer=700, div=0.04):
    """A synthetic genome with M copies of one element at random strands, every insertion followed by a duplicate of the k
    bases in front of it; cores cut from the middle of the copies.  -> (sequence int8, CoreSet, the insertions' (lo, hi))."""
    import numpy as np
    from repeatafterme_amd.datamodel import CoreSet
    rng = np.random.default_rng(seed)
    elem = rng.integers(0, 4, elem_len).astype(np.int8)
    spacers = [rng.integers(0, 4, spacer).astype(np.int8) for _ in range(M + 1)]
    parts, at, where, strands = [], 0, [], []
    for i in range(M):
        copy = elem.copy()
        hit = rng.random(elem_len) < div
        copy[hit] = (copy[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
        minus = bool(rng.random() < 0.4)
        if minus:
            copy = (3 - copy[::-1]).astype(np.int8)
        sp, nxt = spacers[i], spacers[i + 1]
        dup = sp[-k:].copy()
        # the duplication is exactly k long: the base in front of the left word is not the copy's last base, and the base behind
        # the right word is not its first (either would make a word of k + 1 at a shift of one)
        if sp[-k - 1] == copy[-1]:
            sp[-k - 1] = (sp[-k - 1] + 1) % 4
        if nxt[0] == copy[0]:
            nxt[0] = (nxt[0] + 1) % 4
        parts += [sp, copy, dup]
        where.append((at + spacer, at + spacer + elem_len - 1))
        strands.append(minus)
        at += spacer + elem_len + k
    parts.append(spacers[M])
    seq = np.concatenate(parts).astype(np.int8)
    mid = elem_len // 2
    left, right, lower, upper = [], [], [], []
    for (lo, hi), minus in zip(where, strands):
        a, b = lo + mid - core_half, lo + mid + core_half
        # a reverse-strand core's left edge is its upper end in the library
        left.append(b if minus else a)
        right.append(a if minus else b)
        lower.append(max(lo - spacer + 1, 0))
        upper.append(min(hi + spacer - 1, len(seq) - 1))
    ones = np.ones(M, np.int8)
    cores = CoreSet(left_pos=left, right_pos=right, lower=lower, upper=upper, orient=np.array(strands, np.int8), left_ext=ones,
                    right_ext=ones)
    return seq, cores, where


PLANTED = dict(M=48, k=5, seed=11, div=0.08)
_planted = {}


def planted_expectation():
    """The planted family run on the CPU oracle in both directions, once per process: dict with the sequence, the cores before
    and after, the oracle's parameters, the sites of the written-back cores and their records by the restatement."""
    if not _planted:
        from oracle import pyoracle as po
        from repeatafterme_amd.datamodel import new_master
        seq, cores, where = planted_family(**PLANTED)
        p = po.Params.named("20p43g", bandwidth=14, L=300)
        c, m = cores.copy(), new_master(p.L)
        rets = {d: po.oracle_extend(d, c, seq, m, p).ret for d in (1, 0)}
        sites = sites_of(c)
        _planted.update(seq=seq, cores=cores, after=c, master=m, p=p, rets=rets, where=where, sites=sites, records=tsd_all(seq, sites))
    return _planted
