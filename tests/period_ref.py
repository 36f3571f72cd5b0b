"""Brute-force restatement of the tandem-periodicity contract (include/ramx.h, ramx_period): for every period the pairs compared
base by base, the blocks of eight summed, EVERY tract (b0, b1) of a period scored from prefix sums and the best one chosen by the
contract's order of ties -- not the one-pass scan the code under test runs.  Plain Python / numpy on a one-byte-per-base library;
nothing here is shared with the code under test.  Results are cached per input."""
import numpy as np

DEFAULT = dict(pmax=1024, mm=3, min_score=16)
ZERO = (0, 0, 0, 0, 0, 0)
_cache = {}


def classes(codes):
    """Class of every code: 0..3, or 4."""
    c = np.asarray(codes).astype(np.int64)
    return np.where((c >= 0) & (c <= 3), c, np.where((c >= 4) & (c <= 7), c - 4, 4)).astype(np.int8)


def segment_classes(lib, lo, hi):
    """Classes of library positions lo..hi; a position outside the library is class 4."""
    n = hi + 1 - lo
    x = np.full(max(n, 0), 4, np.int8)
    a, b = max(lo, 0), min(hi, len(lib) - 1)
    if a <= b:
        x[a - lo:b + 1 - lo] = classes(lib[a:b + 1])
    return x


def blocks(x, p, mm):
    """(a_b, d_b, s_b) of period p as arrays over the blocks."""
    n = len(x)
    u, v = x[:n - p], x[p:]
    ok = (u < 4) & (v < 4)
    agree, dis = ok & (u == v), ok & (u != v)
    nb = (n - p + 7) // 8
    pad = nb * 8 - (n - p)
    a = np.concatenate((agree, np.zeros(pad, bool))).reshape(nb, 8).sum(1)
    d = np.concatenate((dis, np.zeros(pad, bool))).reshape(nb, 8).sum(1)
    return a, d, a - mm * d


def best_tract(s):
    """(S, b0, b1) of the best tract of one period from all tracts: the largest S, ties to the smallest b1, then the largest b0."""
    nb = len(s)
    P = np.concatenate(([0], np.cumsum(s)))
    M = P[None, 1:] - P[:nb, None]                      # M[b0, b1] = s[b0] + .. + s[b1]
    M = np.where(np.arange(nb)[:, None] <= np.arange(nb)[None, :], M, np.iinfo(np.int64).min)
    S = int(M.max())
    b1 = int(np.nonzero((M == S).any(0))[0][0])
    b0 = int(np.nonzero(M[:, b1] == S)[0][-1])
    return S, b0, b1


def record(x, pmax=1024, mm=3, min_score=16):
    """The record (period, score, start, end, agree, disagree) of a segment given as classes."""
    x = np.asarray(x, np.int8)
    key = (x.tobytes(), pmax, mm, min_score)
    if key in _cache:
        return _cache[key]
    n = len(x)
    best = None
    for p in range(1, min(pmax, n - 1) + 1):
        a, d, s = blocks(x, p, mm)
        S, b0, b1 = best_tract(s)
        if best is None or S > best[0]:                  # ties to the smallest p
            best = (S, p, b0, b1, int(a[b0:b1 + 1].sum()), int(d[b0:b1 + 1].sum()))
    if best is None or best[0] < min_score:
        out = ZERO
    else:
        S, p, b0, b1, ag, dg = best
        out = (p, S, 8 * b0, min(8 * b1 + 7, n - p - 1), ag, dg)
    _cache[key] = out
    return out


def record_of_codes(codes, **params):
    return record(classes(codes), **{**DEFAULT, **params})


def records(lib, segs, **params):
    return [record(segment_classes(lib, int(lo), int(hi)), **{**DEFAULT, **params}) for lo, hi in segs]


def segments_of(cores, which):
    """(lo, hi) per core: which = 0 the left extension, 1 the right one, 2 the whole element."""
    out = []
    for i in range(cores.n):
        lp, rp, ll, rl = int(cores.left_pos[i]), int(cores.right_pos[i]), int(cores.left_len[i]), int(cores.right_len[i])
        if cores.orient[i]:
            out.append([(lp + 1, lp + ll), (rp - rl, rp - 1), (rp - rl, lp + ll)][which])
        else:
            out.append([(lp - ll, lp - 1), (rp + 1, rp + rl), (lp - ll, rp + rl)][which])
    return out


def summary(recs, segs):
    """dict of the fields of ramx_period_hist."""
    h = dict(n=len(recs), n_tract=0, n_mono=0, n_simple=0, n_tandem=0, at_lo=0, at_hi=0, mode=0, mode_count=0)
    count = {}
    for r, (lo, hi) in zip(recs, segs):
        p = r[0]
        if p == 0:
            continue
        h["n_tract"] += 1
        h["n_mono" if p == 1 else "n_simple" if p <= 6 else "n_tandem"] += 1
        h["at_lo"] += r[2] == 0
        h["at_hi"] += r[3] == (hi + 1 - lo) - p - 1
        count[p] = count.get(p, 0) + 1
    for p in sorted(count):
        if count[p] > h["mode_count"]:
            h["mode"], h["mode_count"] = p, count[p]
    return h


def planted_family(M=40, seed=17, elem_len=420, core_half=60, spacer=700, div=0.05, units=(14, 46)):
    """A synthetic genome with M copies of one element at random strands, every copy followed (in its own reading direction) by
    a (CA)n of a length drawn per copy and then by random sequence; cores cut from the middle of the copies.  -> (sequence int8,
    CoreSet, the repeat lengths in bases)."""
    from repeatafterme_amd.datamodel import CoreSet
    rng = np.random.default_rng(seed)
    elem = rng.integers(0, 4, elem_len).astype(np.int8)
    parts, at, where, strands, runs = [], 0, [], [], []
    for i in range(M):
        copy = elem.copy()
        hit = rng.random(elem_len) < div
        copy[hit] = (copy[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
        n_units = int(rng.integers(units[0], units[1]))
        unit = np.concatenate((copy, np.tile(np.array([1, 0], np.int8), n_units)))
        minus = bool(rng.random() < 0.4)
        if minus:
            unit = (3 - unit[::-1]).astype(np.int8)
        sp = rng.integers(0, 4, spacer).astype(np.int8)
        parts += [sp, unit]
        lo = at + spacer + (2 * n_units if minus else 0)
        where.append((lo, lo + elem_len - 1))
        strands.append(minus)
        runs.append(2 * n_units)
        at += spacer + len(unit)
    parts.append(rng.integers(0, 4, spacer).astype(np.int8))
    seq = np.concatenate(parts).astype(np.int8)
    mid = elem_len // 2
    left, right, lower, upper = [], [], [], []
    for (lo, hi), minus in zip(where, strands):
        a, b = lo + mid - core_half, lo + mid + core_half
        left.append(b if minus else a)
        right.append(a if minus else b)
        lower.append(max(lo - spacer + 1, 0))
        upper.append(min(hi + spacer - 1, len(seq) - 1))
    ones = np.ones(M, np.int8)
    cores = CoreSet(left_pos=left, right_pos=right, lower=lower, upper=upper, orient=np.array(strands, np.int8), left_ext=ones,
                    right_ext=ones)
    return seq, cores, runs


PLANTED = dict(M=40, seed=17)
_planted = {}


def planted_expectation():
    """The planted family run on the CPU oracle in both directions, once per process: the sequence, the cores before and after,
    the oracle's parameters and kept rows, and per part (0 left, 1 right, 2 whole) the segments and their records by the
    restatement."""
    if not _planted:
        from oracle import pyoracle as po
        from repeatafterme_amd.datamodel import new_master
        seq, cores, runs = planted_family(**PLANTED)
        p = po.Params.named("20p43g", bandwidth=14, L=300)
        c, m = cores.copy(), new_master(p.L)
        rets = {d: po.oracle_extend(d, c, seq, m, p).ret for d in (1, 0)}
        segs = {w: segments_of(c, w) for w in (0, 1, 2)}
        _planted.update(seq=seq, cores=cores, after=c, master=m, p=p, rets=rets, runs=runs, segs=segs,
                        records={w: records(seq, segs[w]) for w in (0, 1, 2)})
    return _planted
