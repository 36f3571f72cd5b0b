"""Shared test helpers: parameter conversion, golden vectors, result comparison."""
import os

import numpy as np

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import CoreSet, ExtendParams, FlankSet, new_master

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def to_extend_params(p: po.Params) -> ExtendParams:
    return ExtendParams(bandwidth=p.bandwidth, cappenalty=p.cappenalty, minimprovement=p.minimprovement, L=p.L,
                        when_to_stop=p.when_to_stop, l=p.l, gapopen=p.gapopen, gapextn=p.gapextn, matrix=p.matrix)


def load_api_vectors():
    z = np.load(os.path.join(GOLDEN, "api_vectors.npz"))
    out = []
    for k in range(int(z["n_cases"])):
        pre = f"c{k}_"
        cores = CoreSet(**{f: z[pre + f] for f in ("left_pos", "right_pos", "lower", "upper", "orient", "left_ext",
                                                    "right_ext", "seq_idx")})
        W, cap, mini, L, wts, go, ge = [int(v) for v in z[pre + "params"]]
        p = po.Params(bandwidth=W, cappenalty=cap, minimprovement=mini, L=L, when_to_stop=wts, l=1, gapopen=go,
                      gapextn=ge, matrix=z[pre + "matrix"])
        exp = dict(ret=z[pre + "ret"], master=z[pre + "master"], left_len=z[pre + "left_len"],
                   right_len=z[pre + "right_len"], score=z[pre + "score"])
        out.append((k, str(z[pre + "matrix_name"]), z[pre + "sequence"], cores, p, exp))
    return out


def run_both_directions(extend_fn, cores, sequence, p):
    """extend_fn(direction, cores, sequence, master, p) -> object with .ret; right then left like main()."""
    c = cores.copy()
    m = new_master(p.L, p.l)
    rr = extend_fn(1, c, sequence, m, p)
    rl = extend_fn(0, c, sequence, m, p)
    return c, m, rr, rl


def assert_same_result(c1, m1, r1, c2, m2, r2, tag=""):
    assert [r.ret for r in r1] == [r.ret for r in r2], f"{tag}: return values differ"
    assert np.array_equal(m1, m2), f"{tag}: consensus (master) differs at {np.nonzero(m1 != m2)[0][:8]}"
    assert np.array_equal(c1.right_len, c2.right_len), f"{tag}: rightExtensionLen differs"
    assert np.array_equal(c1.left_len, c2.left_len), f"{tag}: leftExtensionLen differs"
    assert np.array_equal(c1.score, c2.score), f"{tag}: score differs"


def gpu_extend(direction, cores, sequence, master, p):
    from repeatafterme_amd.extend import extend_alignment
    return extend_alignment(direction, cores, np.ascontiguousarray(sequence, np.int8), master, to_extend_params(p))


def oracle_extend(direction, cores, sequence, master, p):
    return po.oracle_extend(direction, cores, sequence, master, p)


def ragged_family(n, L, W, K, seed, clip=True):
    """synth_family gives every copy the same length K; clipping every window to 40..L bases beyond its core (drawn per copy
    from `seed`) makes the copies end at different columns of a long extension.  -> (FlankSet, its cores or the clipped ones)"""
    from repeatafterme_amd.synth import synth_family
    fs = synth_family(n, L, W, K=K, seed=seed, both_sides=True, minus_frac=0.4, n_run_frac=0.1)
    cores = fs.cores.copy()
    if clip:
        q = np.random.default_rng(seed).integers(40, L + 1, cores.n)
        cores.upper = np.minimum(cores.upper, cores.right_pos + q)
        cores.lower = np.maximum(cores.lower, cores.left_pos - q)
    return fs, cores


def make_genome(seed: int):
    """A few contigs, each with several diverged copies of one family (cores 3-25 bp), both strands,
    some copies close together / at contig ends, N runs, mixed extendable flags."""
    rng = np.random.default_rng(1000 + seed)
    K = 160
    anc_l = rng.integers(0, 4, K)
    anc_r = rng.integers(0, 4, K)
    core = rng.integers(0, 4, int(rng.integers(3, 26)))

    def mutate(a, div=0.12):
        out = []
        for b in a:
            u = rng.random()
            if u < 0.8 * div:
                out.append((b + rng.integers(1, 4)) & 3)
            elif u < 0.9 * div:
                continue
            elif u < div:
                out.extend([int(rng.integers(0, 4)), b])
            else:
                out.append(b)
        return np.array(out, np.int64)

    records, rows = [], []
    for s in range(int(rng.integers(2, 5))):
        name = f"ctg{s}" if s else "chrUn_long_contig_name_0"
        pieces = [rng.integers(0, 4, int(rng.integers(0, 300)))]
        pos = len(pieces[0])
        for c in range(int(rng.integers(2, 7))):
            fl = int(rng.integers(0, K)) if rng.random() < 0.85 else 0
            fr = int(rng.integers(0, K)) if rng.random() < 0.85 else 0
            left = mutate(anc_l)[::-1][:fl][::-1] if fl else np.zeros(0, np.int64)
            right = mutate(anc_r)[:fr]
            copy = np.concatenate((left, core, right))
            cs = len(left)
            minus = rng.random() < 0.4
            if minus:
                copy = (3 - copy)[::-1]
                cs = len(right)
            if rng.random() < 0.25 and len(copy) > 12:
                a = int(rng.integers(0, len(copy) - 3))
                copy = copy.copy()
                copy[a:a + int(rng.integers(1, 9))] = 99
                copy[cs:cs + len(core)] = (3 - core)[::-1] if minus else core   # keep the core itself clean
            pieces.append(copy)
            rows.append((name, pos + cs, pos + cs + len(core), int(rng.random() < 0.8), int(rng.random() < 0.8),
                         "-" if minus else "+"))
            pos += len(copy)
            gap = rng.integers(0, 4, int(rng.integers(0, 400)) if rng.random() < 0.7 else int(rng.integers(0, 12)))
            pieces.append(gap)
            pos += len(gap)
        records.append((name, np.concatenate(pieces)))
    order = rng.permutation(len(rows))          # the loader must re-sort
    rows = [rows[i] for i in order]
    return records, rows


