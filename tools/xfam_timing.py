#!/usr/bin/env python3
"""Times ramx_dev_seq_pairs (include/ramx_xfam.h) beside ramx_seq_pair_host on 16 host threads, the only other implementation of
these cells: 1,024 pairs of 2,000 x 2,000, 64 pairs of 10,000 x 10,000, and the candidate pairs of a planted batch (fragments of
one 1,200-base element, as tests/xfam_ref.py plants them, on the consensi themselves).  Prints kernel_ms, the call's wall time
and the cell updates per second; every record of the device is compared with the host's.

usage: tools/xfam_timing.py [> profiles/xfam.log]"""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from repeatafterme_amd import xfam            # noqa: E402
from repeatafterme_amd.datamodel import PairParams  # noqa: E402

THREADS = 16


def host_records(seqs, pairs, params):
    def one(p):
        return xfam.seq_pair_host(seqs[p[0]], seqs[p[1]], p[2], params)[0]      # (the library call runs without the interpreter lock)
    t = time.perf_counter()
    with ThreadPoolExecutor(THREADS) as pool:
        recs = list(pool.map(one, pairs))
    return recs, (time.perf_counter() - t) * 1e3


def case(name, seqs, pairs, params=None):
    params = params or PairParams()
    cells = sum(len(seqs[a]) * len(seqs[b]) for a, b, _ in pairs)
    xfam.seq_pairs(seqs[:2], [(0, 1, 0)], params)                               # the session and its first allocation
    best = None
    for _ in range(3):
        t = time.perf_counter()
        got, ms = xfam.seq_pairs(seqs, pairs, params, timing=True)
        wall = (time.perf_counter() - t) * 1e3
        best = (ms, wall) if best is None or ms < best[0] else best
    want, host_ms = host_records(seqs, pairs, params)
    same = all(tuple(g) == tuple(w) for g, w in zip(got, want))
    ms, wall = best
    print(f"{name}: {len(pairs)} pairs, {cells:.3e} cells")
    print(f"  device  kernel_ms {ms:10.3f}  ({cells / ms / 1e6:9.2f} G cell updates/s)   call {wall:10.3f} ms")
    print(f"  host    {THREADS} threads {host_ms:10.3f} ms  ({cells / host_ms / 1e6:9.2f} G cell updates/s)")
    print(f"  device / host: {host_ms / ms:.1f}x by kernel_ms, {host_ms / wall:.1f}x by the call; records {'equal' if same else 'DIFFER'}")
    return ms, host_ms, same


def main():
    rng = np.random.default_rng(1)
    ok = True
    s1 = [rng.integers(0, 4, 2000).astype(np.int8) for _ in range(2048)]
    ms1, host1, same = case("1. 2,000 x 2,000", s1, [(2 * k, 2 * k + 1, k % 2) for k in range(1024)])
    ok &= same
    s2 = [rng.integers(0, 4, 10000).astype(np.int8) for _ in range(128)]
    ok &= case("2. 10,000 x 10,000", s2, [(2 * k, 2 * k + 1, k % 2) for k in range(64)])[2]
    # 3. fragments of one element: four overlapping stretches of it and of its reverse complement, diverged, and an unrelated one
    elem = rng.integers(0, 4, 1200).astype(np.int8)

    def frag(lo, hi, minus):
        x = elem[lo:hi].copy()
        hit = rng.random(len(x)) < 0.05
        x[hit] = (x[hit] + 1) % 4
        return (3 - x[::-1]).astype(np.int8) if minus else x
    s3 = [frag(0, 300, False), frag(420, 1198, False), frag(2, 700, False), frag(820, 1198, False), frag(820, 1198, True), frag(2, 700, True),
          rng.integers(0, 4, 380).astype(np.int8), rng.integers(0, 4, 380).astype(np.int8)]
    owner = [0, 0, 1, 1, 2, 2, 3, 3]
    cand = xfam.candidates(s3, owner, K=16, within=True)
    pairs = [(int(p["a"]), int(p["b"]), int(p["inverted"])) for p in cand]
    ok &= case("3. the planted batch", s3, pairs)[2]
    print("(1) is faster on the device than on the 16 host threads" if ms1 < host1 else
          "(1) is NOT faster on the device than on the 16 host threads: the kernel is not doing its job")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
