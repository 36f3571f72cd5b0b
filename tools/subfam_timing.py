"""Time of one assign + count iteration of the split into subfamilies (C-ABI ramx_dev_subfamilies with max_iter = 1: the HIP-event
times of ramx_subfam_assign_kernel and ramx_subfam_count_kernel, and the wall clock of the whole call with its uploads and
downloads) next to the Gram matrix of the same planes (ramx_dev_plane_gram), on one resident replay, the calls alternating.

    python tools/subfam_timing.py [--n 100000] [--rows 128] [--W 40] [--repeats 7]

The default shape is that of tools/linkage_timing.py: N = 100,000 flanks x 128 columns, W = 40, 14p43g, along the loop's own
consensus.  Both are timed at the first 2,048 of the replay's 8 * rows planes (1,024 at 128 columns: 896 variants and their 128
cover planes), the split with K = 8 and K = 4 patterns drawn at random (one bit in three) -- what the kernels cost does not
depend on what the bits are -- and at the planes ramx_select_planes picks.  The first round warms up and is not counted.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_timing as at                                                 # noqa: E402
from copystats_timing import _line, _median                               # noqa: E402

from repeatafterme_amd.datamodel import PLANE_DTYPE                       # noqa: E402
from repeatafterme_amd.device import select_planes                        # noqa: E402


def _init(planes, K, seed):
    V = int((planes["cls"] != 6).sum())
    init = (np.random.default_rng(seed).integers(0, 3, (V, K)) == 0).astype(np.uint8)
    init[:, 0] = 0
    return init


def measure(name, W, dev, flanks, p, cons, kw, loop_ms, rows_total, repeats):
    os.environ.pop("RAMX_ALIGN_BYTES", None)
    rows = kw["rows"]
    full = np.zeros(min(8 * rows, 2048), PLANE_DTYPE)
    full["row"], full["cls"] = np.arange(len(full)) // 8, np.arange(len(full)) % 8
    s = dev.planes(flanks, p, cons, **kw)
    sel = select_planes(np.asarray(cons).ravel()[:rows], s.cols[0, :rows])
    cases = [("full", full, 8), ("full", full, 4)] + ([("selected", sel, 4)] if len(sel) else [])
    t = {("gram", "call"): [], ("gram", "kernel"): []}
    for tag, pl, K in cases:
        for what in ("call", "assign", "count"):
            t[(tag, K, what)] = []
    sizes = {}
    for i in range(repeats + 1):                                          # the first round warms up
        t0 = time.perf_counter()
        co = dev.plane_gram(full)
        t1 = time.perf_counter()
        if i:
            t[("gram", "call")].append(1e3 * (t1 - t0)); t[("gram", "kernel")].append(dev.plane_gram_ms())
        for tag, pl, K in cases:
            t0 = time.perf_counter()
            r = dev.subfamilies(pl, _init(pl, K, 1), max_iter=1)
            t1 = time.perf_counter()
            a, c = dev.subfam_ms()
            sizes[(tag, K)] = r.size
            if i:
                t[(tag, K, "call")].append(1e3 * (t1 - t0)); t[(tag, K, "assign")].append(a); t[(tag, K, "count")].append(c)
    print(f"{name}: {flanks[1]} flanks, {rows} columns, {(flanks[1] + 63) // 64} tiles; {len(full)} planes in the full list "
          f"({int((full['cls'] != 6).sum())} variants), {len(sel)} selected; {repeats} repeats, the calls alternating", flush=True)
    print(_line(name, f"ramx_dev_plane_gram {len(full)} planes (call)", t[("gram", "call")]))
    print(_line(name, f"ramx_plane_gram_kernel {len(full)} planes", t[("gram", "kernel")]))
    for tag, pl, K in cases:
        what = f"{len(pl)} planes K={K}"
        print(_line(name, f"ramx_dev_subfamilies {what} max_iter=1 (call)", t[(tag, K, "call")]))
        print(_line(name, f"ramx_subfam_assign_kernel {what}", t[(tag, K, "assign")]))
        print(_line(name, f"ramx_subfam_count_kernel {what}", t[(tag, K, "count")]), flush=True)
        assert int(sizes[(tag, K)].sum()) == flanks[1] and np.trace(co) > 0
    both = _median(t[("full", 8, "assign")]) + _median(t[("full", 8, "count")])
    print(f"{name}: one assign + count iteration at {len(full)} planes, K = 8: {both:.3f} ms = "
          f"{both / _median(t[('gram', 'kernel')]):.2f} x the Gram kernel of the same planes", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--W", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    at.big(a.repeats, False, n=a.n, L=a.rows, W=a.W, measure=measure)


if __name__ == "__main__":
    main()
