"""Time of the bit planes and of the Gram matrix of the linkage (C-ABI ramx_dev_planes: HIP events round the forward kernels, the
walk kernels, the pileup kernels + sum and the planes kernel; ramx_dev_plane_gram: wall clock of the whole call, its one kernel
launch with the upload of the lists and the download of the matrix, and the HIP-event time of the kernel alone) next to the pileup of the same flanks and consensus
(ramx_dev_pileup), in one session, the calls alternating.

    python tools/linkage_timing.py [--n 100000] [--rows 128] [--W 40] [--repeats 7]

The default shape is that of tests/test_gpu_fullsize.py: N = 100,000 flanks x 128 columns, W = 40, 14p43g, along the loop's own
consensus (tools/align_timing.py, big); --rows 256 is the smallest shape that has 2,048 planes.  The Gram is timed at the planes ramx_select_planes picks from the call's pileup
(count >= 4, 100 per mille) and at the first 2,048 of the replay's 8 * rows planes.  The first round warms up and is not counted.
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


def measure(name, W, dev, flanks, p, cons, kw, loop_ms, rows_total, repeats):
    os.environ.pop("RAMX_ALIGN_BYTES", None)
    rows = kw["rows"]
    full = np.zeros(min(8 * rows, 2048), PLANE_DTYPE)
    full["row"], full["cls"] = np.arange(len(full)) // 8, np.arange(len(full)) % 8
    pl = dict(forward=[], walk=[], stage=[], wall=[])
    lk = dict(forward=[], walk=[], stage=[], planes=[], wall=[], gram_sel=[], gram_full=[], k_sel=[], k_full=[])
    for i in range(repeats + 1):                                          # the first round warms up
        t0 = time.perf_counter()
        r = dev.pileup(flanks, p, cons, **kw)
        t1 = time.perf_counter()
        s = dev.planes(flanks, p, cons, **kw)
        t2 = time.perf_counter()
        sel = select_planes(np.asarray(cons).ravel()[:rows], s.cols[0, :rows])
        t3 = time.perf_counter()
        co_sel = dev.plane_gram(sel)
        t4 = time.perf_counter()
        k_sel = dev.plane_gram_ms()
        t4b = time.perf_counter()
        co_full = dev.plane_gram(full)
        t5 = time.perf_counter()
        k_full = dev.plane_gram_ms()
        if i:
            pl["forward"].append(r.forward_ms); pl["walk"].append(r.walk_ms); pl["stage"].append(r.pileup_ms); pl["wall"].append(1e3 * (t1 - t0))
            for k, v in zip(("forward", "walk", "stage", "planes"), s.kernel_ms):
                lk[k].append(v)
            lk["wall"].append(1e3 * (t2 - t1)); lk["gram_sel"].append(1e3 * (t4 - t3)); lk["gram_full"].append(1e3 * (t5 - t4b))
            lk["k_sel"].append(k_sel); lk["k_full"].append(k_full)
    assert np.array_equal(r.cols, s.cols) and np.array_equal(np.diag(co_full)[6::8], s.cols["cover"][0, :len(full) // 8])
    print(f"{name}: {flanks[1]} flanks, {rows} columns, {(flanks[1] + 63) // 64} tiles; {len(sel)} selected planes "
          f"({int((sel['cls'] != 6).sum())} variants), {len(full)} planes in the full list; {repeats} repeats, the calls alternating", flush=True)
    for tag, d, third in (("ramx_dev_pileup", pl, "pileup kernels + sum"), ("ramx_dev_planes", lk, "pileup kernels + sum")):
        print(_line(name, f"{tag} forward", d["forward"]))
        print(_line(name, f"{tag} walk", d["walk"]))
        print(_line(name, f"{tag} {third}", d["stage"]))
        if "planes" in d:
            print(_line(name, f"{tag} planes kernel", d["planes"]))
        print(_line(name, f"{tag} whole call", d["wall"]), flush=True)
    print(_line(name, f"ramx_dev_plane_gram {len(sel)} planes (call)", lk["gram_sel"]))
    print(_line(name, f"ramx_dev_plane_gram {len(full)} planes (call)", lk["gram_full"]))
    print(_line(name, f"ramx_plane_gram_kernel {len(sel)} planes", lk["k_sel"]))
    print(_line(name, f"ramx_plane_gram_kernel {len(full)} planes", lk["k_full"]), flush=True)
    print(f"{name}: planes stage = {_median(lk['planes']) / _median(pl['stage']):5.2f} x the pileup stage, "
          f"{_median(lk['planes']) / _median(lk['forward']):6.3f} x its forward pass; sum of the full Gram's diagonal {int(np.trace(co_full))}, "
          f"of the selected {int(np.trace(co_sel)) if len(sel) else 0}", flush=True)


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
