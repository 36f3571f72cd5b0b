"""Time of the terminal repeats (C-ABI ramx_dev_term: HIP events round the pack of the sites' windows, the squeeze into streams
and the alignment) at two shapes, both at tmax 512: 100 sites and 65,536 sites of 1,200 bases.

    python tools/term_timing.py [--out profiles/term.log]

The sites lie at random places of one random library of 128 Mi bases, apart from each other; every fourth site carries its first
200 bases again at its end, every fourth their reverse complement.  The first call of a shape warms up and is not counted; the second one is the measurement -- a single one.
Cells = sites x 2 orientations x T x T.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                       # noqa: E402

from repeatafterme_amd.datamodel import TSD_SITE_DTYPE, TermParams       # noqa: E402
from repeatafterme_amd.device import Device                              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "term.log"))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    lib = rng.integers(0, 4, 1 << 27, dtype=np.int8)
    tp = TermParams()
    length, rep = 1200, 200
    T = min(tp.tmax, length // 2)
    dev = Device(0)
    lines = [f"term: library of {len(lib)} random bases, tmax {tp.tmax}, match {tp.match}, mismatch {tp.mismatch}, gap {tp.gap}, "
             f"min_score {tp.min_score}; one measured call after one warm-up call (a single measurement)"]
    shown = 0
    for n in (100, 65536):
        sites = np.zeros(n, TSD_SITE_DTYPE)
        # (apart, so that a planted repeat is not overwritten by the next site's)
        sites["lo"] = np.sort(rng.choice((len(lib) - length) // length, n, replace=False)) * length
        sites["hi"] = sites["lo"] + length - 1
        sites["seq_lo"], sites["seq_hi"] = 0, len(lib) - 1
        for k, lo in enumerate(sites["lo"]):
            if k % 4 == 0:
                lib[lo + length - rep:lo + length] = lib[lo:lo + rep]
            elif k % 4 == 1:
                lib[lo + length - rep:lo + length] = 3 - lib[lo:lo + rep][::-1]
        dev.load_library(lib)
        cells = n * 2 * T * T
        for i in range(2):
            t1 = time.perf_counter()
            rec, ms = dev.term(sites, tp, timing=True)
            t2 = time.perf_counter()
        lines.append(f"term: {n} sites of {length} bases, T = {T}: {cells:.3e} cells; {int((rec['score'][:, 0] > 0).sum())} direct and "
                     f"{int((rec['score'][:, 1] > 0).sum())} inverted records with a score")
        for what, v in (("pack of the windows", ms[0]), ("squeeze into streams", ms[1]), ("alignment", ms[2]), ("whole call", 1e3 * (t2 - t1))):
            lines.append(f"term:   {what:<24} {v:10.3f} ms")
        lines.append(f"term:   alignment: {cells / (ms[2] * 1e-3):.3e} cells per second")
        print("\n".join(lines[shown:]), flush=True)
        shown = len(lines)
    dev.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
