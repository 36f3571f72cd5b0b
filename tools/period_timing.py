"""Time of the tandem periodicity (C-ABI ramx_dev_period: HIP events round the pack of the segments' windows, the squeeze into
streams and the scan) at three shapes, all at pmax 1024: 100 segments of 500 bases, 100,000 of 500 and 100,000 of 10,000.

    python tools/period_timing.py [--repeats 5] [--out profiles/period.log]

The segments lie at random places of one random library of 16 Mi bases (they overlap at the largest shape: the kernels read
every segment's own window and stream, so that changes nothing they do) with a (CA)20 planted in every sixteenth.  The first call
of a shape warms up and is not counted.  Base comparisons = segments x sum over p of (length - p).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                       # noqa: E402

from repeatafterme_amd.datamodel import PERIOD_SEG_DTYPE, PeriodParams   # noqa: E402
from repeatafterme_amd.device import Device                              # noqa: E402


def _median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "period.log"))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    lib = rng.integers(0, 4, 1 << 24).astype(np.int8)
    pp = PeriodParams(1024, 3, 16)
    dev = Device(0)
    dev.load_library(lib)
    lines = [f"period: library of {len(lib)} random bases, pmax {pp.pmax}, mm {pp.mm}, min_score {pp.min_score}; {a.repeats} repeats after one warm-up call"]
    shown = 0
    for n, length in ((100, 500), (100000, 500), (100000, 10000)):
        segs = np.zeros(n, PERIOD_SEG_DTYPE)
        segs["lo"] = rng.integers(0, len(lib) - length, n)
        segs["hi"] = segs["lo"] + length - 1
        for lo in segs["lo"][::16]:
            lib[lo + 100:lo + 140] = np.tile(np.array([1, 0], np.int8), 20)
        dev.load_library(lib)
        pm = min(pp.pmax, length - 1)
        compares = n * sum(length - p for p in range(1, pm + 1))
        pack, squeeze, scan, wall = [], [], [], []
        for i in range(a.repeats + 1):
            t1 = time.perf_counter()
            rec, ms = dev.period(segs, pp, timing=True)
            t2 = time.perf_counter()
            if i:
                pack.append(ms[0]); squeeze.append(ms[1]); scan.append(ms[2]); wall.append(1e3 * (t2 - t1))
        lines.append(f"period: {n} segments of {length} bases = {compares:.3e} base comparisons; {int((rec['period'] > 0).sum())} records with a tract, "
                     f"{int((rec['period'] == 2).sum())} of period 2")
        for what, v in (("pack of the windows", pack), ("squeeze into streams", squeeze), ("scan", scan), ("whole call", wall)):
            lines.append(f"period:   {what:<24} median {_median(v):10.3f} ms  min {min(v):10.3f}  max {max(v):10.3f} ms")
        lines.append(f"period:   scan: {compares / (_median(scan) * 1e-3):.3e} base comparisons per second")
        print("\n".join(lines[shown:]), flush=True)
        shown = len(lines)
    dev.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
