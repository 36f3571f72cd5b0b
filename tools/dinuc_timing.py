"""Time of the dinucleotide pileup and of the CpG-aware refinement (C-ABI ramx_dev_dinuc / ramx_dev_refine_cpg: HIP events round
the forward kernels, the walk kernels, the pileup kernels with their sum, and the dinucleotide kernels with theirs) next to the
calls they extend: ramx_dev_pileup and ramx_dev_refine on the same shapes.

    python tools/dinuc_timing.py [batch40] [batch80] [big] [--repeats 3] [--max-replays 3]

The shapes and the consensus are those of tools/pileup_timing.py (500 families of 60-150 flanks, W = 40 / 80, 1,000 rows each;
N = 100,000, W = 40, 2,000 rows).  The expectation the numbers are held against: the dinucleotide kernel reads the two column
arrays and the windows the pileup kernel reads, so it should cost about what the pileup kernel costs.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_timing as at                                                 # noqa: E402


def _median(v):
    return sorted(v)[len(v) // 2]


def make_measure(max_replays):
    def measure(name, W, dev, flanks, p, cons, kw, loop_ms, rows_total, repeats):
        os.environ.pop("RAMX_ALIGN_BYTES", None)
        pms, pwall = [], []
        for i in range(repeats + 1):                                      # the first call warms up
            t0 = time.perf_counter()
            r = dev.pileup(flanks, p, cons, **kw)
            if i:
                pms.append(r.pileup_ms)
                pwall.append(1e3 * (time.perf_counter() - t0))
        print(f"{name}: ramx_dev_pileup, {repeats} repeats: pileup + sum median {_median(pms):9.2f} ms; whole call median {_median(pwall):9.2f} ms  "
              f"min {min(pwall):9.2f}  max {max(pwall):9.2f} ms", flush=True)
        for with_pileup in (True, False):
            ms, wall = [], []
            for i in range(repeats + 1):
                t0 = time.perf_counter()
                r = dev.dinuc(flanks, p, cons, pileup=with_pileup, **kw)
                if i:
                    ms.append(r.kernel_ms)
                    wall.append(1e3 * (time.perf_counter() - t0))
            med = [_median([m[k] for m in ms]) for k in range(4)]
            print(f"{name}: ramx_dev_dinuc {'with' if with_pileup else 'without'} cols, {repeats} repeats: forward median {med[0]:9.2f} ms, walk "
                  f"{med[1]:9.2f} ms, pileup + sum {med[2]:9.2f} ms, dinuc + sum {med[3]:9.2f} ms = {med[3] / _median(pms):6.3f} x the pileup stage of "
                  f"ramx_dev_pileup, {med[3] / med[0]:6.3f} x the forward pass", flush=True)
            print(f"{name}: whole ramx_dev_dinuc call {'with' if with_pileup else 'without'} cols: median {_median(wall):9.2f} ms  min {min(wall):9.2f}  "
                  f"max {max(wall):9.2f} ms = {_median(wall) / _median(pwall):5.2f} x the whole ramx_dev_pileup call", flush=True)
        rwall = []
        for i in range(repeats + 1):
            t0 = time.perf_counter()
            rr = dev.refine(flanks, p, cons, max_replays=max_replays, **kw)
            if i:
                rwall.append(1e3 * (time.perf_counter() - t0))
        print(f"{name}: whole ramx_dev_refine call, at most {max_replays} replays (converged {int(rr.converged.sum())} of {len(rr.replays)}): median "
              f"{_median(rwall):9.2f} ms  min {min(rwall):9.2f}  max {max(rwall):9.2f} ms", flush=True)
        wall = []
        for i in range(repeats + 1):
            t0 = time.perf_counter()
            r = dev.refine_cpg(flanks, p, cons, max_replays=max_replays, **kw)
            if i:
                wall.append(1e3 * (time.perf_counter() - t0))
        reps = r.replays
        hist = {int(k): int((reps == k).sum()) for k in sorted(set(reps.tolist()))}
        print(f"{name}: whole ramx_dev_refine_cpg call, at most {max_replays} replays (replays: families {hist}; converged "
              f"{int(r.converged.sum())} of {len(reps)}; CG pairs {int(r.n_cpg.sum())}): median {_median(wall):9.2f} ms  min {min(wall):9.2f}  "
              f"max {max(wall):9.2f} ms = {_median(wall) / _median(rwall):5.2f} x the whole ramx_dev_refine call; kernels of the last call: forward "
              f"{r.kernel_ms[0]:9.2f} ms, walk {r.kernel_ms[1]:9.2f} ms, pileup + sum {r.kernel_ms[2]:9.2f} ms, dinuc + sum {r.kernel_ms[3]:9.2f} ms", flush=True)
    return measure


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["batch40", "batch80", "big"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-replays", type=int, default=3)
    a = ap.parse_args()
    m = make_measure(a.max_replays)
    for s in a.shapes:
        if s == "big":
            at.big(a.repeats, False, measure=m)
        elif s == "batch40":
            at.batch(s, 40, a.repeats, False, measure=m)
        elif s == "batch80":
            at.batch(s, 80, a.repeats, False, measure=m)
        else:
            sys.exit(f"unknown shape {s}")


if __name__ == "__main__":
    main()
