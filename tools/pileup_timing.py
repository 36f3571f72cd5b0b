"""Time of the pileup and of the refinement (C-ABI ramx_dev_pileup / ramx_dev_refine: HIP events round the forward kernels, the
walk kernels, and the pileup kernels with their sum) next to the yardstick: the whole ramx_dev_align call WITH the column
arrays downloaded, which is what a caller had to do before to count a pileup on the host.

    python tools/pileup_timing.py [batch40] [batch80] [big] [--repeats 3] [--no-yardstick]

The shapes and the consensus are those of tools/align_timing.py (500 families of 60-150 flanks, W = 40 / 80, 1,000 rows each;
N = 100,000, W = 40, 2,000 rows).  The refinement starts from the same consensus and is given at most 3 replays; how many it
took is printed.  --no-yardstick leaves the alignment call out (its host arrays take n_padded x rows x 8 bytes).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_timing as at                                                 # noqa: E402


def _median(v):
    return sorted(v)[len(v) // 2]


def make_measure(yardstick, max_replays):
    def measure(name, W, dev, flanks, p, cons, kw, loop_ms, rows_total, repeats):
        os.environ.pop("RAMX_ALIGN_BYTES", None)
        yard = None
        if yardstick:
            wall = []
            for i in range(repeats + 1):                                  # the first call warms up
                t0 = time.perf_counter()
                r = dev.align(flanks, p, cons, columns=True, **kw)
                if i:
                    wall.append(1e3 * (time.perf_counter() - t0))
                fw, wk = r.forward_ms, r.walk_ms
                del r
            yard = _median(wall)
            print(f"{name}: yardstick, whole ramx_dev_align call with col_idx / col_ins downloaded, {repeats} repeats: median {yard:9.2f} ms  "
                  f"min {min(wall):9.2f}  max {max(wall):9.2f} ms (last call: forward {fw:9.2f} ms, walk {wk:9.2f} ms)", flush=True)
        fms, wms, pms, wall = [], [], [], []
        for i in range(repeats + 1):
            t0 = time.perf_counter()
            r = dev.pileup(flanks, p, cons, **kw)
            if i:
                fms.append(r.forward_ms); wms.append(r.walk_ms); pms.append(r.pileup_ms)
                wall.append(1e3 * (time.perf_counter() - t0))
        print(f"{name}: pileup, {repeats} repeats: forward median {_median(fms):9.2f} ms, walk {_median(wms):9.2f} ms, pileup + sum "
              f"{_median(pms):9.2f} ms = {_median(pms) / _median(fms):6.3f} x the forward pass", flush=True)
        print(f"{name}: whole ramx_dev_pileup call (uploads, window pack, kernels, download of rows x 128 bytes): median {_median(wall):9.2f} ms  "
              f"min {min(wall):9.2f}  max {max(wall):9.2f} ms" +
              (f" = {_median(wall) / yard:5.2f} x the yardstick: {'below' if _median(wall) < yard else 'NOT below'}" if yard else "") +
              (f"; {_median(wall) / loop_ms:5.2f} x the loop ({loop_ms:.2f} ms)" if loop_ms else ""), flush=True)
        wall, reps = [], None
        for i in range(repeats + 1):
            t0 = time.perf_counter()
            r = dev.refine(flanks, p, cons, max_replays=max_replays, **kw)
            if i:
                wall.append(1e3 * (time.perf_counter() - t0))
            reps = r.replays
        hist = {int(k): int((reps == k).sum()) for k in sorted(set(reps.tolist()))}
        print(f"{name}: whole ramx_dev_refine call, at most {max_replays} replays (replays: families {hist}; converged "
              f"{int(r.converged.sum())} of {len(reps)}): median {_median(wall):9.2f} ms  min {min(wall):9.2f}  max {max(wall):9.2f} ms; kernels of the last call: "
              f"forward {r.forward_ms:9.2f} ms, walk {r.walk_ms:9.2f} ms, pileup + sum {r.pileup_ms:9.2f} ms", flush=True)
    return measure


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["batch40", "batch80", "big"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--max-replays", type=int, default=3)
    a = ap.parse_args()
    m = make_measure(not a.no_yardstick, a.max_replays)
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
