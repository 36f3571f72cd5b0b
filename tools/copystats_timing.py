"""Time of the per-copy statistics (C-ABI ramx_dev_copy_stats: HIP events round the forward kernels, the walk kernels and the
statistics kernel) next to the pileup of the same flanks and consensus (ramx_dev_pileup: forward, walk, pileup kernels + sum),
in one session, the two calls alternating.

    python tools/copystats_timing.py [--n 100000] [--rows 128] [--W 40] [--repeats 7]

The default shape is that of tests/test_gpu_fullsize.py: N = 100,000 flanks x 128 columns, W = 40, 14p43g, along the loop's own
consensus (tools/align_timing.py, big).  The first pair of calls warms up and is not counted.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_timing as at                                                 # noqa: E402


def _median(v):
    return sorted(v)[len(v) // 2]


def _line(name, what, v):
    return f"{name}: {what:<28} median {_median(v):8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f} ms"


def measure(name, W, dev, flanks, p, cons, kw, loop_ms, rows_total, repeats):
    os.environ.pop("RAMX_ALIGN_BYTES", None)
    pl = dict(forward=[], walk=[], stage=[], wall=[])
    cs = dict(forward=[], walk=[], stage=[], wall=[])
    for i in range(repeats + 1):                                          # the first pair warms up
        t0 = time.perf_counter()
        r = dev.pileup(flanks, p, cons, **kw)
        t1 = time.perf_counter()
        s = dev.copy_stats(flanks, p, cons, **kw)
        t2 = time.perf_counter()
        if i:
            pl["forward"].append(r.forward_ms); pl["walk"].append(r.walk_ms); pl["stage"].append(r.pileup_ms); pl["wall"].append(1e3 * (t1 - t0))
            cs["forward"].append(s.kernel_ms[0]); cs["walk"].append(s.kernel_ms[1]); cs["stage"].append(s.kernel_ms[2]); cs["wall"].append(1e3 * (t2 - t1))
    aligned = int((s.ends["end_row"] >= 0).sum())
    print(f"{name}: {flanks[1]} flanks, {aligned} with an alignment, {int(s.stats['cols'].sum())} covered columns; {repeats} repeats, "
          f"pileup and statistics alternating", flush=True)
    for tag, d, third in (("ramx_dev_pileup", pl, "pileup kernels + sum"), ("ramx_dev_copy_stats", cs, "statistics kernel")):
        print(_line(name, f"{tag} forward", d["forward"]))
        print(_line(name, f"{tag} walk", d["walk"]))
        print(_line(name, f"{tag} {third}", d["stage"]))
        print(_line(name, f"{tag} whole call", d["wall"]), flush=True)
    ratio = _median(cs["stage"]) / _median(pl["stage"])
    print(f"{name}: statistics stage = {ratio:5.2f} x the pileup stage: {'not more' if ratio <= 1 else 'MORE'} than the pileup stage; "
          f"{_median(cs['stage']) / _median(cs['forward']):6.3f} x its forward pass", flush=True)


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
