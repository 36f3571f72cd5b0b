"""Time of the target-site duplications (C-ABI ramx_dev_tsd: HIP events round the pack of the 2 n windows and round the TSD
kernel) next to the statistics kernel of ramx_dev_copy_stats on as many flanks, in one process, the two calls alternating.

    python tools/tsd_timing.py [--n 100000] [--repeats 7] [--out profiles/tsd_replay.log]

n copies of one family on both strands (synth_family, windows on both sides of the core), one site per copy with its ends 60
bases outside the core, default parameters (slack 3, lengths 4..20, one mismatch in 10).  The statistics run along the loop's own
consensus of the right extension: 128 columns, W = 40, 14p43g (the shape of tools/copystats_timing.py).  The first pair of calls
warms up and is not counted.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                       # noqa: E402

from repeatafterme_amd.datamodel import TSD_SITE_DTYPE, TsdParams        # noqa: E402
from repeatafterme_amd.device import Device, resolve_flanks             # noqa: E402
from repeatafterme_amd.scoring import named_params                       # noqa: E402
from repeatafterme_amd.synth import synth_family                         # noqa: E402


def _median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tsd_replay.log"))
    a = ap.parse_args()
    L, W = 128, 40
    t0 = time.time()
    fs = synth_family(a.n, L, W, K=1500, seed=1, both_sides=True, minus_frac=0.3)
    p = named_params("14p43g", bandwidth=W, L=L, when_to_stop=L)
    c = fs.cores
    sites = np.zeros(c.n, TSD_SITE_DTYPE)
    sites["lo"] = np.minimum(c.left_pos, c.right_pos) - 60
    sites["hi"] = np.maximum(c.left_pos, c.right_pos) + 60
    sites["seq_lo"], sites["seq_hi"] = c.lower, c.upper
    dev = Device(0)
    dev.load_library(fs.sequence)
    flanks, _ = resolve_flanks(1, c, W, L)
    dev.begin_direction(flanks, p)
    dev.run_direction()
    cons, _, _ = dev.download()
    rows = len(cons)
    lines = [f"tsd: {a.n} sites = {2 * a.n} windows, slack 3, lengths 4..20, mm_div 10; statistics: {flanks[1]} flanks x {rows} columns, "
             f"W = {W}, 14p43g; {a.repeats} repeats, the two calls alternating (set-up {time.time() - t0:.1f} s)"]
    pack, kern, wall, stat, swall = [], [], [], [], []
    for i in range(a.repeats + 1):                                       # the first pair warms up
        t1 = time.perf_counter()
        rec, ms = dev.tsd(sites, TsdParams(), timing=True)
        t2 = time.perf_counter()
        s = dev.copy_stats(flanks, p, cons, rows=rows)
        t3 = time.perf_counter()
        if i:
            pack.append(ms[0]); kern.append(ms[1]); wall.append(1e3 * (t2 - t1)); stat.append(s.kernel_ms[2]); swall.append(1e3 * (t3 - t2))
    found = int((rec["k"] > 0).sum())
    lines.append(f"tsd: {found} of {a.n} sites show a word (random flanks: chance matches only)")
    for what, v in (("ramx_dev_tsd pack of the windows", pack), ("ramx_dev_tsd TSD kernel", kern), ("ramx_dev_tsd whole call", wall),
                    ("ramx_dev_copy_stats statistics kernel", stat), ("ramx_dev_copy_stats whole call", swall)):
        lines.append(f"tsd: {what:<40} median {_median(v):8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f} ms")
    lines.append(f"tsd: TSD kernel = {_median(kern) / _median(pack):5.2f} x the pack it follows, {_median(kern) / _median(stat):5.2f} x the statistics kernel")
    dev.close()
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
