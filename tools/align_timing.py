"""Time of the alignment replay (C-ABI ramx_dev_align: HIP events round the forward kernels and round the walk kernels) next to
the profile replay with its rows in the global buffer (ramx_dev_profile under RAMX_PROFILE_NO_RESIDENT=1), which moves the same
row state, and next to the loop.

    python tools/align_timing.py [batch40] [batch80] [big] [--repeats 3] [--profile-only]

batch40 / batch80: 500 families of 60-150 flanks, W = 40 / 80, 20p43g, 1,000 rows each; big: N = 100,000, W = 40, 14p43g,
2,000 rows.  The consensus replayed is the one the loop chose, cut or continued (with its own bases, cyclically) to the
fixed number of rows, so that both replays do the same number of rows on the same flanks.  --profile-only measures the
profile side alone and uses nothing but the profile entry: the tool then also runs on a tree that has no alignment replay.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                       # noqa: E402

from repeatafterme_amd import _lib                                       # noqa: E402
from repeatafterme_amd.datamodel import new_master                       # noqa: E402
from repeatafterme_amd.device import Device, resolve_flanks             # noqa: E402
from repeatafterme_amd.extend import extend_batch                        # noqa: E402
from repeatafterme_amd.scoring import named_params                       # noqa: E402
from repeatafterme_amd.synth import synth_family                         # noqa: E402


def _median(v):
    return sorted(v)[len(v) // 2]


def _fixed_rows(cons, have, rows):
    """cons[0..have) cut or continued cyclically to `rows` bases"""
    if have <= 0:
        return np.zeros(rows, np.int8)
    return np.resize(np.asarray(cons[:have], np.int8), rows)


def _measure(name, W, call_profile, call_align, loop_ms, rows_total, repeats, profile_only):
    os.environ["RAMX_PROFILE_NO_RESIDENT"] = "1"
    pms, pwall = [], []
    for i in range(repeats + 1):                                         # the first call warms up
        t0 = time.perf_counter()
        r = call_profile()
        if i:
            pms.append(r.kernel_ms)
            pwall.append(1e3 * (time.perf_counter() - t0))
    os.environ.pop("RAMX_PROFILE_NO_RESIDENT")
    print(f"{name}: profile replay, rows in the global buffer, {repeats} repeats: median {_median(pms):9.2f} ms  min {min(pms):9.2f}  "
          f"max {max(pms):9.2f} ms (whole call: median {_median(pwall):9.2f} ms)", flush=True)
    if profile_only:
        return
    # under the default budget of the decision codes (tiles in groups that fit), and with room for every tile at once
    one_group = (rows_total * (W // 4 + 1) * 256) + (1 << 20)
    for label, budget in (("default budget", None), (f"one group, RAMX_ALIGN_BYTES = {one_group}", one_group)):
        if budget is None:
            os.environ.pop("RAMX_ALIGN_BYTES", None)
        else:
            os.environ["RAMX_ALIGN_BYTES"] = str(budget)
        fms, wms, wall = [], [], []
        for i in range(repeats + 1):
            t0 = time.perf_counter()
            r = call_align()
            if i:
                fms.append(r.forward_ms)
                wms.append(r.walk_ms)
                wall.append(1e3 * (time.perf_counter() - t0))
        ratio = _median(fms) / _median(pms)
        print(f"{name}: alignment forward pass ({label}), {repeats} repeats: median {_median(fms):9.2f} ms  min {min(fms):9.2f}  max "
              f"{max(fms):9.2f} ms = {ratio:5.2f} x the profile replay (bound 1.10): {'within' if ratio <= 1.10 else 'MISSED'}", flush=True)
        print(f"{name}: alignment walk ({label}): median {_median(wms):9.2f} ms  min {min(wms):9.2f}  max {max(wms):9.2f} ms", flush=True)
        print(f"{name}: whole ramx_dev_align call, per-flank records only (uploads, window pack, kernels, download; {label}): median "
              f"{_median(wall):9.2f} ms" + (f" = {_median(wall) / loop_ms:5.2f} x the loop ({loop_ms:.2f} ms)" if loop_ms else ""), flush=True)
    os.environ.pop("RAMX_ALIGN_BYTES", None)


def big(repeats, profile_only, n=100000, L=2000, W=40, measure=None):
    """measure (tools/pileup_timing.py): called as measure(name, W, dev, flanks, p, cons, kw, loop_ms, rows_total, repeats) in place
    of the measurements of this tool"""
    t0 = time.time()
    fs = synth_family(n, L, W, K=1500, seed=1)
    p = named_params("14p43g", bandwidth=W, L=L, when_to_stop=L)
    dev = Device(0)
    dev.load_library(fs.sequence)
    flanks, _ = resolve_flanks(1, fs.cores, W, L)
    print(f"big: N = {n} x {L} rows, W = {W}, 14p43g (set-up {time.time() - t0:.1f} s)", flush=True)
    dev.begin_direction(flanks, p)
    dev.run_direction()
    loops = [dev.run_direction() for _ in range(3)]
    cons, _, _ = dev.download()
    rows = loops[-1].rows_executed
    best = min(i.loop_ms for i in loops)
    print(f"big: loop (persistent={loops[-1].persistent}, packed rows {loops[-1].packed_rows}) {best:9.2f} ms, {rows} rows", flush=True)
    cons = _fixed_rows(cons, rows, L)
    tiles = (flanks[1] + 63) // 64
    if measure is not None:
        measure("big", W, dev, flanks, p, cons, dict(rows=L), best, tiles * L, repeats)
        dev.close()
        return
    _measure("big", W, lambda: dev.profile(flanks, p, cons, rows=L), None if profile_only else lambda: dev.align(flanks, p, cons, rows=L, columns=False),
             best, tiles * L, repeats, profile_only)
    dev.close()


def batch(name, W, repeats, profile_only, F=500, L=1000, measure=None):
    t0 = time.time()
    p = named_params("20p43g", bandwidth=W, L=L)
    fams = [synth_family(int(60 + (i * 37) % 90), L, W, K=300 + (i * 53) % 500, seed=1000 + i) for i in range(F)]
    print(f"{name}: {F} families of 60-150 flanks ({sum(f.cores.n for f in fams)} in all), W = {W}, 20p43g, {L} rows each "
          f"(set-up {time.time() - t0:.1f} s)", flush=True)
    best, infos, masters = None, None, None
    for _ in range(3):
        masters = [new_master(L) for _ in fams]
        infos = extend_batch(1, [(f.cores.copy(), f.sequence, m) for f, m in zip(fams, masters)], p)
        best = infos[0].loop_ms if best is None else min(best, infos[0].loop_ms)
    print(f"{name}: loop (default routes) {best:9.2f} ms for {sum(i.rows_executed for i in infos)} family-columns", flush=True)
    lib = np.concatenate([f.sequence for f in fams])
    offs = np.cumsum([0] + [len(f.sequence) for f in fams])
    res = [resolve_flanks(1, f.cores, W, L)[0] for f in fams]
    first, count, at = [], [], 0
    for fl, nx in res:
        first.append(at)
        count.append(nx)
        at += (nx + 63) // 64 * 64
    arr = (_lib.Flank * max(at, 64))()
    for i in range(len(arr)):
        arr[i].t_lo, arr[i].t_hi, arr[i].step = 1, 0, 1
    for f, (fl, nx) in enumerate(res):
        for i in range(nx):
            arr[first[f] + i] = fl[i]
            arr[first[f] + i].start += int(offs[f])
    rows = [L] * F
    cons = np.zeros((F, L), np.int8)
    for f in range(F):
        cons[f] = _fixed_rows(masters[f][L + p.l:], infos[f].rows_executed, L)
    dev = Device(0)
    dev.load_library(lib)
    kw = dict(rows=rows, fam_first=first, fam_count=count)
    if measure is not None:
        measure(name, W, dev, (arr, at), p, cons, kw, best, (at // 64) * L, repeats)
        dev.close()
        return
    _measure(name, W, lambda: dev.profile((arr, at), p, cons, **kw), None if profile_only else lambda: dev.align((arr, at), p, cons, columns=False, **kw),
             best, (at // 64) * L, repeats, profile_only)
    dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["batch40", "batch80", "big"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--profile-only", action="store_true")
    a = ap.parse_args()
    for s in a.shapes:
        if s == "big":
            big(a.repeats, a.profile_only)
        elif s == "batch40":
            batch(s, 40, a.repeats, a.profile_only)
        elif s == "batch80":
            batch(s, 80, a.repeats, a.profile_only)
        else:
            sys.exit(f"unknown shape {s}")


if __name__ == "__main__":
    main()
