"""Time of the profile replay (C-ABI ramx_dev_profile: HIP events around the replay kernel and its reduction) next to the loop it
replays, and next to the streaming route (RAMX_NO_PERSISTENT=1: one launch per column / the streaming family kernel) on the same
inputs in the same process.

    python tools/profile_timing.py [bench] [cp] [batch] [--repeats 5] [--no-yardstick]

bench: N = 100,000 x 10,000 columns, W = 40, 14p43g (the benchmark's flank set); cp: N = 1,000 x 2,000 (a cell-parallel
shape); batch: 500 families of 60-150 flanks, W = 80, 20p43g.  The consensus replayed is the one the run itself chose.
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


def _streaming(on):
    if on:
        os.environ["RAMX_NO_PERSISTENT"] = "1"
    else:
        os.environ.pop("RAMX_NO_PERSISTENT", None)


def _replays(call, repeats):
    """kernel_ms (HIP events round the two kernels) and the wall time of the whole call, per repeat; the first call warms up"""
    ms, wall = [], []
    for i in range(repeats + 1):
        t0 = time.perf_counter()
        pr = call()
        t1 = time.perf_counter()
        if i:
            ms.append(pr.kernel_ms)
            wall.append(1e3 * (t1 - t0))
    return ms, wall


def one_family(name, n, L, W, matrix, K, seed, repeats, yardstick):
    t0 = time.time()
    fs = synth_family(n, L, W, K=K, seed=seed)
    p = named_params(matrix, bandwidth=W, L=L, when_to_stop=L)
    dev = Device(0)
    dev.load_library(fs.sequence)
    flanks, _ = resolve_flanks(1, fs.cores, W, L)
    print(f"{name}: N = {n} x {L} columns, W = {W}, {matrix} (set-up {time.time() - t0:.1f} s)", flush=True)
    dev.begin_direction(flanks, p)
    dev.run_direction()                                                  # warm-up
    loops = [dev.run_direction() for _ in range(3)]
    cons, _, _ = dev.download()
    rows = loops[-1].rows_executed
    best = min(i.loop_ms for i in loops)
    print(f"{name}: loop (default route: persistent={loops[-1].persistent}, lanes per flank {loops[-1].lanes_per_flank}, "
          f"packed rows {loops[-1].packed_rows}) {best:9.2f} ms = {1e3 * best / rows:7.3f} us per column, {rows} columns", flush=True)
    if yardstick:
        _streaming(True)
        dev.begin_direction(flanks, p)
        dev.run_direction()
        ys = [dev.run_direction() for _ in range(3)]
        _streaming(False)
        yb = min(i.loop_ms for i in ys)
        assert ys[-1].rows_executed == rows and np.array_equal(dev.download()[0], cons)
        print(f"{name}: loop (streaming route: persistent={ys[-1].persistent}, {ys[-1].launches} launches)  {yb:9.2f} ms = "
              f"{1e3 * yb / rows:7.3f} us per column", flush=True)
    cons = np.ascontiguousarray(cons[:rows], np.int8)
    ms, wall = _replays(lambda: dev.profile(flanks, p, cons, rows=rows), repeats)
    print(f"{name}: profile replay, {repeats} repeats: min {min(ms):9.2f} ms  median {sorted(ms)[len(ms) // 2]:9.2f} ms  max {max(ms):9.2f} ms"
          f" = {1e3 * min(ms) / rows:7.3f} us per column (min); {min(ms) / best:5.2f} x the default loop"
          + (f", {min(ms) / yb:5.2f} x the streaming loop" if yardstick else ""), flush=True)
    print(f"{name}: whole ramx_dev_profile call (uploads, window pack, kernels, downloads): min {min(wall):9.2f} ms  median "
          f"{sorted(wall)[len(wall) // 2]:9.2f} ms = {min(wall) / best:5.2f} x the default loop", flush=True)
    if yardstick:
        # the same replay with the rows in the global buffer (the route of the band widths without an on-chip instantiation)
        os.environ["RAMX_PROFILE_NO_RESIDENT"] = "1"
        gms, _ = _replays(lambda: dev.profile(flanks, p, cons, rows=rows), repeats)
        os.environ.pop("RAMX_PROFILE_NO_RESIDENT")
        print(f"{name}: profile replay, rows in the global buffer, {repeats} repeats: min {min(gms):9.2f} ms  median "
              f"{sorted(gms)[len(gms) // 2]:9.2f} ms = {1e3 * min(gms) / rows:7.3f} us per column (min)", flush=True)
    dev.close()


def batch(repeats, yardstick, F=500, W=80, L=1200):
    t0 = time.time()
    p = named_params("20p43g", bandwidth=W, L=L)
    fams = [synth_family(int(60 + (i * 37) % 90), L, W, K=300 + (i * 53) % 500, seed=1000 + i) for i in range(F)]
    print(f"batch: {F} families of 60-150 flanks ({sum(f.cores.n for f in fams)} in all), W = {W}, 20p43g, L = {L} "
          f"(set-up {time.time() - t0:.1f} s)", flush=True)

    def loop():
        best, infos, ms = None, None, None
        for _ in range(3):
            ms = [new_master(L) for _ in fams]
            infos = extend_batch(1, [(f.cores.copy(), f.sequence, m) for f, m in zip(fams, ms)], p)
            best = infos[0].loop_ms if best is None else min(best, infos[0].loop_ms)
        return best, infos, ms
    best, infos, masters = loop()
    cols = sum(i.rows_executed for i in infos)
    print(f"batch: loop (default routes) {best:9.2f} ms for {cols} family-columns", flush=True)
    if yardstick:
        _streaming(True)
        yb, yi, _ = loop()
        _streaming(False)
        assert [i.rows_executed for i in yi] == [i.rows_executed for i in infos]
        print(f"batch: loop (streaming family kernel, persistent={yi[0].persistent}) {yb:9.2f} ms", flush=True)
    # the same layout ramx_extend_batch makes: one library, every family's flanks from a multiple of 64
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
    rows = [i.rows_executed for i in infos]
    cons = np.zeros((F, L), np.int8)
    for f in range(F):
        cons[f, :rows[f]] = masters[f][L + p.l:L + p.l + rows[f]]
    dev = Device(0)
    dev.load_library(lib)
    ms, wall = _replays(lambda: dev.profile((arr, at), p, cons, rows=rows, fam_first=first, fam_count=count), repeats)
    print(f"batch: profile replay, {repeats} repeats: min {min(ms):9.2f} ms  median {sorted(ms)[len(ms) // 2]:9.2f} ms  max {max(ms):9.2f} ms;"
          f" {min(ms) / best:5.2f} x the default loop" + (f", {min(ms) / yb:5.2f} x the streaming loop" if yardstick else ""), flush=True)
    print(f"batch: whole ramx_dev_profile call (uploads, window pack, kernels, downloads): min {min(wall):9.2f} ms  median "
          f"{sorted(wall)[len(wall) // 2]:9.2f} ms = {min(wall) / best:5.2f} x the default loop", flush=True)
    if yardstick:
        os.environ["RAMX_PROFILE_NO_RESIDENT"] = "1"
        gms, _ = _replays(lambda: dev.profile((arr, at), p, cons, rows=rows, fam_first=first, fam_count=count), repeats)
        os.environ.pop("RAMX_PROFILE_NO_RESIDENT")
        print(f"batch: profile replay, rows in the global buffer, {repeats} repeats: min {min(gms):9.2f} ms  median "
              f"{sorted(gms)[len(gms) // 2]:9.2f} ms", flush=True)
    dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["bench", "cp", "batch"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-yardstick", action="store_true")
    a = ap.parse_args()
    for s in a.shapes:
        if s == "bench":
            one_family("bench", 100000, 10000, 40, "14p43g", 1500, 1, a.repeats, not a.no_yardstick)
        elif s == "cp":
            one_family("cp", 1000, 2000, 40, "14p43g", 1500, 3, a.repeats, not a.no_yardstick)
        elif s == "batch":
            batch(a.repeats, not a.no_yardstick)
        else:
            sys.exit(f"unknown shape {s}")


if __name__ == "__main__":
    main()
