"""Time of the pairwise divergence between copies (C-ABI ramx_dev_copy_dist: HIP events round the transposition kernel and round
the pair kernel) next to a host loop that computes the same records from the plane words ramx_dev_plane_gram(..., bits) returns.

    python tools/dist_timing.py [--rows 1000 10000] [--copies 256 1024 2048] [--repeats 3] [--host-copies 8]

One family of 2,048 flanks, W = 14, 14p43g; the consensus replayed is the one the loop chose, cut or continued (with its own
bases, cyclically) to the fixed number of rows.  The host side fetches the words of classes 0..3, 5 and 6 of every row (2,048
planes a call), transposes them with numpy into the five streams per copy the device uses, and counts with numpy popcounts the
pairs of the FIRST --host-copies selected copies with every selected copy; those records are compared with the device's, and
the time of the whole upper triangle is that time scaled by the number of pairs (printed as "scaled": it is not measured).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                       # noqa: E402

from repeatafterme_amd.datamodel import COPY_DIST_DTYPE, PLANE_DTYPE, new_master   # noqa: E402
from repeatafterme_amd.device import Device, resolve_flanks, select_copies         # noqa: E402
from repeatafterme_amd.extend import extend_alignment                   # noqa: E402
from repeatafterme_amd.scoring import named_params                       # noqa: E402
from repeatafterme_amd.synth import synth_family                         # noqa: E402

N, W = 2048, 14


def _median(v):
    return sorted(v)[len(v) // 2]


def _pop(x):
    m1, m2, m4, h = (np.uint64(k) for k in (0x5555555555555555, 0x3333333333333333, 0x0F0F0F0F0F0F0F0F, 0x0101010101010101))
    x = x - ((x >> np.uint64(1)) & m1)
    x = (x & m2) + ((x >> np.uint64(2)) & m2)
    x = (x + (x >> np.uint64(4))) & m4
    return ((x * h) >> np.uint64(56)).astype(np.int64)


def host_streams(d, rows, sel):
    """-> (uint64 [5][C][RW], seconds spent fetching the words, seconds spent transposing)"""
    t0 = time.perf_counter()
    T = (N + 63) // 64
    words = np.zeros((rows, 8, T), np.uint64)
    per_call = 2048 // 6
    for r0 in range(0, rows, per_call):
        r1 = min(rows, r0 + per_call)
        planes = np.zeros((r1 - r0) * 6, PLANE_DTYPE)
        planes["row"] = np.repeat(np.arange(r0, r1), 6)
        planes["cls"] = np.tile([0, 1, 2, 3, 5, 6], r1 - r0)
        _, bits = d.plane_gram(planes, bits=True)
        words[r0:r1, [0, 1, 2, 3, 5, 6]] = bits.reshape(r1 - r0, 6, T)
    t1 = time.perf_counter()
    five = np.stack([words[:, 0] | words[:, 1] | words[:, 2] | words[:, 3], words[:, 1] | words[:, 3], words[:, 2] | words[:, 3],
                     words[:, 5], words[:, 6]])                              # [5][rows][T]
    RW = (rows + 63) // 64
    bit = np.unpackbits(five.view(np.uint8).reshape(5, rows, T, 8), axis=-1, bitorder="little").reshape(5, rows, T * 64)[:, :, sel]
    pad = np.zeros((5, RW * 64, len(sel)), np.uint8)
    pad[:, :rows] = bit
    streams = np.packbits(pad.transpose(0, 2, 1).reshape(5, len(sel), RW, 64), axis=-1, bitorder="little").view(np.uint64).reshape(5, len(sel), RW)
    return np.ascontiguousarray(streams), t1 - t0, time.perf_counter() - t1


def host_pairs(st, k):
    """the records of the first k copies with every copy -> COPY_DIST_DTYPE [k][C]"""
    V, LO, HI, D, CV = st
    out = np.zeros((k, st.shape[1]), COPY_DIST_DTYPE)
    for a in range(k):
        v, x, y, c = V[a] & V, LO[a] ^ LO, HI[a] ^ HI, CV[a] & CV
        out["cover"][a], out["sites"][a] = _pop(c).sum(axis=1), _pop(v).sum(axis=1)
        out["ts"][a], out["tv"][a] = _pop(v & y & ~x).sum(axis=1), _pop(v & x).sum(axis=1)
        out["del_one"][a], out["del_both"][a] = _pop((D[a] ^ D) & c).sum(axis=1), _pop(D[a] & D).sum(axis=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--copies", type=int, nargs="+", default=[256, 1024, 2048])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-copies", type=int, default=8)
    a = ap.parse_args()
    for rows in a.rows:
        L = rows
        fs = synth_family(N, L, W, K=L, seed=9, both_sides=False, minus_frac=0.3, n_run_frac=0.05)
        seq = np.ascontiguousarray(fs.sequence, np.int8)
        ep = named_params("14p43g", bandwidth=W, L=L, when_to_stop=1000)
        master = new_master(L)
        info = extend_alignment(1, fs.cores.copy(), seq, master, ep)
        kept = master[L + ep.l:L + ep.l + info.ret]
        cons = np.resize(np.asarray(kept, np.int8), rows) if info.ret > 0 else np.zeros(rows, np.int8)
        d = Device(0)
        try:
            d.load_library(seq)
            flanks, idx = resolve_flanks(1, fs.cores, W, L)
            t0 = time.perf_counter()
            res = d.planes(flanks, ep, cons)
            print(f"rows {rows}: the loop kept {info.ret} columns; replay with planes of {len(idx)} flanks {1e3 * (time.perf_counter() - t0):.1f} ms "
                  f"(kernels: forward {res.kernel_ms[0]:.2f}, walk {res.kernel_ms[1]:.2f}, pileup {res.kernel_ms[2]:.2f}, planes {res.kernel_ms[3]:.2f} ms)", flush=True)
            for copies in a.copies:
                sel = select_copies(res.ends[:len(idx)], rows, 1, copies)
                tr, pr, wall = [], [], []
                for i in range(a.repeats + 1):                                   # the first call warms up
                    t0 = time.perf_counter()
                    m = d.copy_dist(sel)
                    if i:
                        wall.append(1e3 * (time.perf_counter() - t0))
                        ms = d.copy_dist_ms()
                        tr.append(ms[0]); pr.append(ms[1])
                C = len(sel)
                pairs = C * (C + 1) // 2
                print(f"rows {rows} copies {C}: transposition median {_median(tr):8.3f} ms (min {min(tr):.3f}), pairs median {_median(pr):8.3f} ms "
                      f"(min {min(pr):.3f}), whole call with the {24 * C * C / 1e6:.1f} MB copy back median {_median(wall):8.2f} ms; "
                      f"{pairs * ((rows + 63) // 64) / 1e6 / max(_median(pr), 1e-9):.1f} G pair-words/s", flush=True)
                st, fetch_s, tr_s = host_streams(d, rows, sel)
                k = min(a.host_copies, C)
                t0 = time.perf_counter()
                want = host_pairs(st, k)
                host_s = time.perf_counter() - t0
                same = bool(np.array_equal(want, m[:k]))
                print(f"rows {rows} copies {C}: host loop (numpy): words fetched in {1e3 * fetch_s:.1f} ms, transposed in {1e3 * tr_s:.1f} ms, "
                      f"{k} x {C} pairs in {1e3 * host_s:.1f} ms, equal to the device's records: {same}; scaled to the {pairs} pairs of the "
                      f"upper triangle: {1e3 * host_s * pairs / (k * C):.0f} ms", flush=True)
                if not same:
                    sys.exit("the host loop and the device disagree")
        finally:
            d.close()


if __name__ == "__main__":
    main()
