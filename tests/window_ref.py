"""The transposed 4-bit flank windows (csrc/ramx_kernels_common.h: ramx_pack_kernel, ramx_pack2_kernel) restated in numpy and
loops from the flank descriptors and a one-byte-per-base library alone, and an independent decoder of the packed library's
tables (include/ramx.h ramx_packed_library).  What Device.peek_windows() reads back is compared with this word for word.

Nibble i of word k of flank n is flank position t = 8k + i - W - 8, i.e. library position start + step * t.  Its class is 8
unless t_lo <= t <= t_hi, the position lies in the library and the code there is a base; a complemented flank keeps the case.
The byte form knows the codes 0..7 (A C G T a c g t), the packed form 0..3 only: everything else is N.  Nothing here imports
the product's arithmetic: the window length is restated from the contract."""
import numpy as np

PAD_WORD = 0x88888888


def window_words(L, W):
    """Words of one flank's window: positions t'' = t + W + 8 over [7, L + 2W + 9], a pad word in front, look-ahead behind."""
    return (L + 2 * W + 2) // 8 + 12


def padded_lanes(n):
    """Lanes of a direction's windows: the flanks in whole tiles of 64, at least one tile."""
    return max((n + 63) // 64 * 64, 64)


def descriptors(flanks):
    """(ctypes flank array, n) -> [(start, t_lo, t_hi, step, compl)]"""
    arr, n = flanks
    return [(int(arr[i].start), int(arr[i].t_lo), int(arr[i].t_hi), int(arr[i].step), int(arr[i].compl_)) for i in range(n)]


def fold(lib):
    """Lower case folded into upper case: what the packed form can hold of a byte library."""
    lib = np.asarray(lib, np.int8)
    return np.where((lib >= 4) & (lib <= 7), lib - 4, lib).astype(np.int8)


def flank_classes(lib, desc, W, KW, packed):
    """The 8 * KW classes of one flank's window, nibble after nibble."""
    start, t_lo, t_hi, step, compl = desc
    lib = np.asarray(lib, np.int8)
    t = np.arange(8 * KW, dtype=np.int64) - W - 8
    p = start + step * t
    there = (t >= t_lo) & (t <= t_hi) & (p >= 0) & (p < len(lib))
    b = lib[np.where(there, p, 0)].astype(np.int64) if len(lib) else np.zeros(8 * KW, np.int64)
    base = there & (b >= 0) & (b <= (3 if packed else 7))
    c = ((b & 4) | (3 - (b & 3))) if compl else b
    return np.where(base, c, 8)


def windows(lib, descs, lanes, W, KW, packed=False):
    """-> (words uint32 [KW][lanes], bounds int32 [lanes][2]); lanes from len(descs) on hold no flank."""
    assert lanes >= len(descs)
    words = np.full((KW, lanes), PAD_WORD, np.uint32)
    bounds = np.zeros((lanes, 2), np.int32)
    bounds[:] = (1, 0)
    shifts = 4 * np.arange(8)
    for n, d in enumerate(descs):
        c = flank_classes(lib, d, W, KW, packed).reshape(KW, 8)
        words[:, n] = (c << shifts).sum(axis=1).astype(np.uint32)
        bounds[n] = (d[1] + W, d[2] + W)
    return words, bounds


_TWOBIT_TO_CODE = (3, 1, 0, 2)       # T C A G = 0 1 2 3 in the payload; A C G T = 0 1 2 3 in the library


def decode_tables(t):
    """The one-byte-per-base library a packed library stands for: window i holds positions win_start[i] .. win_start[i + 1] - 1
    from byte win_byte[i] on, its first base at position win_phase[i] of that byte, first base in the top bits; the runs of N
    are laid over it as 99."""
    n = int(t["length"])
    ws, wb, ph, by = (np.asarray(t[k]) for k in ("win_start", "win_byte", "win_phase", "bytes"))
    out = np.full(n, -1, np.int8)
    code = np.array(_TWOBIT_TO_CODE, np.int8)
    for w in range(len(ph)):
        q = np.arange(int(ws[w + 1]) - int(ws[w]), dtype=np.int64) + int(ph[w])
        out[int(ws[w]):int(ws[w + 1])] = code[(by[int(wb[w]) + q // 4].astype(np.int64) >> (6 - 2 * (q % 4))) & 3]
    for s, ln in zip(t["n_start"], t["n_len"]):
        out[int(s):int(s) + int(ln)] = 99
    assert n == 0 or (int(ws[0]) == 0 and int(ws[len(ph)]) == n and (out != -1).all())
    return out


def first_difference(got, want, descs):
    """The first (flank, word) at which two word arrays differ, with the flank's descriptor: the message of a failed comparison."""
    if got.shape != want.shape:
        return f"shapes {got.shape} and {want.shape}"
    bad = np.argwhere((got != want).T)           # flank-major
    if not len(bad):
        return ""
    n, k = (int(v) for v in bad[0])
    d = descs[n] if n < len(descs) else "pad lane"
    return (f"{len(bad)} words differ; first at flank {n} word {k}: got {int(got[k, n]):08x}, want {int(want[k, n]):08x}; "
            f"(start, t_lo, t_hi, step, compl) = {d}")
