"""tests/window_ref.py against windows worked out by hand, its decoder against pack_library and the packed loader, and the
inputs of tests/test_gpu_windows.py (tests/window_cases.py) against the list of things they are there to exercise: counted on
the restatement and the tables alone, with the predicates of ramx_pack2_kernel's two paths restated below.  No GPU."""
from collections import Counter

import numpy as np
import pytest

import window_cases as wc
import window_ref as wr
from repeatafterme_amd.loader import pack_library

# A C G T a c g t N N A C G T T G C A A A
HAND_LIB = np.array([0, 1, 2, 3, 4, 5, 6, 7, 99, 99, 0, 1, 2, 3, 3, 2, 1, 0, 0, 0], np.int8)

# (descriptor, W, words of the byte form, words of the packed form, bounds); nibble 0 is the lowest hex digit
HAND = [
    # forward from position 2, two bases before the core edge, t_hi = 9 cuts word 2 after two bases
    ((2, -2, 9, 1, 0), 0, [0x10888888, 0x88765432, 0x88888810], [0x10888888, 0x88888832, 0x88888810], (-2, 9)),
    # reverse complemented from position 11 over the same bases; it runs off position 0 at t = 12
    ((11, -2, 14, -1, 1), 0, [0x10888888, 0x76548832, 0x88883210], [0x10888888, 0x88888832, 0x88883210], (-2, 14)),
    # forward off the last position: four bases, then nothing
    ((16, 0, 20, 1, 0), 0, [0x88888888, 0x88880001, 0x88888888], [0x88888888, 0x88880001, 0x88888888], (0, 20)),
    # an empty flank
    ((5, 1, 0, 1, 0), 0, [0x88888888, 0x88888888, 0x88888888], [0x88888888, 0x88888888, 0x88888888], (1, 0)),
    # W = 3: word 1 is t = -3 .. 4; t_lo = -3 is its first nibble (a lower-case t, then the N run), t_hi = 5 the first of word 2
    ((10, -3, 5, 1, 0), 3, [0x88888888, 0x33210887, 0x88888882], [0x88888888, 0x33210888, 0x88888882], (0, 8)),
]


def test_hand_worked_windows():
    for desc, W, byte_words, packed_words, bounds in HAND:
        for packed, want in ((False, byte_words), (True, packed_words)):
            words, bnd = wr.windows(HAND_LIB, [desc], 64, W, 3, packed=packed)
            assert [f"{int(w):08x}" for w in words[:, 0]] == [f"{w:08x}" for w in want], (desc, W, packed)
            assert tuple(bnd[0]) == bounds
            assert (words[:, 1:] == wr.PAD_WORD).all() and (bnd[1:] == (1, 0)).all()
    assert wr.window_words(600, 0) == 87 and wr.window_words(600, 3) == 88 and wr.window_words(600, 14) == 90
    assert wr.window_words(600, 40) == 97 and wr.window_words(600, 80) == 107 and wr.window_words(50, 0) == 18


def test_decoder_round_trip_at_every_phase():
    rng = np.random.default_rng(5)
    codes = rng.integers(0, 4, 203).astype(np.int8)
    codes[[0, 17, 18, 19, 100, 202]] = 99
    for ph in range(4):
        for starts in ([0], [0, 1], [0, 5, 6, 50], [0, 3, 101, 202]):            # windows that begin mid-byte of the plain packing
            phases = [(ph + i) % 4 for i in range(len(starts))]
            t = pack_library(codes, starts, phases)
            assert np.array_equal(wr.decode_tables(t), codes), (ph, starts)
            assert np.array_equal(wr.decode_tables(wc.split_runs_at_windows(t)), codes)
    # the payload's code: T C A G = 0 1 2 3, first base in the top bits
    t = pack_library(np.array([3, 1, 0, 2], np.int8))
    assert int(t["bytes"][0]) == 0b00011011 and np.array_equal(wr.decode_tables(t), [3, 1, 0, 2])
    t = pack_library(np.array([2, 2, 0], np.int8), [0], [1])
    assert int(t["bytes"][0]) == 0b00111110


def test_decoder_on_the_loaders_own_tables(tmp_path):
    cases = wc.loader_case(tmp_path)
    c = cases[0]
    fs, t = c.extra["fs"], c.tables["loader"]
    assert np.array_equal(wr.decode_tables(t), fs.sequence)                        # fs.sequence: ramx_packed_decode
    assert len(t["bytes"]) == t["n_bytes"] and len(set(int(p) for p in t["win_phase"])) == 4
    recs = dict(c.extra["recs"])
    assert sorted(len(a) % 4 for a in recs.values()) == [0, 1, 1, 2, 3]
    # ranges reach a record's first and last base: a window begins at offset 0 of a record, another ends at its last base
    lens = np.diff(np.concatenate(([0], fs.boundaries[:-1].astype(np.int64))))
    assert (fs.offsets[:-1] == 0).any() and any(int(o) + int(n) == len(recs[i]) for o, n, i in zip(fs.offsets, lens, fs.identifiers))


# ------------------------------------------------------------------------------ the inputs are not empty ground

def classify(case, tables):
    """Counts of (property, strand) over the (flank, word) pairs of one input on one set of tables; strand '+' is step = +1.
    The predicates are those of ramx_pack2_kernel: a word takes the fast path when its eight positions lie inside [t_lo, t_hi],
    inside the library and inside one window."""
    W, KW, n = case.W, case.KW, int(tables["length"])
    ws = np.asarray(tables["win_start"], np.int64)
    ph = np.asarray(tables["win_phase"], np.int64)
    ns = np.asarray(tables["n_start"], np.int64)
    ne = ns + np.asarray(tables["n_len"], np.int64)
    nl = ne - ns
    touch = set(int(ne[j]) for j in range(len(ns) - 1) if ne[j] == ns[j + 1] and int(ne[j]) in set(int(x) for x in ws))
    cnt = Counter()
    k = np.arange(KW, dtype=np.int64)
    t0 = 8 * k - W - 8

    def window_of(p):
        return np.searchsorted(ws[:-1], p, side="right") - 1

    for start, t_lo, t_hi, step, _ in case.descs:
        s = "+" if step > 0 else "-"
        if t_lo > t_hi:
            cnt["empty flank", s] += 1
            continue
        pa, pb = start + step * t0, start + step * (t0 + 7)
        plo, phi = np.minimum(pa, pb), np.maximum(pa, pb)
        inside = (t0 >= t_lo) & (t0 + 7 <= t_hi)
        inlib = (plo >= 0) & (phi < n)
        wlo, whi = window_of(np.clip(plo, 0, n - 1)), window_of(np.clip(phi, 0, n - 1))
        fast = inside & inlib & (wlo == whi)
        cnt["fast", s] += int(fast.sum())
        cnt["straddles a window", s] += int((inside & inlib & (wlo != whi)).sum())
        cnt["cut by t_lo", s] += int(((t0 < t_lo) & (t_lo <= t0 + 7)).sum())
        cnt["cut by t_hi", s] += int(((t0 <= t_hi) & (t_hi < t0 + 7)).sum())
        ta, tb = np.maximum(t0, t_lo), np.minimum(t0 + 7, t_hi)
        qa, qb = start + step * ta, start + step * tb
        qlo, qhi = np.minimum(qa, qb), np.maximum(qa, qb)
        cnt["cut by position 0", s] += int(((ta <= tb) & (qlo < 0) & (qhi >= 0)).sum())
        cnt["cut by the library's end", s] += int(((ta <= tb) & (qlo < n) & (qhi >= n)).sum())
        for b in touch:
            cnt["runs touch at a window's first base", s] += int((inside & inlib & (plo < b) & (b <= phi)).sum())
        if len(ns):
            i0 = np.searchsorted(ne, plo, side="right")               # first run that ends behind plo
            i1 = np.searchsorted(ns, phi, side="right") - 1           # last run that begins at or before phi
            runs = np.maximum(i1 - i0 + 1, 0)
            f = fast & (runs > 0)
            a0, a1 = np.clip(i0, 0, len(ns) - 1), np.clip(i1, 0, len(ns) - 1)
            cnt["run covers the word", s] += int((f & (runs == 1) & (ns[a0] <= plo) & (ne[a0] > phi)).sum())
            cnt["run begins in the word", s] += int((f & (ns[a1] > plo) & (ne[a1] > phi + 1)).sum())
            cnt["run ends in the word", s] += int((f & (ns[a0] < plo) & (ne[a0] <= phi)).sum())
            cnt["two runs", s] += int((fast & (runs == 2)).sum())
            cnt["three runs", s] += int((fast & (runs == 3)).sum())
            for name, pos in (("run of 1 at nibble 0", pa), ("run of 1 at nibble 7", pb)):
                j = np.clip(np.searchsorted(ns, pos, side="right") - 1, 0, len(ns) - 1)
                cnt[name, s] += int((fast & (ns[j] == pos) & (nl[j] == 1)).sum())
        for v in range(4):
            cnt[f"phase {v}", s] += int((fast & ((plo - ws[wlo] + ph[np.clip(wlo, 0, len(ph) - 1)]) % 4 == v)).sum())
        cnt[f"start mod 8 = {start % 8}", s] += int(fast.sum())
        for row in range((KW + 31) // 32):
            cnt[f"block row {row}", s] += int(fast[32 * row:32 * row + 32].sum())
        if t_lo > 0:
            cnt["t_lo > 0", s] += 1
        # the window of the flank's first base (ramx_flank_window_kernel) against those of its later bases
        tt = np.arange(max(t_lo, 0), min(t_hi, 8 * KW - W - 9) + 1, dtype=np.int64)
        p = start + step * tt
        p = p[(p >= 0) & (p < n)]
        if len(p) and (window_of(p) != window_of(np.clip(start + step * max(t_lo, 0), 0, n - 1))).any():
            cnt["leaves its first window", s] += 1
    return cnt


def total(cases, which):
    out = Counter()
    for c in cases:
        out.update(classify(c, c.tables[which]))
    return out


def require(cnt, names, tag, strands="+-", least=5):
    short = [(nm, s, cnt[nm, s]) for nm in names for s in strands if cnt[nm, s] < least]
    assert not short, f"{tag}: {short}"


def fast_rows(W, L):
    """The block rows of 32 words in which a word can lie inside a flank at all (t_hi <= L + W + 2): every row but, for some
    shapes, the partial last one, which then holds look-ahead words only."""
    KW = wr.window_words(L, W)
    rows = [r for r in range((KW + 31) // 32) if 8 * 32 * r - W - 8 + 7 <= L + W + 2]
    assert len(rows) >= (KW + 31) // 32 - 1
    return [f"block row {r}" for r in rows]


MOD8 = [f"start mod 8 = {v}" for v in range(8)]
PHASES = [f"phase {v}" for v in range(4)]
N_EDGES = ["run begins in the word", "run ends in the word"]       # (a run that covers a word needs eight N in a row: the N-mask library)


def _tables_stand_for_the_library(c):
    for name, t in c.tables.items():
        assert np.array_equal(wr.decode_tables(t), wr.fold(c.lib)), (c.name, name)


@pytest.mark.parametrize("L", wc.SWEEP_L)
@pytest.mark.parametrize("W", wc.SWEEP_W)
def test_sweep_inputs(W, L):
    cases = wc.sweep_cases(W, L)
    KW = wr.window_words(L, W)
    rows = fast_rows(W, L)
    assert KW % 32 != 0 and (L != 600 or (KW + 31) // 32 == (3 if W < 40 else 4))      # the last row is a partial one
    for c in cases:
        _tables_stand_for_the_library(c)
        assert 30 <= len(c.descs) <= 300 and (c.lib >= 4).any() and (c.lib == 99).any()
    for which in ("bounds", "inside"):
        cnt = total(cases, which)
        require(cnt, ["fast", "cut by t_lo", "cut by t_hi"] + rows + MOD8 + PHASES + N_EDGES, f"W {W} L {L} {which}")
    require(total(cases, "inside"), ["straddles a window", "leaves its first window"], f"W {W} L {L}")
    assert total(cases, "bounds")["straddles a window", "+"] == 0


@pytest.mark.parametrize("n", wc.FLANK_COUNTS)
def test_count_inputs(n):
    cnt = Counter()
    for c in wc.count_cases(n):
        _tables_stand_for_the_library(c)
        assert len(c.descs) == n
        cnt.update(classify(c, c.tables["bounds"]))
    require(cnt, ["fast", "cut by t_lo"], f"{n} flanks", strands="+-" if n > 60 else "+", least=5 if n > 1 else 1)


def test_n_mask_inputs():
    c = wc.nmask_case()
    _tables_stand_for_the_library(c)
    assert np.array_equal(wr.decode_tables(c.extra["clean_tables"]), c.extra["clean_lib"]) and not (c.extra["clean_lib"] == 99).any()
    for ln in wc.RUN_LENGTHS:
        assert (c.tables["one"]["n_len"] == ln).sum() >= 2
    assert c.tables["one"]["n_start"][0] == 0 and c.tables["one"]["n_start"][-1] + c.tables["one"]["n_len"][-1] == len(c.lib)
    everything = (["fast", "cut by t_lo", "cut by t_hi", "cut by position 0", "cut by the library's end", "two runs", "three runs",
                   "run of 1 at nibble 0", "run of 1 at nibble 7", "t_lo > 0", "run covers the word"] + N_EDGES + MOD8 + fast_rows(c.W, c.L))
    one, many = classify(c, c.tables["one"]), classify(c, c.tables["windows"])
    require(one, everything + ["phase 0"], "one window")
    assert one["straddles a window", "+"] == 0 and one["runs touch at a window's first base", "+"] == 0
    require(many, everything + PHASES + ["straddles a window", "runs touch at a window's first base", "leaves its first window"],
            "several windows")
    assert len(c.tables["windows"]["n_len"]) == len(c.tables["one"]["n_len"]) + 8
    assert many["empty flank", "+"] == 1


def test_loader_inputs(tmp_path):
    cnt = Counter()
    for c in wc.loader_case(tmp_path):
        _tables_stand_for_the_library(c)
        cnt.update(classify(c, c.tables["loader"]))
    require(cnt, ["fast", "cut by t_lo", "cut by t_hi"] + PHASES + N_EDGES, "loader")


def test_pieces_and_replay_inputs():
    c = wc.pieces_case()
    _tables_stand_for_the_library(c)
    cnt = classify(c, c.tables["bounds"])
    assert c.KW == 117 and len(c.descs) == wc.PIECES_N
    require(cnt, ["fast", "cut by t_lo", "cut by t_hi"] + [f"block row {r}" for r in range(4)] + PHASES, "pieces", strands="+")
    r = wc.replay_case()
    _tables_stand_for_the_library(r)
    first, count = r.extra["first"], r.extra["count"]
    assert first == [0, 192] and count == [70, 100] and len(r.descs) == 320
    assert all(d[1] > d[2] for d in r.descs[70:192] + r.descs[292:])                   # the hole and the tiles' ends are empty flanks
    require(classify(r, r.tables["bounds"]), ["fast", "cut by t_lo"] + PHASES, "replay")


@pytest.mark.parametrize("W", wc.LOOP_W)
def test_loop_inputs(W):
    cases = wc.loop_cases(W)
    for c in cases:
        _tables_stand_for_the_library(c)
    for which in ("bounds", "inside"):
        require(total(cases, which), ["fast", "cut by t_lo", "cut by t_hi"] + PHASES + N_EDGES, f"loop W {W} {which}")
