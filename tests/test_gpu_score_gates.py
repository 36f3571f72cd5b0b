"""Every kernel route at the edge of its score-range gate (tests/score_gates.py restates the gates): a scoring system just inside
takes the narrow arithmetic and must still be exact, one just outside must be turned away -- and computed exactly elsewhere.
Everything is integer-exact against the oracle; where the run info shows the route, it must agree with score_gates."""
import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import new_master
from repeatafterme_amd.synth import synth_family

import score_gates as sg
from helpers import assert_same_result, gpu_extend, oracle_extend, run_both_directions, to_extend_params
from score_gates import edge_scale, gate_family, shape_params

pytestmark = pytest.mark.gpu

ROUTE_VARS = ("RAMX_NO_FAMILY_ROUTE", "RAMX_NO_CP_DEVICE", "RAMX_NO_CP", "RAMX_PROFILE_NO_RESIDENT", "RAMX_NO_PK", "RAMX_NO_FASTPACK", "RAMX_NO_PERSISTENT", "RAMX_PK_SEGMENT",
              "RAMX_TEST_PK_WRONG_EVERY")


def _env(monkeypatch, **env):
    for k in ROUTE_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _run_device(fs, p, peek, monkeypatch, **env):
    """The right direction through seam 2 on the lane-per-flank route: run info, consensus, trimmed highs and positions, and
    the final DP rows of the flanks in `peek`."""
    from repeatafterme_amd.device import Device, resolve_flanks
    _env(monkeypatch, RAMX_NO_FAMILY_ROUTE="1", RAMX_NO_CP_DEVICE="1", **env)
    dev = Device(0)
    try:
        dev.load_library(fs.sequence)
        flanks, idx = resolve_flanks(1, fs.cores, p.bandwidth, p.L)
        assert np.array_equal(idx, np.arange(fs.cores.n))
        dev.begin_direction(flanks, to_extend_params(p))
        info = dev.run_direction()
        cons, th, tp = dev.download()
        state = [dev.peek_state(i) for i in peek]
    finally:
        dev.close()
    return info, cons, th, tp, state


def _assert_equals_oracle(got, fs, p, tag):
    info, cons, th, tp, _ = got
    c, m = fs.cores.copy(), new_master(p.L)
    o = po.oracle_extend(1, c, fs.sequence, m, p)
    assert (info.ret, info.rows_executed, info.limit_warning) == (o.ret, o.rows_executed, o.limit_warning), tag
    assert np.array_equal(cons, m[p.L + p.l:p.L + p.l + o.rows_executed]), f"{tag}: consensus"
    ext = (th > 0) & (tp >= 0)                                    # ram_extend.c:1234-1247
    assert np.array_equal(np.where(ext, tp + 1, 0), c.right_len), f"{tag}: lengths"
    assert np.array_equal(np.where(ext, th, 0), c.score), f"{tag}: scores"


def _assert_same_rows(a, b, tag):
    assert (a[0].ret, a[0].rows_executed, a[0].limit_warning) == (b[0].ret, b[0].rows_executed, b[0].limit_warning), tag
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), tag
    for i, ((ca, ha, pa), (cb, hb, pb)) in enumerate(zip(a[4], b[4])):
        assert np.array_equal(ca, cb), f"{tag}: final DP row of peeked flank {i} differs in cells {np.nonzero((ca != cb).any(axis=1))[0][:8]}"
        assert (ha, pa) == (hb, pb), tag


@pytest.mark.parametrize("shape", ["a", "b", "c", "d", "e", "f"])
@pytest.mark.parametrize("W", [14, 20, 40, 80])
def test_packed_rows_at_the_admission_edge(W, shape, monkeypatch):
    """The packed int16 rows with the largest scale of each shape the plan admits, and the smallest it refuses.  200 flanks (three
    full tiles and a partial one), 320 columns (five checks of every 64th row, a re-centring every 16th), a third of the flanks
    ending while aligned -- their best cell then falls by a deletion per row, the move the plan has to allow for.  Inside the edge
    the packed kernel must run (`packed_rows`; a refusal by its own row checks would show here as 0) and equal the oracle and,
    cell by cell in the final DP rows, the int32 rows (RAMX_NO_PK=1): a cell that stuck at an int16 limit would differ there.
    Shapes b, c, d also in pieces of 64 columns and with every third guess wrong: the bases survive a hand-over and a rollback."""
    n, L = 200, 320
    fs = gate_family(n, L, W, seed=900 + W, K=300)
    short = np.arange(0, n, 3)
    early = int(short[np.argmin(fs.cores.upper[short] - fs.cores.right_pos[short])])
    peek = (0, 1, early, n - 1)                                   # first (ends early), a full one, the one that ends first, last
    s = edge_scale(shape, W)
    for scale, inside in ((s, True), (s + 1, False)):
        p = shape_params(shape, scale, W, L)
        assert sg.pk_plan(W, p.gapopen, p.gapextn, p.matrix).admitted == inside
        tag = f"W={W} shape {shape} scale {scale} go={p.gapopen} ge={p.gapextn} P, mn = {sg.p_mn(p.matrix)}"
        got = _run_device(fs, p, peek, monkeypatch)
        _assert_equals_oracle(got, fs, p, tag)
        ref = _run_device(fs, p, peek, monkeypatch, RAMX_NO_PK="1")
        assert ref[0].packed_rows == 0 and ref[0].persistent == 1, tag
        _assert_same_rows(got, ref, tag)
        assert (got[0].packed_rows > 0) == inside, f"{tag}: packed_rows = {got[0].packed_rows}"
        if inside:
            assert got[0].packed_rows >= L - W and got[0].persistent == 1, tag
            extra = {"b": [{"RAMX_PK_SEGMENT": "64"}], "d": [{"RAMX_TEST_PK_WRONG_EVERY": "3"}],
                     "c": [{"RAMX_PK_SEGMENT": "64", "RAMX_TEST_PK_WRONG_EVERY": "3"}]}.get(shape, [])
            for env in extra:
                x = _run_device(fs, p, peek, monkeypatch, **env)
                assert x[0].packed_rows >= L - W, (tag, env, x[0].packed_rows)
                if "RAMX_TEST_PK_WRONG_EVERY" in env:
                    # rows run ahead of the vote up to W = 40 only (W = 80: no registers for the second copy of the row; the hook then does nothing)
                    assert (x[0].respeculated_rows > 0) == (W <= 40), (tag, env, x[0].respeculated_rows)
                _assert_same_rows(x, ref, f"{tag} {env}")


# ---- fast band: int8 scores and (score << 4 | cell) keys --------------------------------------------------------------------
#
# The fast band is read (`pack_ok`) by the register-resident kernels only -- the int32 rows of the lane-per-flank kernel, the
# family kernel, the resident profile replay -- and all three are closed on the host when go + ge < -32768.  On a kernel that has a
# fast band mx = max(|go| + |ge|, |matrix|) is therefore at most 32,768, and the edge (L + 2W + 4) mx = 2^27 lies at
# L + 2W + 4 = 4096 or beyond: at W = 14 with go + ge = -32768, between L = 4063 and L = 4064.  A shorter direction cannot reach it.

def _system(P, mn, go, ge, W, L, **kw):
    return po.Params(bandwidth=W, cappenalty=-5 * max(P, mn), minimprovement=2 * P, L=L, when_to_stop=kw.pop("when_to_stop", 40), l=1,
                     gapopen=go, gapextn=ge, matrix=sg.shape_matrix(P, mn), **kw)


FAST_BAND = [      # (P, mn, go, ge, L, fast_pack_ok) at W = 14: 4095 x 32,768 < 2^27 = 4096 x 32,768
    (127, 128, -300, -20, 300, True), (128, 128, -300, -20, 300, False), (127, 129, -300, -20, 300, False),
    (127, 128, -32000, -768, 4063, True), (127, 128, -32000, -768, 4064, False),
]
FAMILY_KERNEL = {"RAMX_NO_CP": "1"}
INT32_ROWS = {"RAMX_NO_FAMILY_ROUTE": "1", "RAMX_NO_CP_DEVICE": "1", "RAMX_NO_PK": "1"}
ROUTES = [{}, FAMILY_KERNEL, {"RAMX_NO_FAMILY_ROUTE": "1"}, INT32_ROWS]


@pytest.fixture(scope="module")
def fast_band_families():
    """One family per length: 100 flanks x 300 columns (two tiles, the second partial), and -- for the product edge -- 70 flanks
    aligned over all of 4064 columns with an insertion or deletion every 500 bases or so: rare enough to be worth the 32,768 of
    a gap, so that the scores keep growing to the last row (some 400,000; the gate allows for 2^27)."""
    short = synth_family(100, 300, 14, K=200, seed=611, both_sides=True, minus_frac=0.3, n_run_frac=0.2)
    long = synth_family(70, 4064, 14, K=4100, seed=612, div=0.01, both_sides=True, minus_frac=0.3, n_run_frac=0.2)
    return {300: short, 4063: long, 4064: long}


@pytest.mark.parametrize("P,mn,go,ge,L,ok", FAST_BAND)
def test_fast_band_at_the_edges_of_its_gate(P, mn, go, ge, L, ok, fast_band_families, monkeypatch):
    """Matrix entries of exactly 127 and -128 (int8 tables) against 128 and -129; (L + 2W + 4) mx just under and at 2^27.
    The run info does not show this gate: exact results on both sides, on the default route, the family kernel, the device-wide
    route and the int32 rows, each with and without RAMX_NO_FASTPACK=1.  The run info does show that a kernel WITH a fast band
    ran: `persistent` on the family kernel and the int32 rows, and on every route where neither the cell-parallel kernel nor the
    packed rows take the system (the product edge)."""
    fs = fast_band_families[L]
    p = _system(P, mn, go, ge, 14, L, when_to_stop=40 if L == 300 else L)
    assert sg.fast_pack_ok(14, L, go, ge, p.matrix) == ok
    only_int32 = not sg.cp_value_range_ok(14, L, go, ge, p.matrix) and not sg.pk_plan(14, go, ge, p.matrix).admitted
    assert only_int32 == (L > 4000)
    ref = run_both_directions(oracle_extend, fs.cores, fs.sequence, p)
    assert ref[2].ret > L // 3 and ref[3].ret > L // 3            # the family does extend under this system
    if L > 4000:
        assert ref[2].rows_executed == L and ref[3].rows_executed == L
    for route in ROUTES:
        for nofast in (False, True):
            env = dict(route, **({"RAMX_NO_FASTPACK": "1"} if nofast else {}))
            _env(monkeypatch, **env)
            got = run_both_directions(gpu_extend, fs.cores, fs.sequence, p)
            tag = f"{(P, mn, go, ge, L)} {env}"
            assert_same_result(ref[0], ref[1], ref[2:], got[0], got[1], got[2:], tag)
            assert (ref[2].rows_executed, ref[3].rows_executed) == (got[2].rows_executed, got[3].rows_executed), tag
            if only_int32 or route in (FAMILY_KERNEL, INT32_ROWS):
                for r in got[2:]:
                    assert (r.persistent, r.lanes_per_flank, r.packed_rows) == (1, 1, 0), (tag, r)


@pytest.mark.parametrize("P,mn,go,ge,L,ok", FAST_BAND)
def test_profile_replay_at_the_edges_of_the_fast_band(P, mn, go, ge, L, ok, fast_band_families, monkeypatch):
    """The profile replay shares fast_pack_ok, and reads it in its register-resident kernel (W = 14 has one; go + ge >= -32768
    keeps it): both sides of the int8 edge and of the 2^27 edge through Device.profile, every column's total and every flank's
    kept row best and its cell against the oracle's, with and without the fast band."""
    from repeatafterme_amd.device import Device, resolve_flanks
    fs = fast_band_families[L]
    p = _system(P, mn, go, ge, 14, L, when_to_stop=L)
    assert sg.fast_pack_ok(14, L, go, ge, p.matrix) == ok and sg.go_ge_ok(go, ge)
    o = po.oracle_extend(1, fs.cores.copy(), fs.sequence, new_master(L), p, trace=True, row_trace=True)
    rows = o.rows_executed
    assert rows == L
    for nofast in (False, True):
        _env(monkeypatch, **({"RAMX_NO_FASTPACK": "1"} if nofast else {}))
        d = Device(0)
        try:
            d.load_library(np.ascontiguousarray(fs.sequence, np.int8))
            flanks, idx = resolve_flanks(1, fs.cores, 14, L)
            res = d.profile(flanks, to_extend_params(p), o.col_base[:rows], rows=rows, row_best=True)
        finally:
            d.close()
        nx = len(idx)
        assert np.array_equal(res.cols[0, :rows]["total"], o.col_sums[:rows]), nofast
        assert np.array_equal(res.row_best[:rows, :nx], o.row_best[:rows, idx]), nofast
        assert np.array_equal(res.row_best_idx[:rows, :nx], o.row_best_idx[:rows, idx]), nofast


# ---- cell-parallel kernel: int8 scores, (score << 8 | cell) keys, tilted block totals -------------------------------------------

CELL_PARALLEL = [  # (P, mn, go, ge, L, admitted) at W = 14: 279 x 30,000 < 2^23 <= 280 x 30,000; 200 x 41,943 < 2^23 <= 200 x 41,944
    (127, 128, -300, -20, 200, True), (128, 128, -300, -20, 200, False), (127, 129, -300, -20, 200, False),
    (5, 4, -29000, -1000, 247, True), (5, 4, -29000, -1000, 248, False),
    (5, 4, 0, -41943, 100, True), (5, 4, 0, -41944, 100, False),
]


@pytest.mark.parametrize("P,mn,go,ge,L,ok", CELL_PARALLEL)
def test_cell_parallel_at_the_edges_of_its_gate(P, mn, go, ge, L, ok, monkeypatch):
    """A family of 100 flanks on the default route: several lanes per flank inside the value-range gate, one lane per flank (or
    the streaming kernel) outside, exact results on both sides."""
    _env(monkeypatch)
    fs = synth_family(100, L, 14, K=L - 50, seed=733, both_sides=True, minus_frac=0.3, n_run_frac=0.2)
    p = _system(P, mn, go, ge, 14, L)
    assert sg.cp_value_range_ok(14, L, go, ge, p.matrix) == ok
    ref = run_both_directions(oracle_extend, fs.cores, fs.sequence, p)
    got = run_both_directions(gpu_extend, fs.cores, fs.sequence, p)
    tag = f"{(P, mn, go, ge, L)}"
    assert_same_result(ref[0], ref[1], ref[2:], got[0], got[1], got[2:], tag)
    assert (ref[2].rows_executed, ref[3].rows_executed) == (got[2].rows_executed, got[3].rows_executed), tag
    for r in got[2:]:
        if ok:
            assert r.lanes_per_flank > 1, (tag, r.lanes_per_flank, r.persistent)
        else:
            assert r.lanes_per_flank == 1 or r.persistent == 0, (tag, r.lanes_per_flank, r.persistent)


# ---- int32-row persistent kernel: e - m as int16 -------------------------------------------------------------------------------

@pytest.mark.parametrize("ge,ok", [(-768, True), (-769, False)])
def test_persistent_rows_at_the_go_ge_edge(ge, ok, monkeypatch):
    """go + ge = -32768 keeps the int32-row persistent kernel, -32769 leaves it for the streaming kernel; same exact results."""
    W, L = 14, 120
    fs = gate_family(200, L, W, seed=41, K=100, cut=(30, 110))
    p = _system(5, 4, -32000, ge, W, L, when_to_stop=L)
    assert sg.go_ge_ok(p.gapopen, p.gapextn) == ok and not sg.pk_plan(W, p.gapopen, p.gapextn, p.matrix).admitted
    got = _run_device(fs, p, (0, 1, 199), monkeypatch)
    assert got[0].persistent == (1 if ok else 0) and got[0].packed_rows == 0
    _assert_equals_oracle(got, fs, p, f"ge={ge}")
    ref = _run_device(fs, p, (0, 1, 199), monkeypatch, RAMX_NO_PERSISTENT="1")
    assert ref[0].persistent == 0
    _assert_same_rows(got, ref, f"ge={ge}")
