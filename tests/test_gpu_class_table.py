"""The 9 x 4 class table on every kernel route.  Every kernel scores a base through tab[class][candidate] -- A C G T a c g t N
against the four candidate bases -- and the library restates that table about ten times (the swizzled int16 pairs of the packed
rows, the int8 quadruples of the fast band, the int4 table of the cell-parallel kernel, the s_tab tables of the streaming, family,
profile and align kernels, the lower-case complement of the pack kernel, the N mask of the packed library form).  The built-in
scoring systems hold one constant in the rows of the classes 4..8, so no test on them can see those rows.  Here every route runs
the systems of tests/class_table.py, whose entries can be told apart, on families with a third of the bases soft-masked, N runs
and flanks that end inside the executed columns; every expected value is the oracle's on the family itself -- ret, rows, limit
warning, consensus, lengths and scores, all exactly -- and every case asserts the route it ran on from the run info.
tests/test_class_table_ref.py pins the oracle to the reference on these systems and shows on the CPU what these very (system,
family) pairs can see: every confusion of the table under `distinct` (and every change of one entry by one on the smallest family
of each band width), seven of the nine under `nocase` (the other two give back its matrix), the two N confusions under `n_pays`
and on the packed library form, which holds no lower case."""
import os
from functools import lru_cache

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import new_master
from repeatafterme_amd.synth import synth_family

import align_ref as ar
import class_table as ct
import wide_sums as ws
import window_cases as wc
import window_ref as wr
from helpers import gpu_extend, to_extend_params
from test_gpu_wide_sums import CELL_PARALLEL, FAMILY_KERNEL, INT32_ROWS, PACKED_ROWS, ROUTE_VARS, STREAMING, _env as _route_env

pytestmark = pytest.mark.gpu
MORE_VARS = ("RAMX_CP_SINGLE_MAX", "RAMX_TEST_CP_VOTE_DELAY", "RAMX_PK_CKPT", "RAMX_NO_PK_SPEC", "RAMX_CP_DEVICE_MAXN", "RAMX_NO_LEAN",
             "RAMX_LEADER_MAX", "RAMX_PK_NO_VW")
L, K = 96, 70
ORDINARY = ("distinct", "nocase", "n_pays")


def _env(monkeypatch, **env):
    for k in MORE_VARS:
        monkeypatch.delenv(k, raising=False)
    _route_env(monkeypatch, **env)
    assert not any(k in os.environ for k in ROUTE_VARS + MORE_VARS if k not in env)


def _tuple(info):
    return (info.persistent, info.lanes_per_flank, info.packed_rows, info.launches, info.lean_rows, info.respeculated_rows)


def _assert_direction(run, d, info, tag):
    o = run.direction(d)
    assert (info.ret, info.rows_executed, info.limit_warning) == (o.ret, o.rows_executed, o.limit_warning), (tag, info)
    assert info.overflow32 == 0, (tag, info)


def _assert_results(run, cores, master, tag):
    assert np.array_equal(master, run.master), f"{tag}: consensus differs at {np.nonzero(master != run.master)[0][:8]}"
    for k in ("right_len", "left_len", "score"):
        got, want = getattr(cores, k), getattr(run.cores, k)
        assert np.array_equal(got, want), f"{tag}: {k} differs in copies {np.nonzero(got != want)[0][:8]}"


def _run_case(name, n, W, monkeypatch, env, route):
    """The family (n, W) under the system `name` through extend_alignment, both directions, against the oracle's run of the
    same; route(info, run, d, tag) asserts the kernel route.  -> the run infos."""
    _env(monkeypatch, **env)
    run = ct.oracle_run(name, n, W)
    assert ct.gates(name, W, L) == ct.expected_gates(name, W)
    c, m = run.fs.cores.copy(), new_master(L)
    infos = []
    for d in (1, 0):
        tag = f"{name} {n} copies W={W} {env} direction {d}"
        info = gpu_extend(d, c, run.fs.sequence, m, run.p)
        print(tag, "->", _tuple(info))
        _assert_direction(run, d, info, tag)
        route(info, run, d, tag)
        infos.append(info)
    _assert_results(run, c, m, f"{name} {n} copies W={W} {env}")
    return infos


@pytest.fixture(scope="module", autouse=True)
def _expected_values_of_the_large_families():
    """The oracle's runs of the families of 720 copies and more, side by side rather than one after the other."""
    ct.warm([(name, 2016, W) for name in ORDINARY for W in (14, 80)] + [(name, 4032, W) for name, W in PACKED_CASES] +
            [(name, 720, W) for name in ("distinct", "nocase") for W in (14, 40)] + [("distinct_x11", 720, 14)], threads=12)
    yield


def _is(persistent, lanes, packed=False, one_launch=None):
    def route(info, run, d, tag):
        assert info.persistent == persistent and info.lanes_per_flank == lanes and (info.packed_rows > 0) == packed, (tag, _tuple(info))
        if one_launch is not None:
            assert (info.launches == 1) if one_launch else (info.launches >= info.rows_executed), (tag, info.launches)
    return route


# ---- one lane per flank, int32 rows -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,W", ct.GPU_FAMILIES["streaming"])
@pytest.mark.parametrize("name", ct.SYSTEMS)
def test_streaming_kernel(name, n, W, monkeypatch):
    """One launch per column (ramx_kernels_stream.h, its s_tab with the winner's column): W = 14 has a specialised kernel, W = 9
    has none.  A positive gap-open penalty takes this route whatever the switches say; scores eleven times as large leave int8."""
    env = {"RAMX_NO_FAMILY_ROUTE": "1"} if name == "distinct_go" else STREAMING
    _run_case(name, n, W, monkeypatch, env, _is(0, 1, one_launch=False))


@pytest.mark.parametrize("n,W", ct.GPU_FAMILIES["family kernel"])
@pytest.mark.parametrize("name", ORDINARY)
def test_family_kernel(name, n, W, monkeypatch):
    """One workgroup per family, one lane per flank, through extend_alignment's family route."""
    _run_case(name, n, W, monkeypatch, FAMILY_KERNEL, _is(1, 1, one_launch=True))


@pytest.mark.parametrize("W", [14, 80])
@pytest.mark.parametrize("name", ORDINARY)
def test_int32_row_persistent_kernel(name, W, monkeypatch):
    """One launch per direction, 2,016 copies in several workgroups: the fast band's int8 quadruples (fast_tabs_init,
    fast_tabs_winner of ramx_kernels_resident.h)."""
    _run_case(name, 2016, W, monkeypatch, INT32_ROWS, _is(1, 1, one_launch=True))


def test_refusal_of_scores_outside_int8(monkeypatch):
    """Nothing forced: `distinct` times eleven leaves int8, every narrow route must turn it away -- one lane per flank, no packed
    rows -- and the result is still the oracle's."""
    _env(monkeypatch)
    infos = _run_case("distinct_x11", 720, 14, monkeypatch, {}, lambda info, run, d, tag: None)
    for info in infos:
        assert info.lanes_per_flank == 1 and info.packed_rows == 0, _tuple(info)


# ---- batches ---------------------------------------------------------------------------------------------------------------------------

@lru_cache(maxsize=None)
def _ordinary(W, seed):
    return synth_family(40, L, W, K=L // 2, seed=seed, both_sides=True, minus_frac=0.3, n_run_frac=0.1)


@lru_cache(maxsize=None)
def _ordinary_run(name, W, seed):
    fs, p = _ordinary(W, seed), ct.system(name, W, L)
    return ct.Run(name, fs, p, *ct.run_oracle(fs, p))


def _batch_case(name, n, W, monkeypatch, env, want):
    """The soft-masked family between two ordinary ones (A C G T N only) in one extend_batch call, every family against its own
    oracle run; want(info, tag) asserts the middle family's route."""
    from repeatafterme_amd.extend import extend_batch
    _env(monkeypatch, **env)
    runs = [_ordinary_run(name, W, 4100), ct.oracle_run(name, n, W), _ordinary_run(name, W, 4101)]
    fams = [(r.fs.cores.copy(), r.fs.sequence, new_master(L)) for r in runs]
    for d in (1, 0):
        infos = extend_batch(d, fams, to_extend_params(runs[1].p))
        tag = f"batch {name} {n} copies W={W} {env} direction {d}"
        print(tag, "->", [_tuple(i) for i in infos])
        for r, i in zip(runs, infos):
            _assert_direction(r, d, i, tag)
        want(infos[1], tag)
    for r, (c, _, m), which in zip(runs, fams, ("first", "middle", "last")):
        _assert_results(r, c, m, f"batch {name} {n} copies W={W}: {which} family")


@pytest.mark.parametrize("W", [14, 40])
@pytest.mark.parametrize("name", ORDINARY)
def test_family_kernel_in_a_batch(name, W, monkeypatch):
    def want(info, tag):
        assert (info.persistent, info.lanes_per_flank, info.packed_rows) == (1, 1, 0), (tag, _tuple(info))
    _batch_case(name, 192, W, monkeypatch, FAMILY_KERNEL, want)


@pytest.mark.parametrize("n", [24, 288])
def test_streaming_family_kernel_in_a_batch(n, monkeypatch):
    """The batch's streaming kernel: W = 9 has no resident kernel."""
    def want(info, tag):
        assert (info.persistent, info.lanes_per_flank) == (2, 1), (tag, _tuple(info))
    _batch_case("distinct", n, 9, monkeypatch, {}, want)


# ---- the one-workgroup cell-parallel kernel ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [14, 20, 40, 80])
@pytest.mark.parametrize("name", ["distinct", "nocase"])
def test_cell_parallel_one_workgroup(name, W, monkeypatch):
    """24 copies alone stay in one workgroup with sixteen lanes per flank (ramx_kernels_cp.h and its int4 table)."""
    _run_case(name, 24, W, monkeypatch, {}, _is(1, 16, one_launch=True))


@pytest.mark.parametrize("lanes", [2, 4, 8])
@pytest.mark.parametrize("W", [14, 40, 80])
@pytest.mark.parametrize("name", ["distinct", "nocase"])
def test_cell_parallel_one_workgroup_every_lane_shape_in_a_batch(name, W, lanes, monkeypatch):
    """RAMX_CP_K caps the lanes per flank; 24 x 16 / K copies fill the workgroup the same way at every K.  W = 80 with two lanes
    would be blocks of 81 cells per lane, and the kernel has blocks of up to 41 (ramx_cp.hip cp_max_threads): that family must
    leave the cell-parallel kernel for the batch's streaming kernel -- asserted as such -- and still equal the oracle."""
    fits = (2 * W + 1 + lanes - 1) // lanes <= 41
    assert fits == ((W, lanes) != (80, 2))

    def want(info, tag):
        assert (info.persistent, info.lanes_per_flank, info.launches) == ((1, lanes, 1) if fits else (2, 1, 1)), (tag, _tuple(info))
    _batch_case(name, 24 * 16 // lanes, W, monkeypatch, {"RAMX_CP_K": str(lanes)}, want)


# ---- packed int16 rows --------------------------------------------------------------------------------------------------------------

def _packed(info, run, d, tag):
    r0 = ws.pk_first_row(d, run.fs.cores, run.p.bandwidth, L)
    assert info.persistent == 1 and info.lanes_per_flank == 1 and info.launches == 1, (tag, _tuple(info))
    assert info.packed_rows == info.rows_executed - r0 > 0, (tag, info.packed_rows, info.rows_executed, r0)


PACKED_ENVS = {"one launch": {"RAMX_PK_SEGMENT": "0"}, "pieces of 64 columns": {"RAMX_PK_SEGMENT": "64"},
               "every third guess wrong": {"RAMX_PK_SEGMENT": "0", "RAMX_TEST_PK_WRONG_EVERY": "3"}}
PACKED_CASES = [(name, W) for name in ("distinct", "nocase") for W in (14, 20, 40, 80)] + [("n_pays", 14)]


@pytest.mark.parametrize("how", sorted(PACKED_ENVS))
@pytest.mark.parametrize("name,W", PACKED_CASES)
def test_packed_rows(name, W, how, monkeypatch):
    """4,032 copies on the packed-row kernel (ramx_kernels_packed.h, pkb_tabs_init: 256 class-pair entries swizzled by
    lo ^ ((hi & 3) << 2), rotated by the winner in t4 and plain in tp): in one launch, in pieces of 64 columns, and with every
    third guess wrong (a rolled-back row is scored again through the winner's rotation)."""
    infos = _run_case(name, 4032, W, monkeypatch, dict(PACKED_ROWS, **PACKED_ENVS[how]), _packed)
    if how == "every third guess wrong":
        # rows run ahead of the vote up to W = 40 only (W = 80: no registers for the second copy of the row; the hook does nothing)
        assert all((i.respeculated_rows > 0) == (W <= 40) for i in infos), [_tuple(i) for i in infos]


@pytest.mark.parametrize("name,W", PACKED_CASES)
def test_packed_rows_final_dp_rows_equal_the_int32_rows(name, W, monkeypatch):
    """The final DP rows of the packed kernel, cell by cell, against a RAMX_NO_PK=1 run of the same direction."""
    from test_gpu_persistent import _run_device
    run = ct.oracle_run(name, 4032, W)
    for d in (1, 0):
        _env(monkeypatch, **dict(PACKED_ROWS, RAMX_PK_SEGMENT="0"))
        a = _run_device(run.fs, run.p, d, monkeypatch, True)
        _env(monkeypatch, **dict(PACKED_ROWS, RAMX_NO_PK="1"))
        b = _run_device(run.fs, run.p, d, monkeypatch, True)
        tag = f"{name} W={W} direction {d}"
        assert a[0].packed_rows > 0 and b[0].packed_rows == 0 and a[0].persistent == b[0].persistent == 1, tag
        o = run.direction(d)
        assert (a[0].ret, a[0].rows_executed, a[0].limit_warning) == (b[0].ret, b[0].rows_executed, b[0].limit_warning) == (o.ret, o.rows_executed, o.limit_warning), tag
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), tag
        for (ca, ha, pa), (cb, hb, pb) in zip(a[4], b[4]):
            assert np.array_equal(ca, cb) and (ha, pa) == (hb, pb), tag


def test_lean_band(monkeypatch):
    """The LEAN rows of the packed kernel read the plain table tp: hundreds of soft-masked columns at the cap, then a second copy
    with every other base soft-masked, which the flanks climb again (class_table.lean_family; the CPU module asserts its
    premises and that it sees all nine confusions).  Equal to the oracle, through extend_alignment in both directions and on the
    device session, and cell by cell to a run with RAMX_NO_LEAN=1."""
    from test_gpu_persistent import _run_device
    W, LL = ct.LEAN_W, ct.LEAN_L
    run = ct.lean_run()
    fs, p, o = run.fs, run.p, run.direction(1)
    assert ct.gates("distinct", W, LL) == ct.expected_gates("distinct", W)
    assert o.rows_executed == LL and o.ret > 300 + ct.LEAN_GAP          # the second copy is found again
    _env(monkeypatch, **PACKED_ROWS)
    c, m = fs.cores.copy(), new_master(LL)
    for d in (1, 0):                                                     # (one-sided: the left direction has no flank)
        info = gpu_extend(d, c, fs.sequence, m, p)
        print(f"LEAN family direction {d} ->", _tuple(info))
        _assert_direction(run, d, info, f"LEAN family direction {d}")
        if d:
            assert info.persistent == 1 and info.lanes_per_flank == 1 and info.lean_rows > 50 and info.packed_rows >= LL - W, _tuple(info)
    _assert_results(run, c, m, "LEAN family")
    lean = _run_device(fs, p, 1, monkeypatch, True)
    _env(monkeypatch, **dict(PACKED_ROWS, RAMX_NO_LEAN="1"))
    full = _run_device(fs, p, 1, monkeypatch, True)
    print("LEAN band ->", _tuple(lean[0]), "RAMX_NO_LEAN=1 ->", _tuple(full[0]))
    assert lean[0].persistent == 1 and lean[0].lanes_per_flank == 1
    assert lean[0].lean_rows > 50 and lean[0].packed_rows >= LL - W, _tuple(lean[0])
    assert full[0].lean_rows == 0 and full[0].packed_rows >= LL - W, _tuple(full[0])
    for x in (lean, full):
        assert (x[0].ret, x[0].rows_executed, x[0].limit_warning) == (o.ret, o.rows_executed, o.limit_warning)
        assert np.array_equal(x[1], run.master[LL + 1:LL + 1 + o.rows_executed])
        ext = (x[2] > 0) & (x[3] >= 0)                                # ram_extend.c:1234-1247
        assert np.array_equal(np.where(ext, x[3] + 1, 0), run.cores.right_len) and np.array_equal(np.where(ext, x[2], 0), run.cores.score)
    assert np.array_equal(lean[2], full[2]) and np.array_equal(lean[3], full[3])
    for (ca, ha, pa), (cb, hb, pb) in zip(lean[4], full[4]):
        assert np.array_equal(ca, cb) and (ha, pa) == (hb, pb)


# ---- the device-wide cell-parallel kernel ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,lanes", [(14, 16), (40, 16), (40, 2)], ids=["W14-K16-vote wave", "W40-K16-vote wave", "W40-K2-vote, then band"])
@pytest.mark.parametrize("name", ["distinct", "nocase"])
def test_cell_parallel_device_wide(name, W, lanes, monkeypatch):
    """720 copies over several workgroups (ramx_kernels_cp.h, device-wide mode) in both of its shapes."""
    infos = _run_case(name, 720, W, monkeypatch, dict(CELL_PARALLEL, RAMX_CP_K=str(lanes)), _is(1, lanes, one_launch=True))
    if lanes == 2:
        assert all(i.respeculated_rows == 0 for i in infos), [_tuple(i) for i in infos]      # nothing is computed on a guess


def test_cell_parallel_device_wide_every_third_guess_wrong(monkeypatch):
    infos = _run_case("distinct", 720, 14, monkeypatch, dict(CELL_PARALLEL, RAMX_TEST_CP_WRONG_EVERY="3"), _is(1, 16, one_launch=True))
    assert all(i.respeculated_rows > 0 for i in infos), [_tuple(i) for i in infos]


# ---- the packed library form ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", wc.LOOP_W)
@pytest.mark.parametrize("name", ["n_pays", "distinct"])
def test_packed_library_form(name, W, monkeypatch):
    """The packed form of the library carries N (a mask beside the two-bit payload, ramx_pack2_kernel) but no case: the loop on
    it equals the loop on the folded byte library and the oracle on the folded library, under a system that scores N by
    candidate.  Windows begin inside flanks; N runs cross word and window borders."""
    from repeatafterme_amd.device import Device
    from test_gpu_windows import _equals_oracle, _run, _same_run
    _env(monkeypatch)
    assert ct.gates(name, W, wc.loop_cases(W)[0].L) == ct.expected_gates(name, W)
    dev = Device(0)
    try:
        for c in wc.loop_cases(W):
            direction, idx, fs = (c.extra[k] for k in ("direction", "idx", "fs"))
            p = ct.system(name, W, c.L, when_to_stop=ct.LOOP_WHEN_TO_STOP)
            lib = np.ascontiguousarray(wr.fold(c.lib))
            assert (lib == 99).any() and not ((lib >= 4) & (lib < 8)).any() and ((c.lib >= 4) & (c.lib < 8)).any()
            tables = ct.windows_inside_n_runs(c)
            assert ct.n_runs_cross_borders(tables) == (True, True), c.name
            peek = range(len(c.descs)) if c.extra["seed"] == wc.SWEEP_SEEDS[0] else ()
            dev.load_library_packed(tables)
            a = _run(dev, c, p, peek)
            dev.load_library(lib)
            b = _run(dev, c, p, peek)
            _same_run(a, b, f"{name} {c.name}")
            # the device session's own choice of route: several lanes per flank where the band width has a cell-parallel kernel,
            # the streaming kernel at W = 0 -- and the same on both library forms
            print(f"{name} {c.name} -> packed form", _tuple(a[0]), "byte form", _tuple(b[0]))
            assert _tuple(a[0])[:3] == _tuple(b[0])[:3], c.name
            if W in (14, 40, 80):
                assert a[0].persistent == 1 and a[0].lanes_per_flank > 1 and a[0].packed_rows == 0, (c.name, _tuple(a[0]))
            else:
                assert a[0].persistent == 0 and a[0].lanes_per_flank == 1 and a[0].launches >= a[0].rows_executed, (c.name, _tuple(a[0]))
            o = _equals_oracle(a, direction, fs.cores, idx, lib, p, f"{name} {c.name}")
            assert o.rows_executed > 0
    finally:
        dev.close()


# ---- the replays ---------------------------------------------------------------------------------------------------------------------------

def _assert_replayed_run_route(info, W, tag):
    """The replays report no route of their own (one kernel each, chosen by the band width); the run of the direction beside them
    does: 130 copies on the default route take several lanes per flank at W = 14 and, W = 5 having no resident kernel, one of the
    streaming kernels."""
    if W == 14:
        assert info.persistent == 1 and info.lanes_per_flank > 1 and info.packed_rows == 0, (tag, _tuple(info))
    else:
        assert info.persistent in (0, 2) and info.lanes_per_flank == 1 and info.packed_rows == 0, (tag, _tuple(info))


@pytest.mark.parametrize("W", [14, 5], ids=["W14 fast band", "W5 general band"])
def test_profile_replay(W, monkeypatch):
    """ramx_dev_profile along the oracle's consensus (its own s_tab with the winner's column): every column's totals, base, score
    and cap counts, and every flank's kept row best and its cell."""
    from repeatafterme_amd.extend import extend_alignment
    from test_gpu_profile import check_against_oracle, gpu_rows
    _env(monkeypatch)
    fs, p = ct.family(130, W), ct.system("distinct", W, L)
    c_g, c_o, m_g, m_o = fs.cores.copy(), fs.cores.copy(), new_master(L), new_master(L)
    for d in (1, 0):
        tag = f"profile W={W} direction {d}"
        o = po.oracle_extend(d, c_o, fs.sequence, m_o, p, trace=True, row_trace=True)
        info, prof = extend_alignment(d, c_g, fs.sequence, m_g, to_extend_params(p), profile=True)
        assert (info.ret, info.rows_executed) == (o.ret, o.rows_executed) and prof.ret == o.ret, tag
        print(tag, "->", _tuple(info))
        _assert_replayed_run_route(info, W, tag)
        check_against_oracle(d, o, prof, o.rows_executed, p.cappenalty, tag)
        rows = o.rows_executed
        res, idx = gpu_rows(d, fs.cores, fs.sequence, p, o.col_base[:rows], rows)
        nx = len(idx)
        assert np.array_equal(idx, prof.core_index)
        assert np.array_equal(res.cols[0, :rows]["total"], o.col_sums[:rows]) and np.array_equal(res.cols[0, :rows]["base"], o.col_base[:rows]), tag
        assert np.array_equal(res.row_best[:rows, :nx], o.row_best[:rows, idx]), f"{tag}: row_best"
        assert np.array_equal(res.row_best_idx[:rows, :nx], o.row_best_idx[:rows, idx]), f"{tag}: row_best_idx"
    run = ct.oracle_run("distinct", 130, W)
    _assert_results(run, c_g, m_g, f"profile W={W}")


@pytest.mark.parametrize("W", [14, 5], ids=["W14 fast band", "W5 general band"])
def test_alignment_replay(W, monkeypatch):
    """ramx_dev_align along the oracle's consensus against the CPU walker, whose paths rescore to their own scores through
    matrix[cons][base] per matched column -- the class table read a third way."""
    from repeatafterme_amd.device import Device, resolve_flanks
    from test_gpu_align import check_against_walker
    _env(monkeypatch)
    fs, p = ct.family(130, W), ct.system("distinct", W, L)
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    c_o, m_o = fs.cores.copy(), new_master(L)
    seen = dict(aligned=0, n_ins=0, n_del=0)
    dev = Device(0)
    try:
        dev.load_library(seq)
        for d in (1, 0):
            tag = f"align W={W} direction {d}"
            before = c_o.copy()
            o = po.oracle_extend(d, c_o, seq, m_o, p, trace=True)
            cons = o.col_base[:o.ret]
            widx, results = ar.walk_family(d, before, seq, p, cons)
            lower_matched = 0
            for n, res in zip(widx, results):
                if res["end_row"] >= 0:
                    flank = ar.Flank(d, before, n, W)
                    assert ar.rescore(res, flank, seq, p, cons) == res["score"], (tag, n)
                    lower_matched += sum(1 for op in res["ops"] if op[0] == "M" and 4 <= flank.base(op[2], seq) < 8)
            assert lower_matched > 100, (tag, lower_matched)
            flanks, fidx = resolve_flanks(d, before, W, L)
            assert list(fidx) == widx
            # the loop's own run of the direction beside the replay: its trimmed high score and position are the end cell
            dev.begin_direction(flanks, to_extend_params(p))
            info = dev.run_direction()
            g_cons, th, tp = dev.download()
            print(tag, "->", _tuple(info))
            _assert_replayed_run_route(info, W, tag)
            assert (info.ret, info.rows_executed, info.limit_warning) == (o.ret, o.rows_executed, o.limit_warning), tag
            assert np.array_equal(g_cons[:o.rows_executed], o.col_base[:o.rows_executed]), tag
            res = dev.align(flanks, to_extend_params(p), cons, rows=o.ret)
            nx = len(fidx)
            has = res.ends["end_row"][:nx] >= 0
            assert np.array_equal(has, th > 0), tag
            assert np.array_equal(res.ends["score"][:nx][has], th[has]) and np.array_equal(res.ends["end_idx"][:nx][has], tp[has]), tag
            got = check_against_walker(res.ends[:nx], res.col_idx[:, :nx], res.col_ins[:, :nx], results, o.ret, tag)
            for k in seen:
                seen[k] += got[k]
    finally:
        dev.close()
    assert seen["aligned"] > 0 and seen["n_ins"] > 0 and seen["n_del"] > 0, seen
