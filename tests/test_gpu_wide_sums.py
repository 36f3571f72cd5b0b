"""Column sums past 2^31 on every kernel route.  The reference keeps the four sums of a row in `int`; the library keeps them in int64
and reports in `overflow32` that the reference would have wrapped.  What it must compute there comes from
tests/wide_sums.py: a small family's oracle run, repeated r times -- same return value, rows and consensus, the per-copy results
tiled, `overflow32` exactly when r * max(S[:rows_executed]) > 2^31 - 1.  Every case runs both directions, on both sides of the
edge of either direction (r_lo, r_lo + 1) and with the first wide sum early in the direction, so that most votes, the new maxima
and the stop decision happen above 2^31; every case asserts the route it ran on from the run info.  tests/test_wide_sums_ref.py
pins the premises on the CPU."""
import os
import sys

import numpy as np
import pytest

from repeatafterme_amd.datamodel import new_master

import wide_sums as ws
from helpers import gpu_extend, to_extend_params
from wide_sums import INT32_MAX, check_premises, replicate, small_run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROUTE_VARS = ("RAMX_NO_FAMILY_ROUTE", "RAMX_NO_CP_DEVICE", "RAMX_NO_CP", "RAMX_PROFILE_NO_RESIDENT", "RAMX_NO_PK", "RAMX_NO_FASTPACK",
              "RAMX_NO_PERSISTENT", "RAMX_PK_SEGMENT", "RAMX_TEST_PK_WRONG_EVERY", "RAMX_CP_K", "RAMX_TEST_CP_WRONG_EVERY", "RAMX_PEER_KIND")
STREAMING = {"RAMX_NO_PERSISTENT": "1", "RAMX_NO_FAMILY_ROUTE": "1"}
INT32_ROWS = {"RAMX_NO_FAMILY_ROUTE": "1", "RAMX_NO_CP_DEVICE": "1", "RAMX_NO_PK": "1"}
FAMILY_KERNEL = {"RAMX_NO_CP": "1"}
PACKED_ROWS = {"RAMX_NO_FAMILY_ROUTE": "1", "RAMX_NO_CP_DEVICE": "1"}
CELL_PARALLEL = {"RAMX_NO_FAMILY_ROUTE": "1", "RAMX_CP_K": "16"}      # (the hook also lifts the preference for the packed rows)


def _env(monkeypatch, **env):
    for k in ROUTE_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _assert_direction(run, d, r, info, tag):
    """One direction of the family repeated r times against the small oracle run; -> the first row above int32 (None: none)."""
    o = run.direction(d)
    first = check_premises(run, d, r)
    assert (info.ret, info.rows_executed, info.limit_warning) == (o.ret, o.rows_executed, o.limit_warning), (tag, info)
    assert info.overflow32 == run.overflows(d, r) == (first is not None), (tag, info.overflow32, r * run.top(d))
    assert info.n_extendable == r * run.cfg.m, tag
    return first


def _assert_results(run, r, cores, master, tag):
    assert np.array_equal(master, run.master), f"{tag}: consensus differs at {np.nonzero(master != run.master)[0][:8]}"
    for k in ("right_len", "left_len", "score"):
        assert np.array_equal(getattr(cores, k), np.tile(getattr(run.cores, k), r)), f"{tag}: {k}"


def _run_case(name, monkeypatch, env, route, reps=None):
    """The configuration `name` through extend_alignment at every replication; route(info, run, d) asserts the kernel route.
    -> per replication and direction, (r, d, the first wide row, the run info)."""
    _env(monkeypatch, **env)
    run = small_run(name)
    cfg = run.cfg
    seen = []
    for r in (reps or run.replications()):
        p = ws.params(cfg, r)
        c, m = replicate(run.fs.cores, r), new_master(cfg.L)
        for d in run.directions:
            tag = f"{name} {env} r={r} ({c.n} copies) direction {d}"
            info = gpu_extend(d, c, run.fs.sequence, m, p)
            first = _assert_direction(run, d, r, info, tag)
            route(info, run, d, tag)
            seen.append((r, d, first, info))
        _assert_results(run, r, c, m, f"{name} {env} r={r}")
    for d in run.directions:                   # both sides of the edge, and a direction that is mostly above it
        mine = [f for (_, dd, f, _) in seen if dd == d]
        rows = run.direction(d).rows_executed
        assert None in mine and any(f is not None and f < cfg.deep_at * rows for f in mine), (name, d, mine)
    return seen


def _is(persistent, lanes_one, packed=False):
    def route(info, run, d, tag):
        assert info.persistent == persistent, (tag, info)
        assert (info.lanes_per_flank == 1) == lanes_one, (tag, info)
        assert (info.packed_rows > 0) == packed, (tag, info)
    return route


# ---- one lane per flank, int32 rows -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["stream14", "stream9"])
def test_streaming_kernel(name, monkeypatch):
    """One launch per column, the sums folded and the stop rule applied by the next column's kernel (ramx_kernels_stream.h): the band
    width with a specialised kernel and one without."""
    seen = _run_case(name, monkeypatch, STREAMING, _is(0, True))
    assert all(info.launches >= info.rows_executed for (_, _, _, info) in seen)


@pytest.mark.parametrize("name", ["rows14", "rows80"])
def test_int32_row_persistent_kernel(name, monkeypatch):
    """One launch per direction, the vote through the ticketed 64-bit words (ramx_kernels_resident.h, ramx_kernels_vote.h)."""
    seen = _run_case(name, monkeypatch, INT32_ROWS, _is(1, True))
    assert all(info.launches == 1 for (_, _, _, info) in seen)


def test_family_kernel(monkeypatch):
    """One workgroup per family (up to 512 copies), reached through extend_alignment's family route."""
    _run_case("family14", monkeypatch, FAMILY_KERNEL, _is(1, True))


def test_family_kernel_batch_seam(monkeypatch):
    """Three families in one extend_batch call, only the middle one above 2^31: `overflow32` is per family, the neighbours report 0
    and equal their own small runs."""
    from repeatafterme_amd.extend import extend_batch
    _env(monkeypatch, **FAMILY_KERNEL)
    names = (ws.BATCH_NEIGHBOURS[0], ws.BATCH_MIDDLE, ws.BATCH_NEIGHBOURS[1])
    runs = [small_run(n) for n in names]
    assert len({(x.cfg.W, x.cfg.L, x.cfg.q, x.cfg.stop, x.cfg.P, x.cfg.mn, x.cfg.go, x.cfg.ge) for x in runs}) == 1     # one parameter set
    crossed = set()
    for r in runs[1].replications():
        p = to_extend_params(ws.params(runs[1].cfg, r))
        fams = [(replicate(x.fs.cores, r), x.fs.sequence, new_master(x.cfg.L)) for x in runs]
        for d in (1, 0):
            infos = extend_batch(d, fams, p)
            for x, info, nm in zip(runs, infos, names):
                _assert_direction(x, d, r, info, f"batch {nm} r={r} direction {d}")
                assert (info.persistent, info.lanes_per_flank, info.packed_rows) == (1, 1, 0), (nm, info)
            assert infos[0].overflow32 == 0 and infos[2].overflow32 == 0
            crossed.add(infos[1].overflow32)
        for x, (c, _, m), nm in zip(runs, fams, names):
            _assert_results(x, r, c, m, f"batch {nm} r={r}")
    assert crossed == {0, 1}


# ---- packed int16 rows ---------------------------------------------------------------------------------------------------------

def _packed(info, run, d, tag):
    cfg = run.cfg
    r0 = ws.pk_first_row(d, run.fs.cores, cfg.W, cfg.L)
    assert info.persistent == 1 and info.lanes_per_flank == 1, (tag, info)
    assert info.packed_rows == info.rows_executed - r0 and info.packed_rows >= cfg.L - cfg.W, (tag, info.packed_rows, r0)


@pytest.mark.parametrize("env", [{"RAMX_PK_SEGMENT": "0"}, {"RAMX_PK_SEGMENT": "64"}, {"RAMX_PK_SEGMENT": "0", "RAMX_TEST_PK_WRONG_EVERY": "3"}],
                         ids=["one launch", "pieces of 64 columns", "every third guess wrong"])
def test_packed_rows(env, monkeypatch):
    """The packed-row kernel keeps the stop rule's maximum as two 32-bit words (pkb_stop_rule): in one launch; in pieces of 64
    columns, the maximum handed from piece to piece above 2^31 (the first wide row lies some 1,400 rows before the stop row); and
    with every third guess wrong, so that rows are rolled back while the sums are wide."""
    seen = _run_case("packed14", monkeypatch, dict(PACKED_ROWS, **env), _packed)
    if env["RAMX_PK_SEGMENT"] == "64":
        assert any(f is not None and f + 10 * 64 < info.rows_executed for (_, _, f, info) in seen)
    if "RAMX_TEST_PK_WRONG_EVERY" in env:
        assert all(info.respeculated_rows > 0 for (_, _, _, info) in seen)


def test_packed_rows_behind_the_int32_kernel(monkeypatch):
    """Cores of ten bases: the first rows have out-of-bounds cells at the low end of the band and run on the int32 kernel, which
    hands its stop-rule state to the packed one (pk_r0 > 0)."""
    run = small_run("packed14_short")
    assert ws.pk_first_row(1, run.fs.cores, run.cfg.W, run.cfg.L) > 0
    _run_case("packed14_short", monkeypatch, PACKED_ROWS, _packed)


# ---- several lanes per flank ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wrong", [None, "3"], ids=["plain", "every third guess wrong"])
def test_cell_parallel_device_wide(wrong, monkeypatch):
    """The device-wide cell-parallel kernel splits every sum into halves that it compares unsigned (ramx_kernels_cp.h); int8 scores,
    so the edge takes some 10,000 copies x 2,000 columns.  (The one-workgroup kernel cannot reach it: tests/test_wide_sums_ref.py.)"""
    env = dict(CELL_PARALLEL, **({"RAMX_TEST_CP_WRONG_EVERY": wrong} if wrong else {}))

    def route(info, run, d, tag):
        assert info.persistent == 1 and info.lanes_per_flank > 1 and info.packed_rows == 0, (tag, info)
    seen = _run_case("cells40", monkeypatch, env, route)
    if wrong:
        assert all(info.respeculated_rows > 0 for (_, _, _, info) in seen if info.lanes_per_flank >= 4)    # (two lanes: vote, then band)


# ---- two ranks ------------------------------------------------------------------------------------------------------------------

def _rank(rank, world, port, out, name, r):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from repeatafterme_amd.device import Device
    from repeatafterme_amd.sharded import extend_alignment_sharded, gpu_engine

    def allreduce4(v):
        t = torch.tensor(v, dtype=torch.int64)
        dist.all_reduce(t)
        return t.tolist()

    def all_gather(x):
        outs = [torch.zeros(len(x), dtype=torch.int32) for _ in range(world)]      # (equal shards)
        dist.all_gather(outs, torch.from_numpy(np.ascontiguousarray(x, np.int32)))
        return np.concatenate([o.numpy() for o in outs])

    def ag_bytes(b):
        lst = [None] * world
        dist.all_gather_object(lst, b)
        return lst

    def ar_min(v):
        t = torch.tensor([v]); dist.all_reduce(t, op=dist.ReduceOp.MIN); return int(t.item())

    cfg = ws.CONFIGS[name]
    fs = ws.family(cfg)
    os.environ["RAMX_PEER_KIND"] = "device"
    os.environ["RAMX_NO_CP_DEVICE"] = "1"
    dev = Device(0)
    dev.set_allreduce_callback(allreduce4)
    enabled = dev.peer_setup(rank, world, ag_bytes, ar_min, dist.barrier) and dev.peer_kind == "device"
    dev.load_library(fs.sequence)
    c, m = replicate(fs.cores, r), new_master(cfg.L)
    rets, infos = [], []
    for d in (1, 0):
        rets.append(extend_alignment_sharded(d, c, fs.sequence, m, to_extend_params(ws.params(cfg, r)), rank, world, gpu_engine(dev), all_gather))
        i = dev.last
        infos.append((i.limit_warning, i.overflow32, i.n_extendable, i.persistent, i.lanes_per_flank, i.packed_rows))
    dev.close()
    out[rank] = (rets, infos, m.copy(), c.left_len.copy(), c.right_len.copy(), c.score.copy(), enabled)
    dist.destroy_process_group()


def test_two_ranks_cross_in_the_exchanged_totals():
    """Two ranks with half of the copies each, the votes exchanged through the mailboxes from inside the persistent kernel: with
    2 r_lo repetitions neither rank's own sums leave int32, the totals do -- in most rows of both directions."""
    import torch.multiprocessing as mp
    from test_gpu_sharded import _free_port
    name, world = "rows14", 2
    run = small_run(name)
    r = 2 * min(ws.edge_replications(run.S(d), run.direction(d).rows_executed)[0] for d in (1, 0))
    for d in (1, 0):
        first = check_premises(run, d, r)
        assert (r // 2) * run.top(d) <= INT32_MAX < r * run.top(d)              # (contiguous halves: r / 2 whole repetitions each)
        assert first is not None and first < 0.6 * run.direction(d).rows_executed
    out = mp.Manager().dict()
    mp.spawn(_rank, args=(world, _free_port(), out, name, r), nprocs=world, join=True)
    for rank in range(world):
        rets, infos, m, ll, rl, sc, enabled = out[rank]
        assert enabled, "peer self-test failed"
        for k, d in enumerate((1, 0)):
            o = run.direction(d)
            assert rets[k] == (o.ret, o.rows_executed), (rank, d)
            assert infos[k] == (o.limit_warning, 1, run.cfg.m * r // world, 1, 1, 0), (rank, d, infos[k])
        assert np.array_equal(m, run.master)
        for got, k in ((ll, "left_len"), (rl, "right_len"), (sc, "score")):
            assert np.array_equal(got, np.tile(getattr(run.cores, k), r)), (rank, k)


# ---- profile replay -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("resident", [True, False], ids=["resident", "rows through memory"])
@pytest.mark.parametrize("name", ["profile14", "rows80"])
def test_profile_replay_totals(name, resident, monkeypatch):
    """Device.profile on the repeated family along the small run's consensus: every column's four totals are r * S exactly, most
    of them above 2^31.  profile14 has 300 columns: the sum kernel's second block of 256 rows starts above the first wide row."""
    from repeatafterme_amd.device import Device, resolve_flanks
    _env(monkeypatch, **({} if resident else {"RAMX_PROFILE_NO_RESIDENT": "1"}))
    run = small_run(name)
    cfg = run.cfg
    dev = Device(0)
    try:
        dev.load_library(np.ascontiguousarray(run.fs.sequence, np.int8))
        for r in run.replications():
            big = replicate(run.fs.cores, r)
            for d in (1, 0):
                o = run.direction(d)
                rows = o.rows_executed
                first = check_premises(run, d, r)
                flanks, idx = resolve_flanks(d, big, cfg.W, cfg.L)
                assert len(idx) == big.n
                res = dev.profile(flanks, to_extend_params(ws.params(cfg, r)), o.col_base[:rows], rows=rows)
                want = r * o.col_sums[:rows]
                assert (want.max() > INT32_MAX) == (first is not None)
                assert np.array_equal(res.cols[0, :rows]["total"], want), (name, r, d, np.nonzero(res.cols[0, :rows]["total"] != want)[0][:8])
                assert np.array_equal(res.cols[0, :rows]["base"], o.col_base[:rows])
                if name == "profile14" and r == max(run.replications()):
                    assert rows > 256 and first < 128 and want[256:].max() > INT32_MAX
    finally:
        dev.close()
