"""The vote's tie rule and the stop rule's equality on every kernel route.  A tie at the top of the four candidate sums goes to
the lowest base (ram_extend.c:1081-1085, a strict `>`), and curr == max_ext + dist * minimprovement is a new maximum (:1194-1196,
a `>=`); the library restates the vote some eight times and the stop rule about as often, twice on 32-bit halves, and random
families of 64 copies or more never tie.  tests/decision_edges.py plants 24-copy families on both edges and carries them to any
size by repetition; what every route must compute comes from the 24-copy oracle run through that identity -- ret, rows, limit
warning, consensus and the per-copy results, all exactly -- and every case asserts the route it ran on from the run info.  Both
orders of the copies: tiled (every workgroup sees the tie) and in blocks (np.repeat: the first workgroups hold the group with the
higher base of every two-way tie, so their own argmax is the loser while the last workgroups guess the winner -- one column in
which some workgroups confirm their row and others roll back, without any test hook).  tests/test_decision_edges_ref.py pins the
premises on the CPU."""
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import new_master
from repeatafterme_amd.synth import synth_family

import decision_edges as de
from decision_edges import M, ORDERS, check_premises, small_run
from helpers import gpu_extend, to_extend_params
from test_gpu_wide_sums import CELL_PARALLEL, FAMILY_KERNEL, INT32_ROWS, PACKED_ROWS, ROUTE_VARS, STREAMING, _env as _route_env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MORE_VARS = ("RAMX_CP_SINGLE_MAX", "RAMX_TEST_CP_VOTE_DELAY", "RAMX_PK_CKPT", "RAMX_NO_PK_SPEC", "RAMX_CP_DEVICE_MAXN")


def _env(monkeypatch, **env):
    for k in MORE_VARS:
        monkeypatch.delenv(k, raising=False)
    _route_env(monkeypatch, **env)
    assert not any(k in os.environ for k in ROUTE_VARS + MORE_VARS if k not in env)


def _assert_direction(run, d, r, info, tag):
    o = run.direction(d)
    check_premises(run, d)
    assert (info.ret, info.rows_executed, info.limit_warning) == (o.ret, o.rows_executed, o.limit_warning), (tag, info)
    assert info.overflow32 == 0 and info.n_extendable == r * M, (tag, info)


def _assert_results(run, r, order, cores, master, tag):
    assert np.array_equal(master, run.master), f"{tag}: consensus differs at {np.nonzero(master != run.master)[0][:8]}"
    for k in ("right_len", "left_len", "score"):
        assert np.array_equal(getattr(cores, k), ORDERS[order][1](getattr(run.cores, k), r)), f"{tag}: {k}"


def _run_case(name, monkeypatch, env, r, order, route):
    """The case `name` repeated r times in `order` through extend_alignment, both directions (right only for a one-sided case)
    against the 24-copy oracle run; route(info, run, d, tag) asserts the kernel route.  -> the run infos."""
    _env(monkeypatch, **env)
    run = small_run(name)
    case = run.case
    assert r <= case.r_max
    p = de.case_params(case, r)
    c, m = ORDERS[order][0](run.fs.cores, r), new_master(case.L)
    infos = []
    for d in run.directions:
        tag = f"{name} {env} r={r} {order} ({c.n} copies) direction {d}"
        de.assert_device_order(d, run.fs.cores, c, r, order, case.W, case.L)
        info = gpu_extend(d, c, run.fs.sequence, m, p)
        print(tag, "->", (info.persistent, info.lanes_per_flank, info.packed_rows, info.launches, info.respeculated_rows))
        _assert_direction(run, d, r, info, tag)
        route(info, run, d, tag)
        infos.append(info)
    _assert_results(run, r, order, c, m, f"{name} {env} r={r} {order}")
    return infos


def _is(persistent, lanes, packed=False, one_launch=None):
    def route(info, run, d, tag):
        assert info.persistent == persistent and info.lanes_per_flank == lanes and (info.packed_rows > 0) == packed, (tag, info)
        if one_launch is not None:
            assert (info.launches == 1) if one_launch else (info.launches >= info.rows_executed), (tag, info.launches)
    return route


def _has_two_way_ties(name):
    """Every direction of the case has a tie between two bases: in the block order the copies of the first half then carry the loser."""
    run = small_run(name)
    return all(any(len(t) == 2 for _, t in de.top_ties(run.direction(d).col_sums, run.direction(d).rows_executed)) for d in run.directions)


TIES_AND_EQUALITIES = ["rs14", "m14", "eq_rs", "eq_m14", "plateau", "place14"]


# ---- one lane per flank, int32 rows ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r,order", [(1, "tile"), (12, "tile"), (12, "blocks")])
@pytest.mark.parametrize("name", ["rs14", "rs9", "rs14_gap", "eq_rs", "eq_m14", "plateau"])
def test_streaming_kernel(name, r, order, monkeypatch):
    """One launch per column (ramx_kernels_stream.h): a band width with a specialised kernel, one without, and a positive gap-open
    penalty, which takes this route whatever the switches say; 24 and 288 copies."""
    env = {"RAMX_NO_FAMILY_ROUTE": "1"} if name == "rs14_gap" else STREAMING
    _run_case(name, monkeypatch, env, r, order, _is(0, 1, one_launch=False))


@pytest.mark.parametrize("name", TIES_AND_EQUALITIES + ["m40", "place40"])
def test_family_kernel(name, monkeypatch):
    """One workgroup per family, one lane per flank, through extend_alignment's family route: 24 copies and 192 in blocks."""
    _run_case(name, monkeypatch, FAMILY_KERNEL, 1, "tile", _is(1, 1, one_launch=True))
    _run_case(name, monkeypatch, FAMILY_KERNEL, 8, "blocks", _is(1, 1, one_launch=True))


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("name", TIES_AND_EQUALITIES + ["m80"])
def test_int32_row_persistent_kernel(name, order, monkeypatch):
    """One launch per direction, 2,016 copies in several workgroups, the vote through the ticketed 64-bit words
    (ramx_kernels_resident.h, ramx_kernels_vote.h)."""
    _run_case(name, monkeypatch, INT32_ROWS, 84, order, _is(1, 1, one_launch=True))


# ---- the one-workgroup cell-parallel kernel ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", TIES_AND_EQUALITIES + ["m40", "m80", "place40"])
def test_cell_parallel_one_workgroup(name, monkeypatch):
    """24 copies alone stay in one workgroup with sixteen lanes per flank (ramx_kernels_cp.h: the argmax4_lds / argmax4_lanes
    guesses and the block-local vote)."""
    _run_case(name, monkeypatch, {}, 1, "tile", _is(1, 16, one_launch=True))


@lru_cache(maxsize=None)
def _ordinary(W, L, seed):
    return synth_family(40, L, W, K=L // 2, seed=seed, both_sides=True, minus_frac=0.3, n_run_frac=0.1)


def _batch_case(name, monkeypatch, env, r, order, want):
    """The tie family between two ordinary ones in one extend_batch call: the tie family against the 24-copy oracle run, the
    neighbours against their own oracle runs; want(info) asserts the tie family's route."""
    from repeatafterme_amd.extend import extend_batch
    _env(monkeypatch, **env)
    run = small_run(name)
    case = run.case
    p = de.case_params(case, r)
    sides = [_ordinary(case.W, case.L, 4100), _ordinary(case.W, case.L, 4101)]
    expect = []
    for fs in sides:
        c, m = fs.cores.copy(), po.new_master(case.L)
        expect.append(([po.oracle_extend(d, c, fs.sequence, m, p) for d in (1, 0)], c, m))
    big = ORDERS[order][0](run.fs.cores, r)
    fams = [(sides[0].cores.copy(), sides[0].sequence, new_master(case.L)), (big, run.fs.sequence, new_master(case.L)),
            (sides[1].cores.copy(), sides[1].sequence, new_master(case.L))]
    for k, d in enumerate((1, 0)):
        infos = extend_batch(d, fams, to_extend_params(p))
        tag = f"batch {name} {env} r={r} {order} direction {d}"
        print(tag, "->", [(i.persistent, i.lanes_per_flank, i.launches) for i in infos])
        _assert_direction(run, d, r, infos[1], tag)
        want(infos[1], tag)
        for i, (os_, _, _) in zip((infos[0], infos[2]), expect):
            assert (i.ret, i.rows_executed, i.limit_warning) == (os_[k].ret, os_[k].rows_executed, os_[k].limit_warning), tag
    _assert_results(run, r, order, fams[1][0], fams[1][2], f"batch {name}")
    for (c, _, m), (_, ec, em) in zip((fams[0], fams[2]), expect):
        assert np.array_equal(m, em) and np.array_equal(c.left_len, ec.left_len) and np.array_equal(c.right_len, ec.right_len)
        assert np.array_equal(c.score, ec.score)


@pytest.mark.parametrize("K", [2, 4, 8, 16])
@pytest.mark.parametrize("name", ["rs14", "m40", "eq_rs", "plateau"])
def test_cell_parallel_one_workgroup_every_lane_shape_in_a_batch(name, K, monkeypatch):
    """RAMX_CP_K caps the lanes per flank; 24 x 16 / K copies in blocks fill the workgroup the same way at every K."""
    def want(info, tag):
        assert (info.persistent, info.lanes_per_flank, info.launches) == (1, K, 1), (tag, info)
    _batch_case(name, monkeypatch, {"RAMX_CP_K": str(K)}, 16 // K, "blocks", want)


@pytest.mark.parametrize("name", ["rs14", "eq_m14", "place40"])
def test_family_kernel_in_a_batch(name, monkeypatch):
    def want(info, tag):
        assert (info.persistent, info.lanes_per_flank) == (1, 1), (tag, info)
    _batch_case(name, monkeypatch, FAMILY_KERNEL, 8, "blocks", want)


@pytest.mark.parametrize("name", ["rs9", "rs14_gap"])
def test_streaming_family_kernel_in_a_batch(name, monkeypatch):
    """The batch's streaming kernel: a band width without a resident kernel, and a positive gap-open penalty."""
    def want(info, tag):
        assert (info.persistent, info.lanes_per_flank) == (2, 1), (tag, info)
    _batch_case(name, monkeypatch, {}, 8, "blocks", want)


# ---- packed int16 rows ---------------------------------------------------------------------------------------------------------

def _packed(info, run, d, tag):
    r0 = de.pk_first_row(d, run.fs.cores, run.case.W, run.case.L)
    assert info.persistent == 1 and info.lanes_per_flank == 1, (tag, info)
    assert info.packed_rows == info.rows_executed - r0 > 0, (tag, info.packed_rows, r0)
    # one persistent direction, in one piece or in several: the library reports `launches = 1` for every direction that does not
    # go column by column (ramx_dev_run_direction), so the run info cannot tell a direction in pieces from one launch
    assert info.launches == 1, (tag, info.launches)


PACKED_ENVS = {"one launch": {"RAMX_PK_SEGMENT": "0"}, "pieces of 64 columns": {"RAMX_PK_SEGMENT": "64"},
               "every third guess wrong": {"RAMX_PK_SEGMENT": "0", "RAMX_TEST_PK_WRONG_EVERY": "3"}}


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("how", sorted(PACKED_ENVS))
@pytest.mark.parametrize("name", ["rs14", "m14", "place14", "place40", "handover14", "eq_rs", "eq_m14", "plateau"])
def test_packed_rows(name, how, order, monkeypatch):
    """4,032 copies on the packed-row kernel (ramx_kernels_packed.h: the decision word, the guess from the workgroup's totals, the
    stop rule on two 32-bit words): in one launch; in pieces of 64 columns (place14 / place40 tie in rows 63 and 64); with the
    forced wrong guesses on top.  handover14: the int32 kernel runs rows 0-3, both sides of the hand-over are tie rows.  In the
    block order the tie columns make some workgroups guess wrong and others right with no hook set."""
    infos = _run_case(name, monkeypatch, dict(PACKED_ROWS, **PACKED_ENVS[how]), 168, order, _packed)
    if name == "handover14":
        assert infos[0].packed_rows == infos[0].rows_executed - de.HANDOVER_ROW
    if (order == "blocks" and _has_two_way_ties(name)) or how == "every third guess wrong":
        assert all(i.respeculated_rows > 0 for i in infos), [(i.respeculated_rows, i.rows_executed) for i in infos]


# ---- the device-wide cell-parallel kernel ---------------------------------------------------------------------------------------

# (case, RAMX_CP_K = lanes per flank, vote wave).  Blocks of up to 21 cells per lane: the band waves run ahead on the workgroup's own
# guess and a vote wave confirms it; longer blocks (41 cells: W = 40 with two lanes, W = 80 with four): every workgroup votes,
# then computes its band.
CP_DEVICE_WIDE = [(n, 16, True) for n in ("rs14", "m40", "m80", "place40", "eq_rs", "eq_rs40", "eq_m14", "plateau")] + \
                 [(n, 2, True) for n in ("rs14", "eq_rs", "plateau")] + \
                 [("m40", 2, False), ("place40", 2, False), ("eq_rs40", 2, False), ("m80", 4, False)]


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("name,K,vote_wave", CP_DEVICE_WIDE, ids=[f"{n}-K{k}-{'vote wave' if v else 'vote, then band'}" for n, k, v in CP_DEVICE_WIDE])
def test_cell_parallel_device_wide(name, K, vote_wave, order, monkeypatch):
    """720 copies over several workgroups (ramx_kernels_cp.h, device-wide mode) in both shapes of tests/test_gpu_cp.py's
    test_cp_device_wide_equals_oracle.  In the block order workgroup 0 holds copies that all carry the higher base, so its guess
    is the loser of every two-way tie: with a vote wave the kernel must report recomputed rows, whatever the lanes per flank;
    without one nothing is computed on a guess and it must report none.  (The run info has no field for the vote wave: this
    pair of assertions is what tells the two shapes apart.)"""
    infos = _run_case(name, monkeypatch, dict(CELL_PARALLEL, RAMX_CP_K=str(K)), 30, order, _is(1, K, one_launch=True))
    if vote_wave and order == "blocks":
        assert _has_two_way_ties(name)
        assert all(i.respeculated_rows > 0 for i in infos), [(i.respeculated_rows, i.rows_executed) for i in infos]
    if not vote_wave:
        assert all(i.respeculated_rows == 0 for i in infos), [(i.respeculated_rows, i.rows_executed) for i in infos]


@pytest.mark.parametrize("name", ["rs14", "place40", "eq_rs"])
def test_cell_parallel_device_wide_forced_wrong_guesses_on_top(name, monkeypatch):
    """The hooks of tests/test_gpu_cp.py on top of the planted ties: every third guess replaced, the vote wave held back."""
    env = dict(CELL_PARALLEL, RAMX_TEST_CP_WRONG_EVERY="3", RAMX_TEST_CP_VOTE_DELAY="2")
    infos = _run_case(name, monkeypatch, env, 30, "blocks", _is(1, 16, one_launch=True))
    assert all(i.respeculated_rows > 0 for i in infos)


# ---- two ranks ------------------------------------------------------------------------------------------------------------------

def _rank(rank, world, port, out, names, r, env):
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

    for k in ROUTE_VARS + MORE_VARS:
        os.environ.pop(k, None)
    os.environ.update(env)
    dev = Device(0)
    dev.set_allreduce_callback(allreduce4)
    enabled = dev.peer_setup(rank, world, ag_bytes, ar_min, dist.barrier)       # (the production order of the mailbox transports)
    got = {}
    for name in names:
        run = small_run(name)
        case = run.case
        dev.load_library(run.fs.sequence)
        c, m = de.repeat_blocks(run.fs.cores, r), new_master(case.L)
        rets, infos = [], []
        for d in (1, 0):
            rets.append(extend_alignment_sharded(d, c, run.fs.sequence, m, to_extend_params(de.case_params(case, r)), rank, world,
                                                 gpu_engine(dev), all_gather))
            i = dev.last
            infos.append((i.limit_warning, i.overflow32, i.n_extendable, i.persistent, i.lanes_per_flank, i.packed_rows, i.respeculated_rows))
        got[name] = (rets, infos, m.copy(), c.left_len.copy(), c.right_len.copy(), c.score.copy())
    dev.close()
    out[rank] = (enabled, got)
    dist.destroy_process_group()


@pytest.mark.parametrize("route,names,r", [("packed rows", ("m14",), 168), ("packed rows", ("eq_rs",), 168), ("cell-parallel", ("rs14",), 48),
                                           ("cell-parallel", ("eq_rs",), 48)], ids=["packed rows-m14", "packed rows-eq_rs", "cell-parallel-rs14", "cell-parallel-eq_rs"])
def test_two_ranks_tie_only_in_the_exchanged_totals(route, names, r):
    """Two ranks on one device, the copies in blocks: rank 0 holds the group with the higher base of every two-way tie and rank 1
    the other, so neither rank's own totals tie and the totals exchanged through the mailboxes do."""
    import torch.multiprocessing as mp
    from test_gpu_sharded import _free_port
    world = 2
    from repeatafterme_amd.sharded import partition
    for name in names:
        for d in (1, 0):
            check_premises(small_run(name), d)
        assert name in de.TWO_RANK_CASES and all(de.check_rank_halves(name, world).values())     # no rank ties alone, the total does
        for rank in range(world):                                                  # a rank's shard is its half of the 24 copies, r times
            small, big = partition(M, world, rank), partition(M * r, world, rank)
            assert set(np.repeat(np.arange(M), r)[big]) == set(range(small.start, small.stop)) and big.stop - big.start == M * r // world
    env = {"RAMX_NO_CP_DEVICE": "1", "RAMX_PK_SEGMENT": "0"} if route == "packed rows" else {}
    out = mp.Manager().dict()
    mp.spawn(_rank, args=(world, _free_port(), out, names, r, env), nprocs=world, join=True)
    for rank in range(world):
        enabled, got = out[rank]
        assert enabled, "peer self-test failed"
        for name in names:
            run = small_run(name)
            rets, infos, m, ll, rl, sc = got[name]
            print(route, name, "rank", rank, infos)
            for k, d in enumerate((1, 0)):
                o = run.direction(d)
                assert rets[k] == (o.ret, o.rows_executed), (name, rank, d, rets[k])
                assert infos[k][:4] == (o.limit_warning, 0, M * r // world, 1), (name, rank, d, infos[k])
                if route == "packed rows":
                    assert infos[k][4] == 1 and 0 < infos[k][5] <= o.rows_executed, (name, rank, d, infos[k])
                else:
                    assert infos[k][4] > 1 and infos[k][5] == 0, (name, rank, d, infos[k])
            assert np.array_equal(m, run.master), (name, rank)
            for have, k in ((ll, "left_len"), (rl, "right_len"), (sc, "score")):
                assert np.array_equal(have, np.repeat(getattr(run.cores, k), r)), (name, rank, k)
