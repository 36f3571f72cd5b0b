"""The route plan of a batch (family_plan in csrc/ramx_device.hip) seen from outside: one batch whose family sizes touch every
edge of the cell-parallel classes (16/17, 32/33, 64/65, 128/129, 256/257) and the multi-workgroup route, under every switch
that moves a family from one kernel to another.  Every family equals its own oracle run, and (persistent, lanes_per_flank)
of every family is what the plan says.  Two sequences on the process-wide session follow: batch / batch / whole-set
direction, and a packed-rows direction that stops early (its look-ahead pack may still be in flight) / batch."""
import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import new_master
from repeatafterme_amd.extend import extend_batch
from repeatafterme_amd.synth import synth_family

from helpers import assert_same_result, gpu_extend, oracle_extend, run_both_directions, to_extend_params

pytestmark = pytest.mark.gpu

SIZES = (5, 16, 17, 33, 65, 129, 256, 257, 512, 10)      # the last family has no extendable core
LANES = (16, 16, 16, 8, 4, 2, 2)                         # of the families up to 256 flanks, no switch set
L = 96
ROUTE_VARS = ("RAMX_NO_CP", "RAMX_CP_K", "RAMX_NO_CP_DEVICE", "RAMX_NO_FAMILY_ROUTE", "RAMX_NO_PERSISTENT", "RAMX_NO_PK", "RAMX_PK_SEGMENT",
              "RAMX_CP_PEEK", "RAMX_CP_SINGLE_MAX", "RAMX_CP_DEVICE_MAXN")


@pytest.fixture(autouse=True)
def _plain_routes(monkeypatch):
    for k in ROUTE_VARS:
        monkeypatch.delenv(k, raising=False)


def _params(W):
    return po.Params.named("14p43g", bandwidth=W, L=L, when_to_stop=25)


@pytest.fixture(scope="module")
def batch():
    fams = [synth_family(n, L, 40, K=50 + 7 * i, seed=8100 + i, both_sides=True, minus_frac=0.3, n_run_frac=0.1) for i, n in enumerate(SIZES)]
    fams[-1].cores.right_ext[:] = 0
    fams[-1].cores.left_ext[:] = 0
    want = {}
    for W in (40, 9):
        p = _params(W)
        want[W] = []
        for fs in fams:
            c = fs.cores.copy(); m = new_master(L)
            r1 = po.oracle_extend(1, c, fs.sequence, m, p)
            r0 = po.oracle_extend(0, c, fs.sequence, m, p)
            want[W].append((r1.ret, r0.ret, r1.rows_executed, r0.rows_executed, m, c))
    return fams, want


def _run_batch(batch, W=40):
    """The batch in both directions, every family against its oracle run -> (persistent, lanes_per_flank) per family and
    direction, the consensus and the lengths."""
    fams, want = batch
    cs = [fs.cores.copy() for fs in fams]
    ms = [new_master(L) for _ in fams]
    ep = to_extend_params(_params(W))
    ir = extend_batch(1, [(c, fs.sequence, m) for c, fs, m in zip(cs, fams, ms)], ep)
    il = extend_batch(0, [(c, fs.sequence, m) for c, fs, m in zip(cs, fams, ms)], ep)
    for i, (w, c, m) in enumerate(zip(want[W], cs, ms)):
        tag = f"family {i} ({SIZES[i]} cores, W {W})"
        assert (ir[i].ret, il[i].ret, ir[i].rows_executed, il[i].rows_executed) == w[:4], tag
        assert np.array_equal(m, w[4]), tag + ": consensus"
        assert np.array_equal(c.left_len, w[5].left_len) and np.array_equal(c.right_len, w[5].right_len), tag
        assert np.array_equal(c.score, w[5].score), tag
    return [[(x[i].persistent, x[i].lanes_per_flank) for x in (ir, il)] for i in range(len(fams))], ms, cs


def _default_route(got):
    for i, k in enumerate(LANES):
        assert got[i] == [(1, k)] * 2, (i, got)
    for i in (7, 8):
        assert all(pers == 1 and k > 1 for pers, k in got[i]), (i, got)
    assert got[9] == [(1, 1)] * 2, got


@pytest.mark.parametrize("switch", ["none", "RAMX_NO_CP", "RAMX_NO_CP_DEVICE", "RAMX_NO_PERSISTENT", "RAMX_CP_K", "W9"])
def test_family_routes_under_every_switch(batch, switch, monkeypatch):
    if switch == "RAMX_CP_K":
        monkeypatch.setenv("RAMX_CP_K", "2")
    elif switch not in ("none", "W9"):
        monkeypatch.setenv(switch, "1")
    got, _, _ = _run_batch(batch, 9 if switch == "W9" else 40)
    print(switch, got)
    if switch == "none":
        _default_route(got)
    elif switch == "RAMX_NO_CP":
        assert all(g == [(1, 1)] * 2 for g in got), got
    elif switch == "RAMX_NO_CP_DEVICE":
        for i, k in enumerate(LANES):
            assert got[i] == [(1, k)] * 2, (i, got)
        assert got[7] == got[8] == got[9] == [(1, 1)] * 2, got
    elif switch == "RAMX_NO_PERSISTENT":
        for i, k in enumerate(LANES):
            assert got[i] == [(1, k)] * 2, (i, got)
        assert got[7] == got[8] == got[9] == [(2, 1)] * 2, got          # (the empty family has a lane-per-flank shape too)
    elif switch == "RAMX_CP_K":
        for i in range(len(LANES)):
            assert got[i] == [(1, 2)] * 2, (i, got)
        assert got[7] == got[8] == [(1, 2)] * 2, got                   # (the device-wide plan is capped alike)
    else:
        assert all(g == [(2, 1)] * 2 for g in got), got


def _direction(n, Ldir, K, seed, **kw):
    """A whole-set seam-1 direction pair of n flanks against the oracle -> the device's two RunInfos."""
    fs = synth_family(n, Ldir, 40, K=K, seed=seed, both_sides=True, minus_frac=0.3, n_run_frac=0.1)
    p = po.Params.named("14p43g", bandwidth=40, L=Ldir, **kw)
    a = run_both_directions(oracle_extend, fs.cores, fs.sequence, p)
    b = run_both_directions(gpu_extend, fs.cores, fs.sequence, p)
    assert_same_result(a[0], a[1], a[2:], b[0], b[1], b[2:], f"{n} flanks, L {Ldir}")
    assert (a[2].rows_executed, a[3].rows_executed) == (b[2].rows_executed, b[3].rows_executed)
    return b[2], b[3]


def test_batch_then_lane_per_flank_batch_then_direction(batch, monkeypatch):
    """One session: the batch, the same batch with the cell-parallel kernels off, a whole-set direction of 150 flanks."""
    got, ms, cs = _run_batch(batch)
    _default_route(got)
    monkeypatch.setenv("RAMX_NO_CP", "1")
    got2, ms2, cs2 = _run_batch(batch)
    monkeypatch.delenv("RAMX_NO_CP")
    assert all(g == [(1, 1)] * 2 for g in got2), got2
    for i in range(len(SIZES)):
        assert np.array_equal(ms[i], ms2[i]), i
        assert np.array_equal(cs[i].left_len, cs2[i].left_len) and np.array_equal(cs[i].right_len, cs2[i].right_len), i
    rr, rl = _direction(150, 120, 60, 8200, when_to_stop=25)
    assert rr.persistent == 1 and rl.persistent == 1


def test_batch_after_a_packed_direction_that_stopped_early(batch, monkeypatch):
    """The packed rows run in pieces of 64 columns and pack the next piece's words beside the running one; the copies end
    after a hundred columns of 1,200, so the direction stops with such a pack just enqueued.  The batch that follows uploads
    new flanks and packs into the same buffers: it must wait for that pack (pack_settle).  Pins the sequence; the race
    itself seldom shows."""
    monkeypatch.setenv("RAMX_NO_FAMILY_ROUTE", "1")       # the whole-set direction, on its lane-per-flank route
    monkeypatch.setenv("RAMX_NO_CP_DEVICE", "1")
    monkeypatch.setenv("RAMX_PK_SEGMENT", "64")
    rr, rl = _direction(150, 1200, 100, 8300, when_to_stop=25)
    assert rr.packed_rows > 0 and rl.packed_rows > 0
    assert 64 < rr.rows_executed < 400 and 64 < rl.rows_executed < 400
    for k in ("RAMX_NO_FAMILY_ROUTE", "RAMX_NO_CP_DEVICE", "RAMX_PK_SEGMENT"):
        monkeypatch.delenv(k)
    got, _, _ = _run_batch(batch)
    _default_route(got)
