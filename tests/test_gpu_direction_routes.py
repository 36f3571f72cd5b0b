"""Which kernel a whole-set direction takes (csrc/ramx_device.hip, ramx_dev_run_direction), seen through its run info: the
tuple (persistent, lanes_per_flank, packed_rows > 0) under every switch that moves a flank set from one route to another, several
directions in a row on one device, and the two single-GPU fallbacks followed by a normal direction.  150 flanks (two full tiles
and a partial one) at W = 14 and W = 40; every direction is compared with the oracle.  The gate edges themselves are
tests/test_gpu_score_gates.py's."""
import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import new_master
from repeatafterme_amd.synth import synth_family

import score_gates as sg
from helpers import to_extend_params

pytestmark = pytest.mark.gpu

SWITCHES = ("RAMX_NO_FAMILY_ROUTE", "RAMX_NO_CP_DEVICE", "RAMX_NO_CP", "RAMX_NO_PK", "RAMX_NO_PERSISTENT", "RAMX_FORCE_CHAIN", "RAMX_CP_K",
            "RAMX_CP_DEVICE_MAXN", "RAMX_PK_SEGMENT", "RAMX_NO_LEAN", "RAMX_TEST_PK_SPREAD", "RAMX_TEST_PK_SPREAD_ROWS",
            "RAMX_TEST_CP_DROP_TICKET", "RAMX_TEST_CP_WRONG_EVERY", "RAMX_TEST_PK_WRONG_EVERY")

N, LMAX = 150, 256
CELL, CELL2, PACKED, INT32, COLUMNS = (1, 16, False), (1, 2, False), (1, 1, True), (1, 1, False), (0, 1, False)
NO_CPD, NO_PK, NO_PRK, CHAIN, K2 = ({"RAMX_NO_CP_DEVICE": "1"}, {"RAMX_NO_PK": "1"}, {"RAMX_NO_PERSISTENT": "1"}, {"RAMX_FORCE_CHAIN": "1"},
                                    {"RAMX_CP_K": "2"})


def _set(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def families():
    return {W: synth_family(N, LMAX, W, K=LMAX - 60, seed=5200 + W, both_sides=True, minus_frac=0.3, n_run_frac=0.2) for W in (14, 40)}


def _params(W, L, **kw):
    return po.Params.named("14p43g", bandwidth=W, L=L, when_to_stop=kw.pop("when_to_stop", 30), **kw)


_oracle_cache = {}


def _oracle(fs, p):
    key = (id(fs), p.bandwidth, p.L, p.when_to_stop, p.gapopen, p.gapextn)
    if key not in _oracle_cache:
        c, m = fs.cores.copy(), new_master(p.L)
        o = po.oracle_extend(1, c, fs.sequence, m, p)
        _oracle_cache[key] = (o, m, c)
    return _oracle_cache[key]


def _direction(dev, fs, p):
    """One right direction on an open device: (run info, consensus, trimmed highs, trimmed positions, the final DP rows of the
    first flank, one in the partial tile and the last)."""
    from repeatafterme_amd.device import resolve_flanks
    flanks, idx = resolve_flanks(1, fs.cores, p.bandwidth, p.L)
    assert np.array_equal(idx, np.arange(fs.cores.n))
    dev.begin_direction(flanks, to_extend_params(p))
    info = dev.run_direction()
    cons, th, tp = dev.download()
    return info, cons, th, tp, [dev.peek_state(i) for i in (0, 130, N - 1)]


def _fresh(fs, p):
    from repeatafterme_amd.device import Device
    dev = Device(0)             # (RAMX_FORCE_CHAIN is read when the device is created)
    try:
        dev.load_library(fs.sequence)
        return _direction(dev, fs, p)
    finally:
        dev.close()


def _route(info):
    return (info.persistent, info.lanes_per_flank, info.packed_rows > 0)


def _assert_equals_oracle(got, fs, p, tag):
    info, cons, th, tp, _ = got
    o, m, c = _oracle(fs, p)
    assert (info.ret, info.rows_executed, info.limit_warning) == (o.ret, o.rows_executed, o.limit_warning), tag
    assert np.array_equal(cons, m[p.L + p.l:p.L + p.l + o.rows_executed]), f"{tag}: consensus"
    ext = (th > 0) & (tp >= 0)                                    # ram_extend.c:1234-1247
    assert np.array_equal(np.where(ext, tp + 1, 0), c.right_len), f"{tag}: lengths"
    assert np.array_equal(np.where(ext, th, 0), c.score), f"{tag}: scores"


def _counts(info):
    """What a direction's run info says apart from times (and from the two counts that depend on the order in which the waves
    of a launch arrive: rows recomputed after a wrong guess, rows on the LEAN band)."""
    return (info.ret, info.rows_executed, info.limit_warning, info.overflow32, info.n_extendable, info.launches, info.persistent,
            info.lanes_per_flank, info.packed_rows)


def _assert_same_direction(a, b, tag):
    assert _counts(a[0]) == _counts(b[0]), tag
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), tag
    for (ca, ha, pa), (cb, hb, pb) in zip(a[4], b[4]):
        assert np.array_equal(ca, cb) and (ha, pa) == (hb, pb), f"{tag}: final DP rows"


ROUTE_TABLE = [
    ({}, CELL), (NO_PK, CELL), (K2, CELL2), ({**K2, **NO_PK}, CELL2),
    (NO_CPD, PACKED), ({**NO_CPD, **K2}, PACKED),
    ({**NO_CPD, **NO_PK}, INT32), ({"RAMX_NO_CP": "1", **NO_PK}, INT32),
    (NO_PRK, COLUMNS), (CHAIN, COLUMNS), ({**NO_PRK, **K2}, COLUMNS), ({**CHAIN, **NO_CPD}, COLUMNS), ({**NO_PRK, **NO_CPD, **NO_PK}, COLUMNS),
]


@pytest.mark.parametrize("W", [14, 40])
def test_route_table(W, families, monkeypatch):
    """Sixteen lanes per flank by default; the packed rows without the device-wide cell-parallel kernel; the int32 rows without
    the packed ones too; per-column launches without the persistent kernels or with the full candidate recurrence forced.
    RAMX_CP_K=2 caps the lanes per flank (and lifts the preference for the packed rows below four); RAMX_NO_PK alone changes
    nothing where the cell-parallel kernel goes first.  L = 160: two checkpoints of 64 columns and a rest on the column route."""
    fs, p = families[W], _params(W, 160)
    assert sg.pk_plan(W, p.gapopen, p.gapextn, p.matrix).admitted and sg.cp_value_range_ok(W, p.L, p.gapopen, p.gapextn, p.matrix)
    for env, want in ROUTE_TABLE:
        _set(monkeypatch, env)
        got = _fresh(fs, p)
        assert _route(got[0]) == want, (W, env, _route(got[0]))
        assert got[0].launches == 1 if want[0] else got[0].launches >= got[0].rows_executed, (W, env, got[0].launches)
        _assert_equals_oracle(got, fs, p, f"W={W} {env}")


@pytest.mark.parametrize("W", [14, 40])
def test_route_with_a_positive_gap_penalty(W, families, monkeypatch):
    """A positive gap penalty needs the full candidate recurrence: per-column launches, whatever the switches say."""
    fs = families[W]
    for go, ge in ((2, -5), (-30, 1)):
        p = _params(W, 128, gapopen=go, gapextn=ge)
        for env in ({}, NO_CPD, K2):
            _set(monkeypatch, env)
            got = _fresh(fs, p)
            assert _route(got[0]) == COLUMNS, (W, go, ge, env, _route(got[0]))
            _assert_equals_oracle(got, fs, p, f"W={W} go={go} ge={ge} {env}")


@pytest.mark.parametrize("W", [14, 40])
def test_one_device_through_every_route_in_a_row(W, families, monkeypatch):
    """Packed rows, per-column launches, cell-parallel, int32 rows, and the packed rows once more, on ONE device and with a
    different length each: every direction's run info, results and final DP rows equal those of a device that has run nothing
    before (and the oracle's).  What one route leaves behind -- the first packed row, the words packed so far, a pack still in
    flight, the control blocks -- must not reach the next."""
    from repeatafterme_amd.device import Device
    fs = families[W]
    steps = [(NO_CPD, PACKED, 224), (NO_PRK, COLUMNS, 96), ({}, CELL, 256), ({**NO_CPD, **NO_PK}, INT32, 160), (NO_CPD, PACKED, 128)]
    _set(monkeypatch, {})
    dev = Device(0)
    try:
        dev.load_library(fs.sequence)
        for env, want, L in steps:
            p = _params(W, L, when_to_stop=25)
            _set(monkeypatch, env)
            got = _direction(dev, fs, p)
            tag = f"W={W} L={L} {env}"
            assert _route(got[0]) == want, (tag, _route(got[0]))
            _assert_equals_oracle(got, fs, p, tag)
            _assert_same_direction(got, _fresh(fs, p), tag)
    finally:
        dev.close()


@pytest.mark.parametrize("W", [14, 40])
def test_refused_packed_rows_then_a_normal_direction(W, families, monkeypatch, capfd):
    """RAMX_TEST_PK_SPREAD=5: the packed-row kernel refuses the rows it is handed, the direction is repeated with per-column
    launches; the next direction on the same device takes the packed rows again."""
    from repeatafterme_amd.device import Device
    fs, p = families[W], _params(W, 192)
    _set(monkeypatch, NO_CPD)
    dev = Device(0)
    try:
        dev.load_library(fs.sequence)
        monkeypatch.setenv("RAMX_TEST_PK_SPREAD", "5")
        capfd.readouterr()
        got = _direction(dev, fs, p)
        said = capfd.readouterr().err
        assert "the packed-row kernel refused the rows it was handed" in said and "repeating the direction with per-column launches" in said, said
        assert _route(got[0]) == COLUMNS and got[0].launches >= got[0].rows_executed, _counts(got[0])
        _assert_equals_oracle(got, fs, p, f"W={W} refused")
        monkeypatch.delenv("RAMX_TEST_PK_SPREAD")
        nxt = _direction(dev, fs, p)
        assert "repeating the direction" not in capfd.readouterr().err
        assert _route(nxt[0]) == PACKED, _counts(nxt[0])
        _assert_equals_oracle(nxt, fs, p, f"W={W} after the refusal")
        _assert_same_direction(nxt, _fresh(fs, p), f"W={W} after the refusal")
    finally:
        dev.close()


@pytest.mark.parametrize("W", [14, 40])
def test_lost_ticket_then_a_normal_direction(W, families, monkeypatch, capfd):
    """RAMX_TEST_CP_DROP_TICKET=7: the device-wide vote of the cell-parallel launch gives up at its bounded spin and the
    direction is repeated on the lane-per-flank route -- the packed rows, which this set takes without the cell-parallel kernel;
    the next direction on the same device runs cell-parallel again."""
    from repeatafterme_amd.device import Device
    fs, p = families[W], _params(W, 192)
    _set(monkeypatch, {})
    dev = Device(0)
    try:
        dev.load_library(fs.sequence)
        monkeypatch.setenv("RAMX_TEST_CP_DROP_TICKET", "7")
        capfd.readouterr()
        got = _direction(dev, fs, p)
        said = capfd.readouterr().err
        assert "device-wide vote of the cell-parallel launch timed out (bounded spin)" in said, said
        assert _route(got[0]) == PACKED and got[0].launches == 1, _counts(got[0])
        _assert_equals_oracle(got, fs, p, f"W={W} lost ticket")
        monkeypatch.delenv("RAMX_TEST_CP_DROP_TICKET")
        nxt = _direction(dev, fs, p)
        assert "repeating the direction" not in capfd.readouterr().err
        assert _route(nxt[0]) == CELL, _counts(nxt[0])
        _assert_equals_oracle(nxt, fs, p, f"W={W} after the lost ticket")
        _assert_same_direction(nxt, _fresh(fs, p), f"W={W} after the lost ticket")
    finally:
        dev.close()
