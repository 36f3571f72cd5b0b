"""Checkpoints of the packed-row kernel (csrc/ramx_kernels_packed.h): a speculating workgroup keeps the state at the top of a
column (row, chain registers, records) at most once per 1, 2, 4 or 8 columns instead of before every row, and logs the confirmed
winner of every row since.  After a wrong guess at row r the checkpoint comes back, the rows between it and r run again in
silence on the logged winners, and row r runs on the device's winner.  RAMX_PK_CKPT = 1 / 2 / 4 / 8 fixes the distance (1 is the
backup per row the kernel took before); unset, the distance is 8, falls to 1 for 32 columns after a wrong guess and doubles from
there.

Every case runs on the device-wide lane-per-flank route, forces wrong guesses with RAMX_TEST_PK_WRONG_EVERY=n (rows r with
r % n == 0: 7 and 9 walk through every offset of a block of eight, 8 and 16 hit block starts only, 1 is every row; 3, 7 and 9
between them hit rebase rows, r = 15 mod 16, and rows of the span check, r = 63 mod 64, below column 260) and compares return
value, stop row, consensus, trim words and final DP rows, cell by cell, with the RAMX_PK_CKPT=1 run under the same hook, the
count of rows computed twice included, and the results with the oracle's."""
import contextlib
import functools
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.synth import synth_family

from helpers import assert_same_result, gpu_extend, oracle_extend, run_both_directions, to_extend_params
from test_gpu_leader_path import _family as _leader_family
from test_gpu_persistent import _two_copy_family

pytestmark = pytest.mark.gpu

L = 260
N = 1500                                     # three 512-thread workgroups: the device-wide vote is a real one
CKPTS = (None, "1", "2", "4", "8")
EVERY = ("0", "1", "3", "5", "7", "8", "9", "16")
ENV_VARS = ("RAMX_NO_FAMILY_ROUTE", "RAMX_NO_CP_DEVICE", "RAMX_NO_CP", "RAMX_NO_PK", "RAMX_NO_LEAN", "RAMX_NO_PERSISTENT", "RAMX_CP_K",
            "RAMX_PK_NO_VW", "RAMX_PK_NO_256", "RAMX_PK_WG_PER_CU", "RAMX_LEADER_MAX", "RAMX_NO_PK_SPEC", "RAMX_TEST_PK_WRONG_EVERY",
            "RAMX_PK_SEGMENT", "RAMX_PK_CKPT")
SHAPES = {"320 threads": {}, "256 threads": {"RAMX_PK_NO_VW": "1"}, "512 threads": {"RAMX_PK_NO_256": "1"}}
MATRIX = {40: "14p43g", 14: "20p43g", 20: "25p43g"}


@contextlib.contextmanager
def _env(env):
    """The lane-per-flank route and `env`, nothing else of the kernel's switches; put back afterwards."""
    saved = {k: os.environ.get(k) for k in ENV_VARS}
    for k in ENV_VARS:
        os.environ.pop(k, None)
    os.environ["RAMX_NO_FAMILY_ROUTE"] = "1"
    os.environ["RAMX_NO_CP_DEVICE"] = "1"
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _two_copy(W):
    """The first 260 columns of the two-copy family (300 aligned columns; 4 % of the flanks end early).  Never modified."""
    return _two_copy_family(N, 720, W, 60, seed=5200 + W, short_frac=0.04)


@functools.lru_cache(maxsize=None)
def _ending(W):
    """120 aligned columns, then random ones: the alignment ends inside the run, guesses go wrong by themselves, every flank
    sinks to its cap and the stop rule fires in the middle of a block.  Never modified."""
    return synth_family(N, L, W, K=120, seed=5300 + W, core_len=12)


FAMILIES = {"two-copy": _two_copy, "ending": _ending}


@functools.lru_cache(maxsize=None)
def _oracle(family, W, stop):
    p = po.Params.named(MATRIX[W], bandwidth=W, L=L, when_to_stop=stop)
    fs = FAMILIES[family](W)
    return p, run_both_directions(oracle_extend, fs.cores, fs.sequence, p)


def _run_device(fs, p, env):
    from repeatafterme_amd.device import Device, resolve_flanks
    with _env(env):
        dev = Device(0)
        dev.load_library(fs.sequence)
        flanks, idx = resolve_flanks(1, fs.cores, p.bandwidth, p.L)
        dev.begin_direction(flanks, to_extend_params(p))
        info = dev.run_direction()
        cons, th, tp = dev.download()
        state = [dev.peek_state(i) for i in range(0, len(idx), 3)] + [dev.peek_state(len(idx) - 1)]
        dev.close()
    assert info.persistent == 1 and info.lanes_per_flank == 1 and info.packed_rows > 0, (env, info)
    return info, cons, th, tp, state


_REFS = {}


def _reference(key, fs, p, env):
    """The RAMX_PK_CKPT=1 run of a configuration: computed once, shared, never modified."""
    if key not in _REFS:
        _REFS[key] = _run_device(fs, p, dict(env, RAMX_PK_CKPT="1"))
    return _REFS[key]


def _assert_equal_runs(got, ref, tag):
    assert (got[0].ret, got[0].rows_executed, got[0].limit_warning) == (ref[0].ret, ref[0].rows_executed, ref[0].limit_warning), tag
    assert np.array_equal(got[1], ref[1]), f"{tag}: consensus differs at {np.nonzero(got[1] != ref[1])[0][:8]}"
    assert np.array_equal(got[2], ref[2]), f"{tag}: trim high differs in flanks {np.nonzero(got[2] != ref[2])[0][:8]}"
    assert np.array_equal(got[3], ref[3]), f"{tag}: trim pos differs in flanks {np.nonzero(got[3] != ref[3])[0][:8]}"
    for f, ((ca, ha, pa), (cb, hb, pb)) in enumerate(zip(got[4], ref[4])):
        assert np.array_equal(ca, cb) and (ha, pa) == (hb, pb), f"{tag}: final row of sampled flank {f}"
    assert got[0].respeculated_rows == ref[0].respeculated_rows, (tag, got[0].respeculated_rows, ref[0].respeculated_rows)


def _assert_oracle(got, p, ora, tag):
    right = ora[2]
    assert (got[0].ret, got[0].rows_executed) == (right.ret, right.rows_executed), (tag, got[0].ret, got[0].rows_executed)
    rows = right.rows_executed
    want = ora[1][p.L + p.l:p.L + p.l + rows]
    assert np.array_equal(got[1][:rows], want), f"{tag}: consensus differs from the oracle's at {np.nonzero(got[1][:rows] != want)[0][:8]}"


def _cross(family, W, stop, ckpt, everies, shape="512 threads", extra=None):
    p, ora = _oracle(family, W, stop)
    fs = FAMILIES[family](W)
    for every in everies:
        env = dict(SHAPES[shape], **(extra or {}))
        env["RAMX_TEST_PK_WRONG_EVERY"] = every
        tag = f"{family} W={W} stop={stop} {shape} {extra} every={every} ckpt={ckpt}"
        ref = _reference((family, W, stop, shape, tuple(sorted((extra or {}).items())), every), fs, p, env)
        _assert_oracle(ref, p, ora, tag + " (reference run)")
        if every in ("1", "3"):
            assert ref[0].respeculated_rows > 0, tag                 # the hook really makes rows run twice
        got = _run_device(fs, p, env if ckpt is None else dict(env, RAMX_PK_CKPT=ckpt))
        _assert_equal_runs(got, ref, tag)
        _assert_oracle(got, p, ora, tag)


@pytest.mark.parametrize("ckpt", CKPTS, ids=lambda c: f"ckpt-{c or 'unset'}")
def test_wrong_guess_at_every_offset_of_a_block(ckpt):
    """W = 40, three 512-thread workgroups, the whole cross of distances and hook values."""
    _cross("two-copy", 40, L, ckpt, EVERY)


@pytest.mark.parametrize("W", [14, 20])
def test_other_band_widths(W):
    for ckpt in (None, "8"):
        _cross("two-copy", W, L, ckpt, ("7", "9"))


@pytest.mark.parametrize("ckpt", CKPTS, ids=lambda c: f"ckpt-{c or 'unset'}")
@pytest.mark.parametrize("stop", [L, 30, 1])
def test_stop_rule_and_an_alignment_that_ends(stop, ckpt):
    """A stop and a last row in the middle of a block, a wrong guess at the stop row (every = 1), guesses that go wrong by
    themselves where the alignment ends, LEAN rows behind it."""
    p, ora = _oracle("ending", 40, stop)
    if stop < L:
        assert ora[2].rows_executed < L, (stop, ora[2].rows_executed)       # the stop rule really fires inside the run
    _cross("ending", 40, stop, ckpt, ("0", "1", "7", "9"))
    if stop < L:
        _cross("two-copy", 40, stop, ckpt, ("1", "7"))


def test_whole_extension_equals_the_oracle():
    """Both directions through the public entry, scores and extension lengths included, for every fixed distance."""
    for family in FAMILIES:
        p, ora = _oracle(family, 40, 30)
        fs = FAMILIES[family](40)
        for ckpt in CKPTS:
            with _env(dict({"RAMX_TEST_PK_WRONG_EVERY": "7"}, **({} if ckpt is None else {"RAMX_PK_CKPT": ckpt}))):
                dev = run_both_directions(gpu_extend, fs.cores, fs.sequence, p)
            assert_same_result(ora[0], ora[1], ora[2:], dev[0], dev[1], dev[2:], f"{family} ckpt={ckpt}")
            assert dev[2].packed_rows > 0, (family, ckpt)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("seg", ["16", "50", "13"])
def test_pieces_start_inside_a_block(seg, shape):
    """The direction in launches of 16, 50 and 13 columns: piece starts that are and are not multiples of 8, the first column of
    a launch speculative, a checkpoint due there."""
    for ckpt in (None, "8", "4"):
        _cross("two-copy", 40, L, ckpt, ("1", "7", "9"), shape=shape, extra={"RAMX_PK_SEGMENT": seg})


@pytest.mark.parametrize("leader_max", [None, "0"], ids=["leaders", "no-leaders"])
def test_silent_replay_of_leader_rows(leader_max):
    """The family of test_gpu_leader_path.py (chosen lanes stay leaders to the end): wrong guesses 7 and 9 columns apart make
    the silent replay run pkb_leader_rows."""
    W, matrix, seed, n = 40, "14p43g", 7340, 700
    fs, p, anc2, ora = _leader_family(W, matrix, seed, n, False)
    extra = {} if leader_max is None else {"RAMX_LEADER_MAX": leader_max}
    for every in ("7", "9"):
        env = dict(extra, RAMX_TEST_PK_WRONG_EVERY=every)
        ref = _run_device(fs, p, dict(env, RAMX_PK_CKPT="1"))
        _assert_oracle(ref, p, ora, f"leaders {env} (reference run)")
        assert ref[0].respeculated_rows > 0
        for ckpt in (None, "8", "2"):
            got = _run_device(fs, p, env if ckpt is None else dict(env, RAMX_PK_CKPT=ckpt))
            _assert_equal_runs(got, ref, f"leaders {env} ckpt={ckpt}")


def test_adaptive_distance():
    """A wrong guess every 40 columns: the distance falls to 1, comes back to 8 and falls again.  Results only, no timing."""
    for family in FAMILIES:
        _cross(family, 40, L, None, ("40",))
