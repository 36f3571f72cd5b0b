"""The leader wave's column in the packed-row kernel (csrc/ramx_kernels_packed.h): a LEAN wave that holds a few flanks which still
set records ("leaders", pkb_leader_rows) reduces the leaders' four maxima together (wave_max4_i32, the deletion term folded in per
lane) and a wave whose sums come after its row takes its four sums together (wave_sum4_nonneg31) -- with one, two, three, four
and five leaders in a wave, a last wave with padding lanes, leaders that run out, rollbacks, and launches in pieces.

The family: 150 aligned columns, then a handful of chosen flanks carry copies (3 % substitutions) of a SECOND ancestor to the end
while every other flank is random there.  Behind column ~200 everybody but the chosen flanks sits at the cap and the chosen ones
decide every vote and set records in every column: wave 0 holds one leader (lane 5), wave 1 two (3, 40), wave 2 three (1, 30, 63),
wave 3 four (0, 9, 31, 50: above the default leader_max of 3, so FULL by default and a leader wave with RAMX_LEADER_MAX=64),
every further wave five drawn lanes.  n = 700 leaves the last wave 60 flanks and four padding lanes.  A second variant lets two of
the chosen flanks (one of wave 1's two, one of wave 3's four) end at about column 400: a wave's set of leaders changes, and
wave 3 goes from FULL to LEAN with three leaders.

Every case: the oracle's properties of the family (so that a family without leaders fails instead of passing vacuously), results
equal to the oracle's, and consensus, trim words and final DP rows equal, cell by cell, to a run with RAMX_LEADER_MAX=0 for
RAMX_LEADER_MAX unset / 1 / 64, with and without speculation, under forced wrong guesses (rollbacks of leader rows, rebase rows
included) and with the direction in pieces of 64 columns; on the three workgroup shapes (320, 256 and 512 threads)."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.synth import synth_family

from helpers import assert_same_result, gpu_extend, oracle_extend, run_both_directions, to_extend_params

pytestmark = pytest.mark.gpu

K, L, CORE = 150, 600, 12
# the second ancestor's generator: seed + ANC2_SEED.  In the first columns behind the alignment nobody is at the cap yet and the
# ~50 chosen flanks vote against ~650 random ones; whether they win there is a property of the draw, which is why the oracle's
# properties are asserted in every case (the oracle alone: ret = rows = 600 and consensus = second ancestor in 99.2-100 % of the
# columns for every case below)
ANC2_SEED = 1000
FIXED = {0: (5,), 1: (3, 40), 2: (1, 30, 63), 3: (0, 9, 31, 50)}
ENV_VARS = ("RAMX_NO_FAMILY_ROUTE", "RAMX_NO_CP_DEVICE", "RAMX_NO_CP", "RAMX_NO_PK", "RAMX_NO_LEAN", "RAMX_NO_PERSISTENT", "RAMX_CP_K",
            "RAMX_PK_NO_VW", "RAMX_PK_NO_256", "RAMX_PK_WG_PER_CU", "RAMX_LEADER_MAX", "RAMX_NO_PK_SPEC", "RAMX_TEST_PK_WRONG_EVERY",
            "RAMX_PK_SEGMENT")
SHAPES = {"320 threads": {}, "256 threads": {"RAMX_PK_NO_VW": "1"}, "512 threads": {"RAMX_PK_NO_256": "1"}}
#          W   matrix     seed   n
CASES = [(40, "14p43g", 7340, 700), (40, "14p43g", 7343, 700), (14, "20p43g", 7314, 700), (20, "25p43g", 7320, 700),
         (40, "14p43g", 7341, 1100)]
SHORT_CASES = [CASES[0], CASES[2]]


def _chosen(n, seed):
    rng = np.random.default_rng(seed + 2)
    out = []
    for wave in range((n + 63) // 64):
        width = min(64, n - 64 * wave)
        lanes = FIXED[wave] if wave in FIXED else sorted(rng.choice(width, size=5, replace=False).tolist())
        out += [64 * wave + l for l in lanes]
    return np.array(out)


@functools.lru_cache(maxsize=None)
def _family(W, matrix, seed, n, short):
    """-> (FlankSet, Params, the second ancestor, the oracle's run of both directions).  Computed once, never modified."""
    fs = synth_family(n, L, W, K=K, seed=seed, core_len=CORE)
    win = len(fs.sequence) // n
    seq = fs.sequence.reshape(n, win).copy()
    rng = np.random.default_rng(seed + ANC2_SEED)
    tail = win - (CORE + K)
    anc2 = rng.integers(0, 4, size=tail, dtype=np.int8)
    chosen = _chosen(n, seed)
    block = np.broadcast_to(anc2, (len(chosen), tail)).copy()
    sub = rng.random(block.shape) < 0.03
    block[sub] = (block[sub] + rng.integers(1, 4, size=int(sub.sum()))) & 3
    seq[chosen, CORE + K:] = block
    fs.sequence = np.ascontiguousarray(seq.reshape(-1))
    if short:                       # a leader that runs out: one of wave 1's two and one of wave 3's four end at about column 400
        for f, at in ((64 + 3, 400), (192 + 9, 404)):
            fs.cores.upper[f] = fs.cores.right_pos[f] + at
    p = po.Params.named(matrix, bandwidth=W, L=L, when_to_stop=L)
    ora = run_both_directions(oracle_extend, fs.cores, fs.sequence, p)
    return fs, p, anc2, ora


def _agreement(cons, anc2):
    """Best share of columns K+50 .. L-10 in which the consensus is the second ancestor, over shifts of up to 8 columns."""
    cols = np.arange(K + 50, L - 10)
    return max(float(np.mean(cons[cols] == anc2[cols - K + s])) for s in range(-8, 9))


def _run_device(fs, p, monkeypatch, env):
    from repeatafterme_amd.device import Device, resolve_flanks
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dev = Device(0)
    dev.load_library(fs.sequence)
    flanks, idx = resolve_flanks(1, fs.cores, p.bandwidth, p.L)
    dev.begin_direction(flanks, to_extend_params(p))
    info = dev.run_direction()
    cons, th, tp = dev.download()
    state = [dev.peek_state(i) for i in range(len(idx))]
    dev.close()
    for k in env:
        monkeypatch.delenv(k)
    return info, cons, th, tp, state


def _assert_equal_runs(got, ref, tag):
    assert (got[0].ret, got[0].rows_executed, got[0].limit_warning) == (ref[0].ret, ref[0].rows_executed, ref[0].limit_warning), tag
    assert np.array_equal(got[1], ref[1]), f"{tag}: consensus differs at {np.nonzero(got[1] != ref[1])[0][:8]}"
    assert np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3]), f"{tag}: trim words"
    for f, ((ca, ha, pa), (cb, hb, pb)) in enumerate(zip(got[4], ref[4])):       # final DP rows, cell by cell, of every flank
        assert np.array_equal(ca, cb) and (ha, pa) == (hb, pb), f"{tag}: final row of flank {f}"


def _check(case, short, shape, monkeypatch):
    W, matrix, seed, n = case
    fs, p, anc2, ora = _family(W, matrix, seed, n, short)
    tag = f"W={W} {matrix} seed={seed} n={n} short={short} {shape}"
    # ---- the family does what it is built for (the oracle alone) ----
    right = ora[2]
    assert right.ret == right.rows_executed == L, (tag, right.ret, right.rows_executed)
    agree = _agreement(ora[1][L + p.l:L + p.l + L], anc2)
    print(f"{tag}: consensus = second ancestor in {100 * agree:.1f} % of columns {K + 50} .. {L - 10}")
    assert agree >= 0.95, (tag, agree)
    # ---- 1. the oracle's results ----
    for k in ENV_VARS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RAMX_NO_CP_DEVICE", "1")
    for k, v in SHAPES[shape].items():
        monkeypatch.setenv(k, v)
    dev = run_both_directions(gpu_extend, fs.cores, fs.sequence, p)
    assert_same_result(ora[0], ora[1], ora[2:], dev[0], dev[1], dev[2:], tag)
    assert (dev[2].rows_executed, dev[2].ret) == (right.rows_executed, right.ret), tag
    assert dev[2].persistent == 1 and dev[2].lanes_per_flank == 1 and dev[2].packed_rows >= L - W, (tag, dev[2])
    # ---- 2. cell by cell against the run without leaders ----
    ref = _run_device(fs, p, monkeypatch, {"RAMX_LEADER_MAX": "0"})
    assert ref[0].packed_rows >= L - W and np.array_equal(ref[1], ora[1][L + p.l:L + p.l + L]), tag
    runs = {}
    for lm in (None, "1", "64"):
        for nospec in (False, True):
            env = {} if lm is None else {"RAMX_LEADER_MAX": lm}
            if nospec:
                env["RAMX_NO_PK_SPEC"] = "1"
            runs[(lm, nospec)] = _run_device(fs, p, monkeypatch, env)
            _assert_equal_runs(runs[(lm, nospec)], ref, f"{tag} {env}")
    for env in ({"RAMX_TEST_PK_WRONG_EVERY": "3"}, {"RAMX_TEST_PK_WRONG_EVERY": "16"}, {"RAMX_TEST_PK_WRONG_EVERY": "3", "RAMX_LEADER_MAX": "64"},
                {"RAMX_PK_SEGMENT": "64"}, {"RAMX_PK_SEGMENT": "64", "RAMX_LEADER_MAX": "64"}):
        got = _run_device(fs, p, monkeypatch, env)
        _assert_equal_runs(got, ref, f"{tag} {env}")
        if "RAMX_TEST_PK_WRONG_EVERY" in env:
            # 3. the hook really makes rows run twice
            assert got[0].respeculated_rows > 0, (tag, env)
    # ---- 3. the path is taken: wave 0 holds exactly one leader over the ~400 steady-state columns (100: the transition).
    # `lean_rows` counts the first wave's LEAN rows among the passes that ran on a CONFIRMED winner; a row computed on a guess
    # that stood is not counted, and the workgroup that holds the leaders always has a guess -- so both sides of the comparison
    # run without speculation (the figures with speculation are printed) ----
    ref_nospec = _run_device(fs, p, monkeypatch, {"RAMX_LEADER_MAX": "0", "RAMX_NO_PK_SPEC": "1"})
    _assert_equal_runs(ref_nospec, ref, f"{tag} no leaders, no speculation")
    default, default_nospec = runs[(None, False)][0], runs[(None, True)][0]
    print(f"{tag}: lean_rows {default_nospec.lean_rows} with leaders, {ref_nospec[0].lean_rows} without "
          f"(with speculation: {default.lean_rows}, {ref[0].lean_rows})")
    assert default_nospec.lean_rows >= ref_nospec[0].lean_rows + 300, (tag, default_nospec.lean_rows, ref_nospec[0].lean_rows)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"W{c[0]}-{c[1]}-{c[2]}-n{c[3]}")
def test_leader_wave_sums_equal_the_run_without_leaders(case, shape, monkeypatch):
    _check(case, False, shape, monkeypatch)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("case", SHORT_CASES, ids=lambda c: f"W{c[0]}-{c[1]}-{c[2]}-n{c[3]}")
def test_a_leader_that_runs_out(case, shape, monkeypatch):
    _check(case, True, shape, monkeypatch)
