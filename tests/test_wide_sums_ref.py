"""The premises of tests/test_gpu_wide_sums.py, pinned on the oracle (CPU only).  The oracle restates the reference and keeps its
column sums in `int`, so it cannot say what the library computes past 2^31; tests/wide_sums.py derives that from a small family
repeated r times.  Here: the restated vote is the oracle's, the identity holds on the oracle itself while r * S still fits, the
sums are never negative, and every configuration the GPU file uses meets the conditions under which the identity decides."""
import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.synth import synth_adversarial, synth_family

import score_gates as sg
import wide_sums as ws
from wide_sums import INT32_MAX, CONFIGS, check_premises, replicate, small_run, vote

FUZZ = [  # (family, parameters): the stop rule fires in some, the limit is reached in others, one stops at once
    (dict(n=40, L=120, W=14, K=70, seed=5, both_sides=True, minus_frac=0.3, n_run_frac=0.2, div=0.05), dict(when_to_stop=30)),
    (dict(n=25, L=90, W=20, K=80, seed=8, both_sides=True, minus_frac=0.5, n_run_frac=0.3), dict(when_to_stop=100)),
    (dict(n=33, L=100, W=9, K=30, seed=9, both_sides=True, minus_frac=0.2), dict(when_to_stop=5)),
    (dict(n=12, L=60, W=14, K=0, seed=10, both_sides=True), dict(when_to_stop=3)),
    (dict(n=50, L=80, W=40, K=60, seed=11, both_sides=True, minus_frac=0.4, n_run_frac=0.1, div=0.2), dict(when_to_stop=20, minimprovement=60)),
    (dict(n=20, L=70, W=14, K=69, seed=12, both_sides=True), dict(when_to_stop=1)),
]


def _fuzz_families():
    for kw, pk in FUZZ:
        fs = synth_family(**kw)
        yield fs, po.Params.named("14p43g", bandwidth=kw["W"], L=kw["L"], **pk)
    for seed in (300, 301):
        fs = synth_adversarial(seed, n_windows=10, L=110, W=20, K=70)
        yield fs, po.Params.named("repeatscout" if seed % 2 else "20p43g", bandwidth=20, L=110, when_to_stop=25)


def _both(cores, sequence, p, trace=True):
    c, m = cores.copy(), po.new_master(p.L)
    return c, m, [po.oracle_extend(d, c, sequence, m, p, trace=trace) for d in (1, 0)]


def test_restated_vote_is_the_oracles():
    """vote() on the oracle's traced sums gives back its return value, rows, limit warning and consensus -- on families where the stop
    rule fires early, late, at once, and where the limit L is reached -- and every traced sum is >= 0: a copy contributes
    max(best, 0) or its record plus the cap penalty, whichever is larger (ram_extend.c:1042-1061).  The unsigned hi / lo compare of
    the cell-parallel kernels' sums is correct only because of that."""
    fired = limit = 0
    for fs, p in _fuzz_families():
        for o in _both(fs.cores, fs.sequence, p)[2]:
            rows = o.rows_executed
            got = vote(o.col_sums, p.minimprovement, p.when_to_stop)
            assert got[:3] == (o.ret, rows, o.limit_warning)
            assert np.array_equal(got[3], o.col_base[:rows])
            assert vote(o.col_sums, p.minimprovement, p.when_to_stop, wrap=True)[:3] == got[:3]     # nothing to wrap here
            assert o.col_sums.min() >= 0
            fired += rows < p.L
            limit += rows == p.L
    assert fired >= 4 and limit >= 2


@pytest.mark.parametrize("r", [2, 3, 7])
def test_replication_identity_on_the_oracle(r):
    """While r * S fits int32 the oracle itself must obey the identity: the family repeated r times with r times the minimprovement
    goes where the small one goes, its sums are r * S, its per-copy results the small family's tiled."""
    for fs, p in _fuzz_families():
        c1, m1, small = _both(fs.cores, fs.sequence, p)
        assert r * max(int(o.col_sums.max()) for o in small) <= INT32_MAX and p.L * r * abs(p.minimprovement) <= INT32_MAX
        pr = po.Params(**{**p.__dict__, "minimprovement": r * p.minimprovement})
        cr, mr, big = _both(replicate(fs.cores, r), fs.sequence, pr)
        assert cr.n == r * fs.cores.n
        for o, b in zip(small, big):
            assert (b.ret, b.rows_executed, b.limit_warning) == (o.ret, o.rows_executed, o.limit_warning)
            assert np.array_equal(b.col_sums[:o.rows_executed], r * o.col_sums[:o.rows_executed])
        assert np.array_equal(mr, m1)
        for k in ("left_len", "right_len", "score"):
            assert np.array_equal(getattr(cr, k), np.tile(getattr(c1, k), r)), k


def test_vote_tells_wide_sums_from_wrapped_ones():
    """The restated rule itself: a sum of 2^31 wins wide and loses wrapped; a maximum above 2^31 holds wide and is lost wrapped."""
    S = np.array([[5, 2 ** 31, 7, 0], [1, 2, 3, 2 ** 31 + 10]], np.int64)
    wide, wrapped = vote(S, 3, 10), vote(S, 3, 10, wrap=True)
    assert list(wide[3]) == [1, 3] and list(wrapped[3]) == [2, 2]
    assert wide[0] == 2 and wrapped[0] == 1
    assert vote(np.zeros((0, 4), np.int64), 3, 10)[:3] == (0, 0, 0)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_configurations_meet_the_premises(name):
    """Every configuration of the GPU file, both directions, at every replication it is run with: the small run stays within int32,
    L * r * q does too, the wide vote on r * S is the small run, and above the edge the wrapped vote goes elsewhere.  The edge is a
    real one: r_lo keeps every executed sum within int32 and r_lo + 1 does not."""
    run = small_run(name)
    cfg = run.cfg
    neighbour = name in ws.BATCH_NEIGHBOURS
    reps = small_run(ws.BATCH_MIDDLE).replications() if neighbour else run.replications()
    for d in run.directions:
        o = run.direction(d)
        assert o.rows_executed > cfg.K // 2 and o.ret > cfg.K // 2              # the family does extend
        r_lo, r_hi = ws.edge_replications(o.col_sums, o.rows_executed)
        assert (run.overflows(d, r_lo), run.overflows(d, r_hi)) == (0, 1)
        firsts = [check_premises(run, d, r) for r in reps]
        if neighbour:
            assert firsts == [None] * len(reps)                                  # the neighbours of the batch never cross
        else:
            deep = ws.deep_replication(o.col_sums, o.rows_executed, cfg.deep_at)
            assert deep in reps and check_premises(run, d, deep) < cfg.deep_at * o.rows_executed
            assert any(f is not None for f in firsts) and any(f is None for f in firsts)


def test_configurations_are_on_the_right_side_of_the_route_gates():
    """The scoring systems against the gates restated in tests/score_gates.py: what each route of the GPU file needs in order to run."""
    def system(name):
        cfg = CONFIGS[name]
        return cfg, ws.params(cfg).matrix
    for name in ("rows14", "rows80", "family14", "family14_a", "family14_b", "profile14"):
        cfg, m = system(name)
        assert sg.go_ge_ok(cfg.go, cfg.ge)                                       # register-resident kernels
        assert not sg.pk_plan(cfg.W, cfg.go, cfg.ge, m).admitted and not sg.cp_value_range_ok(cfg.W, cfg.L, cfg.go, cfg.ge, m)
    for name in ("packed14", "packed14_short"):
        cfg, m = system(name)
        assert sg.pk_plan(cfg.W, cfg.go, cfg.ge, m).admitted and sg.go_ge_ok(cfg.go, cfg.ge)
        for d in small_run(name).directions:                                     # packed_rows >= L - W needs the rows to get there
            r0 = ws.pk_first_row(d, small_run(name).fs.cores, cfg.W, cfg.L)
            assert (r0 > 0) == (name == "packed14_short")                        # short cores: the int32 kernel runs the first rows
            assert cfg.L - cfg.W + r0 <= small_run(name).direction(d).rows_executed < cfg.L      # ... and the stop rule fires all the same
    cfg, m = system("cells40")
    assert sg.cp_value_range_ok(cfg.W, cfg.L, cfg.go, cfg.ge, m)
    for name in ("family14", "family14_a", "family14_b"):
        assert CONFIGS[name].max_copies == 512 and CONFIGS[name].W in (14, 20, 40)


def test_one_workgroup_cell_parallel_kernel_cannot_reach_the_edge():
    """No GPU case for the one-workgroup cell-parallel kernel: its gate keeps every cell, hence every copy's contribution, below
    2^23 ((L + 2W + 4) mx < 2^23, score_gates.cp_value_range_ok), and one workgroup holds at most 512 threads / 2 lanes = 256
    copies: 256 (2^23 - 1) < 2^31.  Checked on the systems at the edge of that gate and on the cell-parallel configuration."""
    edge = [(127, 128, -300, -20, 200, 14), (5, 4, -29000, -1000, 247, 14), (5, 4, 0, -41943, 100, 14), (127, 127, -4000, -17, 2000, 40),
            (CONFIGS["cells40"].P, CONFIGS["cells40"].mn, CONFIGS["cells40"].go, CONFIGS["cells40"].ge, CONFIGS["cells40"].L, 40)]
    for P, mn, go, ge, L, W in edge:
        m = sg.shape_matrix(P, mn)
        assert sg.cp_value_range_ok(W, L, go, ge, m)
        per_copy = (L + 2 * W + 4) * sg._mx(go, ge, m)
        assert per_copy < 2 ** 23 and 256 * per_copy <= INT32_MAX
    assert 256 * (2 ** 23 - 1) <= INT32_MAX < 257 * 2 ** 23
