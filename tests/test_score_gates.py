"""The premises of the packed-row admission plan (csrc/ramx_packed.hip ramx_pk_plan, restated in tests/score_gates.py) against
the oracle's own rows -- no GPU.

The packed kernel keeps a flank's row as int16 relative to a base that follows the row's best cell every 16th row; its adds
saturate, so it is exact only if the plan's two bounds are TRUE for every admitted scoring system: how far the best cell moves
within 16 rows (`lag - PK_REBASE`) and how far an in-bounds cell lies below its row's best (`spread`).  Here both are measured on
the oracle's rows for six shapes of scoring system, each at the largest scale the plan admits.

Measured with the plan as it was before this test existed (lag = PK_REBASE + 16 max(P, mn)), each shape at the largest scale THAT
plan admitted, 130 flanks x 200 columns: the largest move of a best cell within 16 rows was
  W = 14: (b) (P, mn, GO, GE) = (38, 38, 0, 380): 5,700 where 608 were allowed; (c) (77, 77, 4620, 154): 7,007 against 1,232;
  W = 40: (b) (13, 13, 0, 130): 2,080 against 208; (c) (37, 37, 2220, 74): 3,404 against 592;
(a), (d), (e), (f) stayed within it ((d) and (f) reach 16 P exactly).  Cause: a flank that ends while aligned has its best cell on
the far boundary, and only a deletion carries it on.  The plan now takes max(16 P, 16 mn, GO + GE + 15 max(mn, GE)) -- the argument
is in score_gates.pk_drift16 -- and (b) and (c) reach that bound exactly at W = 40 (1,920 and 3,036), to within 1 % at W = 14.  The
spread bound is loose everywhere: at most 62 % of it is used, by (d) at W = 14."""
import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import new_master

import score_gates as sg
from score_gates import SHAPES, edge_scale, gate_family, shape_params

SENT = -987654321            # what the reference writes into cells beyond a flank's end


def oracle_rows(fs, p):
    """The right extension's kept rows, cell by cell: best[r][n] (the oracle's own row bests), lowest[r][n] (lowest in-bounds
    cell; best where the row has none), on_far[r][n] (the best cell is the flank's last base), real[r][n]."""
    N, W, L = fs.cores.n, p.bandwidth, p.L
    B = 2 * W + 1
    c = fs.cores
    assert not c.orient.any() and c.right_ext.all()
    o = po.oracle_extend(1, c.copy(), fs.sequence, new_master(L), p, trace=True, row_trace=True)
    assert o.rows_executed == L
    cons = o.col_base
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    score = np.zeros((2, N, B, 2), np.int32)
    for off in range(-W, W + 1):
        score[1, :, off + W, :] = 0 if off == 0 else abs(off) * p.gapextn + p.gapopen
    best = np.zeros((L, N), np.int64)
    lowest = np.zeros((L, N), np.int64)
    on_far = np.zeros((L, N), bool)
    t_hi = c.upper - c.right_pos - 1                      # flank position of the last base
    t_lo = c.lower - c.right_pos - 1
    offs = np.arange(-W, W + 1)
    for r in range(L):
        for n in range(N):
            b, bidx = po.oracle_nw_row(1, r, n, N, int(cons[r]), int(c.left_pos[n]), int(c.right_pos[n]), 0, score.reshape(-1),
                                       int(c.lower[n]), int(c.upper[n]), seq, p.matrix, p.gapopen, p.gapextn, W)
            assert b == o.row_best[r, n]
            best[r, n] = b
            on_far[r, n] = bidx == t_hi[n]
        cells = score[r % 2].max(axis=2).astype(np.int64)                 # [N][B]
        inb = (r + offs[None, :] <= t_hi[:, None]) & (r + offs[None, :] >= t_lo[:, None])
        assert not (cells[inb] == SENT).any()
        lowest[r] = np.where(inb, cells, np.iinfo(np.int64).max).min(axis=1)
        lowest[r] = np.where(inb.any(axis=1), lowest[r], best[r])
    real = best > SENT // 2
    return best, lowest, on_far, real


def measure(shape, W, n=130, L=200, seed=5):
    s = edge_scale(shape, W)
    p = shape_params(shape, s, W, L)
    plan = sg.pk_plan(W, p.gapopen, p.gapextn, p.matrix)
    best, lowest, on_far, real = oracle_rows(gate_family(n, L, W, seed), p)
    drift = 0
    for k in range(1, 17):
        ok = real[k:] & real[:-k]
        drift = max(drift, int(np.abs(best[k:] - best[:-k])[ok].max()))
    spread = int((best - lowest)[real].max())
    run = np.zeros(best.shape[1], np.int64)              # longest run of rows with the best cell on the far boundary
    longest = 0
    for r in range(L):
        run = np.where(on_far[r] & real[r], run + 1, 0)
        longest = max(longest, int(run.max()))
    rise = int(np.where(real, best, 0).max())
    # the kernel's base, flank by flank: the best cell of the row the flank enters with, then -- looked at every 16th row -- the
    # row's best cell once that is more than PK_REBASE away (a wave re-centres all its flanks when one of them is: only closer)
    base = best[0].copy()
    above = below = low = 0
    for r in range(L):
        ok = real[r]
        if ok.any():
            above = max(above, int((best[r] - base)[ok].max()))
            below = max(below, int((base - best[r])[ok].max()))
            low = max(low, int((base - lowest[r])[ok].max()))
        if r % 16 == 15:
            base = np.where(ok & (np.abs(best[r] - base) > sg.PK_REBASE), best[r], base)
    return dict(scale=s, plan=plan, drift=drift, spread=spread, far_rows=longest, rise=rise, above=above, below=below, low=low, p=p)


@pytest.mark.parametrize("W", [14, 40])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_packed_plan_premises_hold_on_the_oracles_rows(shape, W):
    m = measure(shape, W)
    plan, p = m["plan"], m["p"]
    P, mn = sg.p_mn(p.matrix)
    GO, GE = -p.gapopen, -p.gapextn
    print(f"shape {shape} W={W}: scale {m['scale']} (P, mn, GO, GE) = {(P, mn, GO, GE)} plan total {plan.total} spread {plan.spread} "
          f"lag {plan.lag}; measured drift {m['drift']} spread {m['spread']} far-boundary rows {m['far_rows']} rise {m['rise']}; "
          f"re-centred every 16th row: best above base {m['above']} below {m['below']} lowest cell below base {m['low']}")
    over = shape_params(shape, m["scale"] + 1, W, 200)
    assert plan.admitted and not sg.pk_plan(W, over.gapopen, over.gapextn, over.matrix).admitted      # really the edge
    # the case is not a soft one
    assert m["far_rows"] >= 16
    if shape == "d":
        assert m["rise"] > 2 * sg.PK_REBASE
    if shape in "bc":
        assert m["drift"] > 16 * max(P, mn)
    # the plan's premises
    assert m["drift"] <= plan.lag - sg.PK_REBASE
    assert m["spread"] <= plan.spread
    # and what the kernel forms from them, MEASURED against a base re-centred as the kernel does it: the lag of the base, sub + go
    # and e of the lowest in-bounds cell, a substitution onto the best one
    assert max(m["above"], m["below"]) <= plan.lag
    assert m["low"] + mn + GO + GE < sg.PK_LIMIT - sg.PK_MARGIN + 1
    assert m["above"] + P < sg.PK_LIMIT - sg.PK_MARGIN + 1


def test_gates_at_their_edges():
    """The restated gates themselves: each flips exactly where its inequality does."""
    m = sg.shape_matrix(127, 128)
    assert sg.fast_pack_ok(14, 300, -5, -1, m) and sg.cp_value_range_ok(14, 300, -5, -1, m)
    for bad in (sg.shape_matrix(128, 1), sg.shape_matrix(1, 129)):
        assert not sg.fast_pack_ok(14, 300, -5, -1, bad) and not sg.cp_value_range_ok(14, 300, -5, -1, bad)
    m = sg.shape_matrix(5, 4)
    # (L + 2W + 4) mx against 2^27 and 2^23
    assert sg.fast_pack_ok(14, 300, -400000, -4270, m) and not sg.fast_pack_ok(14, 300, -400000, -4271, m)
    assert (300 + 32) * 404270 < (1 << 27) <= (300 + 32) * 404271
    # ... which no kernel that has a fast band sees below L + 2W + 4 = 4096: they all need go + ge >= -32768
    m127 = sg.shape_matrix(127, 128)
    assert sg.fast_pack_ok(14, 4063, -32000, -768, m127) and not sg.fast_pack_ok(14, 4064, -32000, -768, m127)
    assert sg.go_ge_ok(-32000, -768) and (4063 + 32) * 32768 < (1 << 27) == (4064 + 32) * 32768
    assert sg.cp_value_range_ok(14, 247, -29000, -1000, m) and not sg.cp_value_range_ok(14, 248, -29000, -1000, m)
    assert (247 + 32) * 30000 < (1 << 23) <= (248 + 32) * 30000
    assert sg.cp_value_range_ok(14, 10, 0, -41943, m) and not sg.cp_value_range_ok(14, 10, 0, -41944, m)
    assert sg.go_ge_ok(-32000, -768) and not sg.go_ge_ok(-32000, -769)
    # P and mn come from the class table only: entries outside [0..3] x {0..7, 99} do not count
    m2 = m.copy().reshape(100, 100)
    m2[4, 0] = 30000
    m2[0, 8] = -30000
    assert sg.p_mn(m2.reshape(-1)) == (5, 4)
    # the four built-in matrices stay admitted at every width, with thousands to spare
    for name in ("14p43g", "20p43g", "25p43g", "repeatscout"):
        for W in sg.PK_WIDTHS:
            p = po.Params.named(name)
            plan = sg.pk_plan(W, p.gapopen, p.gapextn, p.matrix)
            assert plan.admitted and plan.total <= sg.PK_LIMIT - 5000, (name, W, plan)
    # largest_scale: the edge of a monotone gate
    assert sg.largest_scale(lambda s: s <= 37) == 37 and sg.largest_scale(lambda s: False) == 0
    assert sg.largest_scale(lambda s: True, hi=1000) == 1000 and sg.largest_pk_scale(14, np.zeros(10000, np.int32), 0, 0) == 1 << 20
    for W in sg.PK_WIDTHS:
        s = sg.largest_pk_scale(W, sg.shape_matrix(1, 1), -150, -1)
        inside = sg.scale_system(sg.shape_matrix(1, 1), -150, -1, s)
        outside = sg.scale_system(sg.shape_matrix(1, 1), -150, -1, s + 1)
        assert sg.pk_plan(W, inside[1], inside[2], inside[0]).admitted and not sg.pk_plan(W, outside[1], outside[2], outside[0]).admitted
