"""The CPU walker of tests/align_ref.py pinned on the oracle alone (no GPU): its score is the oracle's best cell at the end
row and equals the rescored path, on five corpora whose paths hold every kind of move and tie -- asserted, so that a corpus
cannot go soft unnoticed.  And the C-ABI declares and exports the two entries the GPU tests compare against it."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd import _lib
from repeatafterme_amd.datamodel import new_master
from repeatafterme_amd.synth import synth_family

import align_ref as ar
from helpers import ROOT

# (matrix, W, L, n, seed, extra parameters, affine gap costs: opening differs from extending)
CORPORA = [
    ("repeatscout", 14, 80, 40, 7, dict(match=2, mismatch=-2, gap=-6, cappenalty=-10), False),
    ("repeatscout", 5, 60, 37, 8, dict(match=1, mismatch=-1, gap=-2, cappenalty=-10), False),
    ("14p43g", 14, 80, 40, 9, {}, True),
    ("25p43g", 20, 120, 37, 10, dict(cappenalty=-10), True),
    ("14p43g", 5, 60, 65, 11, {}, True),
]


@pytest.mark.parametrize("matrix,W,L,n,seed,kw,affine", CORPORA)
def test_walker_score_is_the_oracles_and_the_rescored_one(matrix, W, L, n, seed, kw, affine):
    fs = synth_family(n, L, W, K=L // 2, seed=seed, both_sides=True, minus_frac=0.4, n_run_frac=0.1)
    p = po.Params.named(matrix, bandwidth=W, L=L, when_to_stop=30, **dict(kw))
    cores, master = fs.cores.copy(), new_master(L)
    seq = np.ascontiguousarray(fs.sequence, np.int8)
    tot = dict(flanks=0, n_ins=0, n_del=0, ties_state=0, ties_insdel=0, early_end=0, gap_end=0, edge_end=0, bound_end=0, none=0)
    for direction in (1, 0):
        before = cores.copy()
        o = po.oracle_extend(direction, cores, seq, master, p, trace=True, row_trace=True)
        cons = o.col_base[:o.ret]
        idx, results = ar.walk_family(direction, before, seq, p, cons)
        for i, res in zip(idx, results):
            tag = (matrix, W, direction, i)
            tot["flanks"] += 1
            # the walker's own rows are the oracle loop's rows
            assert res["row_best"] == list(o.row_best[:o.ret, i]) and res["row_best_idx"] == list(o.row_best_idx[:o.ret, i]), tag
            if res["end_row"] < 0:
                tot["none"] += 1
                continue
            assert res["score"] == o.row_best[res["end_row"], i] == max(res["row_best"]), tag
            assert res["end_idx"] == o.row_best_idx[res["end_row"], i], tag
            assert ar.rescore(res, ar.Flank(direction, before, i, W), seq, p, cons) == res["score"], tag
            assert ar.consumed_is_contiguous(res), tag
            # the loop's own trimmed end point (ram_extend.c:1234-1247) is this end cell
            got_len = (cores.right_len if direction else cores.left_len)[i]
            assert got_len == (res["end_idx"] + 1 if res["end_idx"] >= 0 else 0), tag
            for k in ("n_ins", "n_del", "ties_state", "ties_insdel", "early_end", "gap_end", "edge_end", "bound_end"):
                tot[k] += res[k]
    assert tot["flanks"] >= n
    assert tot["n_ins"] > 0 and tot["n_del"] > 0 and tot["ties_state"] > 0 and tot["early_end"] > 0, tot
    if affine:
        assert tot["ties_insdel"] > 0, tot
    # what these corpora do not hold (the constructed cases of the GPU tests do)
    assert tot["none"] == 0 and tot["edge_end"] == 0 and tot["gap_end"] == 0, tot


def test_header_declares_and_library_exports_the_align_entries():
    txt = open(os.path.join(ROOT, "include", "ramx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert os.path.exists(_lib.LIB_PATH), "build libramx.so first (__graft_entry__.build())"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ramx_dev_align", "ramx_set_align_sink"):
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} is not declared in include/ramx.h"
        assert hasattr(lib, name), f"{name} is not exported by libramx.so"
        assert name in _lib.EXPORTS
