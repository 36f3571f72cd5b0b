#!/usr/bin/env python3
"""Records the cases of tests/class_table.py ref_cases() -- the scoring systems whose 36 class-table entries can be told apart, on
soft-masked families and adversarial sets -- and what the COMPILED REFERENCE (oracle/_ref, `make -C oracle ref`) gives for them
into tests/golden/class_table_vectors.npz.  Run where the reference is built:

    python tests/golden/make_class_table_golden.py

The file holds data only: per family its sequence and cores (once, whatever the system), per case the two return values, the
consensus and the per-copy lengths and scores.  tests/test_class_table_ref.py runs the oracle against it.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import pyoracle as po  # noqa: E402
import class_table as ct  # noqa: E402

CORE_FIELDS = ("left_pos", "right_pos", "lower", "upper", "orient", "left_ext", "right_ext", "seq_idx")
OUT = os.path.join(HERE, "class_table_vectors.npz")


def main():
    assert po.have_ref(), "build oracle/_ref first (make -C oracle ref)"
    data, fam_of, cases = {}, {}, []
    rets, masters, per_copy = [], [], []
    for kind, seed, W, name in ct.ref_cases():
        fs = ct.ref_family(kind, seed, W)
        key = (kind, seed, W)
        if key not in fam_of:
            j = fam_of[key] = len(fam_of)
            data[f"f{j}_sequence"] = fs.sequence
            data[f"f{j}_cores"] = np.array([getattr(fs.cores, f) for f in CORE_FIELDS], np.int64)
            data[f"f{j}_boundaries"] = fs.boundaries
        p = ct.system(name, W, ct.REF_L)
        c, m = fs.cores.copy(), po.new_master(p.L)
        rr = po.ref_extend(1, c, fs.sequence, m, p, boundaries=fs.boundaries)
        rl = po.ref_extend(0, c, fs.sequence, m, p, boundaries=fs.boundaries)
        cases.append((fam_of[key], ("soft", "adversarial").index(kind), seed, W, ct.SYSTEMS.index(name)))
        rets.append((rr.ret, rl.ret))
        masters.append(m.copy())
        per_copy.append(np.array([c.left_len, c.right_len, c.score], np.int32))
    data["cases"] = np.array(cases, np.int32)               # (family, kind, seed, W, system)
    data["systems"] = np.array(ct.SYSTEMS)
    for name in ct.SYSTEMS:                                  # the scoring systems as the reference was handed them
        m, go, ge = ct.matrix_of(name)
        data[f"table_{name}"] = np.array([[m[a * 100 + b] for b in ct.CLASS_CODES] for a in range(4)], np.int32)
        data[f"gaps_{name}"] = np.array([go, ge], np.int32)
    p = ct.system("distinct", 14, ct.REF_L)
    data["stop"] = np.array([p.cappenalty, p.minimprovement, p.L, p.when_to_stop], np.int32)
    data["ret"] = np.array(rets, np.int32)
    data["master"] = np.array(masters, np.int8)
    data["per_copy"] = np.concatenate(per_copy, axis=1)      # [left_len, right_len, score][copies of case 0, of case 1, ...]
    np.savez_compressed(OUT, **data)
    print(len(cases), "cases,", len(fam_of), "families,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
