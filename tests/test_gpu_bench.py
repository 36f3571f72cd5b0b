"""bench.py on the GPU, small workload: a plain run times exactly --steps steps, runs none of the --full legs, and
--dump-outputs writes what the last timed step computed -- equal to the oracle on the same synthetic set."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd.datamodel import new_master
from repeatafterme_amd.scoring import get_matrix
from repeatafterme_amd.synth import synth_family

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_last_step_equal_to_the_oracle(tmp_path):
    N, L, W = 1000, 600, 40
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "RAMX_BENCH_BACKEND"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--flanks", str(N), "--L", str(L), "--bandwidth", str(W), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-800:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["full"] is False
    assert line["unit"] == "flank-bp/s" and line["higher_is_better"] is True and line["dtype"] == "int32"
    assert line["checks"] is None and line["cpu_baseline"] is None and line["seam1"] is None and line["configs1_n1000"] is None

    got = {n: np.load(tmp_path / f"{n}.npy") for n in ("ret", "consensus", "extension_len", "score")}
    assert all(a.dtype == np.float64 for a in got.values())

    mat, go, ge = get_matrix("14p43g")
    fs = synth_family(N, L, W, K=1500, seed=1)          # bench.py's own set for one GPU
    p = po.Params(bandwidth=W, cappenalty=-90, minimprovement=27, L=L, when_to_stop=L, l=1, gapopen=go, gapextn=ge, matrix=mat)
    c = fs.cores.copy()
    m = new_master(L)
    s0 = c.score.copy()
    o = po.oracle_extend(1, c, fs.sequence, m, p)
    assert int(got["ret"][0]) == o.ret
    assert np.array_equal(got["consensus"], m[L + 1:L + 1 + o.rows_executed])
    assert np.array_equal(got["extension_len"], c.right_len)
    assert np.array_equal(got["score"], c.score - s0)
