"""bench.py's launcher contract, the part that needs no GPU: `python3 bench.py --gpus N` with fewer than N devices is an error
(exit 2, nothing on stdout), never a silent one-GPU run."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_more_ranks_than_devices_is_an_error():
    import torch
    n = torch.cuda.device_count() + 1 if torch.cuda.device_count() > 0 else 2
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "RAMX_BENCH_BACKEND"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 2, (r.returncode, r.stderr[-400:])
    assert r.stdout.strip() == ""
    assert "device(s) visible" in r.stderr


def test_dump_outputs_writes_float64_and_caps_the_size(tmp_path, monkeypatch):
    """--dump-outputs: every array as float64 DIR/<name>.npy; above the cap the per-flank arrays are one fixed seeded sample."""
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    cons = (np.arange(3000) % 4).astype(np.int8)
    ext = np.arange(50000, dtype=np.int32)
    sc = 3 * ext
    bench.dump_outputs(str(tmp_path / "all"), 1500, cons, ext, sc)
    got = {f[:-4]: np.load(tmp_path / "all" / f) for f in os.listdir(tmp_path / "all")}
    assert sorted(got) == ["consensus", "extension_len", "ret", "score"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["ret"].tolist() == [1500] and np.array_equal(got["consensus"], cons) and np.array_equal(got["score"], sc)

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 256 << 10)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), 1500, cons, ext, sc)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 256 << 10
    idx = np.load(tmp_path / "a" / "sample_index.npy")
    assert 0 < len(idx) < len(ext) and np.array_equal(idx, np.load(tmp_path / "b" / "sample_index.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "score.npy"), 3 * idx)
