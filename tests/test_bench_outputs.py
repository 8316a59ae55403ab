"""bench.py --dump-outputs and the plain / --full split: the writer on the CPU (names,
float32, the 64 MB budget and its seeded sample of envs), and one short plain run on the
GPU (the line keeps its keys, runs neither the gather phase nor the CPU baseline, and
writes what the last timed step computed)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _fake_outputs(E):
    import torch
    g = torch.Generator().manual_seed(1)
    return {"obs": torch.rand((E, 8, 95), generator=g), "reward": torch.rand((E, 8), generator=g),
            "done": torch.randint(0, 2, (E, 8), generator=g, dtype=torch.uint8),
            "step": torch.arange(E, dtype=torch.int32)}


def test_dump_writes_every_array_as_float32(tmp_path):
    import bench
    out = _fake_outputs(50)
    bench.dump_outputs(str(tmp_path / "d"), out)
    assert sorted(os.listdir(tmp_path / "d")) == ["done.npy", "obs.npy", "reward.npy", "step.npy"]
    for k, v in out.items():
        a = np.load(tmp_path / "d" / f"{k}.npy")
        assert a.dtype == np.float32 and a.shape == tuple(v.shape)
        assert np.array_equal(a, v.numpy().astype(np.float32)), k


def test_dump_samples_the_same_envs_above_the_budget(tmp_path):
    import bench
    out = _fake_outputs(5000)  # 15.4 MB as float32
    budget = 1_000_000
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out, budget=budget)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["done.npy", "env_index.npy", "obs.npy", "reward.npy", "step.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= budget
    idx = np.load(tmp_path / "a" / "env_index.npy")
    assert idx.dtype == np.float32 and len(idx) > 300 and np.all(np.diff(idx) > 0)
    pick = idx.astype(np.int64)
    for k, v in out.items():
        a, b = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert np.array_equal(a, b), k  # the same sample every time
        assert np.array_equal(a, v.numpy()[pick].astype(np.float32)), k
    assert np.array_equal(np.load(tmp_path / "a" / "step.npy"), idx)  # (step was arange(E): rows line up)


def test_dump_names_other_ranks(tmp_path):
    import bench
    bench.dump_outputs(str(tmp_path), _fake_outputs(4), rank=3)
    assert sorted(os.listdir(tmp_path)) == ["done.rank3.npy", "obs.rank3.npy", "reward.rank3.npy", "step.rank3.npy"]


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_last_step(tmp_path):
    K, W, E = 3, 2, 4096
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup",
                        str(W), "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(r.stdout.strip().splitlines()) == 1, r.stdout
    d = json.loads(r.stdout)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == K and d["warmup"] == W and d["ms_per_step"] > 0
    # value and ms_per_step are the same measurement (ms_per_step is rounded to 5 decimals)
    assert d["value"] == pytest.approx(E * 8 * 1e3 / d["ms_per_step"], rel=6e-6 / d["ms_per_step"] + 1e-6)
    assert d["gather_to_root"] is None and d["cpu_baseline"] is None  # (--full's)
    shapes = {"obs": (E, 8, 95), "reward": (E, 8), "done": (E, 8), "status": (E, 8), "terminated": (E,),
              "truncated": (E,), "agents_alive": (E,), "step": (E,)}
    assert sorted(os.listdir(tmp_path / "out")) == sorted(f"{k}.npy" for k in shapes)
    got = {k: np.load(tmp_path / "out" / f"{k}.npy") for k in shapes}
    for k, s in shapes.items():
        assert got[k].dtype == np.float32 and got[k].shape == s and np.isfinite(got[k]).all(), k
    assert np.all(got["step"] == W + K)  # the last timed step's outputs (no env ends this early)
    assert np.all(got["agents_alive"] == 8) and not got["terminated"].any()
