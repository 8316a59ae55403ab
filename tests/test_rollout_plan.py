"""plan_rollout (csrc/mev_plan.h): the k_rollout row of the rollout tests' shapes, the refused shapes
(obs_dim 31 + 129, a fused LDS above 64 KB) and the launch's invariants over a grid of shapes
(tests/native/rollout_plan_check.cpp)."""
import subprocess

import native_build


def test_rollout_plan():
    exe = native_build.build("rollout_plan_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    assert "ROLLOUT PLAN OK" in r.stdout
