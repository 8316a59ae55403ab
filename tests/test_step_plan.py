"""plan_step (csrc/mev_plan.h) chooses, for every shape of a grid around its thresholds and
for the named shapes, the kernel, launch and reported pack / split that the policy functions
and launch ladders before it chose (tests/native/step_plan_check.cpp)."""
import subprocess

import native_build


def test_step_plan_matches_recorded_choices():
    exe = native_build.build("step_plan_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    assert "STEP PLAN OK" in r.stdout
