"""plan_step (csrc/mev_plan.h) with StepShape::world set -- a handle whose world is the
reference's: every chosen key has a kernel, the plan is the member-0 plan in everything but
StepKey::wc, and wc is set exactly where a specialised kernel exists
(tests/native/step_plan_world_check.cpp)."""
import subprocess

import native_build


def test_step_plan_world_only_adds_the_wc_field():
    exe = native_build.build("step_plan_world_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    assert "STEP PLAN WORLD OK" in r.stdout
