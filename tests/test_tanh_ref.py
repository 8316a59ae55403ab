"""tanh_c (csrc/mev_act.h, the rollout policies' tanh as stated f32 arithmetic) keeps its stated properties and its
recorded error against tanh in double: tests/native/tanh_check.cpp on a strided sweep of every binade and
exhaustively around every value the sequence branches on (`tanh_check exhaustive` visits every float -- DESIGN.md
3.2n records its figures, which the program asserts rounded up to whole ulps)."""
import subprocess

import native_build


def test_tanh_c_properties_and_error():
    exe = native_build.build("tanh_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "TANH OK" in r.stdout
