"""mev_roadbound.h on the host (tests/native/roadbound_check.cpp): every bound
is safe against the reference's road predicate, lidar_body's march with the
old and the entry bound stops where the probe-by-probe march stops, and the
entry bound needs no more march iterations than road_safe."""
import subprocess

import native_build


def test_road_bounds_are_safe_exact_and_no_looser():
    exe = native_build.build("roadbound_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ROADBOUND OK" in r.stdout
