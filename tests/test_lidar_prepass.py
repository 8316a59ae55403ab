"""What LiDAR phase 1's agent pre-pass and the per-handle beam model hoist out of the beam passes
(csrc/mev_roadbound.h, csrc/mev_beams.h), on the host (tests/native/lidar_prepass_check.cpp):
the pre-pass's region and on-screen bits equal the per-lane comparisons they replace (one ulp either
side of every border, 0 and 750, negative, NaN and infinite coordinates); road_entry_safe_uniform with
the bits supplied returns road_entry_safe's bits over the grid of roadbound_regions_check.cpp; and
beam_model's fields have the bits of phase 3's former per-step expressions for 64, 96 and 128 beams at
fov 360 and 120, a reversed list and a single beam."""
import re
import subprocess

import native_build


def test_prepass_bits_and_beam_model():
    exe = native_build.build("lidar_prepass_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PREPASS OK" in r.stdout
    rows = re.findall(r"lanes (\d): (\d+) origin-direction pairs, (\d+) differ, (\d+) origins with other bits; origins: "
                      r"cross (\d+), vertical arm (\d+), horizontal arm (\d+), general (\d+); on screen (\d+), off (\d+)",
                      r.stdout)
    assert [int(x[0]) for x in rows] == [2, 3, 4]
    for x in rows:
        assert int(x[1]) >= 4104 * 76 * 76 and int(x[2]) == 0 and int(x[3]) == 0, x
        assert all(int(c) > 0 for c in x[4:]), x
    beams = re.findall(r"beams (\S+) +R +(\d+) .* (ok|DIFFER)", r.stdout)
    assert [b[0] for b in beams] == ["64/fov360", "64/fov120", "96/fov360", "96/fov120", "128/fov360", "128/fov120",
                                     "64/reversed", "1/fov360"], beams
    assert all(b[2] == "ok" for b in beams), beams
