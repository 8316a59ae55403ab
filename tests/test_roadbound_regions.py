"""road_entry_safe_uniform (csrc/mev_roadbound.h), phase 1's entry bound specialised by the road
region of the shared start point, returns the bits of the general road_entry_safe: origins on a
lattice and one ulp either side of every region border, 4096 angles and the axis directions, roads
of 2, 3 and 4 lanes (tests/native/roadbound_regions_check.cpp).  Every region must occur."""
import re
import subprocess

import native_build


def test_uniform_entry_bound_has_the_general_forms_bits():
    exe = native_build.build("roadbound_regions_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "REGIONS OK" in r.stdout
    rows = re.findall(r"lanes (\d): (\d+) origin-direction pairs, (\d+) differ; origins: cross (\d+), "
                      r"vertical arm (\d+), horizontal arm (\d+), general (\d+)", r.stdout)
    assert [int(x[0]) for x in rows] == [2, 3, 4]
    for x in rows:
        assert int(x[1]) >= 4104 * 61 * 61 and int(x[2]) == 0, x
        assert all(int(c) > 0 for c in x[3:]), x
