"""obs_split (csrc/mev_obs_chunks.h), the cut of an observation row's head or LiDAR block into
16-byte chunks and single floats that the step kernel stores by: exhaustively over base phase
0..3 floats, obs_ld 31+LS .. 31+LS+40, LS 1..128, rows 0..15 and both slice starts, every float
of the slice is written exactly once, by an aligned chunk wholly inside the slice or a single
float, and nothing outside it (tests/native/obs_chunks_check.cpp); the same program again as a
stand-alone binary under AddressSanitizer and UBSan, its rows in a heap block of their exact size."""
import os
import subprocess

import native_build


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "OBS CHUNKS OK" in r.stdout
    assert " 0 failures" in r.stdout


def test_obs_split_covers_every_slice_exactly_once():
    _run(native_build.build("obs_chunks_check"))


def test_obs_split_sanitized():
    src = os.path.join(native_build.HERE, "native", "obs_chunks_check.cpp")
    os.makedirs(native_build.OUT, exist_ok=True)
    exe = os.path.join(native_build.OUT, "obs_chunks_check_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", native_build.CSRC, src, "-o", exe], check=True, capture_output=True)
    _run(exe)
