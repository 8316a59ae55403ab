"""Build helpers for the host-side native checks (tests/native/*.cpp)."""
import hashlib
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "marl-traffic-intersection_amd", "csrc")
OUT = os.path.join(tempfile.gettempdir(), f"mev_native_tests_{os.getuid()}")  # (one per user: /tmp is shared)


def build(name: str, c_sources=()) -> str:
    """tests/native/<name>.cpp, plus plain-C sources (compiled as C and linked in)."""
    os.makedirs(OUT, exist_ok=True)
    src = os.path.join(HERE, "native", name + ".cpp")
    deps = [src] + list(c_sources) + sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h"))
    # the program's name carries a digest of its sources: OUT is shared by every checkout of this user, and
    # file times do not tell a program built from another checkout's sources from this one's
    dig = hashlib.sha256()
    for d in deps:
        with open(d, "rb") as f:
            dig.update(os.path.basename(d).encode() + b"\0" + f.read() + b"\0")
    tag = dig.hexdigest()[:16]
    exe = os.path.join(OUT, f"{name}_{tag}")
    if os.path.exists(exe):
        return exe
    objs = []
    for c in c_sources:  # the same flags as oracle.build()
        o = os.path.join(OUT, f"{os.path.basename(c)}_{tag}_{os.getpid()}.o")
        subprocess.run(["gcc", "-O2", "-std=c11", "-ffp-contract=off", "-c", c, "-o", o], check=True,
                       capture_output=True)
        objs.append(o)
    # same rounding discipline as the device build: no contraction, plain x86-64
    tmp = f"{exe}.{os.getpid()}.tmp"  # (renamed into place: another process may be building the same program)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-I", CSRC, src, *objs, "-o", tmp,
                    "-lm"], check=True, capture_output=True)
    os.replace(tmp, exe)
    for o in objs:
        os.remove(o)
    return exe
