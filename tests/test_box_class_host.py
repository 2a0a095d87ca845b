"""The exact-box classifier of vn_create (csrc/env_plan.h: room_is_exact_box,
rooms_box_exact) decides which envs launch the step kernels that compute the
ray record instead of loading it.  tests/host/test_box_class.cpp is a
stand-alone program with its own expectations (boxes of five sizes; a pillar,
an opened ceiling, a doubled wall, a room without interior, mixed sets); this
test builds it under g++ with AddressSanitizer and UBSan and runs it as a child
process.
"""
import shutil
import subprocess

from helpers import REPO

CSRC = REPO / "3d-navigation-reinforcement-learning_amd" / "csrc"
DRIVER = REPO / "tests" / "host" / "test_box_class.cpp"
CXXFLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
            "-fno-sanitize-recover=all"]


def test_box_classifier(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/host/test_box_class.cpp"
    exe = tmp_path / "test_box_class"
    r = subprocess.run([cxx, *CXXFLAGS, "-I", str(CSRC), "-I", str(REPO / "include"), str(DRIVER), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout}\n{p.stderr[-4000:]}"
    lines = p.stdout.splitlines()
    assert lines[-1] == "ok" and "WRONG" not in p.stdout, p.stdout
    assert len(lines) == 2 * 5 + 1 + 2 * 3 + 1 + 3 + 1, p.stdout      # every case printed its line
