"""csrc/head_loss.h on the host: the loss kernels' LDS carve and partial-row layout (HeadLayout, the
constexpr description the kernel and the launcher both use) compiled as a stand-alone program
(tests/host/head_loss_layout_check.cpp) with g++ under AddressSanitizer and UBSan and run as a
child process: all 32 (A, F) pairs for 4 and 5 stats, 16-B alignment of every carve offset and
float4-stored segment, 8-B alignment of the f64 sums, slot() a bijection, the total within 64 KB.
"""
import shutil
import subprocess

from helpers import REPO

CSRC = REPO / "3d-navigation-reinforcement-learning_amd" / "csrc"
DRIVER = REPO / "tests" / "host" / "head_loss_layout_check.cpp"
CXXFLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_head_loss_layout(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/host/head_loss_layout_check.cpp"
    exe = tmp_path / "head_loss_layout_check"
    r = subprocess.run([cxx, *CXXFLAGS, "-I", str(CSRC), str(DRIVER), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-4000:]}\n{p.stderr[-4000:]}"
    assert p.stdout.strip().splitlines()[-1] == "checked 64 layouts"
