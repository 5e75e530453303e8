"""The host side of the forward-backward check (csrc/vio_flow_host.h: the config check, flow_back_args, the unpacking of the backward
rows over items of 0, 1 and 140 points; csrc/vio_flow_math.h: the verdict), compiled by g++ with tests/cpp/flow_back_host_main.cpp into
a stand-alone program under ASan and UBSan, with no HIP header, and run directly.  It is never loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visual-inertial-odometry_amd", "csrc")


def test_host_side_under_the_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.fail("g++ not found")
    exe = tmp_path / "flow_back_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-g", "-I" + CSRC, "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "flow_back_host_main.cpp")])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
