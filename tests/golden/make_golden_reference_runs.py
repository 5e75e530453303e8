#!/usr/bin/env python3
"""Generates tests/golden/reference_runs/*.npz: what the COMPILED REFERENCE (oracle/_ref/libvio_ref.so) returns on the inputs of the
tests that compare the oracle with it (the `ref_runs` fixture of tests/conftest.py).  Where the reference is, those tests compute
its side live; everywhere else they read it from these files.  This script runs them once with VIO_RECORD_REFERENCE=1, which makes
the fixture write what it computed.

Run only in the container that mounts /root/reference:   python tests/golden/make_golden_reference_runs.py
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TESTS = ["tests/test_oracle_vs_reference.py", "tests/test_marg_kat.py", "tests/test_monoba.py", "tests/test_real_imu.py",
         "tests/test_stream.py", "tests/test_xyz_landmarks.py", "tests/test_feature_manager_golden.py"]

if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import __graft_entry__
    __graft_entry__.build()         # (the listed modules also hold tests of the product library's host code)
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libvio_ref.so")):
        raise SystemExit("oracle/_ref/libvio_ref.so was not built: the reference tree is not here")
    env = dict(os.environ, VIO_RECORD_REFERENCE="1")
    sys.exit(subprocess.call([sys.executable, "-m", "pytest", "-q", "-m", "not gpu"] + TESTS, cwd=ROOT, env=env))
