"""The forward-backward check's restatement (tests/flow_back_reference.py) on its fixture: the outcome counts the fixture was built to
reach, in both modes and at two level counts, and the verdict function of csrc/vio_flow_math.h compiled for the host against the
restatement bit for bit (the way tests/test_flow_host_mirror.py holds the rest of that header)."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_back_reference as fb  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visual-inertial-odometry_amd", "csrc")
WRAPPER = '''
#define __device__
#define __forceinline__ inline
#include "vio_flow_math.h"
extern "C" int verdict_host(int back_ok, float px, float py, float bx, float by, double max_dist, double *d2) {
    const double max_d2 = max_dist * max_dist;          // (the host's one product)
    return flow_back_verdict(back_ok != 0, px, py, bx, by, max_d2, *d2);
}
'''
# (inverse, back_levels) -> forward OK, forward lost, back lost, back far, kept
COUNTS = {(0, 2): (132, 8, 7, 61, 64), (0, 0): (132, 8, 7, 62, 63), (1, 2): (132, 8, 6, 65, 61)}


@pytest.mark.parametrize("inverse,back_levels", sorted(COUNTS))
def test_fixture_reaches_every_outcome(inverse, back_levels):
    ref = fb.fixture_reference(inverse, back_levels)
    c = fb.counts(ref)
    assert (c["forward_ok"], c["forward_lost"], c["back_lost"], c["back_far"], c["kept"]) == COUNTS[(inverse, back_levels)], c
    # a condition on the fixture, not a tolerance: every outcome class has members to compare
    assert min(c["forward_lost"], c["back_lost"], c["back_far"], c["kept"]) >= 5, c
    st, bst = ref["status"], ref["back_status"]
    ran = bst != fb.BACK_NOT_RUN
    assert np.all(np.isin(st[~ran], (fb.FAIL_LOST, fb.FAIL_BORDER, fb.NOT_FINITE))) and np.all(np.isin(st[ran], (fb.OK, fb.FAIL_BACK_LOST, fb.FAIL_BACK_FAR)))
    assert np.all(np.isnan(ref["back_d2"][~ran])) and np.all(np.isnan(ref["back_pts"][~ran])) and np.all(np.isfinite(ref["back_d2"][ran]))
    assert np.all((st == fb.FAIL_BACK_LOST) == (bst == fb.FAIL_LOST))
    kept = st == fb.OK
    assert np.all(ref["back_d2"][kept] <= 0.25) and np.all(ref["back_d2"][st == fb.FAIL_BACK_FAR] > 0.25)


def test_the_level_count_is_visible_in_the_fixture():
    two, all3 = fb.fixture_reference(0, 2), fb.fixture_reference(0, 0)
    assert two["next_pts"].tobytes() == all3["next_pts"].tobytes()             # the forward pass is the same
    assert two["status"].tobytes() != all3["status"].tobytes() and two["back_pts"].tobytes() != all3["back_pts"].tobytes()
    # no verdict of the fixture hangs on the last bits of the threshold
    for inv in (0, 1):
        r = fb.fixture_reference(inv, 2)
        d = np.sqrt(r["back_d2"][r["back_status"] == fb.OK])
        assert np.min(np.abs(d - 0.5)) > 5e-3


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ not found")
    d = tmp_path_factory.mktemp("flow_back_mirror")
    src, so = d / "mirror.cpp", d / "libmirror.so"
    src.write_text(WRAPPER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CSRC, "-o", str(so), str(src)])
    lib = C.CDLL(str(so))
    lib.verdict_host.argtypes = [C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_double, C.c_void_p]
    return lib


def test_verdict_matches_the_restatement(mirror):
    f32 = np.float32
    cases = []
    # d2 exactly at the threshold: (0.5, 0) from p, max_dist 0.5; (3, 4) from p, max_dist 5; one ulp of max_dist^2 above and below it
    for p, b, md in (((10.0, 20.0), (10.5, 20.0), 0.5), ((1.0, 2.0), (4.0, 6.0), 5.0), ((7.25, 3.5), (7.25, 3.0), 0.5)):
        d2 = fb.verdict(True, p, b, md)[1]
        assert d2 == md * md
        cases += [(1, p, b, md, fb.OK)]
        lim_up, lim_dn = np.sqrt(np.nextafter(md * md, np.inf)), np.sqrt(np.nextafter(md * md, 0.0))
        for m in (lim_up, lim_dn, np.nextafter(md, np.inf), np.nextafter(md, 0.0)):
            cases.append((1, p, b, float(m), fb.OK if d2 <= np.float64(m) * np.float64(m) else fb.FAIL_BACK_FAR))
    # one float ulp of the position either side of the threshold
    p = (f32(10.0), f32(20.0))
    for bx, want in ((np.nextafter(f32(10.5), f32(11)), fb.FAIL_BACK_FAR), (np.nextafter(f32(10.5), f32(10)), fb.OK)):
        cases.append((1, p, (bx, f32(20.0)), 0.5, want))
    # NaN, max_dist 0, a lost pass
    cases += [(1, p, (np.nan, 20.0), 0.5, fb.FAIL_BACK_FAR), (1, p, (10.0, np.nan), 1e30, fb.FAIL_BACK_FAR), (1, p, (np.inf, 20.0), 1e30, fb.FAIL_BACK_FAR),
              (1, p, p, 0.0, fb.OK), (1, p, (np.nextafter(f32(10.0), f32(11)), f32(20.0)), 0.0, fb.FAIL_BACK_FAR),
              (1, p, (3e28, -3e28), 1e30, fb.OK), (1, p, (3e38, -3e38), 1e30, fb.FAIL_BACK_FAR), (0, p, p, 0.5, fb.FAIL_BACK_LOST), (0, p, (np.nan, 1.0), 0.5, fb.FAIL_BACK_LOST)]
    rng = np.random.RandomState(3)
    for _ in range(500):
        q = rng.uniform(0, 100, 2).astype(f32)
        cases.append((1, q, (q + rng.uniform(-1, 1, 2) * 10.0 ** rng.uniform(-4, 0)).astype(f32), 0.5, None))
    seen = set()
    for ok, p, b, md, want in cases:
        st, d2 = fb.verdict(bool(ok), p, b, md)
        got = np.zeros(1)
        s = mirror.verdict_host(ok, f32(p[0]), f32(p[1]), f32(b[0]), f32(b[1]), float(md), got.ctypes.data)
        assert s == st and got.tobytes() == np.array([d2]).tobytes(), (ok, p, b, md, s, st, got, d2)
        assert want is None or st == want, (ok, p, b, md, st, want)
        seen.add(st)
    assert seen == {fb.OK, fb.FAIL_BACK_LOST, fb.FAIL_BACK_FAR}
